"""CPU: the coordinate lift specification itself (tests/lift_spec.py) against the alignment rows of tests/msa_export_spec.py
and against the pattern search's restatement (tests/locate_oracle.py), and the per-query device code
(edsparser_amd/csrc/lift_core.hpp) as host code under the address and undefined-behaviour sanitizers
(tests/cpp/test_lift_core.cpp, a program of its own)."""
import itertools
import os
import random
import struct
import subprocess

import pytest

import lift_spec as ls
import locate_oracle as lo
import msa_export_spec as ms
import oracle_lib as o
import path_spec as ps
import query_oracle as qo
from test_paths_cpu import ROOT, _random_msa, merge_fixture_inputs, vcf_fixture_outputs


def random_eds(rng, n_symbols, paths=4):
    """Symbols of 1-3 strings of 0-4 characters: empty strings, symbols of width 0, strings no path takes and symbols that
    some path misses included."""
    eds, seds = [], []
    for _ in range(n_symbols):
        k = rng.choice([1, 1, 2, 3])
        strings = ["" if rng.random() < 0.25 else "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 4))) for _ in range(k)]
        if rng.random() < 0.1:
            strings = [""] * k
        eds.append("{" + ",".join(strings) + "}")
        for _ in range(k):
            x = rng.random()
            ids = {0} if x < 0.15 else set(rng.sample(range(1, paths + 1), rng.randint(1, min(2, paths))))
            seds.append("{" + ",".join(str(i) for i in sorted(ids)) + "}")
    return "".join(eds).encode(), "".join(seds).encode()


def check_properties(eds, seds):
    """The properties of the restatement on one EDS -> number of (a, b, x) triples"""
    m = ls.Model(eds, seds)
    gap = next(bytes([g]) for g in b"-.*#" if bytes([g]) not in eds)
    rows = {p: ms.row(m.syms, m.sets, p, gap)[0] for p in range(1, m.P + 1)}
    seqs = {p: ps.spell(m.syms, m.sets, p)[0] for p in range(1, m.P + 1)}
    before = {p: [0] + list(itertools.accumulate(c != gap[0] for c in rows[p])) for p in rows}   # non-gap bytes of row[:c]
    triples = 0
    for a in range(1, m.P + 1):
        assert m.site(a, len(seqs[a])) == (ls.NO_SITE, ls.RANGE) and m.site(a, ls.U64_MAX) == (ls.NO_SITE, ls.RANGE)
        for b in range(1, m.P + 1):
            last = 0
            for x in range(len(seqs[a])):
                pos, st, site = m.lift(a, x, b)
                column = site[3]
                assert m.syms[site[0]][site[1]][site[2]] == seqs[a][x]
                assert rows[a][column] == seqs[a][x]
                assert pos == before[b][column]
                assert (st < ls.GAP) == (rows[b][column:column + 1] != gap)
                if st == ls.SAME:
                    assert seqs[b][pos] == seqs[a][x]
                if a == b:
                    assert (pos, st) == (x, ls.SAME)
                assert last <= pos <= len(seqs[b])
                last = pos
                triples += 1
    return triples


def test_properties_on_random_eds():
    rng = random.Random(20261019)
    triples = sum(check_properties(*random_eds(rng, rng.randint(1, 14), rng.randint(1, 5))) for _ in range(400))
    print("triples:", triples)
    assert triples > 20000


def test_properties_on_fixtures():
    ran = 0
    for eds, seds in merge_fixture_inputs() + vcf_fixture_outputs():
        try:
            ps.parse(eds, seds)
        except ValueError:                                       # fixtures whose sources do not match their text
            continue
        check_properties(eds, seds)
        ran += 1
    assert ran >= 250


def test_properties_on_msa2eds_results():
    rng = random.Random(5)
    ran = 0
    while ran < 60:
        msa, rows = _random_msa(rng, wrap=ran % 2 == 1)
        if len(set(rows)) < 2 or not any(rows):
            continue
        for l in (0, 3):
            check_properties(*o.msa(msa, l))
        ran += 1


def test_sites_are_locate_hits():
    """The closed loop with the pattern search: the L characters of path p from x on are found at the site of (p, x),
    under the site's common_pos, whenever p takes a string in every symbol of that stretch (a symbol p misses has no string
    the walk could take)."""
    rng = random.Random(77)
    kept = left_out = 0
    for _ in range(150):
        eds, seds = lo.random_eds(rng, rng.randint(2, 12), True)
        e = qo.Eds(eds, seds)
        m = ls.Model(eds.encode(), seds.encode())
        found = {}
        for p in range(1, m.P + 1):
            seq = ps.spell(m.syms, m.sets, p)[0]
            for x in range(len(seq)):
                for L in (1, 3, 6):
                    if x + L > len(seq):
                        continue
                    s0, s1 = m.site(p, x)[0], m.site(p, x + L - 1)[0]
                    if None in m.chosen[p][s0[0]:s1[0] + 1]:
                        left_out += 1
                        continue
                    pat = seq[x:x + L]
                    if pat not in found:
                        r = lo.locate(e, [pat], max_hits=10 ** 6)
                        assert r["flags"] == [0]
                        found[pat] = set(r["hits"])             # (common_pos, symbol, string, offset)
                    assert (s0[4],) + s0[:3] in found[pat], (eds, seds, p, x, L)
                    kept += 1
    print("kept %d, left out %d" % (kept, left_out))
    assert kept > 5000 and left_out <= 0.25 * (kept + left_out)


# ---- the host twin ---------------------------------------------------------------------------------------------------
def tables(m):
    """The device tables of every path of a model, row p - 1 for path p (path_device.hip): the words of one case"""
    n, nc = m.n, 0
    fixed = [len(s) == 1 and 0 in m.sets[f] for s, f in zip(m.syms, m.first)]
    cf, rank = [0], [0]
    for s, fx in zip(m.syms, fixed):
        cf.append(cf[-1] + (len(s[0]) if fx else 0))
        rank.append(rank[-1] + (0 if fx else 1))
    nc = rank[-1]
    str_off = [0]
    for s in m.syms:
        for t in s:
            str_off.append(str_off[-1] + len(t))
    csid, S = [], [0]
    for p in range(1, m.P + 1):
        for i in range(n):
            if not fixed[i]:
                j = m.chosen[p][i]
                csid.append(ls.U64_MAX if j is None else m.first[i] + j)
                S.append(S[-1] + (0 if j is None else len(m.syms[i][j])))
    words = [n, m.first[-1], nc, m.P]
    arrays = [[len(s) for s in m.syms], m.first[:-1], str_off, cf, rank, m.col, m.cc] + ([csid, S] if nc else [])
    return words, arrays


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    d = tmp_path_factory.mktemp("lift_core")
    exe = str(d / "test_lift_core")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-I", os.path.join(ROOT, "edsparser_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_lift_core.cpp"), "-o", exe], check=True)
    return exe, d


def test_lift_core_under_sanitizers(twin):
    exe, d = twin
    rng = random.Random(31)
    texts = [random_eds(rng, rng.randint(1, 14), rng.randint(1, 5)) for _ in range(120)]
    texts += [(b"{ACGT}", b"{1}"), (b"{ACGT}{GG}", b"{0}{0}"), (b"{}{A,}{}", b"{2}{1}{3}{1}"), (b"{A,C}", b"{1}{2,3}")]
    texts += [e for e in merge_fixture_inputs()[:40]]
    blob, expect = [], []
    for k, (eds, seds) in enumerate(texts):
        try:
            m = ls.Model(eds, seds)
        except ValueError:
            continue
        if m.P == 0:
            continue
        words, arrays = tables(m)
        finds = [(p - 1, x) for p in range(1, m.P + 1) for x in list(range(m.pos[p][-1] + 2)) + [ls.U64_MAX]]
        places = [(p - 1, i, j, q) for p in range(1, m.P + 1) for i in range(m.n + 1)
                  for j in range(len(m.syms[i]) + 1 if i < m.n else 1)
                  for q in list(range(len(m.syms[i][j]) + 1 if i < m.n and j < len(m.syms[i]) else 1)) + [ls.U64_MAX]]
        flat = words + [(1, 2, 3, 2048)[k % 4]] + [v for a in arrays for v in a]
        flat += [len(finds)] + [v for f in finds for v in f] + [len(places)] + [v for q in places for v in q]
        blob.append(struct.pack("<%dQ" % len(flat), *flat))
        for row, x in finds:
            site, st = m.site(row + 1, x)
            expect += [st] + list(site)
        for row, i, j, q in places:
            pos, st = m.place(i, j, q, row + 1)
            expect += [st, pos]
    cf, rf = str(d / "cases.bin"), str(d / "results.bin")
    open(cf, "wb").write(b"".join(blob))
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([exe, cf, rf], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-6000:]
    data = open(rf, "rb").read()
    got = list(struct.unpack("<%dQ" % (len(data) // 8), data))
    assert len(got) == len(expect) > 50000
    assert got == expect


def test_lift_core_offsets_above_32_bits(twin):
    """Tables are numbers: symbols of 3 * 10^9 and 5 * 10^9 characters around a choice symbol, so that the offsets, columns and common
    positions of the third symbol lie on both sides of 2^32; the answers in closed form."""
    exe, d = twin
    A, B = 3_000_000_000, 5_000_000_000
    none, T = ls.U64_MAX, 2 ** 32
    # {A x a}{ccccc,}{B x b}: path 1 takes "ccccc", path 2 the empty string; sources {0}{1}{2}{0}
    words = [3, 4, 1, 2, 2048]
    arrays = [[1, 2, 1], [0, 1, 3], [0, A, A + 5, A + 5, A + 5 + B], [0, A, A, A + B], [0, 0, 1, 1], [0, A, A + 5, A + 5 + B],
              [0, A, A, A + B], [1, 2], [0, 5, 5]]
    finds, expect = [], []
    for x in (0, A - 1, A, A + 4, A + 5, T - 1, T, T + 1, A + B - 1, A + B, A + B + 4, A + B + 5, none):
        finds.append((0, x))
        if x < A:
            expect += [0, 0, 0, x, x, x]
        elif x < A + 5:
            expect += [0, 1, 0, x - A, x, none]
        elif x < A + 5 + B:
            expect += [0, 2, 0, x - A - 5, x, x - 5]
        else:
            expect += [ls.RANGE] + [none] * 5
        finds.append((1, x))
        if x < A:
            expect += [0, 0, 0, x, x, x]
        elif x < A + B:
            expect += [0, 2, 0, x - A, x + 5, x]
        else:
            expect += [ls.RANGE] + [none] * 5
    places = [(0, 2, 0, T), (1, 2, 0, T), (1, 1, 0, 3), (0, 1, 1, 0), (0, 2, 0, B), (1, 2, 0, B - 1), (1, 0, 0, A - 1), (0, 3, 0, 0), (0, 2, 1, 0)]
    expect += [ls.SAME, A + 5 + T, ls.SAME, A + T, ls.GAP, A, ls.RANGE, none, ls.RANGE, none, ls.SAME, A + B - 1, ls.SAME, A - 1,
               ls.RANGE, none, ls.RANGE, none]
    flat = words + [v for a in arrays for v in a] + [len(finds)] + [v for f in finds for v in f] + [len(places)] + [v for q in places for v in q]
    cf, rf = str(d / "big.bin"), str(d / "big.out")
    open(cf, "wb").write(struct.pack("<%dQ" % len(flat), *flat))
    r = subprocess.run([exe, cf, rf], capture_output=True, text=True, env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert r.returncode == 0, r.stderr[-6000:]
    data = open(rf, "rb").read()
    assert list(struct.unpack("<%dQ" % (len(data) // 8), data)) == expect
