"""CPU: the region slice specification itself (tests/slice_spec.py) against its two invariants - the alignment rows of a
slice are the column window of the rows of the input (tests/msa_export_spec.py), and column regions that tile a window
spell what the window spells - the per-region device code (edsparser_amd/csrc/slice_core.hpp) as host code under the
address and undefined-behaviour sanitizers (tests/cpp/test_slice_core.cpp, a program of its own), and the region grammar
of edsparser-slice (tests/cpp/test_slice_args.cpp)."""
import os
import random
import struct
import subprocess

import pytest

import lift_spec as ls
import msa_export_spec as ms
import oracle_lib as o
import path_spec as ps
import slice_spec as ss
from test_lift_cpu import tables
from test_paths_cpu import ROOT, _random_msa, merge_fixture_inputs, vcf_fixture_outputs


def random_eds(rng, n_symbols, paths):
    """String lengths from {0, 0, 1, 2, 3, 5}; 60 % of the one-string symbols are universal, so that few paths are empty"""
    eds, seds = [], []
    for _ in range(n_symbols):
        k = rng.choice([1, 1, 2, 3])
        eds.append("{" + ",".join("".join(rng.choice("ACGT") for _ in range(rng.choice([0, 0, 1, 2, 3, 5]))) for _ in range(k)) + "}")
        for _ in range(k):
            ids = {0} if k == 1 and rng.random() < 0.6 else set(rng.sample(range(1, paths + 1), rng.randint(1, min(2, paths))))
            seds.append("{" + ",".join(str(i) for i in sorted(ids)) + "}")
    return "".join(eds).encode(), "".join(seds).encode()


def check_invariants(eds, seds, rng, cap=40):
    """Both invariants on one EDS, on every region when there are at most `cap` per path, else on `cap` drawn ones
    -> (path regions, column regions, (EDS, path) pairs, pairs skipped because the anchor path is empty)"""
    m = ss.Model(eds, seds)
    gap = next(bytes([g]) for g in b"-.*#" if bytes([g]) not in eds)
    rows = {p: ms.row(m.syms, m.sets, p, gap)[0] for p in range(1, m.P + 1)}
    seqs = {p: ps.spell(m.syms, m.sets, p)[0] for p in range(1, m.P + 1)}
    n_path = n_col = skipped = 0
    for a in range(m.P + 1):
        L = m.length(a)
        if a and L == 0:
            skipped += 1
            continue
        assert m.cut(a, 0, L + 1) is None and m.cut(a, 1, 1) is None and (L == 0 or m.cut(a, 0, L) is not None)
        if L * (L + 1) // 2 <= cap:
            regions = [(s, e) for s in range(L) for e in range(s + 1, L + 1)]
        else:
            regions = [(s, rng.randint(s + 1, L)) for s in (rng.randrange(L) for _ in range(cap))]
        for s, e in regions:
            syms, sets, ends = m.cut(a, s, e)
            # the renderer writes what the parser reads (a set that holds 0 comes back as {0})
            assert ps.parse(*ss.render(syms, sets))[:2] == (syms, [{0} if 0 in q else q for q in sets])
            assert len(syms) == ends[1] - ends[0] + 1 and [len(x) for x in syms] == [len(x) for x in m.syms[ends[0]:ends[1] + 1]]
            for p in range(1, m.P + 1):
                assert ms.row(syms, sets, p, gap)[0] == rows[p][ends[4]:ends[5]], (eds, seds, a, s, e, p)
            if a:
                assert ps.spell(syms, sets, a)[0] == seqs[a][s:e]
                n_path += 1
            else:
                assert ends[4:] == (s, e)
                n_col += 1
    if m.W >= 2:                                                 # tiling: [a, b) in three pieces, empty ones left out
        a, b = sorted(rng.sample(range(m.W + 1), 2))
        cuts = sorted([a, b, rng.randint(a, b), rng.randint(a, b)])
        whole = m.cut(0, a, b)
        for p in range(1, m.P + 1):
            parts = b"".join(ps.spell(*m.cut(0, x, y)[:2], p)[0] for x, y in zip(cuts, cuts[1:]) if x < y)
            assert parts == ps.spell(whole[0], whole[1], p)[0]
    return n_path, n_col, m.P, skipped


def test_invariants_on_random_eds():
    rng = random.Random(20261019)
    tot = [0, 0, 0, 0]
    for _ in range(500):
        tot = [x + y for x, y in zip(tot, check_invariants(*random_eds(rng, rng.randint(1, 8), rng.randint(1, 5)), rng))]
    print("path regions %d, column regions %d, pairs %d, skipped %d" % tuple(tot))
    assert tot[0] > 10000 and tot[1] > 5000
    assert tot[3] < 0.15 * tot[2]


def test_invariants_on_fixtures():
    rng = random.Random(3)
    ran, pairs, skipped = 0, 0, 0
    for eds, seds in merge_fixture_inputs() + vcf_fixture_outputs():
        try:
            ps.parse(eds, seds)
        except ValueError:                                       # fixtures whose sources do not match their text
            continue
        r = check_invariants(eds, seds, rng, 12)
        pairs += r[2]
        skipped += r[3]
        ran += 1
    assert ran >= 250
    assert skipped < 0.15 * pairs


def test_invariants_on_msa2eds_results():
    rng = random.Random(5)
    ran = pairs = skipped = 0
    while ran < 40:
        msa, rows = _random_msa(rng, wrap=ran % 2 == 1)
        if len(set(rows)) < 2 or not any(rows):
            continue
        for l in (0, 3):
            r = check_invariants(*o.msa(msa, l), rng, 12)
            pairs += r[2]
            skipped += r[3]
        ran += 1
    assert skipped < 0.15 * pairs


# ---- the host twin ---------------------------------------------------------------------------------------------------
def set_text(q):
    return b"{0}" if 0 in q else b"{" + b",".join(str(x).encode() for x in sorted(q)) + b"}"


def numbers(lens, set_bytes, ends):
    """What tests/cpp/test_slice_core.cpp writes for a region that is not RANGE, from lengths alone: lens[i][j] the
    length of string j of symbol i, set_bytes per string, ends = (i0, i1, o0, o1e, c0, c1e)"""
    i0, i1, o0, o1e = ends[:4]
    first, str_off, sb = [0], [0], [0]
    for s in lens:
        first.append(first[-1] + len(s))
        for t in s:
            str_off.append(str_off[-1] + t)
    for b in set_bytes:
        sb.append(sb[-1] + b)
    per, at, sat = [], 0, 0
    lo = hi = None
    for i in range(i0, i1 + 1):
        at += 1                                                  # '{'
        for j, t in enumerate(lens[i]):
            begin = min(t, o0) if i == i0 else 0
            kept = max((min(t, o1e) if i == i1 else t) - begin, 0)
            slot = j if i == i0 else len(lens[i0]) + j if i == i1 else ss.U64_MAX
            g = first[i] + j
            per += [at, begin, kept, sat, slot]
            if g == first[i0]:
                lo = str_off[g] + begin
            hi = str_off[g] + begin + kept                       # (of the last string in the end)
            at += kept + 1                                       # the string and ',' or '}'
            sat += set_bytes[g]
    strings = first[i1 + 1] - first[i0]
    chars = at - strings - (i1 - i0 + 1)
    edge = len(lens[i0]) + (len(lens[i1]) if i1 != i0 else 0)
    return list(ends) + [strings, chars, at + 1, sat + 1, edge, lo, hi] + per


def from_texts(m, p, s, e):
    """the same from the rendered texts of the specification: where every string and every set begins"""
    c = m.cut(p, s, e)
    if c is None:
        return None
    syms, sets, ends = c
    te, ts = ss.render(syms, sets)
    dst, sdst, at, sat = [], [], 0, 0
    for x in syms:
        at += 1
        for t in x:
            dst.append(at)
            at += len(t) + 1
    for q in sets:
        sdst.append(sat)
        sat += len(set_text(q))
    assert at + 1 == len(te) and sat + 1 == len(ts)
    return ends, dst, sdst, [len(t) for x in syms for t in x], len(te), len(ts)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    d = tmp_path_factory.mktemp("slice_core")
    exe = str(d / "test_slice_core")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-I", os.path.join(ROOT, "edsparser_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_slice_core.cpp"), "-o", exe], check=True)
    return exe, d


def run_twin(twin, name, flat):
    exe, d = twin
    cf, rf = str(d / (name + ".bin")), str(d / (name + ".out"))
    open(cf, "wb").write(struct.pack("<%dQ" % len(flat), *flat))
    r = subprocess.run([exe, cf, rf], capture_output=True, text=True, env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert r.returncode == 0, r.stderr[-6000:]
    data = open(rf, "rb").read()
    return list(struct.unpack("<%dQ" % (len(data) // 8), data))


def test_slice_core_under_sanitizers(twin):
    """every (start, end) of every path and every column window of small EDSs, one past the end included"""
    rng = random.Random(31)
    texts = [random_eds(rng, rng.randint(1, 7), rng.randint(1, 5)) for _ in range(60)]
    texts += [(b"{ACGT}", b"{1}"), (b"{ACGT}{GG}", b"{0}{0}"), (b"{}{A,}{}", b"{2}{1}{3}{1}"), (b"{A,C}", b"{1}{2,3}"),
              (b"{}{AC}{G,TTT,}{A}{}{,}{CG,C}{T}", b"{0}{0}{1}{2}{3}{0}{0}{1}{2}{1}{3}{0}"),
              (b"{AC,G}{T}{,A}", b"{9,10}{99,100,130}{0}{1000}{64,65}")]
    flat, expect = [], []
    for eds, seds in texts:
        lm, m = ls.Model(eds, seds), ss.Model(eds, seds)
        words, arrays = tables(lm)
        W = m.P // 64 + 1
        bits = [sum(1 << (x - 64 * w) for x in q if 64 * w <= x < 64 * w + 64) for q in m.sets for w in range(W)]
        regions = [(p, s, e) for p in range(m.P + 1) for L in [m.length(p)] for s in range(L + 2) for e in range(s, L + 2)]
        if m.P:
            regions.append((1, 0, 0))                            # end - 1 wraps
        flat += words + [W] + [v for a in arrays for v in a] + bits + [len(regions)] + [v for q in regions for v in q]
        lens, sbytes = [[len(t) for t in x] for x in m.syms], [len(set_text(q)) for q in m.sets]
        sb = [0]
        for b in sbytes:
            sb.append(sb[-1] + b)
        expect += sb
        for p, s, e in regions:
            t = from_texts(m, p, s, e)
            if t is None:
                expect.append(ss.RANGE)
                continue
            want = numbers(lens, sbytes, t[0])
            # the arithmetic restatement against the texts: where the strings and sets begin, how long they are, the sizes
            assert want[6:10] == [len(t[1]), sum(t[3]), t[4], t[5]]
            assert want[13::5] == t[1] and want[15::5] == t[3] and want[16::5] == t[2]
            expect += [ss.OK] + want
    got = run_twin(twin, "cases", flat)
    assert len(got) == len(expect) > 100000
    assert got == expect


def test_slice_core_offsets_above_32_bits(twin):
    """Tables are numbers: {A x a}{ccccc,}{B x b} with A = 3 * 10^9 and B = 5 * 10^9, sources {0}{1}{2}{0}: cuts, columns,
    destinations and copy spans on both sides of 2^32; the answers from the lengths alone"""
    A, B, T = 3_000_000_000, 5_000_000_000, 2 ** 32
    lens, sbytes = [[A], [5, 0], [B]], [3, 3, 3, 3]
    words = [3, 4, 1, 2, 1]
    arrays = [[1, 2, 1], [0, 1, 3], [0, A, A + 5, A + 5, A + 5 + B], [0, A, A, A + B], [0, 0, 1, 1], [0, A, A + 5, A + 5 + B],
              [0, A, A, A + B], [1, 2], [0, 5, 5], [1, 2, 4, 1]]
    at = {0: arrays[5], 1: [0, A, A + 5, A + 5 + B], 2: [0, A, A, A + B]}
    regions = [(1, 0, A + 5 + B), (1, 0, A + 5 + B + 1), (1, A - 1, A + 1), (1, T - 5, T + 5), (1, A + 2, A + 3), (1, A - 3, A + 5 + T + 7),
               (2, T, A + B), (2, A - 1, A + 1), (2, 0, A + B + 1), (0, 5, A + 5 + B), (0, T - 1, T + 1), (0, A + 4, A + 6), (0, 0, A + 5 + B + 1),
               (2, T + 1, T + 1)]
    expect, gone = [0, 3, 6, 9, 12], 0
    for p, s, e in regions:
        if s >= e or e > at[p][-1]:
            expect.append(ss.RANGE)
            gone += 1
            continue
        i0 = max(i for i in range(3) if at[p][i] <= s)
        i1 = max(i for i in range(3) if at[p][i] <= e - 1)
        o0, o1 = s - at[p][i0], e - 1 - at[p][i1]
        expect += [ss.OK] + numbers(lens, sbytes, (i0, i1, o0, o1 + 1, at[0][i0] + o0, at[0][i1] + o1 + 1))
    flat = words + [v for a in arrays for v in a] + [len(regions)] + [v for q in regions for v in q]
    got = run_twin(twin, "big", flat)
    assert got == expect
    assert gone == 4 and max(expect) > A + B > T


# ---- the tool's region grammar -------------------------------------------------------------------------------------------
def test_region_grammar(tmp_path):
    exe = str(tmp_path / "test_slice_args")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-I", os.path.join(ROOT, "edsparser_amd", "host", "tools"), os.path.join(ROOT, "tests", "cpp", "test_slice_args.cpp"),
                    "-o", exe], check=True)
    cases = [("r 7:10-20", "7 10 20 7_10_20"), ("r hap7:0-1", "7 0 1 7_0_1"), ("r 0:0-5", "bad"), ("r 7:10", "bad"), ("r 7-10-20", "bad"),
             ("r x7:1-2", "bad"), ("r 7:-1-2", "bad"), ("r 7:1-2x", "bad"), ("r 7:5-5", "7 5 5 7_5_5"), ("r hap:1-2", "bad"), ("r :1-2", "bad"),
             ("r 18446744073709551615:0-18446744073709551615", "18446744073709551615 0 18446744073709551615 18446744073709551615_0_18446744073709551615"),
             ("r 1:0-18446744073709551616", "bad"),
             ("c 0-5000", "0 0 5000 cols_0_5000"), ("c 5000", "bad"), ("c a-b", "bad"), ("c 3-2", "0 3 2 cols_3_2"),
             ("b hap2\t3\t12\tgene one\t+", "2 3 12 gene one"), ("b 4\t0\t5", "4 0 5 4_0_5"), ("b 4\t0\t5\t", "4 0 5 4_0_5"),
             ("b 4\t0\t5\t\t+", "4 0 5 4_0_5"), ("b # a comment", "skip"), ("b 4\t0\t5\r", "4 0 5 4_0_5"), ("b 4 0 5", "bad"),
             ("b 4\t0", "bad"), ("b chr1\t0\t5", "bad"), ("b 0\t0\t5", "bad"), ("b 4\t0\t5\ta/b", "bad"), ("b 4\t0\t5\t..", "bad"),
             ("b 4\t-1\t5", "bad")]
    (tmp_path / "cases.txt").write_bytes(b"".join(c.encode() + b"\n" for c, _ in cases))
    r = subprocess.run([exe, str(tmp_path / "cases.txt"), "hap"], capture_output=True, text=True,
                       env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split("\n")[:-1] == [w for _, w in cases]
