"""CPU: the linkage disequilibrium specification itself (tests/ld_spec.py) against the squared Pearson correlation of the
carrier indicator vectors, and its filters against each other; and the per-item device code (edsparser_amd/csrc/ld_core.hpp)
as host code under the address and undefined-behaviour sanitizers (tests/cpp/test_ld_core.cpp, a program of its own): the
symbol walk across the word seam, the listing rule, partner and tile ranges, and ld::r2 bit for bit."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import ld_cases as lc
import ld_spec as ls
import path_spec as ps
from test_paths_cpu import ROOT


def random_cases(seed, count):
    rng = random.Random(seed)
    return [lc.random_eds(rng, rng.randint(2, 8), rng.randint(2, 10)) for _ in range(count)]


@pytest.fixture(scope="module")
def cases():
    return random_cases(1, 300)


def indicator(T, both):
    return [1.0 if p in T else 0.0 for p in sorted(both)]


def test_r2_is_the_squared_correlation_of_the_carrier_indicators(cases):
    """another formula for the same number: rounding differs, within 1e-9 for counts of at most 10"""
    defined = undefined = 0
    for eds, seds in cases:
        syms, sets, P = ps.parse(eds, seds)
        cs = ls.carriers(syms, sets, set(range(1, P + 1)))
        where = {i: (T, U) for i, T, U in cs}
        res = ls.ld(eds, seds, window=3, min_count=0, all_strings=True)
        got = {p[:4]: p[8] for p in res["pairs"]}
        for i, j, i2, j2, n_ab, n_a, n_b, n in res["candidates"]:
            both = where[i][1] & where[i2][1]
            a, b = indicator(where[i][0][j], both), indicator(where[i2][0][j2], both)
            assert (n_ab, n_a, n_b, n) == (sum(x * y for x, y in zip(a, b)), sum(a), sum(b), len(both))
            constant = len(set(a)) < 2 or len(set(b)) < 2          # (also: no path present at both)
            assert constant == ((i, j, i2, j2) not in got)        # undefined pairs are exactly those with a constant indicator
            if constant:
                undefined += 1
                continue
            want = float(np.corrcoef(a, b)[0, 1]) ** 2
            assert abs(got[(i, j, i2, j2)] - want) <= 1e-9 and 0.0 <= got[(i, j, i2, j2)] <= 1.0
            defined += 1
        assert res["info"]["undefined_pairs"] == len(res["candidates"]) - len(got)
    assert defined > 2000 and undefined > 300


def test_candidates_add_up_and_filters_commute(cases):
    reported = 0
    for eds, seds in cases:
        for kw in (dict(min_count=1), dict(min_count=0, all_strings=True)):
            full = ls.ld(eds, seds, window=4, min_r2=0.0, **kw)
            rank = {i: r for r, (i, _, _) in enumerate(ls.carriers(*ps.parse(eds, seds)[:2], set()))}
            for w in (1, 2, 3):
                a, b = ls.ld(eds, seds, window=w, **kw), ls.ld(eds, seds, window=w + 1, **kw)
                assert a["pairs"] == [p for p in b["pairs"] if rank[p[2]] - rank[p[0]] <= w]
            for t in (0.1, 1 / 3, 1.0):
                part = ls.ld(eds, seds, window=4, min_r2=t, **kw)
                assert part["pairs"] == [p for p in full["pairs"] if p[8] >= t]
                i = part["info"]
                assert i["candidate_pairs"] == i["undefined_pairs"] + part["below_pairs"] + i["pairs"] == full["info"]["candidate_pairs"]
            assert full["pairs"] == sorted(full["pairs"], key=lambda p: p[:4])
            reported += len(full["pairs"])
    assert reported > 3000


def test_counts_over_all_strings_sum_to_present(cases):
    for eds, seds in cases:
        P = ps.parse(eds, seds)[2]
        for paths in (None, [1, P, P]) if P else (None,):         # (P = 0: every set is universal)
            res = ls.ld(eds, seds, paths, window=1, min_count=0, all_strings=True)
            per = {}
            for sym, j, count, present in res["alleles"]:
                per.setdefault(sym, [present, 0])[1] += count
            assert len(per) == res["info"]["choice_symbols"] and all(p == c for p, c in per.values())
            assert res["info"]["paths"] == (P if paths is None else len(set(paths)))
    with pytest.raises(ValueError, match=r"Path id 4 out of range \(1..3\)"):
        ls.ld(b"{A,C}", b"{1}{3}", [4])


def test_text_formats():
    eds, seds = b"{A,C}{G}{T,A,}{C,G}", b"{1,2}{3,4}{0}{1}{2,3}{4}{1,3}{2,4}"
    res = ls.ld(eds, seds, window=1)
    assert res["alleles"] == [(0, 1, 2, 4), (2, 1, 2, 4), (2, 2, 1, 4), (3, 1, 2, 4)]
    assert [p[:8] for p in res["pairs"]] == [(0, 1, 2, 1, 1, 2, 2, 4), (0, 1, 2, 2, 1, 2, 1, 4), (2, 1, 3, 1, 1, 2, 2, 4), (2, 2, 3, 1, 1, 1, 2, 4)]
    assert ls.pair_text(res["pairs"][1:2]) == b"symbol_a\tstring_a\tsymbol_b\tstring_b\tn_ab\tn_a\tn_b\tn\tr2\n0\t1\t2\t2\t1\t2\t1\t4\t0.333333\n"
    assert ls.freq_text(res["alleles"][:1]) == b"symbol\tstring\tcount\tpresent\tfreq\n0\t1\t2\t4\t0.5\n"


# ---- the host twin -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    d = tmp_path_factory.mktemp("ld_core")
    exe = str(d / "test_ld_core")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-I", os.path.join(ROOT, "edsparser_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_ld_core.cpp"), "-o", exe], check=True)
    return exe, d


def run_twin(twin, name, blob):
    exe, d = twin
    cf, rf = str(d / (name + ".bin")), str(d / (name + ".out"))
    open(cf, "wb").write(blob)
    r = subprocess.run([exe, cf, rf], capture_output=True, text=True, env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert r.returncode == 0, r.stderr[-6000:]
    data = open(rf, "rb").read()
    return list(struct.unpack("<%dQ" % (len(data) // 8), data))


def u64s(*v):
    return struct.pack("<%dQ" % len(v), *v)


def row(paths):
    return sum(1 << (p - 1) for p in paths)


def words(x, WP):
    return [(x >> (64 * w)) & (2 ** 64 - 1) for w in range(WP)]


def eds_record(eds, seds, paths, min_count, all_strings, windows):
    """record kind 0 of tests/cpp/test_ld_core.cpp: the tables of the session as the device holds them, and the request"""
    syms, sets, P = ps.parse(eds, seds)
    W, WP = P // 64 + 1, (P + 63) // 64
    size = [len(s) for s in syms]
    ent_off = [sum(size[:i]) for i in range(len(syms))]
    cidx = [i for i, s in enumerate(syms) if not (len(s) == 1 and 0 in sets[ent_off[i]])]
    bits = [sum(1 << (x - 64 * w) for x in q if 64 * w <= x < 64 * w + 64) for q in sets for w in range(W)]
    M = ls.requested(P, paths)
    return u64s(0, len(syms), len(sets), len(cidx), P, W, *size, *ent_off, *cidx, *bits, WP, *words(row(M), WP), min_count,
                int(all_strings), len(windows), *windows)


def check_eds_result(got, at, eds, seds, paths, min_count, all_strings, windows):
    """the twin's answer for one EDS record from got[at:] -> the next position"""
    syms, sets, P = ps.parse(eds, seds)
    WP = (P + 63) // 64
    cs = ls.carriers(syms, sets, ls.requested(P, paths))
    want, T_rows, ar, afirst = [], [], [], [0]
    for r, (i, T, U) in enumerate(cs):
        want.append(len(U))
        for j, t in enumerate(T):
            is_listed = (j >= 1 or all_strings) and min_count <= len(t) <= len(U) - min_count
            want += [len(t), int(is_listed)]
            if is_listed:
                T_rows.append(row(t)); ar.append(r)
        afirst.append(len(ar))
    A, nc = len(ar), len(cs)
    want += [A] + afirst + [w for t in T_rows for w in words(t, WP)] + [w for _, _, U in cs for w in words(row(U), WP)]
    assert all(t >> P == 0 for t in T_rows)                      # zero padding
    for window in windows:
        lohi = [(afirst[r + 1], afirst[min(nc, r + window + 1)]) for r in ar]
        want += [v for p in lohi for v in p]
        RT = (A + 63) // 64
        want.append(RT)
        tiles = []
        for t in range(RT):
            lo, hi = lohi[64 * t][0], lohi[min(A, 64 * t + 64) - 1][1]
            c0, c1 = (lo // 64, (hi + 63) // 64) if hi > lo else (0, 0)
            want += [c0, c1]
            tiles += [t] * (c1 - c0)
            for x in range(64 * t, min(A, 64 * t + 64)):          # every partner of the tile's alleles lies in its column tiles
                assert lohi[x][0] >= lohi[x][1] or (64 * c0 <= lohi[x][0] and lohi[x][1] <= 64 * c1)
        want += [len(tiles)] + tiles + [sum(hi - lo for lo, hi in lohi)]
    assert got[at:at + len(want)] == want, (eds[:80], paths, min_count, all_strings)
    return at + len(want)


def test_ld_core_under_sanitizers(twin):
    """the walk for P on both sides of the word seam, a symbol of 300 strings, small random EDSs and boundary shapes;
    partner and tile ranges for windows below, at and above nc"""
    rng = random.Random(31)
    runs = []
    for P in (1, 63, 64, 65, 128, 129):
        eds, seds = lc.panel_eds(rng, P, 7, p_missing=0.1 if P > 1 else 0.0, universal="middle")
        nc = len(ls.carriers(*ps.parse(eds, seds)[:2], set()))
        runs.append((eds, seds, None, 1, False, [1, nc - 1, nc, nc + 5]))
        runs.append((eds, seds, [P, 1, P], 0, True, [2]))
    many = lc.render([[b"AC"], [b"%c%c%c" % (65 + k % 7, 65 + k // 7 % 7, 65 + k // 49) for k in range(300)], [b"G", b"T"]],
                     [{0}] + [{k + 1} for k in range(300)] + [{1, 2, 200}, {300, 64, 65}])
    runs += [many + (None, 1, False, [1, 2, 3]), many + (None, 0, True, [1])]
    runs += [c + (None, 1, rng.random() < 0.5, [rng.randint(1, 4)]) for c in random_cases(32, 300)]
    shapes = lc.boundary_shapes()
    for name in ("alleles65", "alleles200", "wide70", "missing", "windows"):
        eds, seds, reqs = shapes[name]
        for kw in reqs:
            runs.append((eds, seds, kw.get("paths"), kw.get("min_count", 1), kw.get("all_strings", False), [kw["window"]]))
    got = run_twin(twin, "cases", b"".join(eds_record(*r) for r in runs))
    at = 0
    for r in runs:
        at = check_eds_result(got, at, *r)
    assert at == len(got) > 20000


def test_r2_bit_equal_to_python(twin):
    rng = random.Random(33)
    items = [(4, 2, 2, 1), (4, 2, 2, 2), (4, 2, 2, 0), (4, 0, 2, 0), (4, 4, 2, 2), (0, 0, 0, 0), (3, 1, 2, 1),
             (9_999_999, 3_333_333, 7_777_777, 3_000_001), (9_999_999, 1, 9_999_998, 0), (9_999_999, 4_999_999, 5_000_000, 2_500_000)]
    while len(items) < 4000:
        n = rng.choice([rng.randint(1, 12), rng.randint(1, 2000), rng.randint(1, 9_999_999)])
        n_a, n_b = rng.randint(0, n), rng.randint(0, n)
        items.append((n, n_a, n_b, rng.randint(max(0, n_a + n_b - n), min(n_a, n_b))))
    got = run_twin(twin, "r2", u64s(1, len(items), *[v for it in items for v in it]))
    want = []
    for n, n_a, n_b, n_ab in items:
        v = ls.r2_of(n_ab, n_a, n_b, n)
        want += [0, 0] if v is None else [1, struct.unpack("<Q", struct.pack("<d", v))[0]]
    assert got == want and sum(want[::2]) > 3000
