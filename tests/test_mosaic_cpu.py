"""CPU: the mosaic specification itself (tests/mosaic_spec.py) against properties that follow from its definition and
against an independent dynamic programme for the fewest pieces; and the per-item device code
(edsparser_amd/csrc/mosaic_core.hpp) as host code under the address and undefined-behaviour sanitizers
(tests/cpp/test_mosaic_core.cpp, a program of its own, nothing preloaded): the march emulated word by word with the donors
across one lane and across 64, every record and target_off against the specification."""
import os
import subprocess

import pytest

import dist_cases as dc
import dist_spec as ds
import ibs_cases as ic
import mosaic_cases as mc
import mosaic_spec as msp
import path_spec as ps
from test_dist_cpu import eds_record, random_cases, u64s
from test_dist_cpu import run_twin as run_program
from test_paths_cpu import ROOT

N = msp.NONE


def fewest_pieces(eds, seds, t, donors):
    """the fewest pieces that tile [0, n - 1], a piece being an interval over which one eligible donor agrees with t
    throughout, or an interval of symbols at none of which an eligible donor agrees: f[e] over every way to end a piece
    at e, no greedy choice anywhere"""
    syms, sets, _ = ps.parse(eds, seds)
    n = len(syms)
    ch = {p: ds.chosen(syms, sets, p) for p in set(donors) | {t}}
    eligible, a = [d for d in donors if d != t], ch[t]
    shared = [any(ch[d][i] == a[i] for d in eligible) for i in range(n)]
    f = [0] + [10 ** 9] * n
    for s in range(n):
        for d in eligible:
            e = s
            while e < n and a[e] == ch[d][e]:
                e += 1
                f[e] = min(f[e], f[s] + 1)
        e = s
        while e < n and not shared[e]:
            e += 1
            f[e] = min(f[e], f[s] + 1)
    return f[n]


# ---- the specification ---------------------------------------------------------------------------------------------------
def test_segments_tile_copy_and_are_fewest():
    targets = small = private = 0
    for eds, seds in random_cases(21, 300) + [dc.EDGE, ic.GAPS, ic.NONE, ic.ENDS, ic.ADJACENT, ic.FIXED, mc.TIE]:
        syms, sets, P = ps.parse(eds, seds)
        if P == 0:
            continue
        n = len(syms)
        got = msp.mosaic(eds, seds)
        off, recs = got["target_off"], got["segments"]
        ch = {p: ds.chosen(syms, sets, p) for p in range(1, P + 1)}
        assert len(off) == P + 1 and off[0] == 0 and off[-1] == len(recs) == got["info"]["segments"]
        assert got["info"]["switches"] == len(recs) - P
        for x in range(P):
            t, mine = x + 1, recs[off[x]:off[x + 1]]
            eligible = [y for y in range(P) if y + 1 != t]
            agrees = lambda y, i: ch[y + 1][i] == ch[t][i]
            targets += 1
            # they tile [0, n - 1]
            assert mine[0][2] == 0 and mine[-1][3] == n - 1 and all(r[0] == x and r[2] <= r[3] for r in mine)
            assert all(a[3] + 1 == b[2] for a, b in zip(mine, mine[1:]))
            inside = set()
            for k, (_, y, sf, sl, _, _, _) in enumerate(mine):
                if y == N:
                    # private symbols are those where no eligible donor agrees
                    assert not any(agrees(d, i) for d in eligible for i in range(sf, sl + 1))
                    inside |= set(range(sf, sl + 1))
                    continue
                # a copied segment agrees throughout, nobody reaches further, and nobody of a smaller position as far
                assert y in eligible and all(agrees(y, i) for i in range(sf, sl + 1))
                assert sl == n - 1 or not agrees(y, sl + 1)
                for d in eligible:
                    reach = next((i for i in range(sf, n) if not agrees(d, i)), n)
                    assert reach <= sl + 1 and (reach <= sl or d >= y)
                if k + 1 < len(mine) and mine[k + 1][1] == N:
                    assert not any(agrees(d, sl + 1) for d in eligible)
            assert inside == {i for i in range(n) if not any(agrees(d, i) for d in eligible)}
            private += len(inside)
            if P <= 8 and n <= 60:
                assert fewest_pieces(eds, seds, t, list(range(1, P + 1))) == len(mine), (eds, seds, x)
                small += 1
    assert targets > 900 and small > 900 and private > 100


def test_by_hand():
    eds, seds = ic.ENDS
    got = msp.mosaic(eds, seds)
    assert got["segments"] == [(0, 2, 0, 2, 2, 0, 4), (1, N, 0, 0, 1, 0, 1), (1, 0, 1, 1, 0, 1, 3), (1, N, 2, 2, 1, 3, 4), (2, 0, 0, 2, 2, 0, 4)]
    assert got["target_off"] == [0, 1, 4, 5]
    assert got["info"] == {"targets": 3, "donors": 3, "choice_symbols": 2, "segments": 5, "private_segments": 2, "private_symbols": 2,
                           "switches": 2}
    assert msp.mosaic(*ic.FIXED, [1], [1])["segments"] == [(0, N, 0, 2, 0, 0, 6)]
    none = [r for r in msp.mosaic(*ic.NONE)["segments"] if r[0] == 2]
    assert [r[:4] for r in none] == [(2, 3, 0, 4), (2, 0, 5, 6)]             # two paths without a string agree
    assert msp.mosaic(*ic.ADJACENT)["segments"] == [(0, N, 0, 1, 2, 0, 2), (1, N, 0, 1, 2, 0, 2)]
    # the tie: donors 2 and 3 go with path 1 over symbol 0 alike; the smaller request position has it
    assert msp.mosaic(*mc.TIE, [1])["segments"] == [(0, 1, 0, 0, 1, 0, 1), (0, 3, 1, 2, 1, 1, 3)]
    assert msp.mosaic(*mc.TIE, [1], [3, 2, 4])["segments"] == [(0, 0, 0, 0, 1, 0, 1), (0, 2, 1, 2, 1, 1, 3)]
    assert msp.text(eds, seds, [2], prefix=b"hap") == msp.HEADER + b"hap1\t.\t0\t0\t1\t0\t1\t1\nhap1\thap0\t1\t1\t0\t1\t3\t2\nhap1\t.\t2\t2\t1\t3\t4\t1\n"
    assert msp.text(eds, seds, [3], [2, 1], names=[b"a", b"b", b"c"]) == msp.HEADER + b"c\ta\t0\t2\t2\t0\t4\t4\n"
    assert msp.breakpoints(eds, seds, [2, 3]) == msp.BREAKPOINT_HEADER + b"s1\t.\ts0\t1\t1\ns1\ts0\t.\t2\t3\n"
    with pytest.raises(ValueError, match=r"Path id 4 out of range \(1..3\)"):
        msp.mosaic(eds, seds, [1], [1, 4])
    with pytest.raises(ValueError, match=r"Path id 0 out of range \(1..3\)"):
        msp.mosaic(eds, seds, [0])


def test_request_order_duplicates_and_the_target_among_the_donors():
    eds, seds = dc.EDGE
    targets, donors = [66, 4, 4, 1], [1, 4, 4, 65, 1]
    got = msp.mosaic(eds, seds, targets, donors)
    for x, t in enumerate(targets):
        mine = [r[1:] for r in got["segments"][got["target_off"][x]:got["target_off"][x + 1]]]
        keep = [y for y, d in enumerate(donors) if d != t]       # the target's own path is not there for it
        alone = msp.mosaic(eds, seds, [t], [donors[y] for y in keep])["segments"]
        assert mine == [((N if r[1] == N else keep[r[1]]),) + r[2:] for r in alone]
    n = len(ps.parse(eds, seds)[0])
    assert [r[1:4] for r in msp.mosaic(eds, seds, [4], [4, 4])["segments"]] == [(N, 0, n - 1)]      # donors = [t] only
    assert all(r[1] in (N, 0, 1, 3) for r in got["segments"])    # of equal donors the first position, never 2 or 4


def test_the_planted_recombinant_comes_back():
    eds, seds, requests = mc.shapes()["planted"]
    n, (b1, b2) = mc.PLANTED_SYMBOLS, mc.PLANTED_BREAKS
    assert [r[:4] for r in msp.mosaic(eds, seds, **requests[0])["segments"]] == [(0, 0, 0, b1 - 1), (0, 1, b1, b2 - 1), (0, 2, b2, n - 1)]
    assert [r[:4] for r in msp.mosaic(eds, seds, **requests[1])["segments"]] == [(0, 2, 0, b1 - 1), (0, 1, b1, b2 - 1), (0, 0, b2, n - 1)]
    desc, _ = dc.classes(eds, seds, "strings")
    assert len(desc) == 2 * n and desc[64][0] == b1 and desc[mc.CHUNK_COLUMNS][0] == b2      # the breaks start a word and a chunk


def test_shapes_are_what_they_claim():
    shapes = mc.shapes()
    assert ps.parse(*shapes["wide"][:2])[2] == 130 and ps.parse(*shapes["crowd"][:2])[2] == 300
    for c in (63, 64, 65, mc.CHUNK_COLUMNS - 1, mc.CHUNK_COLUMNS, mc.CHUNK_COLUMNS + 1):
        eds, seds, requests = shapes["columns%d" % c]
        assert len(dc.classes(eds, seds, "strings")[0]) == c
        got = msp.mosaic(eds, seds, **requests[1])
        assert got["info"]["segments"] > 2 * got["info"]["targets"]
    assert msp.mosaic(*shapes["crowd"][:2], **shapes["crowd"][2][1])["info"]["donors"] == 302


# ---- the host twin -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    d = tmp_path_factory.mktemp("mosaic_core")
    exe = str(d / "test_mosaic_core")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-I", os.path.join(ROOT, "edsparser_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_mosaic_core.cpp"), "-o", exe], check=True)
    return exe, d


def call_record(eds, seds, targets, donors, lanes):
    targets, donors = msp.requested(eds, seds, targets, donors)
    return eds_record(eds, seds) + u64s(len(targets), *targets, len(donors), *donors, lanes)


def check_call(got, at, eds, seds, targets, donors, lanes):
    want = msp.mosaic(eds, seds, targets, donors)
    C = len(dc.classes(eds, seds, "strings")[0])
    T, total, where = want["info"]["targets"], want["info"]["segments"], (eds[:80], seds[:80], targets, donors, lanes)
    assert got[at:at + 4] == [C, total, want["info"]["private_segments"], want["info"]["private_symbols"]], where
    at += 4
    assert got[at:at + T + 1] == want["target_off"], where
    at += T + 1
    assert [tuple(got[at + 7 * k:at + 7 * k + 7]) for k in range(total)] == want["segments"], where
    return at + 7 * total


def test_mosaic_core_under_sanitizers(twin):
    """300 random EDSs and every shape, the donors across one lane and across 64: with one lane a donor is a bit of an alive
    word and donor 64 opens the second word, with 64 lanes the 130 and 300 paths take three and five bits per lane"""
    calls = []
    for eds, seds in random_cases(33, 300):
        if ps.parse(eds, seds)[2]:
            calls += [(eds, seds, None, None, 1), (eds, seds, None, None, 64)]
    for name, (eds, seds, requests) in sorted(mc.shapes().items()):
        for k, kw in enumerate(requests):
            if name == "crowd" and k == 0:
                kw = dict(targets=[2, 299])                      # (all 300 targets: the device test)
            for lanes in (1, 64):
                calls.append((eds, seds, kw.get("targets"), kw.get("donors"), lanes))
    got = run_program(twin, "cases", b"".join(call_record(*c) for c in calls))
    at = 0
    for c in calls:
        at = check_call(got, at, *c)
    assert at == len(got) and len(calls) > 600
