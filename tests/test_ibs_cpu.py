"""CPU: the shared-segment specification itself (tests/ibs_spec.py) against properties that follow from its definition and
against the `strings` distances of tests/dist_spec.py; and the per-item device code (edsparser_amd/csrc/ibs_core.hpp) as
host code under the address and undefined-behaviour sanitizers (tests/cpp/test_ibs_core.cpp, a program of its own, nothing
preloaded): the scan and the stitch emulated chunk by chunk, every segment list and pair_off against the specification."""
import os
import random
import subprocess

import pytest

import dist_cases as dc
import dist_spec as ds
import ibs_cases as ic
import ibs_spec as isp
import path_spec as ps
from test_dist_cpu import eds_record, random_cases, u64s
from test_dist_cpu import run_twin as run_program
from test_paths_cpu import ROOT


# ---- the specification ---------------------------------------------------------------------------------------------------
def test_segments_tile_the_agreeing_symbols():
    """with thresholds 0, 0 the segments of a pair are disjoint, ascending and not adjacent, the symbols outside them are
    exactly those where the pair differs, and their sites add up to the choice symbols less the `strings` distance"""
    pairs = 0
    for eds, seds in random_cases(21, 300) + [dc.EDGE, ic.GAPS, ic.NONE]:
        syms, sets, P = ps.parse(eds, seds)
        if P == 0:
            continue
        got = isp.ibs(eds, seds, None, 0, 0)
        D = ds.matrix(eds, seds, None, "strings")[0]
        off, n = got["pair_off"], len(syms)
        assert len(off) == P * (P - 1) // 2 + 1 and off[0] == 0 and off[-1] == len(got["segments"]) == got["info"]["segments"]
        q = 0
        for x in range(P):
            for y in range(x + 1, P):
                segs = got["segments"][off[q]:off[q + 1]]
                q += 1
                pairs += 1
                assert all(s[:2] == (x, y) and s[2] <= s[3] for s in segs)
                assert all(a[3] + 1 < b[2] for a, b in zip(segs, segs[1:]))
                inside = sum(s[3] - s[2] + 1 for s in segs)
                assert n - inside == D[x][y]
                assert sum(s[4] for s in segs) == got["info"]["choice_symbols"] - D[x][y]
    assert pairs > 1000


def test_thresholds_select_and_order_is_kept():
    eds, seds = ic.GAPS
    every = isp.ibs(eds, seds, None, 0, 0)["segments"]
    assert every == sorted(every) and {s[4] for s in every} >= {0, 1}
    for ms, mc in ((1, 0), (0, 1), (2, 2), (0, 3), (9, 0)):
        assert isp.ibs(eds, seds, None, ms, mc)["segments"] == [s for s in every if s[4] >= ms and s[6] - s[5] >= mc]
    assert isp.ibs(eds, seds, None, 0, 0)["info"]["candidate_segments"] == isp.ibs(eds, seds, None, 5, 5)["info"]["candidate_segments"] == len(every)


def test_by_hand():
    eds, seds = ic.ENDS
    assert isp.ibs(eds, seds, None, 0, 0)["segments"] == [(0, 1, 1, 1, 0, 1, 3), (0, 2, 0, 2, 2, 0, 4), (1, 2, 1, 1, 0, 1, 3)]
    assert isp.ibs(eds, seds)["segments"] == [(0, 2, 0, 2, 2, 0, 4)] and isp.ibs(eds, seds)["pair_off"] == [0, 0, 1, 1]
    assert isp.ibs(*ic.ADJACENT, None, 0, 0) == {"segments": [], "pair_off": [0, 0],
                                                 "info": {"paths": 2, "choice_symbols": 2, "pairs": 1, "candidate_segments": 0, "segments": 0}}
    assert isp.ibs(*ic.FIXED, None, 0, 0)["segments"] == [(0, 1, 0, 2, 0, 0, 6), (0, 2, 0, 2, 0, 0, 6), (1, 2, 0, 2, 0, 0, 6)]
    assert isp.ibs(*ic.FIXED)["segments"] == [] and isp.ibs(*ic.FIXED, [2])["pair_off"] == [0]
    none = isp.ibs(*ic.NONE, None, 0, 0)["segments"]
    assert [s[2:4] for s in none if s[:2] == (2, 3)] == [(0, 4), (6, 6)]      # both without a string at symbol 1: they agree
    assert [s[2:4] for s in none if s[:2] == (0, 2)] == [(0, 0), (2, 6)]      # one has a string, the other none
    assert isp.text(eds, seds, [3, 1], names=[b"c", b"a"]) == isp.HEADER + b"c\ta\t0\t2\t2\t0\t4\t4\n"
    assert isp.text(eds, seds, prefix=b"hap") == isp.HEADER + b"hap0\thap2\t0\t2\t2\t0\t4\t4\n"
    with pytest.raises(ValueError, match=r"Path id 4 out of range \(1..3\)"):
        isp.ibs(eds, seds, [1, 4])


def test_request_order_and_duplicates():
    eds, seds = dc.EDGE
    req = [66, 4, 4, 1, 65]
    got = isp.ibs(eds, seds, req, 0, 0)
    q = 0
    for x in range(5):
        for y in range(x + 1, 5):
            mine = [s[2:] for s in got["segments"][got["pair_off"][q]:got["pair_off"][q + 1]]]
            assert mine == [s[2:] for s in isp.ibs(eds, seds, [req[x], req[y]], 0, 0)["segments"]]
            q += 1
    assert [s[2:4] for s in got["segments"] if s[:2] == (1, 2)] == [(0, len(ps.parse(eds, seds)[0]) - 1)]


def test_boundary_shapes_are_what_they_claim():
    shapes = ic.boundary_shapes()
    for c in (63, 64, 65, 4095, 4096, 4097):
        eds, seds, _ = shapes["columns%d" % c]
        desc, _ = dc.classes(eds, seds, "strings")
        assert len(desc) == c
        for seam in range(64, c, 64):                            # one symbol's columns on both sides of every word seam
            assert desc[seam - 1][0] == desc[seam][0]
        if c < 65:
            continue
        rank = desc[63][0]                                       # and there the paths 1 and 3 differ, 1 and 2 do not
        every = isp.ibs(eds, seds, [1, 3, 2], 0, 0)["segments"]
        choice = [i for i, f in enumerate(isp.layout(*ps.parse(eds, seds)[:2])[0]) if f]
        assert not any(s[2] <= choice[rank] <= s[3] for s in every if s[:2] == (0, 1))
        assert any(s[2] <= choice[rank] <= s[3] for s in every if s[:2] == (0, 2))
    assert ps.parse(*shapes["wide"][:2])[2] == 130


# ---- the host twin -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    d = tmp_path_factory.mktemp("ibs_core")
    exe = str(d / "test_ibs_core")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-I", os.path.join(ROOT, "edsparser_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_ibs_core.cpp"), "-o", exe], check=True)
    return exe, d


def call_record(eds, seds, paths, min_sites, min_columns, chunk_words):
    P = ps.parse(eds, seds)[2]
    ids = list(paths) if paths else list(range(1, P + 1))
    return eds_record(eds, seds) + u64s(len(ids), *ids, min_sites, min_columns, chunk_words)


def check_call(got, at, eds, seds, paths, min_sites, min_columns, chunk_words):
    want = isp.ibs(eds, seds, paths, min_sites, min_columns)
    C = len(dc.classes(eds, seds, "strings")[0])
    words, npairs, total = (C + 63) // 64, want["info"]["pairs"], want["info"]["segments"]
    chunks = (words + chunk_words - 1) // chunk_words if chunk_words else (words + 63) // 64
    where = (eds[:80], seds[:80], paths, min_sites, min_columns, chunk_words)
    assert got[at:at + 4] == [C, chunks, want["info"]["candidate_segments"], total], where
    at += 4
    assert got[at:at + npairs + 1] == want["pair_off"], where
    at += npairs + 1
    assert [tuple(got[at + 7 * k:at + 7 * k + 7]) for k in range(total)] == want["segments"], where
    return at + 7 * total


def test_ibs_core_under_sanitizers(twin):
    """300 random EDSs, larger ones cut into chunks of one and of two words, and the boundary shapes with the geometry of the
    device and with one word per chunk, so that every word seam is a chunk seam as well"""
    rng = random.Random(31)
    calls = []
    for eds, seds in random_cases(32, 300):
        if ps.parse(eds, seds)[2]:
            calls.append((eds, seds, None, rng.choice([0, 0, 1]), rng.choice([0, 0, 2]), 0))
    for _ in range(30):
        eds, seds = dc.random_eds(rng, 70, 6)
        calls.append((eds, seds, None, rng.choice([0, 1]), 0, rng.choice([1, 2])))
    calls.append((*dc.EDGE, [3, 1, 1, 66, 2], 0, 0, 1))
    for name, (eds, seds, requests) in sorted(ic.boundary_shapes().items()):
        for kw in requests:
            if name == "wide" and len(kw.get("paths", [])) not in (65, 6, 2, 1):
                continue                                         # (the twin walks 64 x 64 lanes per tile: a few requests do)
            for cw in ((0, 1) if name.startswith("columns") else (0,)):
                calls.append((eds, seds, kw.get("paths"), kw.get("min_sites", 1), kw.get("min_columns", 0), cw))
    got = run_program(twin, "cases", b"".join(call_record(*c) for c in calls))
    at = 0
    for c in calls:
        at = check_call(got, at, *c)
    assert at == len(got) and len(calls) > 350


def test_pair_index_on_both_sides_of_32_bits(twin):
    T = 2 ** 32
    asks = [(2, 0, 1), (3, 0, 2), (3, 1, 2), (130, 64, 65), (130, 128, 129), (T, 0, T - 1), (T, 1, 2), (T + 5, T, T + 4), (T + 6, T + 1, T + 3)]
    want = []
    for K, x, y in asks:
        want += [x * (2 * K - x - 1) // 2 + (y - x - 1), K * (K - 1) // 2]
    assert want[:6] == [0, 1, 1, 3, 2, 3]
    got = run_program(twin, "numbers", u64s(1, len(asks), *[v for a in asks for v in a]))
    assert got == want
    K = 7                                                        # row-major over the upper triangle
    assert [x * (2 * K - x - 1) // 2 + (y - x - 1) for x in range(K) for y in range(x + 1, K)] == list(range(21))
