"""CPU: the path distance specification itself (tests/dist_spec.py) against the Hamming distances of the alignment rows of
tests/msa_export_spec.py, its metric properties, and its invariance under path subsetting (tests/subset_spec.py); and the
per-descriptor device code (edsparser_amd/csrc/dist_core.hpp) as host code under the address and undefined-behaviour
sanitizers (tests/cpp/test_dist_core.cpp, a program of its own): its class lists against the Python restatement in
tests/dist_cases.py, and V - popcount(R[a] & R[b]) over its bit rows against the specification's matrices."""
import os
import random
import struct
import subprocess

import pytest

import dist_cases as dc
import dist_spec as ds
import msa_export_spec as ms
import path_spec as ps
import subset_spec as sub
from test_paths_cpu import ROOT


def random_cases(seed, count):
    rng = random.Random(seed)
    return [dc.random_eds(rng, rng.randint(1, 8), rng.randint(1, 6)) for _ in range(count)]


def test_columns_are_the_hamming_distances_of_the_alignment_rows():
    """with a gap byte that occurs in no string, "no character" and the gap are the same thing"""
    n = 0
    for eds, seds in random_cases(1, 300) + [dc.EDGE]:
        gap = next(bytes([g]) for g in b".*#+" if bytes([g]) not in eds)
        rows = [r for _, r in ms.rows_of(ms.align(eds, seds, None, 0, gap=gap)[0])]
        D, miss, units = ds.matrix(eds, seds, None, "columns")
        assert units == ms.info(eds, seds)["n_columns"] and miss == ms.align(eds, seds, None, 0, gap=gap)[1]
        assert D == [[sum(x != y for x, y in zip(a, b)) for b in rows] for a in rows]
        n += len(rows)
    assert n > 900


def test_metric_properties():
    pairs = apart = 0
    for eds, seds in random_cases(2, 300):
        Dc, Ds = ds.matrix(eds, seds, None, "columns")[0], ds.matrix(eds, seds, None, "strings")[0]
        K = len(Dc)
        for D in (Dc, Ds):
            for a in range(K):
                assert D[a][a] == 0
                for b in range(K):
                    assert D[a][b] == D[b][a]
                    for c in range(K):
                        assert D[a][c] <= D[a][b] + D[b][c]
        for a in range(K):
            for b in range(K):
                pairs += 1
                apart += Ds[a][b] > 0
                if Ds[a][b] == 0:
                    assert Dc[a][b] == 0
    assert pairs > 3000 and 0.3 * pairs < apart


def test_request_order_and_duplicates():
    eds, seds = dc.EDGE
    for metric in ds.METRICS:
        full = ds.matrix(eds, seds, None, metric)
        req = [66, 4, 4, 1, 65]
        D, miss, units = ds.matrix(eds, seds, req, metric)
        assert units == full[2] and miss == [full[1][p - 1] for p in req]
        assert D == [[full[0][a - 1][b - 1] for b in req] for a in req]
    with pytest.raises(ValueError, match=r"Path id 68 out of range \(1..67\)"):
        ds.matrix(eds, seds, [1, 68])


def test_subset_invariance():
    """the matrix of the subset to Q is rows and columns Q of the matrix of the whole, under both metrics"""
    rng = random.Random(3)
    ran = 0
    for eds, seds in random_cases(4, 300):
        P = ps.parse(eds, seds)[2]
        if P == 0:
            continue
        Q = sorted(rng.sample(range(1, P + 1), rng.randint(1, P)))
        e2, s2, _ = sub.subset(eds, seds, Q)
        for metric in ds.METRICS:
            full = ds.matrix(eds, seds, None, metric)[0]
            if ps.parse(e2, s2)[2] == 0:                         # every kept symbol became common: one sequence
                assert all(full[a - 1][b - 1] == 0 for a in Q for b in Q)
                continue
            part = ds.matrix(e2, s2, None, metric)[0]
            assert len(part) <= len(Q)                           # (the last kept paths may appear in no set any more)
            assert all(part[x][y] == full[Q[x] - 1][Q[y] - 1] for x in range(len(part)) for y in range(len(part)))
            ran += 1
    assert ran > 400


def test_text_formats():
    eds, seds = b"{AC}{G,T}{A,}", b"{0}{1}{2,3}{1,2}{3}"
    assert ds.matrix(eds, seds)[0] == [[0, 1, 2], [1, 0, 1], [2, 1, 0]]
    assert ds.text(eds, seds) == b"path\ts0\ts1\ts2\ns0\t0\t1\t2\ns1\t1\t0\t1\ns2\t2\t1\t0\n"
    assert ds.text(eds, seds, [3, 1], fmt="phylip", normalize=True, names=[b"x", b"y"]) == b"2\nx 0.000000 0.500000\ny 0.500000 0.000000\n"
    assert ds.text(eds, seds, [2], metric="strings", prefix=b"hap") == b"path\thap1\nhap1\t0\n"


# ---- the host twin -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    d = tmp_path_factory.mktemp("dist_core")
    exe = str(d / "test_dist_core")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-I", os.path.join(ROOT, "edsparser_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_dist_core.cpp"), "-o", exe], check=True)
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


def eds_record(eds, seds):
    """record kind 0 of tests/cpp/test_dist_core.cpp: the tables of the session as the device holds them"""
    syms, sets, P = ps.parse(eds, seds)
    W = P // 64 + 1
    size = [len(s) for s in syms]
    ent_off = [sum(size[:i]) for i in range(len(syms))]
    strings = [t for s in syms for t in s]
    str_off = [0]
    for t in strings:
        str_off.append(str_off[-1] + len(t))
    chars = b"".join(strings)
    cidx = [i for i, s in enumerate(syms) if not (len(s) == 1 and 0 in sets[ent_off[i]])]
    bits = [sum(1 << (x - 64 * w) for x in q if 64 * w <= x < 64 * w + 64) for q in sets for w in range(W)]
    return (u64s(0, len(syms), len(strings), len(cidx), P, W, len(chars), *size, *ent_off, *str_off) +
            chars + b"\0" * (-len(chars) % 8) + u64s(*cidx, *bits))


def check_eds_result(got, at, eds, seds):
    """the twin's answer for one EDS record from got[at:] -> the next position"""
    syms, sets, P = ps.parse(eds, seds)
    choice = [i for i, s in enumerate(syms) if not (len(s) == 1 and 0 in sets[sum(len(x) for x in syms[:i])])]
    nc = len(choice)
    widths = [max(len(t) for t in syms[i]) for i in choice]
    at += nc                                                     # may_miss: through the class lists below
    assert got[at:at + nc + 1] == [sum(widths[:k]) for k in range(nc + 1)]
    at += nc + 1
    for metric in ds.METRICS:
        want, V = dc.classes(eds, seds, metric)
        C = len(want)
        assert got[at:at + 2] == [V, C], (eds, seds, metric)
        shift = 9 if metric == "columns" else 24
        assert got[at + 2:at + 2 + C] == [u << shift | v for u, v in want], (eds, seds, metric)
        at += 2 + C
        words = (C + 63) // 64
        rows = [sum(got[at + p * words + w] << (64 * w) for w in range(words)) for p in range(P)]
        at += P * words
        D = ds.matrix(eds, seds, None, metric)[0] if P else []
        for a in range(P):
            assert bin(rows[a]).count("1") == V and rows[a] >> C == 0     # one class per listed unit, zero padding
            assert [V - bin(rows[a] & rows[b]).count("1") for b in range(P)] == D[a], (eds, seds, metric, a)
    return at


def test_dist_core_under_sanitizers(twin):
    """every descriptor and every bit row of small EDSs, of the boundary shapes, of bytes from 0x80 on and of a symbol with
    300 strings"""
    rng = random.Random(11)
    many = dc.render([[b"AC"], [b"%c%c%c" % (65 + k % 7, 65 + k // 7 % 7, 65 + k // 49) for k in range(300)], [b"\xfe", b"\x80\x81"]],
                     [{0}] + [{k + 1} for k in range(300)] + [{1, 2}, {300}])
    texts = random_cases(12, 300) + [dc.random_eds(rng, 6, 70, bytes(range(0x80, 0x100))) for _ in range(20)] + [many]
    texts += [(e, s) for name, (e, s, _) in dc.boundary_shapes().items() if name in ("wide", "fixed", "edge", "columns65")]
    got = run_twin(twin, "cases", b"".join(eds_record(e, s) for e, s in texts))
    at = 0
    for eds, seds in texts:
        at = check_eds_result(got, at, eds, seds)
    assert at == len(got) > 20000


def test_dist_core_numbers_on_both_sides_of_32_bits(twin):
    """descriptors, the symbol search and the launch geometry are numbers: offsets and ranks on both sides of 2^32"""
    T = 2 ** 32
    entries = [(0, 0, 0, 0), (T - 1, 255, T - 1, 1), (T, 256, T, dc.NOSTRING), (T + 1, 0x80, T + 7, dc.NOSTRING - 1),
               (2 ** 55 - 1, 256, 2 ** 40 - 1, 12345), (5 * T + 3, 0xff, 3 * T, 0)]
    blob = u64s(1, len(entries), *[v for e in entries for v in e])
    want = []
    for unit, value, r, index in entries:
        want += [unit << 9 | value, unit, value, r << 24 | index, r, index]
    # symbols of widths 3, 0, T - 3, 0, 0, 5, 2 T: units around every edge
    widths = [3, 0, T - 3, 0, 0, 5, 2 * T]
    ccol = [sum(widths[:k]) for k in range(len(widths) + 1)]
    units = [0, 2, 3, T - 1, T, T + 4, T + 5, 2 * T, 3 * T + 4]
    blob += u64s(2, len(widths), *ccol, len(units), *units)
    want += [max(k for k in range(len(widths)) if ccol[k] <= u) for u in units]
    assert want[-len(units):] == [0, 0, 2, 2, 5, 5, 6, 6, 6]
    # geometry: K = 129 has 3 tiles and 6 tile pairs; chunks of 4096 columns until there would be more than 8192 workgroups
    for K, C in ((129, 4097), (64, 4096 * 8192), (64, 4096 * 8192 + 1), (100000, 10 ** 7), (1, 0), (1000, 2 * T)):
        tiles = (K + 63) // 64
        tp = tiles * (tiles + 1) // 2
        words = (C + 63) // 64
        most = max(1, 8192 // tp)
        cw = 64 if (words + 63) // 64 <= most else ((words + most - 1) // most + 63) // 64 * 64
        pairs = [(r, c) for r in range(tiles) for c in range(r, tiles)]
        ask = sorted(set([0, tp - 1, tp // 2, min(tiles, tp - 1)]))
        blob += u64s(3, K, C, len(ask), *ask)
        want += [tiles, tp, words, cw, (words + cw - 1) // cw] + [v for q in ask for v in (pairs[q] if tiles < 100 else tile_pair(tiles, q))]
        assert ((words + cw - 1) // cw) * tp <= max(8192, tp)
    present = [0, 1, 63, 64, 65, 127, 128, 200, 255]
    blob += u64s(4, len(present), *present)
    want += [len(present)] + [v for b in range(256) for v in (int(b in present), sum(1 for x in present if x < b))]
    assert run_twin(twin, "numbers", blob) == want


def tile_pair(tiles, q):
    r = 0
    while q >= tiles - r:
        q -= tiles - r
        r += 1
    return r, r + q
