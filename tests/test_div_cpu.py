"""CPU: the diversity specification itself (tests/div_spec.py) on hand-worked examples with the numbers written out and
against the closed forms it does not use; the per-item device code (edsparser_amd/csrc/div_core.hpp) as host code under the
address and undefined-behaviour sanitizers (tests/cpp/test_div_core.cpp, a program of its own); the derived statistics of
edsparser_amd/host/div_stats.hpp bit for bit against the specification's; the C++ shim's test program built against the
public header; and every command line of edsparser-diversity that ends before device work."""
import os
import random
import struct
import subprocess
from fractions import Fraction

import pytest

import div_cases as dc
import div_spec as ds
import ld_cases as lc
import ld_spec as ls
import path_spec as ps
from test_paths_cpu import ROOT
from test_tools_front_cpu import BUILD, HELP, HOST, NO_INPUT, NO_SOURCES, REQUIRED, UNKNOWN, X, _bad, _run

INC = os.path.join(ROOT, "include")
NO_LD_PRELOAD = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


# ---- the specification on hand-worked examples ---------------------------------------------------------------------------
EDS, SEDS = b"{A,C}{G}{T,A,}{C,G}", b"{1,2}{3,4}{0}{1}{2,3}{4}{1,3}{2,4}"


def test_numbers_written_out():
    """choice symbols: {12|34}, {1|23|4}, {13|24}"""
    r = ds.diversity(EDS, SEDS, sfs=True)
    assert r["windows"] == [(0, 3, 0, 3)] and r["groups"] == [[(3, 12)]] and r["pairs"] == [[(13, 18)]] and r["sfs"] == [[0, 1, 3, 0, 0]]
    assert r["info"] == {"groups": 1, "paths": 4, "choice_symbols": 3, "windows": 1, "pairs": 1, "row_words": 1, "extent": 3}
    r = ds.diversity(EDS, SEDS, groups=[[1, 2], [3, 4, 4]], size=1, sfs=True)
    assert r["windows"] == [(0, 1, 0, 1), (1, 2, 1, 2), (2, 3, 2, 3)]
    assert r["pairs"] == [[(0, 1), (4, 4), (0, 1)], [(1, 1), (3, 4), (1, 1)], [(1, 1), (2, 4), (1, 1)]]
    assert r["groups"] == [[(0, 2), (0, 2)], [(1, 2), (1, 2)], [(1, 2), (1, 2)]]
    assert r["sfs"] == [[2, 2, 0], [0, 3, 1]]                    # j >= 1: {34}; {23}, {4}; {24} - by the paths of each group
    # columns: the symbols are 1, 1, 1, 1 wide; windows of 2 columns with a step of 3 leave column 2 (the third symbol) out
    r = ds.diversity(EDS, SEDS, unit="columns", size=2, step=3)
    assert r["info"]["extent"] == 4 and r["windows"] == [(0, 2, 0, 1), (3, 4, 2, 3)] and r["pairs"] == [[(4, 6)], [(4, 6)]]
    # a lone string that names only some paths: present below K, and a group of one path has no pair
    r = ds.diversity(b"{AC}{G,T}", b"{1,2}{1}{2,3}", groups=[[1, 2], [3]])
    assert r["groups"] == [[(1, 4), (0, 1)]] and r["pairs"] == [[(1, 2), (1, 2), (0, 0)]]
    assert ds.ratio(0, 0) is None and "NA" in ds.group_text(r).decode().split("\n")[2]
    assert ds.diversity(b"{ACGT}{GG}{}", b"{0,3}{0}{0,1}")["windows"] == []
    for groups, text in (([[1], [5]], r"Path id 5 out of range \(1..4\)"), ([[1], []], "Group 1 is empty"),
                         ([[2, 3], [1], [3, 2]], "Path id 2 is in groups 0 and 2"), ([[1]] * 17, "17 groups, above the limit of 16")):
        with pytest.raises(ValueError, match=text):
            ds.diversity(EDS, SEDS, groups=groups)
    with pytest.raises(ValueError, match="Diversity has 3 windows, above the limit of 2"):
        ds.diversity(EDS, SEDS, size=1, max_windows=2)


def test_fst_and_tajima_d_against_fractions():
    # F_ST of the two groups over the whole range: pi_0 = 2 / 3, pi_1 = 2 / 3, d_xy = 9 / 12
    r = ds.diversity(EDS, SEDS, groups=[[1, 2], [3, 4]])
    (d0, c0), (dx, cx), (d1, c1) = r["pairs"][0]
    assert (d0, c0, dx, cx, d1, c1) == (2, 3, 9, 12, 2, 3)
    f = ds.fst(ds.ratio(d0, c0), ds.ratio(d1, c1), ds.ratio(dx, cx))
    exact = 1 - (Fraction(2, 3) + Fraction(2, 3)) / 2 / Fraction(9, 12)
    assert exact == Fraction(1, 9) and abs(Fraction(f) - exact) < Fraction(1, 10 ** 15)
    # Tajima's D of all four paths: S = 3, k = 13 / 6, a1 = 11 / 6, a2 = 49 / 36
    r = ds.diversity(EDS, SEDS)
    (seg, present), (diff, comp) = r["groups"][0][0], r["pairs"][0][0]
    d = ds.tajima_d(4, seg, diff, present, 3)
    n, S, a1, a2 = 4, 3, Fraction(11, 6), Fraction(49, 36)
    b1, b2 = Fraction(n + 1, 3 * (n - 1)), Fraction(2 * (n * n + n + 3), 9 * n * (n - 1))
    c1, c2 = b1 - 1 / a1, b2 - Fraction(n + 2) / (a1 * n) + a2 / (a1 * a1)
    var = c1 / a1 * S + c2 / (a1 * a1 + a2) * S * (S - 1)
    num = Fraction(13, 6) - S / a1
    assert var > 0 and abs(Fraction(d) ** 2 - num * num / var) < Fraction(1, 10 ** 12) and (d > 0) == (num > 0)
    assert abs(Fraction(ds.theta_w(seg, 4)) - Fraction(3) / a1) < Fraction(1, 10 ** 15)
    assert ds.tajima_d(4, seg, diff, present - 1, 3) is None and ds.tajima_d(2, 1, 1, 2, 1) is None and ds.theta_w(1, 1) is None
    text = ds.group_text(r).decode().split("\n")
    assert text[0] == ds.GROUP_HEADER[:-1] and text[1] == "0\t3\t3\tall\t4\t3\t12\t13\t18\t0.722222\t1.63636\t%.6g" % d


def test_pair_enumeration_equals_the_closed_forms():
    rng = random.Random(7)
    checked = 0
    for _ in range(150):
        eds, seds = lc.random_eds(rng, rng.randint(2, 8), rng.randint(2, 10))
        syms, sets, P = ps.parse(eds, seds)
        if P < 2:
            continue
        ids = list(range(1, P + 1))
        rng.shuffle(ids)
        cut = sorted(rng.sample(range(1, P), min(P - 1, rng.randint(1, 3))))
        groups = [ids[a:b] for a, b in zip([0] + cut, cut + [P - rng.randint(0, 1)])]
        groups = [g for g in groups if g]
        r = ds.diversity(eds, seds, groups=groups, size=1)
        M = [set(g) for g in groups]
        for w, (_, T, _) in enumerate(ls.carriers(syms, sets, set(range(1, P + 1)))):
            c = [[len(t & m) for t in T] for m in M]
            n = [sum(x) for x in c]
            for g in range(len(M)):
                assert r["groups"][w][g] == (1 if sum(1 for x in c[g] if x) >= 2 else 0, n[g])
                for h in range(g, len(M)):
                    s = sum(a * b for a, b in zip(c[g], c[h]))
                    want = ((n[g] * n[g] - s) // 2, n[g] * (n[g] - 1) // 2) if g == h else (n[g] * n[h] - s, n[g] * n[h])
                    assert r["pairs"][w][ds.pair_index(len(M), g, h)] == want
                    checked += 1
    assert checked > 2000


# ---- the host twin of the device code ------------------------------------------------------------------------------------
def u64s(*v):
    return struct.pack("<%dQ" % len(v), *v)


def build(tmp, name, flags, includes):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g"] + flags + [a for i in includes for a in ("-I", i)] +
                   [os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe], check=True)
    return exe


def run_program(exe, tmp, name, blob):
    cf, rf = str(tmp / (name + ".bin")), str(tmp / (name + ".out"))
    open(cf, "wb").write(blob)
    r = subprocess.run([exe, cf, rf], capture_output=True, text=True, env=NO_LD_PRELOAD)
    assert r.returncode == 0, r.stderr[-6000:]
    data = open(rf, "rb").read()
    return list(struct.unpack("<%dQ" % (len(data) // 8), data))


def core_record(eds, seds, groups, requests):
    syms, sets, P = ps.parse(eds, seds)
    W, WP = P // 64 + 1, (P + 63) // 64
    size = [len(s) for s in syms]
    ent_off = [sum(size[:i]) for i in range(len(syms))]
    cidx = [i for i, s in enumerate(syms) if not (len(s) == 1 and 0 in sets[ent_off[i]])]
    bit_words = [sum(1 << (x - 64 * w) for x in q if 64 * w <= x < 64 * w + 64) for q in sets for w in range(W)]
    width = [max(len(t) for t in s) for s in syms]
    col = [sum(width[:i]) for i in range(len(syms) + 1)]
    M = ds.group_sets(P, groups)
    masks = [(sum(1 << (p - 1) for p in m) >> (64 * w)) & (2 ** 64 - 1) for m in M for w in range(WP)]
    return u64s(len(syms), len(sets), len(cidx), P, W, *size, *ent_off, *cidx, *bit_words, *col, max(col[-1], 1), WP, len(M), *masks, len(requests),
                *[v for unit, size_, step in requests for v in (ds_unit(unit), size_, step)])


def ds_unit(unit):
    return {"symbols": 0, "columns": 1}[unit]


def core_want(eds, seds, groups, requests):
    per_site = ds.diversity(eds, seds, groups=groups, size=1, sfs=True)
    want = []
    for g, p in zip(per_site["groups"], per_site["pairs"]):
        want += [v for x in g for v in x] + [v for x in p for v in x]
    want += [v for s in per_site["sfs"] for v in s] if per_site["windows"] else [0] * sum(k + 1 for k in per_site["K"])
    for unit, size, step in requests:
        r = ds.diversity(eds, seds, groups=groups, unit=unit, size=size, step=step)
        want.append(len(r["windows"]))
        for w, g, p in zip(r["windows"], r["groups"], r["pairs"]):
            want += list(w) + [v for x in g for v in x] + [v for x in p for v in x]
    return want


def test_div_core_under_sanitizers(tmp_path):
    """the walk and the group counts for P on both sides of the word seam, a symbol of 300 strings, the edge symbols, small
    random EDSs; windows of both units below, at and above the extent, overlapping and with gaps"""
    exe = build(tmp_path, "test_div_core", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan"],
                [os.path.join(ROOT, "edsparser_amd", "csrc")])
    rng = random.Random(43)
    windows = [("symbols", 0, 0), ("symbols", 1, 0), ("symbols", 3, 2), ("symbols", 2, 5), ("symbols", 1000, 0), ("columns", 0, 3),
               ("columns", 1, 0), ("columns", 4, 3), ("columns", 3, 7), ("columns", 1000, 1000)]
    runs = []
    for P in (1, 63, 64, 65, 128, 129):
        eds, seds = lc.panel_eds(rng, P, 7, p_missing=0.1 if P > 1 else 0.0, universal="middle")
        runs.append((eds, seds, None, windows))
        if P > 2:
            runs.append((eds, seds, [[P, 1, P], list(range(2, P, 2))], windows[2:5]))
            runs.append((eds, seds, dc.split(P, min(P, 16), leave=1), windows[6:8]))
    many = lc.render([[b"AC"], [b"%c%c%c" % (65 + k % 7, 65 + k // 7 % 7, 65 + k // 49) for k in range(300)], [b"G", b"T"]],
                     [{0}] + [{k + 1} for k in range(300)] + [{1, 2, 200}, {300, 64, 65}])
    runs += [many + (None, windows[:3]), many + ([list(range(1, 100)), list(range(200, 301))], windows[5:7])]
    e, s = dc.edge_symbols_eds()
    runs += [(e, s, g, windows) for g in (None, [[1, 2, 3], [4, 5, 6]], [[6], [1, 2]])]
    runs.append((b"{ACGT}{GG}{}", b"{0,3}{0}{0,1}", [[1], [2, 3]], windows[:2] + windows[5:7]))
    for _ in range(200):
        eds, seds = lc.random_eds(rng, rng.randint(2, 8), rng.randint(2, 10))
        P = ps.parse(eds, seds)[2]
        groups = None if P < 2 or rng.random() < 0.3 else dc.split(P, rng.randint(1, min(P, 4)), leave=rng.randint(0, 1) if P > 4 else 0)
        runs.append((eds, seds, groups, [rng.choice(windows), rng.choice(windows)]))
    got = run_program(exe, tmp_path, "cases", b"".join(core_record(*r) for r in runs))
    at = 0
    for r in runs:
        want = core_want(*r)
        assert got[at:at + len(want)] == want, (r[0][:80], r[2], r[3])
        at += len(want)
    assert at == len(got) > 20000


def test_div_stats_bit_equal_to_the_specification(tmp_path):
    """the tool's arithmetic, built as the tool is built (without contraction), against the same operations in Python"""
    exe = build(tmp_path, "test_div_stats", ["-O2", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                             "-static-libasan"], [os.path.join(ROOT, "edsparser_amd", "host")])
    rng = random.Random(47)
    items = [(4, 3, 13, 18, 12, 3, 2, 3, 9, 12), (1, 0, 0, 0, 5, 5, 0, 0, 0, 0), (2, 1, 1, 1, 2, 1, 0, 1, 0, 4), (3, 0, 0, 3, 3, 1, 1, 3, 0, 0)]
    while len(items) < 3000:
        K = rng.choice([rng.randint(1, 12), rng.randint(2, 3000)])
        sites = rng.randint(1, 2000)
        seg = rng.randint(0, sites)
        comp = sites * (K * (K - 1) // 2) if rng.random() < 0.7 else rng.randint(0, 10 ** 9)
        present = sites * K - (0 if rng.random() < 0.7 else rng.randint(0, K))
        ch, cx = rng.randint(0, 10 ** 9), rng.randint(0, 10 ** 12)
        items.append((K, seg, rng.randint(0, max(comp, 1)), comp, present, sites, rng.randint(0, ch), ch, rng.randint(0, cx), cx))
    got = run_program(exe, tmp_path, "stats", u64s(*[v for it in items for v in it]))
    want, defined = [], [0, 0, 0, 0]
    for K, seg, diff, comp, present, sites, dh, ch, dx, cx in items:
        pi = ds.ratio(diff, comp)
        for k, v in enumerate((pi, ds.theta_w(seg, K), ds.tajima_d(K, seg, diff, present, sites), ds.fst(pi, ds.ratio(dh, ch), ds.ratio(dx, cx)))):
            want += [0, 0] if v is None else [1, bits(v)]
            defined[k] += v is not None
    assert got == want and min(defined) > 1000


def test_div_shim_builds_against_the_public_header(tmp_path):
    """compiled only: running it needs the GPU (tests/test_div_gpu.py)"""
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", INC, "-c", os.path.join(ROOT, "tests", "cpp", "test_div_shim.cpp"),
                    "-o", str(tmp_path / "test_div_shim.o")], check=True)


# ---- the command lines that end before any device work ---------------------------------------------------------------------
TOOL = "edsparser-diversity"
CLI = [REQUIRED, UNKNOWN, NO_INPUT, NO_SOURCES, _bad("unit", "sites"), _bad("window", "x"), _bad("step", "-1"), _bad("max-windows", "1.5"),
       _bad("group", "1,2", "-g"), _bad("group", "=1,2", "-g"), (X + ["-g", "a=1,x"], "Error: the argument ('1,x') for option '--group' is invalid\n"),
       (X + ["-g", "a b=1"], "Error: A group name is empty or holds a tab, blank or line feed\n"),
       (X + ["--groups", "{d}/none.tsv"], "Error: Cannot open groups file: {d}/none.tsv\n"),
       (X + ["--groups", "{d}/ids.txt"], "Error: A line of the groups file is not path<TAB>group: 1\n"),
       (X + ["--groups", "{d}/names.txt", "--names", "{d}/none.txt"], "Error: Cannot open names file: {d}/none.txt\n")]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    subprocess.run(["make", "-s", "-C", HOST], check=True)        # (libedsx.so itself comes from build())
    d = tmp_path_factory.mktemp("div_front")
    eds, seds = dc.edge_symbols_eds()
    (d / "x.eds").write_bytes(eds)
    (d / "x.seds").write_bytes(seds)
    (d / "y.eds").write_bytes(eds)                               # without its sources
    (d / "names.txt").write_text("a\nb\nc\nd\ne\nf\n")
    (d / "ids.txt").write_text("1\n2\n")
    return d


def test_cli_without_device(inputs):
    before = sorted(os.listdir(inputs))
    for args, err in CLI:
        assert _run(TOOL, args, inputs) == (1, "", err.replace("{d}", str(inputs)) + "[Performance]\n"), args
    assert _run(TOOL, ["--help"], inputs) == (0, open(os.path.join(HELP, TOOL + ".txt")).read(), "[Performance]\n")
    assert _run(TOOL, X + ["-h"], inputs)[1:] == _run(TOOL, ["--help"], inputs)[1:]
    assert sorted(os.listdir(inputs)) == before                  # none of these runs writes a file
    assert os.path.exists(os.path.join(BUILD, TOOL))
