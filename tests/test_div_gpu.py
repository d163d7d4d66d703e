"""GPU: edsx_paths_diversity / edsx_eds_diversity (k_div_sites / k_div_windows and the scans between them) against the
Python restatement of the specification (tests/div_spec.py) on the boundary shapes of the kernels (tests/div_cases.py) and
the fixture sets: every integer equal.  Two routes that do not use the specification: the `strings` distances of a
transformed alignment, and overlapping windows against the sums of disjoint ones.  Then the spectrum against the allele
counts of PathSession.ld, path subsets against edsparser-subset, limits, errors, timing, the tool and the C++ shim."""
import os
import random
import subprocess

import numpy as np
import pytest

import div_cases as dc
import div_spec as ds
import path_spec as ps
from test_paths_cpu import BUILD, HOST, INC, LIBDIR, ROOT, merge_fixture_inputs, vcf_fixture_outputs

pytestmark = pytest.mark.gpu

SHAPES = dc.boundary_shapes()


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    return edsparser_amd.Context(0)


def _error(fn, *a, **kw):
    import edsparser_amd
    with pytest.raises(edsparser_amd.EdsxError) as ei:
        fn(*a, **kw)
    return ei.value.code, ei.value.message, ei.value.info


def check(got, eds, seds, kw):
    windows, groups, pairs, sfs, info = got
    want = ds.diversity(eds, seds, **kw)
    assert windows.dtype.names == ds.WINDOW_FIELDS and groups.dtype.names == ds.GROUP_FIELDS and pairs.dtype.names == ds.PAIR_FIELDS
    assert info == want["info"], kw
    assert [tuple(w) for w in windows.tolist()] == want["windows"], kw
    assert groups.shape == (info["windows"], info["groups"]) and pairs.shape == (info["windows"], info["pairs"])
    assert [[tuple(x) for x in row] for row in groups.tolist()] == want["groups"], kw
    assert [[tuple(x) for x in row] for row in pairs.tolist()] == want["pairs"], kw
    if kw.get("sfs"):
        assert [s.tolist() for s in sfs] == want["sfs"], kw
    else:
        assert sfs is None
    return info, want


# ---- boundary shapes against the specification ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_boundary_shapes(ctx, name):
    eds, seds, requests = SHAPES[name]
    with ctx.paths_open(eds, seds) as s:
        for kw in requests:
            info, want = check(s.diversity(**kw), eds, seds, kw)
    if name == "paths2049":
        assert info["row_words"] == 33
    if name == "paths8200":
        assert info["row_words"] == 129
    if name == "paths64":
        assert info["row_words"] == 1
    if name == "many":
        assert info["choice_symbols"] == 4500
    if name == "edges":                                           # the trailing zero-width symbol lies in the last window
        assert want["windows"][-1][3] == info["choice_symbols"] == 6 and info["extent"] == 47
    if name == "fixed":
        assert info == {"groups": 2, "paths": 3, "choice_symbols": 0, "windows": 0, "pairs": 3, "row_words": 1, "extent": 6}


def test_one_shot_call_and_numbers(ctx):
    eds, seds = b"{A,C}{G}{T,A,}{C,G}", b"{1,2}{3,4}{0}{1}{2,3}{4}{1,3}{2,4}"
    w, g, p, sfs, info = ctx.eds_diversity(eds, seds, sfs=True)
    assert info == {"groups": 1, "paths": 4, "choice_symbols": 3, "windows": 1, "pairs": 1, "row_words": 1, "extent": 3}
    assert w.tolist() == [(0, 3, 0, 3)] and g.tolist() == [[(3, 12)]]
    assert p.tolist() == [[(4 + 5 + 4, 18)]]                     # {12|34}: 4 of 6 pairs differ; {1|23|4}: 5; {13|24}: 4
    assert sfs[0].tolist() == [0, 1, 3, 0, 0]                     # the strings j >= 1 have 2; 2, 1; 2 carriers
    w, g, p, sfs, info = ctx.eds_diversity(eds, seds, groups=[[1, 2], [3, 4, 4]], size=1)
    assert p.tolist() == [[(0, 1), (4, 4), (0, 1)], [(1, 1), (3, 4), (1, 1)], [(1, 1), (2, 4), (1, 1)]] and sfs is None
    check(ctx.eds_diversity(eds, seds, groups=[[4], [1, 2]], unit="columns", size=2, sfs=True), eds, seds,
          dict(groups=[[4], [1, 2]], unit="columns", size=2, sfs=True))
    assert _error(ctx.eds_diversity, eds, None)[:2] == (3, "Path spelling needs sources (.seds)")
    assert _error(ctx.eds_diversity, eds, seds, [[5]])[:2] == (3, "Path id 5 out of range (1..4)")


# ---- two routes that do not use the specification ------------------------------------------------------------------------
def test_whole_range_diff_is_the_sum_of_the_string_distances(ctx):
    rng = np.random.default_rng(23)
    rows, cols = 37, 400
    A = np.full((rows, cols), ord("A"), dtype=np.uint8)
    for c in np.sort(rng.choice(cols, 90, replace=False)):
        A[rng.random(rows) < rng.uniform(0.1, 0.6), c] = ord("C")
        if c % 7 == 0:
            A[rng.random(rows) < 0.2, c] = ord("G")
    msa = b"".join(b">s%d\n%s\n" % (k, A[k].tobytes()) for k in range(rows))
    eds, seds = ctx.msa_transform(msa, 0)
    groups = [list(range(1, 11)), list(range(11, 30)), [30], list(range(31, 38))]
    with ctx.paths_open(eds, seds) as s:
        D, missing, _ = s.distances(metric="strings")
        assert not np.asarray(missing).any()                     # every path has a string at every symbol
        _, _, pairs, _, info = s.diversity(groups=groups)
    D = np.asarray(D).reshape(rows, rows)
    assert info["windows"] == 1 and D.sum() > 1000
    for g in range(4):
        for h in range(g, 4):
            total = int(D[np.ix_([p - 1 for p in groups[g]], [p - 1 for p in groups[h]])].sum())
            assert int(pairs[0, ds.pair_index(4, g, h)]["diff"]) == (total // 2 if g == h else total), (g, h)


def test_overlapping_windows_are_sums_of_disjoint_ones(ctx):
    eds, seds, _ = SHAPES["many"]
    groups = [[1, 2, 3], [4, 5], [6, 7]]
    step = 37
    with ctx.paths_open(eds, seds) as s:
        w1, g1, p1, _, i1 = s.diversity(groups=groups, size=step)
        w3, g3, p3, _, i3 = s.diversity(groups=groups, size=3 * step, step=step)
    assert i1["windows"] == i3["windows"] == (4500 + step - 1) // step
    for field, a, b in (("segregating", g1, g3), ("present", g1, g3), ("diff", p1, p3), ("comp", p1, p3)):
        x = a[field].astype(object)
        padded = np.concatenate([x, np.zeros((2,) + x.shape[1:], dtype=object)])
        assert (b[field].astype(object) == padded[:-2] + padded[1:-1] + padded[2:]).all(), field
    assert p3["diff"].sum() > 1000 and (w3["start"] == w1["start"]).all()


# ---- the spectrum against the allele counts of ld -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["windows", "universal_first", "wide70"])
def test_sfs_of_one_group_is_the_histogram_of_ld_counts_on_complete_sites(ctx, name):
    eds, seds, _ = SHAPES[name]
    with ctx.paths_open(eds, seds) as s:
        _, alleles, li = s.ld(window=1, min_count=0)              # every string j >= 1 of every choice symbol
        *_, sfs, info = s.diversity(sfs=True)
    K = info["paths"]
    want = np.bincount(alleles["count"][alleles["present"] == K].astype(np.int64), minlength=K + 1)
    assert sfs[0].tolist() == want.tolist() and want.sum() > 0


# ---- path subsets and the fixture sets -----------------------------------------------------------------------------------
def test_group_equals_the_whole_of_its_subset(ctx):
    """edsparser-subset keeps the symbols at which the kept paths still have a choice: the whole-range sums of a group are
    those of all paths of the subset wherever subsetting dropped no segregating or incomplete symbol, which holds for sums
    of diff and segregating always (a dropped symbol has neither); comp and present are compared where nc is unchanged"""
    eds, seds, _ = SHAPES["paths129"]
    rng = random.Random(5)
    with ctx.paths_open(eds, seds) as s:
        for _ in range(3):
            keep = sorted(rng.sample(range(1, 130), rng.choice([2, 40, 100])))
            _, g, p, _, info = s.diversity(groups=[keep])
            e2, s2, _ = ctx.eds_subset(eds, seds, keep)
            _, g2, p2, _, info2 = ctx.eds_diversity(e2, s2)
            assert info2["paths"] == len(keep)
            assert int(p[0, 0]["diff"]) == int(p2[0, 0]["diff"]) and int(g[0, 0]["segregating"]) == int(g2[0, 0]["segregating"])
            if info2["choice_symbols"] == info["choice_symbols"]:
                assert p.tolist() == p2.tolist() and g.tolist() == g2.tolist()


@pytest.mark.parametrize("which", ["merge", "vcf"])
def test_fixture_sets(ctx, which):
    ran = differing = 0
    for eds, seds in (merge_fixture_inputs() if which == "merge" else vcf_fixture_outputs()):
        try:
            P = ps.parse(eds, seds)[2]
        except ValueError:                                       # fixtures whose sources do not match their text
            continue
        if P == 0:
            continue
        kw = dict(size=3, step=2, sfs=True) if P < 2 else dict(groups=[list(range(1, P // 2 + 1)), list(range(P // 2 + 1, P + 1))],
                                                               unit="columns", size=16, sfs=True)
        info, want = check(ctx.eds_diversity(eds, seds, **kw), eds, seds, kw)
        differing += sum(d for row in want["pairs"] for d, _ in row)
        ran += 1
    assert ran >= 100 and differing > 100


# ---- the session ---------------------------------------------------------------------------------------------------------
def test_limits_and_errors_leave_the_session_usable(ctx):
    eds, seds, _ = SHAPES["groups16"]
    kw = dict(groups=dc.split(70, 3), size=2, step=1, sfs=True)
    with ctx.paths_open(eds, seds) as s:
        info, _ = check(s.diversity(**kw), eds, seds, kw)
        nw = info["windows"]
        assert nw == 15
        code, text, got = _error(s.diversity, max_windows=nw - 1, **kw)
        assert (code, text) == (3, "Diversity has %d windows, above the limit of %d" % (nw, nw - 1)) and got == info
        assert check(s.diversity(max_windows=nw, **kw), eds, seds, kw)[0] == info
        t = s.timing
        assert t["bytes_written"] == nw * (32 + 3 * 16 + 6 * 16) + 8 * (70 + 3) and t["copy_ms"] > 0 and t["scan_ms"] > 0
        for groups, text in (([[1, 0]], "Path id 0 out of range (1..70)"), ([[3], [71]], "Path id 71 out of range (1..70)"),
                             ([[1], [], [2]], "Group 1 is empty"), ([[5, 9], [7, 5, 9], [9], [5]], "Path id 5 is in groups 0 and 1"),
                             ([[k + 1] for k in range(17)], "Diversity has 17 groups, above the limit of 16")):
            code, got_text, got = _error(s.diversity, groups=groups)
            assert (code, got_text) == (3, text) and got["windows"] == 0
        assert _error(s.diversity, unit=2)[0] == 3
        with pytest.raises(ValueError):
            s.diversity(unit="sites")
        need = 8 * (2 * 3 + 2 * 6) * (info["choice_symbols"] + 1)
        try:
            os.environ["EDSX_PATHS_BUDGET"] = str(need - 1)      # the per-symbol sums alone are one byte too many
            code, text, got = _error(s.diversity, **kw)
            assert code == 4 and "(%d bytes)" % need in text and str(need - 1) in text and got == info
        finally:
            del os.environ["EDSX_PATHS_BUDGET"]
        check(s.diversity(**kw), eds, seds, kw)
        assert s.spell([1], 0)[0] == ps.fasta(eds, seds, [1], 0)[0]      # the other calls of the session go on


def test_kernels_come_back_by_name(ctx):
    eds, seds, _ = SHAPES["groups16"]
    with ctx.paths_open(eds, seds) as s:
        s.diversity()
        assert not [name for name, *_ in ctx.get_timing() if name.startswith("k_div_")]
        ctx.set_timing(True)
        try:
            s.diversity(groups=dc.split(70, 16, leave=6))
            names = {name: launches for name, _, launches in ctx.get_timing()}
        finally:
            ctx.set_timing(False)
    assert {"k_div_sites", "scan_div", "k_div_windows"} <= set(names)
    assert names["k_div_sites"] == 10 and names["k_div_windows"] == 1        # four tiles of four groups: 4 + 6 launches


# ---- the tool and the C++ shim ---------------------------------------------------------------------------------------------
CLI = dc.edge_symbols_eds()


def test_edsparser_diversity_cli(tmp_path):
    subprocess.run(["make", "-s", "-C", HOST], check=True)        # (libedsx.so itself comes from build())
    exe = os.path.join(BUILD, "edsparser-diversity")
    eds, seds = CLI
    (tmp_path / "x.eds").write_bytes(eds)
    (tmp_path / "x.seds").write_bytes(seds)
    base = [exe, "-i", str(tmp_path / "x.eds")]
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "EDS diversity" in r.stdout and "Diversity complete!" in r.stdout and "[Performance] Runtime:" in r.stderr
    assert (tmp_path / "x.div").read_bytes() == ds.group_text(ds.diversity(eds, seds)) and not (tmp_path / "x.div.pairs").exists()
    (tmp_path / "groups.tsv").write_text("1\teast\n2\teast\n5\twest\n6\twest\n4\twest\n")
    runs = [(["-g", "a=1-3", "-g", "b=4,5,6,6", "--window", "2"], dict(groups=[[1, 2, 3], [4, 5, 6]], size=2), ["a", "b"]),
            (["-g", "x=6", "-g", "y=1-2", "-g", "z=3,5", "--unit", "columns", "--window", "8", "--step", "5"],
             dict(groups=[[6], [1, 2], [3, 5]], unit="columns", size=8, step=5), ["x", "y", "z"]),
            (["--groups", str(tmp_path / "groups.tsv")], dict(groups=[[1, 2], [5, 6, 4]]), ["east", "west"]),
            (["--window", "3", "--step", "1"], dict(size=3, step=1), None)]
    for k, (args, kw, names) in enumerate(runs):
        out, sf = tmp_path / ("o%d.txt" % k), tmp_path / ("f%d.txt" % k)
        r = subprocess.run(base + ["-s", str(tmp_path / "x.seds"), "-o", str(out), "--sfs", str(sf)] + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        want = ds.diversity(eds, seds, sfs=True, **kw)
        assert out.read_bytes() == ds.group_text(want, names), args
        assert sf.read_bytes() == ds.sfs_text(want, names), args
        if names:
            assert (tmp_path / ("o%d.txt.pairs" % k)).read_bytes() == ds.pair_text(want, names), args
    no = tmp_path / "no.txt"
    for args, text in ((["-g", "a=7"], "Error: Path id 7 out of range (1..6)"), (["-g", "a=1,2", "-g", "b=2"], "Error: Path id 2 is in groups 0 and 1"),
                       (["--window", "1", "--max-windows", "2"], "Error: Diversity has 6 windows, above the limit of 2"),
                       (["-s", str(tmp_path / "none.seds")], "Path spelling needs sources (.seds)")):
        r = subprocess.run(base + ["-o", str(no)] + args, capture_output=True, text=True)
        assert r.returncode == 1 and text in r.stderr and "[Performance] Runtime:" in r.stderr and not no.exists(), (args, r.stderr)


def test_path_diversity_cpp_shim(tmp_path):
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    exe = os.path.join(BUILD, "test_div_shim")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC,
                    os.path.join(ROOT, "tests", "cpp", "test_div_shim.cpp"), os.path.join(BUILD, "libedsparser_lib.a"), "-L", LIBDIR, "-ledsx",
                    "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    eds, seds = CLI
    cmds = [(b"D", eds, seds, b"-", b"symbols", b"0", b"0"), (b"D", eds, seds, b"1,2,3;4,5,6,6", b"columns", b"8", b"5"),
            (b"D", eds, seds, b"1;7", b"symbols", b"0", b"0"), (b"D", eds, seds, b"1;;2", b"symbols", b"0", b"0")]
    (tmp_path / "cmds.txt").write_bytes(b"".join(b"\t".join(c) + b"\n" for c in cmds))
    r = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split(b"\n")[:-1]
    for line, kw in zip(out, (dict(), dict(groups=[[1, 2, 3], [4, 5, 6, 6]], unit="columns", size=8, step=5))):
        w = ds.diversity(eds, seds, sfs=True, **kw)
        i = w["info"]
        text = "%s#%s#%s#%s#%d,%d,%d,%d,%d" % ("".join("%d,%d,%d,%d;" % x for x in w["windows"]),
                                              "".join("%d,%d;" % x for row in w["groups"] for x in row),
                                              "".join("%d,%d;" % x for row in w["pairs"] for x in row),
                                              "".join("%d," % v for s in w["sfs"] for v in s),
                                              i["groups"], i["paths"], i["choice_symbols"], i["windows"], i["extent"])
        assert line.decode() == text
    assert out[2] == b"invalid_argument:Path id 7 out of range (1..6)"
    assert out[3] == b"invalid_argument:Group 1 is empty"
