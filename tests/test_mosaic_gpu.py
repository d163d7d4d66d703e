"""GPU: edsx_paths_mosaic / edsx_eds_mosaic (k_mosaic_donors and k_mosaic in its COUNT and FILL passes) against the Python
restatement of the specification (tests/mosaic_spec.py) on the shapes of tests/mosaic_cases.py, every number an exact
integer; and by routes that do not use the specification: the shared segments of PathSession.ibs, and the rows of a planted
alignment handed to msa_transform with the `strings` distances on PathSession.slice of a segment's columns.  Then table
batches, limits, errors, timing, the edsparser-mosaic tool and the C++ shim."""
import os
import random
import subprocess

import numpy as np
import pytest

import dist_cases as dc
import ibs_cases as ic
import ibs_spec as isp
import mosaic_cases as mc
import mosaic_spec as msp
import path_spec as ps
from test_paths_cpu import BUILD, HOST, INC, LIBDIR, ROOT

pytestmark = pytest.mark.gpu

SHAPES = mc.shapes()
N = msp.NONE


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    return edsparser_amd.Context(0)


def _error(fn, *a, **kw):
    import edsparser_amd
    with pytest.raises(edsparser_amd.EdsxError) as ei:
        fn(*a, **kw)
    return ei.value.code, ei.value.message


def check(got, eds, seds, kw):
    segs, off, info = got
    want = msp.mosaic(eds, seds, **kw)
    assert segs.dtype.names == msp.FIELDS and off.dtype == np.uint64
    assert off.tolist() == want["target_off"], kw
    assert [tuple(s) for s in segs.tolist()] == want["segments"], kw
    assert {k: info[k] for k in want["info"]} == want["info"], kw
    return info


# ---- the shapes against the specification --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes(ctx, name):
    eds, seds, requests = SHAPES[name]
    C = len(dc.classes(eds, seds, "strings")[0])
    with ctx.paths_open(eds, seds) as s:
        for kw in requests:
            info = check(s.mosaic(**kw), eds, seds, kw)
            assert info["class_columns"] == C
    if name.startswith("columns"):
        assert C == int(name[7:])                                # the shape has the class columns its name claims
    if name == "fixed":
        assert info["choice_symbols"] == 0 and C == 0


def test_one_shot_call_and_the_hand_cases(ctx):
    eds, seds = ic.ENDS
    segs, off, info = ctx.eds_mosaic(eds, seds)
    assert [tuple(s) for s in segs.tolist()] == [(0, 2, 0, 2, 2, 0, 4), (1, N, 0, 0, 1, 0, 1), (1, 0, 1, 1, 0, 1, 3), (1, N, 2, 2, 1, 3, 4),
                                                 (2, 0, 0, 2, 2, 0, 4)]
    assert off.tolist() == [0, 1, 4, 5]
    assert info == {"targets": 3, "donors": 3, "choice_symbols": 2, "class_columns": 4, "segments": 5, "private_segments": 2,
                    "private_symbols": 2, "switches": 2}
    segs, off, info = ctx.eds_mosaic(*ic.FIXED, targets=[1], donors=[1])
    assert [tuple(s) for s in segs.tolist()] == [(0, N, 0, 2, 0, 0, 6)] and off.tolist() == [0, 1] and info["switches"] == 0
    segs, off, info = ctx.eds_mosaic(*ic.NONE)
    assert [tuple(s)[:4] for s in segs[int(off[2]):int(off[3])].tolist()] == [(2, 3, 0, 4), (2, 0, 5, 6)]
    segs, off, info = ctx.eds_mosaic(*mc.TIE, targets=[1], donors=[3, 2, 4])
    assert [tuple(s)[:4] for s in segs.tolist()] == [(0, 0, 0, 0), (0, 2, 1, 2)]
    import edsparser_amd
    assert edsparser_amd.MOSAIC_PRIVATE == N and [f for f, _ in edsparser_amd.MOSAIC_SEGMENT] == list(msp.FIELDS)
    assert _error(ctx.eds_mosaic, eds, None) == (3, "Path spelling needs sources (.seds)")
    assert _error(ctx.eds_mosaic, eds, seds, [4]) == (3, "Path id 4 out of range (1..3)")
    assert _error(ctx.eds_mosaic, eds, seds, [1], [2, 0]) == (3, "Path id 0 out of range (1..3)")


# ---- routes that do not use the specification ----------------------------------------------------------------------------
def test_copied_segments_lie_in_shared_segments_that_nobody_outlasts(ctx):
    """PathSession.ibs with thresholds 0, 0 has every maximal shared interval of every pair: a copied segment [s, e] of target
    t from donor y lies inside one of (t, y) that ends at e, no eligible donor's interval that holds s ends beyond e, nor
    ends there at a smaller position; and a private symbol lies in no interval of the target"""
    rng = random.Random(61)
    copied = private = 0
    for eds, seds in [SHAPES["wide"][:2], dc.EDGE, SHAPES["columns4097"][:2], ic.NONE, ic.GAPS] + [dc.random_eds(rng, 40, 9) for _ in range(5)]:
        P = min(ps.parse(eds, seds)[2], 30)
        req = list(range(1, P + 1))
        with ctx.paths_open(eds, seds) as s:
            segs, off, info = s.mosaic(req, req)
            isegs = s.ibs(req, 0, 0)[0]
        shared = {}
        for x, y, sf, sl in zip(*(isegs[f].tolist() for f in ("x", "y", "symbol_first", "symbol_last"))):
            shared.setdefault((x, y), []).append((sf, sl))
        holding = lambda t, d, i: next((iv for iv in shared.get((min(t, d), max(t, d)), []) if iv[0] <= i <= iv[1]), None)
        for t, y, sf, sl in zip(*(segs[f].tolist() for f in ("target", "donor", "symbol_first", "symbol_last"))):
            others = [d for d in range(P) if d != t]
            if y == N:
                assert not any(holding(t, d, i) for d in others for i in range(sf, sl + 1))
                private += 1
                continue
            iv = holding(t, y, sf)
            assert y != t and iv and iv[1] == sl
            for d in others:
                iv = holding(t, d, sf)
                assert not iv or iv[1] < sl or (iv[1] == sl and d >= y)
            copied += 1
    assert copied > 500 and private > 20


PIECES = ((0, 700, 3), (700, 1536, 1), (1536, 2300, 7), (2300, 3000, 3))


def test_a_planted_recombinant_of_alignment_rows(ctx):
    """rows 0..9 of an alignment are parents, a hundredth of their columns mutated each; row 10 is pieced together from
    parents 3, 1, 7 and 3 again, each seam between columns nobody mutated.  Its mosaic by the parents has at most the planted
    pieces and no private symbol, the donor's row equals the target's over a copied segment's columns, and the slice of
    those columns is an EDS on which target and donor are at `strings` distance 0"""
    rng = random.Random(10)
    cols = PIECES[-1][1]
    nrng = np.random.default_rng(rng.randrange(1 << 30))
    A = np.tile(np.frombuffer(bytes(rng.choice(b"ACGT") for _ in range(cols)), dtype=np.uint8), (11, 1))
    hit = nrng.random((10, cols)) < 0.01
    for c0, _, _ in PIECES[1:]:
        hit[:, c0 - 2:c0 + 2] = False                            # a piece starts between two columns that every row shares
    A[:10][hit] = nrng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(hit.sum()))
    for c0, c1, p in PIECES:
        A[10, c0:c1] = A[p, c0:c1]
    msa = b"".join(b">s%d\n%s\n" % (k, A[k].tobytes()) for k in range(11))
    eds, seds = ctx.msa_transform(msa, 0)
    P = ps.parse(eds, seds)[2]
    assert P == 11
    donors = list(range(1, 11))
    with ctx.paths_open(eds, seds) as s:
        segs, off, info = s.mosaic([11], donors)
        assert off.tolist() == [0, len(segs)] and 2 <= len(segs) <= len(PIECES) and info["private_segments"] == 0
        assert segs["column_first"][0] == 0 and segs["column_end"][-1] == cols and (segs["column_end"][:-1] == segs["column_first"][1:]).all()
        for y, cf, ce in zip(segs["donor"].tolist(), segs["column_first"].tolist(), segs["column_end"].tolist()):
            assert (A[10, cf:ce] == A[donors[y] - 1, cf:ce]).all()
        every = s.mosaic()[0]                                    # each parent by the others and the recombinant
        e, q, reg = s.slice([0] * len(segs), segs["column_first"].tolist(), segs["column_end"].tolist())
    assert len(every) > 11 and (every["target"][1:] >= every["target"][:-1]).all()
    assert not reg["status"].any()
    for k, y in enumerate(segs["donor"].tolist()):
        pe = e[int(reg["eds_off"][k]):int(reg["eds_off"][k] + reg["eds_len"][k])]
        pq = q[int(reg["seds_off"][k]):int(reg["seds_off"][k] + reg["seds_len"][k])]
        D = ctx.eds_distances(pe, pq, None, "strings")[0]
        assert len(D) == P and D[10][donors[y] - 1] == 0


# ---- the session ---------------------------------------------------------------------------------------------------------
def _need(info, K, n_segments):
    """the bytes a call takes: the bit rows of K distinct paths; the donor rows, the alive words, the counts and the row
    numbers; the records"""
    words, T, D = (info["class_columns"] + 63) // 64, info["targets"], info["donors"]
    rows = 8 * K * words
    scratch = 8 * D * words + 8 * T * ((((D + 255) // 256) + 63) // 64) * 256 + 8 * (T + 1) + 8 * (T + D)
    return rows, scratch, 56 * n_segments


def test_forced_table_batches_equal_one_batch(ctx):
    """EDSX_PATHS_BUDGET stands in for the free HBM: choice tables of one and of two of the four distinct paths at a time;
    the rows, the scratch and the few records of the planted recombinant fit it"""
    eds, seds, _ = SHAPES["planted"]
    targets, donors = [4, 4], [3, 2, 1, 2, 5]
    with ctx.paths_open(eds, seds) as s:
        nc = s.info["n_choice_symbols"]
        assert nc > 1000
        want = s.mosaic(targets, donors)
        check(want, eds, seds, dict(targets=targets, donors=donors))
        need = sum(_need(want[2], 5, len(want[0])))
        budgets = (16 * nc + 64, 2 * (16 * nc + 64))
        assert len(want[0]) == 6 and need <= budgets[0]
        try:
            for budget in budgets:
                os.environ["EDSX_PATHS_BUDGET"] = str(budget)
                got = s.mosaic(targets, donors)
                assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and got[2] == want[2], budget
        finally:
            os.environ.pop("EDSX_PATHS_BUDGET", None)


def test_limits_and_errors_leave_the_session_usable(ctx):
    import edsparser_amd
    eds, seds = SHAPES["wide"][:2]
    kw = dict(targets=list(range(1, 11)), donors=list(range(5, 25)))
    with ctx.paths_open(eds, seds) as s:
        info = check(s.mosaic(**kw), eds, seds, kw)
        n = info["segments"]
        assert n > 30
        t = s.timing
        assert t["bytes_written"] == 56 * n + 8 * 11 and t["copy_ms"] > 0 and t["scan_ms"] > 0 and t["choose_ms"] > 0
        with pytest.raises(edsparser_amd.EdsxError) as ei:
            s.mosaic(max_segments=n - 1, **kw)
        assert (ei.value.code, ei.value.message) == (3, "Mosaic has %d segments, above the limit of %d" % (n, n - 1))
        assert ei.value.info == info                             # filled in although the call failed
        assert check(s.mosaic(max_segments=n, **kw), eds, seds, kw) == info
        assert _error(s.mosaic, [1, 0]) == (3, "Path id 0 out of range (1..130)")
        assert _error(s.mosaic, None, [131]) == (3, "Path id 131 out of range (1..130)")
        rows, scratch, records = _need(info, 24, n)
        try:
            os.environ["EDSX_PATHS_BUDGET"] = str(rows + scratch - 1)      # the rows and the scratch are one byte too many
            code, text = _error(s.mosaic, **kw)
            assert code == 4 and "(%d bytes)" % rows in text and "(%d bytes)" % scratch in text and str(rows + scratch - 1) in text
            assert "request fewer paths at a time" in text
            os.environ["EDSX_PATHS_BUDGET"] = str(rows + scratch + records - 1)      # the records are
            code, text = _error(s.mosaic, **kw)
            assert code == 4 and "(%d bytes)" % records in text and "request fewer paths at a time" in text
            os.environ["EDSX_PATHS_BUDGET"] = str(max(rows + scratch + records, 16 * s.info["n_choice_symbols"] + 64))
            check(s.mosaic(**kw), eds, seds, kw)
        finally:
            del os.environ["EDSX_PATHS_BUDGET"]
        check(s.mosaic(**kw), eds, seds, kw)
        assert s.spell([1], 0)[0] == ps.fasta(eds, seds, [1], 0)[0]      # the other calls of the session go on
        req = list(range(1, 8))
        assert s.ibs(req, 0, 0)[2]["segments"] == isp.ibs(eds, seds, req, 0, 0)["info"]["segments"]      # (it shares the rows)


def test_kernels_come_back_by_name(ctx):
    eds, seds = SHAPES["wide"][:2]
    with ctx.paths_open(eds, seds) as s:
        s.mosaic()
        assert not [name for name, *_ in ctx.get_timing() if name.startswith("k_mosaic")]
        ctx.set_timing(True)
        try:
            s.mosaic()
            names = {name: launches for name, _, launches in ctx.get_timing()}
        finally:
            ctx.set_timing(False)
    assert {"k_dist_rows", "k_mosaic_donors", "k_mosaic", "scan_segments"} <= set(names)
    assert names["k_mosaic"] == 2 and names["k_mosaic_donors"] == 1        # the COUNT and the FILL pass


# ---- the tool and the C++ shim ---------------------------------------------------------------------------------------------
CLI = (b"{ACGTAC}{A,ACA,}{CGTTTTT}{,T}{GG}{C,G}{TTTTTTTTTT}{A,C,G}{}", b"{0}{1,3}{2}{4}{0}{1,2}{3,4}{0}{1,2,3}{5,6}{0}{1,5}{2,6}{3}{0}")


def test_edsparser_mosaic_cli(tmp_path):
    subprocess.run(["make", "-s", "-C", HOST], check=True)        # (libedsx.so itself comes from build())
    exe = os.path.join(BUILD, "edsparser-mosaic")
    eds, seds = CLI
    (tmp_path / "x.eds").write_bytes(eds)
    (tmp_path / "x.seds").write_bytes(seds)
    all_names = [b"alpha", b"beta", b"gamma", b"delta", b"epsilon", b"zeta"]
    (tmp_path / "names.txt").write_bytes(b"\n".join(all_names) + b"\n")
    (tmp_path / "bad.txt").write_text("alpha\nbe ta\n")
    base = [exe, "-i", str(tmp_path / "x.eds")]
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "EDS path mosaics" in r.stdout and "Mosaic complete!" in r.stdout and "[Performance] Runtime:" in r.stderr
    want = msp.mosaic(eds, seds)
    assert want["info"]["segments"] >= 10 and want["info"]["private_segments"] >= 1
    assert (tmp_path / "x.mosaic").read_bytes() == msp.text(eds, seds)
    assert len(msp.breakpoints(eds, seds).split(b"\n")) - 2 == want["info"]["switches"] > 3
    runs = [(["--breakpoints"], msp.breakpoints, dict()),
            (["-t", "6,1,3-4,1", "-d", "2-5", "--prefix", "hap"], msp.text, dict(targets=[6, 1, 3, 4, 1], donors=[2, 3, 4, 5], prefix=b"hap")),
            (["--targets", "2", "--donors", "2,2"], msp.text, dict(targets=[2], donors=[2, 2])),
            (["--names", str(tmp_path / "names.txt"), "-t", "4,2", "--breakpoints"], msp.breakpoints, dict(targets=[4, 2], names=all_names)),
            (["--names", str(tmp_path / "names.txt"), "-d", "6,5,1"], msp.text, dict(donors=[6, 5, 1], names=all_names))]
    for k, (args, fn, kw) in enumerate(runs):
        out = tmp_path / ("o%d.txt" % k)
        r = subprocess.run(base + ["-s", str(tmp_path / "x.seds"), "-o", str(out)] + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == fn(eds, seds, **kw), args
    no = tmp_path / "no.txt"
    for args, text in ((["--max-segments", "x"], "for option '--max-segments' is invalid"), (["-t", "7"], "Error: Path id 7 out of range (1..6)"),
                       (["-d", "1,0"], "Error: Path id 0 out of range (1..6)"), (["-d", "1,,2"], "for option '--donors' is invalid"),
                       (["--max-segments", "1"], "segments, above the limit of 1"),
                       (["--names", str(tmp_path / "bad.txt"), "-t", "2", "-d", "1"], "The name of path 2 is empty or holds a tab, blank or line feed"),
                       (["--names", str(tmp_path / "bad.txt"), "-t", "1", "-d", "3"], "The names file has no name for path 3"),
                       (["-s", str(tmp_path / "none.seds")], "Path spelling needs sources (.seds)")):
        r = subprocess.run(base + ["-o", str(no)] + args, capture_output=True, text=True)
        assert r.returncode == 1 and text in r.stderr and "[Performance] Runtime:" in r.stderr and not no.exists(), (args, r.stderr)


def test_path_mosaic_cpp_shim(tmp_path):
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    exe = os.path.join(BUILD, "test_mosaic_shim")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, os.path.join(ROOT, "tests", "cpp", "test_mosaic_shim.cpp"),
                    os.path.join(BUILD, "libedsparser_lib.a"), "-L", LIBDIR, "-ledsx", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    eds, seds = CLI
    cmds = [(b"M", eds, seds, b"-", b"-", b"0"), (b"M", eds, seds, b"6,1,1,2", b"3,3,2,6", b"0"), (b"M", eds, seds, b"1", b"7", b"0"),
            (b"M", eds, seds, b"-", b"-", b"3")]
    (tmp_path / "cmds.txt").write_bytes(b"".join(b"\t".join(c) + b"\n" for c in cmds))
    r = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split(b"\n")[:-1]
    for line, kw in zip(out, (dict(), dict(targets=[6, 1, 1, 2], donors=[3, 3, 2, 6]))):
        w = msp.mosaic(eds, seds, **kw)
        recs = "".join(",".join("%d" % v for v in s) + ";" for s in w["segments"])
        i = w["info"]
        assert w["segments"] and line.decode() == "%s#%s#%d,%d,%d,%d,%d,%d" % (
            recs, ",".join("%d" % v for v in w["target_off"]), i["targets"], i["donors"], i["choice_symbols"], i["private_segments"],
            i["private_symbols"], i["switches"])
    assert out[2] == b"invalid_argument:Path id 7 out of range (1..6)"
    assert out[3].startswith(b"invalid_argument:Mosaic has ") and out[3].endswith(b"segments, above the limit of 3")
