"""GPU: edsx_paths_ibs / edsx_eds_ibs (k_ibs_scan and k_ibs_stitch in their COUNT and FILL passes) against the Python
restatement of the specification (tests/ibs_spec.py) on the boundary shapes of the kernels (tests/ibs_cases.py) and the
fixture sets, every number an exact integer; and by routes that do not use the specification: the `strings` distances of
PathSession.distances, the rows of an alignment handed to msa_transform, and the distances on PathSession.slice of a
segment's columns.  Then table batches, limits, errors, timing, the edsparser-ibs tool and the C++ shim."""
import os
import random
import subprocess

import numpy as np
import pytest

import dist_cases as dc
import dist_spec as ds
import ibs_cases as ic
import ibs_spec as isp
import path_spec as ps
from test_paths_cpu import BUILD, HOST, INC, LIBDIR, ROOT, merge_fixture_inputs, vcf_fixture_outputs

pytestmark = pytest.mark.gpu

SHAPES = ic.boundary_shapes()


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
    want = isp.ibs(eds, seds, **kw)
    assert segs.dtype.names == isp.FIELDS and off.dtype == np.uint64
    assert off.tolist() == want["pair_off"], kw
    assert [tuple(s) for s in segs.tolist()] == want["segments"], kw
    assert {k: info[k] for k in want["info"]} == want["info"], kw
    return info


# ---- boundary shapes against the specification ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_boundary_shapes(ctx, name):
    eds, seds, requests = SHAPES[name]
    C = len(dc.classes(eds, seds, "strings")[0])
    with ctx.paths_open(eds, seds) as s:
        for kw in requests:
            info = check(s.ibs(**kw), eds, seds, kw)
            if info["pairs"]:
                assert info["class_columns"] == C and info["chunk_columns"] == ic.CHUNK_COLUMNS
                assert info["chunks"] == ((C + 63) // 64 + 63) // 64
    if name.startswith("columns"):
        assert C == int(name[7:])                                # the shape has the class columns its name claims
    if name == "columns4097":
        assert info["chunks"] == 2
    if name == "fixed":
        assert info["choice_symbols"] == 0 and info["chunks"] == 0


def test_one_shot_call_and_numbers(ctx):
    eds, seds = ic.ENDS
    segs, off, info = ctx.eds_ibs(eds, seds, min_sites=0)
    assert [tuple(s) for s in segs.tolist()] == [(0, 1, 1, 1, 0, 1, 3), (0, 2, 0, 2, 2, 0, 4), (1, 2, 1, 1, 0, 1, 3)]
    assert off.tolist() == [0, 1, 2, 3]
    assert info == {"paths": 3, "choice_symbols": 2, "class_columns": 4, "chunk_columns": 4096, "chunks": 1, "pairs": 3,
                    "candidate_segments": 3, "segments": 3}
    segs, off, info = ctx.eds_ibs(eds, seds, [3, 1])
    assert [tuple(s) for s in segs.tolist()] == [(0, 1, 0, 2, 2, 0, 4)] and off.tolist() == [0, 1]
    segs, off, info = ctx.eds_ibs(eds, seds, [2])
    assert len(segs) == 0 and off.tolist() == [0] and info["pairs"] == 0
    assert _error(ctx.eds_ibs, eds, None) == (3, "Path spelling needs sources (.seds)")
    assert _error(ctx.eds_ibs, eds, seds, [4]) == (3, "Path id 4 out of range (1..3)")


@pytest.mark.parametrize("which", ["merge", "vcf"])
def test_fixture_sets(ctx, which):
    ran = reported = 0
    for eds, seds in (merge_fixture_inputs() if which == "merge" else vcf_fixture_outputs()):
        try:
            P = ps.parse(eds, seds)[2]
        except ValueError:                                       # fixtures whose sources do not match their text
            continue
        if P == 0:
            continue
        reported += check(ctx.eds_ibs(eds, seds, **ic.EVERY), eds, seds, ic.EVERY)["segments"]
        ran += 1
    assert ran >= 100 and reported > 100


# ---- routes that do not use the specification ----------------------------------------------------------------------------
def test_sites_add_up_to_the_choice_symbols_less_the_strings_distance(ctx):
    rng = random.Random(51)
    for eds, seds in [SHAPES["wide"][:2], dc.EDGE, SHAPES["columns4097"][:2]] + [dc.random_eds(rng, 40, 9) for _ in range(5)]:
        with ctx.paths_open(eds, seds) as s:
            segs, off, info = s.ibs(**ic.EVERY)
            D = s.distances(None, "strings")[0]
            nc, K = s.info["n_choice_symbols"], len(D)
        sums = np.add.reduceat(np.append(segs["sites"], 0), off[:-1].astype(np.int64))
        sums[off[:-1] == off[1:]] = 0                            # (reduceat gives the next entry for an empty pair)
        iu = np.triu_indices(K, 1)
        assert len(off) == K * (K - 1) // 2 + 1 and (sums == nc - D[iu]).all()


def _alignment(rng, rows, cols):
    base = np.frombuffer(bytes(rng.choice(b"ACGT") for _ in range(cols)), dtype=np.uint8)
    nrng = np.random.default_rng(rng.randrange(1 << 30))
    A = np.tile(base, (rows, 1))
    hit = nrng.random((rows, cols)) < 0.01
    A[hit] = nrng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(hit.sum()))
    return A, b"".join(b">s%d\n%s\n" % (k, A[k].tobytes()) for k in range(rows))


def test_segments_of_a_transformed_alignment_are_where_its_rows_are_equal(ctx):
    """rows x and y are equal on [column_first, column_end) and differ in the symbol before and in the symbol behind; and
    the slice of a segment's columns is an EDS on which the two paths are at distance 0 under both metrics"""
    A, msa = _alignment(random.Random(9), 40, 3000)
    eds, seds = ctx.msa_transform(msa, 0)
    syms, sets, P = ps.parse(eds, seds)
    col = isp.layout(syms, sets)[1]
    assert P == 40 and col[-1] == 3000
    with ctx.paths_open(eds, seds) as s:
        segs, off, info = s.ibs(**ic.EVERY)
        assert info["segments"] == len(segs) > 2000
        inner = 0
        for x, y, sf, sl, sites, cf, ce in segs.tolist():
            assert (cf, ce) == (col[sf], col[sl + 1]) and (A[x, cf:ce] == A[y, cf:ce]).all()
            if sf > 0:
                assert (A[x, col[sf - 1]:cf] != A[y, col[sf - 1]:cf]).any()
            if sl + 1 < len(syms):
                assert (A[x, ce:col[sl + 2]] != A[y, ce:col[sl + 2]]).any()
            inner += sf > 0 and sl + 1 < len(syms)
        assert inner > 1000
        pick = segs[np.argsort(segs["sites"])[-6:]]
        assert pick["sites"].min() > 0
        e, q, reg = s.slice([0] * len(pick), pick["column_first"].tolist(), pick["column_end"].tolist())
    assert not reg["status"].any()
    for k, (x, y) in enumerate(zip(pick["x"].tolist(), pick["y"].tolist())):
        pe = e[int(reg["eds_off"][k]):int(reg["eds_off"][k] + reg["eds_len"][k])]
        pq = q[int(reg["seds_off"][k]):int(reg["seds_off"][k] + reg["seds_len"][k])]
        for metric in ("columns", "strings"):
            D = ctx.eds_distances(pe, pq, None, metric)[0]
            assert len(D) == P and D[x][y] == 0


# ---- the session ---------------------------------------------------------------------------------------------------------
def test_forced_table_batches_equal_one_batch(ctx):
    """EDSX_PATHS_BUDGET stands in for the free HBM: choice tables of one and of two paths; the rows, the scratch and the
    records fit it"""
    eds, seds, _ = ctx.genrandomeds(400_000, seed=11)
    req = [4, 1, 2, 3, 3, 1, 2]
    with ctx.paths_open(eds, seds) as s:
        nc = s.info["n_choice_symbols"]
        assert nc > 1000
        every = s.ibs(req, 0, 0)[0]
        t = int(np.sort(every["sites"])[-100]) + 1               # a threshold that leaves fewer than a hundred records
        want = s.ibs(req, t, 0)
        assert 0 < len(want[0]) < 100 and (want[0] == every[every["sites"] >= t]).all()
        info = want[2]
        words, pairs = (info["class_columns"] + 63) // 64, 21
        need = 8 * len(req) * words + pairs * (32 * info["chunks"] + 8) + 8 + 8 * (pairs + 1) + 56 * len(want[0])
        try:
            for budget in (16 * nc + 64, 2 * (16 * nc + 64)):
                assert need <= budget
                os.environ["EDSX_PATHS_BUDGET"] = str(budget)
                got = s.ibs(req, t, 0)
                assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and got[2] == info, budget
        finally:
            del os.environ["EDSX_PATHS_BUDGET"]


def test_limits_and_errors_leave_the_session_usable(ctx):
    import edsparser_amd
    eds, seds = SHAPES["wide"][:2]
    req = list(range(1, 11))
    kw = dict(paths=req, min_sites=0)
    with ctx.paths_open(eds, seds) as s:
        info = check(s.ibs(**kw), eds, seds, kw)
        n = info["segments"]
        assert n > 100
        t = s.timing
        assert t["bytes_written"] == 56 * n + 8 * 46 and t["copy_ms"] > 0 and t["scan_ms"] > 0 and t["choose_ms"] > 0
        with pytest.raises(edsparser_amd.EdsxError) as ei:
            s.ibs(max_segments=n - 1, **kw)
        assert (ei.value.code, ei.value.message) == (3, "IBS has %d segments, above the limit of %d" % (n, n - 1))
        assert ei.value.info == info                             # filled in although the call failed
        assert check(s.ibs(max_segments=n, **kw), eds, seds, kw) == info
        assert _error(s.ibs, [1, 0]) == (3, "Path id 0 out of range (1..130)")
        assert _error(s.ibs, [131]) == (3, "Path id 131 out of range (1..130)")
        words = (info["class_columns"] + 63) // 64
        rows, scratch = 8 * 10 * words, 45 * (32 * info["chunks"] + 8) + 8 + 8 * 46
        try:
            os.environ["EDSX_PATHS_BUDGET"] = str(rows + scratch - 1)      # the rows and the scratch are one byte too many
            code, text = _error(s.ibs, **kw)
            assert code == 4 and "(%d bytes)" % rows in text and "(%d bytes)" % scratch in text and str(rows + scratch - 1) in text
            assert "request fewer paths at a time" in text
            os.environ["EDSX_PATHS_BUDGET"] = str(rows + scratch + 56 * n - 1)      # the records are
            code, text = _error(s.ibs, **kw)
            assert code == 4 and "(%d bytes)" % (56 * n) in text and "request fewer paths at a time" in text
            os.environ["EDSX_PATHS_BUDGET"] = str(max(rows + scratch + 56 * n, 16 * s.info["n_choice_symbols"] + 64))
            check(s.ibs(**kw), eds, seds, kw)
        finally:
            del os.environ["EDSX_PATHS_BUDGET"]
        check(s.ibs(**kw), eds, seds, kw)
        assert s.spell([1], 0)[0] == ps.fasta(eds, seds, [1], 0)[0]      # the other calls of the session go on
        assert s.distances(req, "strings")[0].tolist() == ds.matrix(eds, seds, req, "strings")[0]      # (it shares the rows)


def test_kernels_come_back_by_name(ctx):
    eds, seds = SHAPES["wide"][:2]
    with ctx.paths_open(eds, seds) as s:
        s.ibs()
        assert not [name for name, *_ in ctx.get_timing() if name.startswith("k_ibs_")]
        ctx.set_timing(True)
        try:
            s.ibs()
            names = {name: launches for name, _, launches in ctx.get_timing()}
        finally:
            ctx.set_timing(False)
    assert {"k_dist_rows", "k_ibs_scan", "k_ibs_stitch", "scan_segments"} <= set(names)
    assert names["k_ibs_scan"] == 2 and names["k_ibs_stitch"] == 2          # the COUNT and the FILL pass


# ---- the tool and the C++ shim ---------------------------------------------------------------------------------------------
CLI = (b"{ACGTAC}{A,ACA,}{CGTTTTT}{,T}{GG}{C,G}{TTTTTTTTTT}{A,C,G}{}", b"{0}{1,3}{2}{4}{0}{1,2}{3,4}{0}{1,2,3}{5,6}{0}{1,5}{2,6}{3}{0}")


def test_edsparser_ibs_cli(tmp_path):
    subprocess.run(["make", "-s", "-C", HOST], check=True)        # (libedsx.so itself comes from build())
    exe = os.path.join(BUILD, "edsparser-ibs")
    eds, seds = CLI
    (tmp_path / "x.eds").write_bytes(eds)
    (tmp_path / "x.seds").write_bytes(seds)
    (tmp_path / "names.txt").write_text("alpha\nbeta\ngamma\ndelta\nepsilon\nzeta\n")
    (tmp_path / "bad.txt").write_text("alpha\nbe ta\n")
    base = [exe, "-i", str(tmp_path / "x.eds")]
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "EDS shared segments" in r.stdout and "IBS complete!" in r.stdout and "[Performance] Runtime:" in r.stderr
    assert len(isp.ibs(eds, seds)["segments"]) >= 5 and (tmp_path / "x.ibs").read_bytes() == isp.text(eds, seds)
    runs = [(["--min-sites", "0"], dict(min_sites=0)),
            (["-p", "6,1,3-4,1", "--min-sites", "2", "--prefix", "hap"], dict(paths=[6, 1, 3, 4, 1], min_sites=2, prefix=b"hap")),
            (["--min-sites", "0", "--min-columns", "8"], dict(min_sites=0, min_columns=8)),
            (["--names", str(tmp_path / "names.txt"), "-p", "4,2"], dict(paths=[4, 2], names=[b"delta", b"beta"]))]
    for k, (args, kw) in enumerate(runs):
        out = tmp_path / ("o%d.txt" % k)
        r = subprocess.run(base + ["-s", str(tmp_path / "x.seds"), "-o", str(out)] + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == isp.text(eds, seds, **kw), args
    no = tmp_path / "no.txt"
    for args, text in ((["--min-sites", "x"], "for option '--min-sites' is invalid"), (["-p", "7"], "Error: Path id 7 out of range (1..6)"),
                       (["--min-sites", "0", "--max-segments", "1"], "segments, above the limit of 1"),
                       (["--names", str(tmp_path / "bad.txt"), "-p", "2"], "The name of path 2 is empty or holds a tab, blank or line feed"),
                       (["--names", str(tmp_path / "bad.txt"), "-p", "3"], "The names file has no name for path 3"),
                       (["-s", str(tmp_path / "none.seds")], "Path spelling needs sources (.seds)")):
        r = subprocess.run(base + ["-o", str(no)] + args, capture_output=True, text=True)
        assert r.returncode == 1 and text in r.stderr and "[Performance] Runtime:" in r.stderr and not no.exists(), (args, r.stderr)
    (tmp_path / "alone.eds").write_bytes(eds)                     # no .seds beside it
    r = subprocess.run([exe, "-i", str(tmp_path / "alone.eds")], capture_output=True, text=True)
    assert r.returncode == 1 and "Path spelling needs sources (.seds)" in r.stderr


def test_path_ibs_cpp_shim(tmp_path):
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    exe = os.path.join(BUILD, "test_ibs_shim")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, os.path.join(ROOT, "tests", "cpp", "test_ibs_shim.cpp"),
                    os.path.join(BUILD, "libedsparser_lib.a"), "-L", LIBDIR, "-ledsx", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    eds, seds = CLI
    cmds = [(b"I", eds, seds, b"-", b"1", b"0", b"0"), (b"I", eds, seds, b"6,1,1,2,3", b"0", b"2", b"0"),
            (b"I", eds, seds, b"7", b"1", b"0", b"0"), (b"I", eds, seds, b"-", b"0", b"0", b"3")]
    (tmp_path / "cmds.txt").write_bytes(b"".join(b"\t".join(c) + b"\n" for c in cmds))
    r = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split(b"\n")[:-1]
    for line, kw in zip(out, (dict(), dict(paths=[6, 1, 1, 2, 3], min_sites=0, min_columns=2))):
        w = isp.ibs(eds, seds, **kw)
        recs = "".join(",".join("%d" % v for v in s) + ";" for s in w["segments"])
        i = w["info"]
        assert w["segments"] and line.decode() == "%s#%s#%d,%d,%d" % (recs, ",".join("%d" % v for v in w["pair_off"]), i["paths"],
                                                                        i["choice_symbols"], i["candidate_segments"])
    assert out[2] == b"invalid_argument:Path id 7 out of range (1..6)"
    assert out[3].startswith(b"invalid_argument:IBS has ") and out[3].endswith(b"segments, above the limit of 3")
