"""GPU: edsx_paths_distances / edsx_eds_distances (k_dist_symbols / _count / _fill / _rows / _pairs / _finish) against the
Python restatement of the specification (tests/dist_spec.py) on the boundary shapes of the kernels (tests/dist_cases.py)
and the fixture sets, every number an exact integer; and by routes that do not use the specification: the Hamming
distances of the rows PathSession.align returns, of the rows of an alignment handed to msa_transform, the sub-matrix after
Context.eds_subset, and the sum over PathSession.slice column windows.  Then batches, errors, timing, the edsparser-dist
tool and the C++ shim."""
import os
import random
import subprocess

import numpy as np
import pytest

import dist_cases as dc
import dist_spec as ds
import msa_export_spec as ms
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
    return ei.value.code, ei.value.message


def check(got, eds, seds, req, metric):
    D, miss, info = got
    want, wmiss, units = ds.matrix(eds, seds, req, metric)
    assert D.dtype == np.uint64 and D.shape == (len(want), len(want))
    assert D.tolist() == want, (req, metric)
    assert miss.tolist() == wmiss and info["units"] == units
    return info


def geometry(info, eds, seds, metric):
    """the info struct against the class list restated in Python and the chunk rule for few workgroups"""
    desc, V = dc.classes(eds, seds, metric)
    words = (len(desc) + 63) // 64
    assert (info["variable_units"], info["class_columns"]) == (V, len(desc))
    assert info["chunk_columns"] == dc.CHUNK_COLUMNS and info["chunks"] == (words + 63) // 64
    return len(desc)


# ---- boundary shapes against the specification ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ds.METRICS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_boundary_shapes(ctx, name, metric):
    eds, seds, requests = SHAPES[name]
    P = ps.parse(eds, seds)[2]
    with ctx.paths_open(eds, seds) as s:
        for req in requests:
            info = check(s.distances(req, metric), eds, seds, req, metric)
            if s.info["n_choice_symbols"]:
                C = geometry(info, eds, seds, metric)
            else:
                C = 0
                assert (info["variable_units"], info["class_columns"], info["chunks"]) == (0, 0, 0)
    if name.startswith("columns"):
        assert C == int(name[7:])                                # the shape has the class columns its name claims
    if name == "long" and metric == "columns":
        assert info["chunks"] == 2 and C == 6000                 # one symbol spans two chunks by itself
    if name == "wide":
        assert P == 130


def test_one_shot_call_and_numbers(ctx):
    eds, seds = b"{AC}{G,T}{A,}", b"{0}{1}{2,3}{1,2}{3}"
    D, miss, info = ctx.eds_distances(eds, seds)
    assert D.tolist() == [[0, 1, 2], [1, 0, 1], [2, 1, 0]] and miss.tolist() == [0, 0, 0]
    assert info == {"units": 4, "variable_units": 2, "class_columns": 4, "chunk_columns": 4096, "chunks": 1}
    D, miss, info = ctx.eds_distances(eds, seds, [3, 3, 1], "strings")
    assert D.tolist() == [[0, 0, 2], [0, 0, 2], [2, 2, 0]] and info["units"] == 3
    assert _error(ctx.eds_distances, eds, None) == (3, "Path spelling needs sources (.seds)")
    assert _error(ctx.eds_distances, eds, seds, [4]) == (3, "Path id 4 out of range (1..3)")


@pytest.mark.parametrize("which", ["merge", "vcf"])
def test_fixture_sets(ctx, which):
    ran = 0
    for eds, seds in (merge_fixture_inputs() if which == "merge" else vcf_fixture_outputs()):
        try:
            P = ps.parse(eds, seds)[2]
        except ValueError:                                       # fixtures whose sources do not match their text
            continue
        if P == 0:
            continue
        with ctx.paths_open(eds, seds) as s:
            for metric in ds.METRICS:
                check(s.distances(None, metric), eds, seds, None, metric)
        ran += 1
    assert ran >= 100


# ---- routes that do not use the specification ----------------------------------------------------------------------------
def hamming(rows):
    a = np.array([np.frombuffer(r, dtype=np.uint8) for r in rows])
    return (a[:, None, :] != a[None, :, :]).sum(axis=2).astype(np.uint64)


def test_columns_equal_the_hamming_distances_of_align(ctx):
    rng = random.Random(41)
    for eds, seds in [SHAPES["wide"][:2], dc.EDGE] + [dc.random_eds(rng, 30, 9) for _ in range(5)]:
        gap = next(bytes([g]) for g in b".*#+" if bytes([g]) not in eds)
        with ctx.paths_open(eds, seds) as s:
            rows = [r for _, r in ms.rows_of(s.align(None, 0, gap=gap)[0])]
            D = s.distances(None, "columns")[0]
        assert len(rows) == len(D) and (D == hamming(rows)).all()


def _alignment(rng, rows, cols, gaps):
    base = np.frombuffer(bytes(rng.choice(b"ACGT") for _ in range(cols)), dtype=np.uint8)
    nrng = np.random.default_rng(rng.randrange(1 << 30))
    A = np.tile(base, (rows, 1))
    hit = nrng.random((rows, cols)) < 0.03
    A[hit] = nrng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(hit.sum()))
    if gaps:
        A[nrng.random((rows, cols)) < 0.01] = ord("-")
    return A, b"".join(b">s%d\n%s\n" % (k, A[k].tobytes()) for k in range(rows))


def test_distances_of_a_transformed_alignment_are_its_row_distances(ctx):
    A, msa = _alignment(random.Random(5), 70, 3000, gaps=False)
    want = (A[:, None, :] != A[None, :, :]).sum(axis=2).astype(np.uint64)
    assert want.max() > 100
    for l in (0, 4):
        eds, seds = ctx.msa_transform(msa, l)
        D, miss, info = ctx.eds_distances(eds, seds)
        assert (D == want).all() and not miss.any() and info["units"] == 3000


def test_subset_gives_the_sub_matrix(ctx):
    rng = random.Random(6)
    eds, seds = SHAPES["wide"][:2]
    Q = sorted(rng.sample(range(1, 131), 37))
    e2, s2, _ = ctx.eds_subset(eds, seds, Q)
    for metric in ds.METRICS:
        full = ctx.eds_distances(eds, seds, None, metric)[0]
        part = ctx.eds_distances(e2, s2, None, metric)[0]
        assert len(part) == len(Q)
        assert (part == full[np.ix_(np.array(Q) - 1, np.array(Q) - 1)]).all()
        assert (ctx.eds_distances(eds, seds, Q, metric)[0] == part).all()


def test_columns_add_up_over_column_windows(ctx):
    A, msa = _alignment(random.Random(7), 20, 1500, gaps=True)
    eds, seds = ctx.msa_transform(msa, 0)
    with ctx.paths_open(eds, seds) as s:
        W, P = s.align_info()["n_columns"], s.info["num_paths"]
        full = s.distances(None, "columns")[0]
        cuts = [0] + sorted(random.Random(8).sample(range(1, W), 5)) + [W]
        e, q, reg = s.slice([0] * 6, cuts[:-1], cuts[1:])
    assert P == 20 and not reg["status"].any() and full.max() > 20
    total = np.zeros((P, P), dtype=np.uint64)
    for k in range(6):
        pe = e[int(reg["eds_off"][k]):int(reg["eds_off"][k] + reg["eds_len"][k])]
        pq = q[int(reg["seds_off"][k]):int(reg["seds_off"][k] + reg["seds_len"][k])]
        D = ctx.eds_distances(pe, pq)[0]
        assert len(D) in (0, P)                                  # a window of common symbols only has no paths: they agree there
        if len(D):
            total += D
    assert (total == full).all()


# ---- the session ---------------------------------------------------------------------------------------------------------
def test_forced_table_batches_equal_one_batch(ctx):
    """EDSX_PATHS_BUDGET stands in for the free HBM: choice tables of one and of two paths; the rows and the matrix fit it"""
    eds, seds, _ = ctx.genrandomeds(400_000, seed=11)
    req = [4, 1, 2, 3, 3, 1, 2]
    with ctx.paths_open(eds, seds) as s:
        nc = s.info["n_choice_symbols"]
        assert nc > 1000
        want = {m: s.distances(req, m) for m in ds.METRICS}
        assert (want["columns"][0] == hamming([r for _, r in ms.rows_of(s.align(req, 0, gap="#")[0])])).all()
        try:
            for budget in (16 * nc + 64, 2 * (16 * nc + 64)):
                os.environ["EDSX_PATHS_BUDGET"] = str(budget)
                for m in ds.METRICS:
                    info = want[m][2]
                    assert 8 * len(req) * ((info["class_columns"] + 63) // 64) + 8 * len(req) ** 2 <= budget
                    got = s.distances(req, m)
                    assert (got[0] == want[m][0]).all() and (got[1] == want[m][1]).all() and got[2] == info, (budget, m)
        finally:
            del os.environ["EDSX_PATHS_BUDGET"]


def test_metrics_alternate_and_errors_leave_the_session_usable(ctx):
    eds, seds = dc.EDGE
    with ctx.paths_open(eds, seds) as s:
        for metric in ("strings", "columns", "strings", "columns"):
            check(s.distances([67, 1, 2, 66], metric), eds, seds, [67, 1, 2, 66], metric)
        t = s.timing
        assert t["bytes_written"] == 8 * 16 and t["copy_ms"] > 0 and t["choose_ms"] > 0
        assert _error(s.distances, [1, 0]) == (3, "Path id 0 out of range (1..67)")
        assert _error(s.distances, [68]) == (3, "Path id 68 out of range (1..67)")
        check(s.distances([2, 1], "columns"), eds, seds, [2, 1], "columns")
        assert _error(s.distances, [1, 2], 2)[0] == 3 and _error(s.distances, [1, 2], -1)[0] == 3
        with pytest.raises(ValueError):
            s.distances([1, 2], "rows")
        n = 8 * 67 * 67
        assert _error(s.distances, None, "columns", n - 1) == (3, "Distance matrix has %d bytes, above the limit of %d" % (n, n - 1))
        check(s.distances(None, "columns", n), eds, seds, None, "columns")
        info = s.distances([1, 2, 3], "columns")[2]
        need = 8 * 3 * ((info["class_columns"] + 63) // 64) + 8 * 9
        try:
            os.environ["EDSX_PATHS_BUDGET"] = str(need - 1)     # the rows and the matrix are one byte too many
            code, text = _error(s.distances, [1, 2, 3], "columns")
            assert code == 4 and "(%d bytes)" % (need - 72) in text and "(72 bytes)" in text and str(need - 1) in text
            os.environ["EDSX_PATHS_BUDGET"] = str(need)
            check(s.distances([1, 2, 3], "columns"), eds, seds, [1, 2, 3], "columns")
        finally:
            del os.environ["EDSX_PATHS_BUDGET"]
        check(s.distances(None, "strings"), eds, seds, None, "strings")
        assert s.spell([1], 0)[0] == ps.fasta(eds, seds, [1], 0)[0]      # the other calls of the session go on


def test_kernels_come_back_by_name(ctx):
    eds, seds = SHAPES["wide"][:2]
    with ctx.paths_open(eds, seds) as s:
        s.distances(None, "columns")
        assert not [name for name, *_ in ctx.get_timing() if name.startswith("k_dist_")]
        ctx.set_timing(True)
        try:
            s.distances(None, "strings")                         # the first call of this metric: its class list
            s.distances(None, "columns")                         # the class list of this one is session state already
            names = {name: launches for name, _, launches in ctx.get_timing()}
        finally:
            ctx.set_timing(False)
    assert {"k_dist_count", "scan_classes", "k_dist_fill", "k_dist_rows", "k_dist_pairs", "k_dist_finish"} <= set(names)
    assert names["k_dist_count"] == 1 and names["k_dist_pairs"] == 2


# ---- the tool and the C++ shim ---------------------------------------------------------------------------------------------
def test_edsparser_dist_cli(tmp_path):
    subprocess.run(["make", "-s", "-C", HOST], check=True)        # (libedsx.so itself comes from build())
    exe = os.path.join(BUILD, "edsparser-dist")
    eds, seds = b"{ACGTAC}{A,ACA,}{CGTTTTT}{,T}{GG}{C,G}{TTTTTTTTTT}{}", b"{0}{1,3}{2}{4}{0}{1,2}{3,4}{0}{1,2,3}{5}{0}{0}"
    (tmp_path / "x.eds").write_bytes(eds)
    (tmp_path / "x.seds").write_bytes(seds)
    (tmp_path / "names.txt").write_text("alpha\nbeta\ngamma\ndelta\nepsilon\n")
    (tmp_path / "bad.txt").write_text("alpha\nbe ta\n")
    base = [exe, "-i", str(tmp_path / "x.eds")]
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "EDS path distances" in r.stdout and "Distances complete!" in r.stdout and "[Performance] Runtime:" in r.stderr
    assert "Warning: path 5 has no string in 2 symbols" in r.stderr
    assert (tmp_path / "x.dist").read_bytes() == ds.text(eds, seds)
    runs = [(["-p", "5,1,3-4", "--metric", "strings"], dict(paths=[5, 1, 3, 4], metric="strings")),
            (["--normalize", "--format", "phylip"], dict(fmt="phylip", normalize=True)),
            (["--format", "phylip", "--prefix", "hap", "-p", "2,2"], dict(fmt="phylip", paths=[2, 2], prefix=b"hap")),
            (["--normalize", "--metric", "strings", "--names", str(tmp_path / "names.txt"), "-p", "4,2"],
             dict(normalize=True, metric="strings", paths=[4, 2], names=[b"delta", b"beta"]))]
    for k, (args, kw) in enumerate(runs):
        out = tmp_path / ("o%d.txt" % k)
        r = subprocess.run(base + ["-s", str(tmp_path / "x.seds"), "-o", str(out)] + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == ds.text(eds, seds, **kw), args
    no = tmp_path / "no.txt"
    for args, text in ((["-p", "6"], "Error: Path id 6 out of range (1..5)"), (["--metric", "rows"], "for option '--metric' is invalid"),
                       (["--format", "csv"], "for option '--format' is invalid"),
                       (["--names", str(tmp_path / "bad.txt"), "-p", "2"], "The name of path 2 is empty or holds a tab, blank or line feed"),
                       (["--names", str(tmp_path / "bad.txt"), "-p", "3"], "The names file has no name for path 3"),
                       (["--prefix", "a b"], "The name of path 1 is empty or holds a tab, blank or line feed")):
        r = subprocess.run(base + ["-o", str(no)] + args, capture_output=True, text=True)
        assert r.returncode == 1 and text in r.stderr and "[Performance] Runtime:" in r.stderr and not no.exists(), (args, r.stderr)
    (tmp_path / "u.eds").write_bytes(b"{,}{}")                    # no column at all: 0 / 0 prints 0.000000
    (tmp_path / "u.seds").write_bytes(b"{1}{2}{0}")
    r = subprocess.run([exe, "-i", str(tmp_path / "u.eds"), "--normalize"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "u.dist").read_bytes() == b"path\ts0\ts1\ns0\t0.000000\t0.000000\ns1\t0.000000\t0.000000\n"


def test_path_distances_cpp_shim(tmp_path):
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    exe = os.path.join(BUILD, "test_dist_shim")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, os.path.join(ROOT, "tests", "cpp", "test_dist_shim.cpp"),
                    os.path.join(BUILD, "libedsparser_lib.a"), "-L", LIBDIR, "-ledsx", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    eds, seds = b"{ACGTAC}{A,ACA,}{CGTTTTT}{,T}{GG}{C,G}{TTTTTTTTTT}{}", b"{0}{1,3}{2}{4}{0}{1,2}{3,4}{0}{1,2,3}{5}{0}{0}"
    cmds = [(b"D", eds, seds, b"-", b"columns"), (b"D", eds, seds, b"5,1,1", b"strings"), (b"D", eds, seds, b"6", b"columns"),
            (b"D", eds, seds, b"-1", b"columns")]
    (tmp_path / "cmds.txt").write_bytes(b"".join(b"\t".join(c) + b"\n" for c in cmds))
    r = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split(b"\n")[:-1]
    for line, (req, metric) in zip(out, ((None, "columns"), ([5, 1, 1], "strings"))):
        D, miss, units = ds.matrix(eds, seds, req, metric)
        assert line == b"%d#%s#%s#%d" % (len(D), b",".join(b"%d" % d for row in D for d in row), b",".join(b"%d" % m for m in miss), units)
    assert out[2] == b"invalid_argument:Path id 6 out of range (1..5)"
    assert out[3] == b"invalid_argument:Path id 0 out of range (1..5)"
