"""GPU: edsx_paths_ld / edsx_eds_ld (k_ld_count / _rows / _tiles / _pairs) against the Python restatement of the
specification (tests/ld_spec.py) on the boundary shapes of the kernels (tests/ld_cases.py) and the fixture sets: every
integer field equal, r² bit-equal, the order checked; a threshold at which the specification alone decides membership; and a
route that does not use the specification: the squared correlation of the columns of an alignment handed to msa_transform.
Then path subsets, limits, errors, timing, the edsparser-ld tool and the C++ shim."""
import math
import os
import random
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import ld_cases as lc
import ld_spec as ls
import path_spec as ps
from test_paths_cpu import BUILD, HOST, INC, LIBDIR, ROOT, merge_fixture_inputs, vcf_fixture_outputs

pytestmark = pytest.mark.gpu

SHAPES = lc.boundary_shapes()


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    return edsparser_amd.Context(0)


def _error(fn, *a, **kw):
    import edsparser_amd
    with pytest.raises(edsparser_amd.EdsxError) as ei:
        fn(*a, **kw)
    return ei.value.code, ei.value.message


def bits(values):
    return [struct.unpack("<Q", struct.pack("<d", v))[0] for v in values]


def check(got, eds, seds, kw):
    pairs, alleles, info = got
    want = ls.ld(eds, seds, **kw)
    assert alleles.dtype.names == ls.ALLELE_FIELDS and pairs.dtype.names == ls.PAIR_FIELDS
    assert [tuple(a) for a in alleles.tolist()] == want["alleles"], kw
    assert [tuple(p)[:8] for p in pairs.tolist()] == [p[:8] for p in want["pairs"]], kw
    assert pairs["r2"].view(np.uint64).tolist() == bits(p[8] for p in want["pairs"]), kw          # bit-equal
    keys = [tuple(p)[:4] for p in pairs.tolist()]
    assert keys == sorted(keys)
    assert {k: info[k] for k in want["info"]} == want["info"], kw
    assert info["row_words"] == (ps.parse(eds, seds)[2] + 63) // 64
    return info


# ---- boundary shapes against the specification ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_boundary_shapes(ctx, name):
    eds, seds, requests = SHAPES[name]
    with ctx.paths_open(eds, seds) as s:
        for kw in requests:
            info = check(s.ld(**kw), eds, seds, kw)
            for t in (0.05, 0.5):                                # FILL skips the tiles without a reported pair
                check(s.ld(min_r2=t, **kw), eds, seds, dict(kw, min_r2=t))
    if name.startswith("alleles"):
        assert info["alleles"] == int(name[7:])                  # the shape has the alleles its name claims
    if name == "paths2049":
        assert info["row_words"] == 33 and info["choice_symbols"] == 6    # a second LDS stage with a 1-word tail
    if name == "paths64":
        assert info["row_words"] == 1
    if name == "wide70":
        assert info["tiles"] >= 4 and info["alleles"] > 128
    if name == "windows":
        assert info["choice_symbols"] == 10
    if name == "fixed":
        assert info == {"paths": 3, "choice_symbols": 0, "alleles": 0, "candidate_pairs": 0, "undefined_pairs": 0, "pairs": 0,
                        "row_words": 1, "tiles": 0}


def test_one_shot_call_and_numbers(ctx):
    eds, seds = b"{A,C}{G}{T,A,}{C,G}", b"{1,2}{3,4}{0}{1}{2,3}{4}{1,3}{2,4}"
    pairs, alleles, info = ctx.eds_ld(eds, seds, window=1)
    assert [tuple(a) for a in alleles.tolist()] == [(0, 1, 2, 4), (2, 1, 2, 4), (2, 2, 1, 4), (3, 1, 2, 4)]
    assert [tuple(p) for p in pairs.tolist()] == [(0, 1, 2, 1, 1, 2, 2, 4, 0.0), (0, 1, 2, 2, 1, 2, 1, 4, 1 / 3), (2, 1, 3, 1, 1, 2, 2, 4, 0.0),
                                                 (2, 2, 3, 1, 1, 1, 2, 4, 1 / 3)]
    assert info == {"paths": 4, "choice_symbols": 3, "alleles": 4, "candidate_pairs": 4, "undefined_pairs": 0, "pairs": 4,
                    "row_words": 1, "tiles": 1}
    check(ctx.eds_ld(eds, seds, [4, 4, 1, 2], window=2, all_strings=True), eds, seds, dict(paths=[4, 4, 1, 2], window=2, all_strings=True))
    assert _error(ctx.eds_ld, eds, None) == (3, "Path spelling needs sources (.seds)")
    assert _error(ctx.eds_ld, eds, seds, [5]) == (3, "Path id 5 out of range (1..4)")


# ---- the threshold: the specification alone decides membership -----------------------------------------------------------
@pytest.mark.parametrize("name", ["missing", "paths129", "wide70"])
def test_threshold(ctx, name):
    eds, seds, _ = SHAPES[name]
    t = 1 / math.pi
    kw = dict(window=6, all_strings=True)
    cand = ls.ld(eds, seds, **kw)["candidates"]
    exact = [ls.r2_of(*c[4:], exact=True) for c in cand]
    assert len(cand) > 400 and all(v is None or abs(v - Fraction(t)) > Fraction(1, 10 ** 12) for v in exact)
    want = [c[:4] for c, v in zip(cand, exact) if v is not None and v >= Fraction(t)]
    pairs, _, info = ctx.eds_ld(eds, seds, min_r2=t, **kw)
    assert [tuple(p)[:4] for p in pairs.tolist()] == want and 0 < len(want) < len(cand)
    check((pairs, _, info), eds, seds, dict(kw, min_r2=t))


# ---- a route that does not use the specification -------------------------------------------------------------------------
def test_r2_of_a_transformed_alignment_is_the_squared_correlation_of_its_columns(ctx):
    rng = np.random.default_rng(17)
    rows, cols = 40, 300
    A = np.full((rows, cols), ord("A"), dtype=np.uint8)
    variable = np.sort(rng.choice(cols, 70, replace=False))
    for c in variable:
        A[rng.random(rows) < rng.uniform(0.15, 0.6), c] = ord("C")
    for c in variable[::9]:                                      # a few columns with three letters
        A[rng.random(rows) < 0.2, c] = ord("G")
    msa = b"".join(b">s%d\n%s\n" % (k, A[k].tobytes()) for k in range(rows))
    eds, seds = ctx.msa_transform(msa, 0)
    syms = ps.parse(eds, seds)[0]
    with ctx.paths_open(eds, seds) as s:
        assert s.info["num_paths"] == rows
        pairs, alleles, info = s.ld(window=8, all_strings=True)
        _, st, sites = s.lift([1] * cols, list(range(cols)), [1] * cols, with_sites=True)
    assert not st.any()
    column = {}
    for q in range(cols):
        column.setdefault(int(sites["symbol"][q]), int(sites["column"][q]))
    single = lambda i: all(len(t) == 1 for t in syms[i])
    ran = 0
    for p in pairs.tolist():
        sa, ja, sb, jb = p[:4]
        if not (single(sa) and single(sb)):
            continue
        a = (A[:, column[sa]] == syms[sa][ja][0]).astype(float)
        b = (A[:, column[sb]] == syms[sb][jb][0]).astype(float)
        assert p[7] == rows and abs(p[8] - float(np.corrcoef(a, b)[0, 1]) ** 2) <= 1e-9
        ran += 1
    assert ran > 300 and info["undefined_pairs"] == 0


# ---- path subsets and the fixture sets -----------------------------------------------------------------------------------
def test_path_subsets(ctx):
    eds, seds, _ = SHAPES["subset"]
    rng = random.Random(3)
    with ctx.paths_open(eds, seds) as s:
        for _ in range(4):
            M = [rng.randint(1, 130) for _ in range(rng.choice([2, 40, 90, 200]))]     # duplicates included
            for kw in (dict(paths=M, window=3), dict(paths=M, window=5, all_strings=True, min_count=2)):
                assert check(s.ld(**kw), eds, seds, kw)["paths"] == len(set(M))
        check(s.ld(list(range(1, 131)), window=3), eds, seds, dict(window=3))


@pytest.mark.parametrize("which", ["merge", "vcf"])
def test_fixture_sets(ctx, which):
    ran = reported = 0
    kw = dict(window=3, all_strings=True, min_count=0)
    for eds, seds in (merge_fixture_inputs() if which == "merge" else vcf_fixture_outputs()):
        try:
            P = ps.parse(eds, seds)[2]
        except ValueError:                                       # fixtures whose sources do not match their text
            continue
        if P == 0:
            continue
        reported += check(ctx.eds_ld(eds, seds, **kw), eds, seds, kw)["pairs"]
        ran += 1
    assert ran >= 100 and reported > 100


# ---- the session ---------------------------------------------------------------------------------------------------------
def test_limits_and_errors_leave_the_session_usable(ctx):
    import edsparser_amd
    eds, seds, _ = SHAPES["missing"]
    kw = dict(window=4, all_strings=True)
    with ctx.paths_open(eds, seds) as s:
        info = check(s.ld(**kw), eds, seds, kw)
        n = info["pairs"]
        assert n > 100
        with pytest.raises(edsparser_amd.EdsxError) as ei:
            s.ld(max_pairs=n - 1, **kw)
        assert (ei.value.code, ei.value.message) == (3, "LD has %d pairs, above the limit of %d" % (n, n - 1))
        assert ei.value.info == info                             # filled in although the call failed
        assert check(s.ld(max_pairs=n, **kw), eds, seds, kw) == info
        t = s.timing
        assert t["bytes_written"] == 72 * n + 32 * info["alleles"] and t["copy_ms"] > 0 and t["scan_ms"] > 0
        assert _error(s.ld, window=0)[0] == 3
        for bad in (-0.1, 1.5, float("nan")):
            assert _error(s.ld, window=3, min_r2=bad)[0] == 3
        assert _error(s.ld, [1, 0], window=3) == (3, "Path id 0 out of range (1..40)")
        assert _error(s.ld, [41], window=3) == (3, "Path id 41 out of range (1..40)")
        need = 8 * info["row_words"] * info["alleles"]
        try:
            os.environ["EDSX_PATHS_BUDGET"] = str(need - 1)      # the allele rows alone are one byte too many
            code, text = _error(s.ld, **kw)
            assert code == 4 and "(%d bytes)" % need in text and str(need - 1) in text
        finally:
            del os.environ["EDSX_PATHS_BUDGET"]
        check(s.ld(**kw), eds, seds, kw)
        assert s.spell([1], 0)[0] == ps.fasta(eds, seds, [1], 0)[0]      # the other calls of the session go on


def test_kernels_come_back_by_name(ctx):
    eds, seds, _ = SHAPES["paths129"]
    with ctx.paths_open(eds, seds) as s:
        s.ld(window=3)
        assert not [name for name, *_ in ctx.get_timing() if name.startswith("k_ld_")]
        ctx.set_timing(True)
        try:
            s.ld(window=3)
            names = {name: launches for name, _, launches in ctx.get_timing()}
        finally:
            ctx.set_timing(False)
    assert {"k_ld_count", "scan_alleles", "k_ld_rows", "k_ld_tiles", "scan_tiles", "k_ld_pairs", "scan_pairs"} <= set(names)
    assert names["k_ld_count"] == 1 and names["k_ld_pairs"] == 2  # the COUNT and the FILL pass


# ---- the tool and the C++ shim ---------------------------------------------------------------------------------------------
CLI = (b"{ACGTAC}{A,ACA,}{CGTTTTT}{,T}{GG}{C,G}{TTTTTTTTTT}{A,C,G}{}", b"{0}{1,3}{2}{4}{0}{1,2}{3,4}{0}{1,2,3}{5,6}{0}{1,5}{2,6}{3}{0}")


def test_edsparser_ld_cli(tmp_path):
    subprocess.run(["make", "-s", "-C", HOST], check=True)        # (libedsx.so itself comes from build())
    exe = os.path.join(BUILD, "edsparser-ld")
    eds, seds = CLI
    (tmp_path / "x.eds").write_bytes(eds)
    (tmp_path / "x.seds").write_bytes(seds)
    base = [exe, "-i", str(tmp_path / "x.eds")]
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "EDS linkage disequilibrium" in r.stdout and "LD complete!" in r.stdout and "[Performance] Runtime:" in r.stderr
    want = ls.ld(eds, seds, window=100, min_r2=0.2)
    assert want["pairs"] and (tmp_path / "x.ld").read_bytes() == ls.pair_text(want["pairs"])
    runs = [(["--window", "1", "--min-r2", "0", "--all-strings"], dict(window=1, all_strings=True)),
            (["-p", "6,1,3-4,1", "--min-r2", "0.05", "--min-count", "0"], dict(paths=[6, 1, 3, 4, 1], min_r2=0.05, min_count=0)),
            (["--min-count", "2", "--min-r2", "0", "--all-strings", "--window", "2"], dict(min_count=2, all_strings=True, window=2))]
    for k, (args, kw) in enumerate(runs):
        out, frq = tmp_path / ("o%d.txt" % k), tmp_path / ("f%d.txt" % k)
        r = subprocess.run(base + ["-s", str(tmp_path / "x.seds"), "-o", str(out), "--freq", str(frq)] + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        want = ls.ld(eds, seds, **kw)
        assert out.read_bytes() == ls.pair_text(want["pairs"]) and frq.read_bytes() == ls.freq_text(want["alleles"]), args
    no = tmp_path / "no.txt"
    for args, text in ((["--window", "0"], "for option '--window' is invalid"), (["--window", "x"], "for option '--window' is invalid"),
                       (["--min-r2", "1.5"], "for option '--min-r2' is invalid"), (["-p", "7"], "Error: Path id 7 out of range (1..6)"),
                       (["--min-r2", "0", "--max-pairs", "1"], "pairs, above the limit of 1"),
                       (["-s", str(tmp_path / "none.seds")], "Path spelling needs sources (.seds)")):
        r = subprocess.run(base + ["-o", str(no)] + args, capture_output=True, text=True)
        assert r.returncode == 1 and text in r.stderr and "[Performance] Runtime:" in r.stderr and not no.exists(), (args, r.stderr)
    (tmp_path / "alone.eds").write_bytes(eds)                     # no .seds beside it
    r = subprocess.run([exe, "-i", str(tmp_path / "alone.eds")], capture_output=True, text=True)
    assert r.returncode == 1 and "Path spelling needs sources (.seds)" in r.stderr


def test_path_ld_cpp_shim(tmp_path):
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    exe = os.path.join(BUILD, "test_ld_shim")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, os.path.join(ROOT, "tests", "cpp", "test_ld_shim.cpp"),
                    os.path.join(BUILD, "libedsparser_lib.a"), "-L", LIBDIR, "-ledsx", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    eds, seds = CLI
    cmds = [(b"L", eds, seds, b"-", b"100", b"0", b"1", b"0"), (b"L", eds, seds, b"6,1,1,2,3", b"2", b"0.1", b"0", b"1"),
            (b"L", eds, seds, b"7", b"3", b"0", b"1", b"0"), (b"L", eds, seds, b"-", b"0", b"0", b"1", b"0")]
    (tmp_path / "cmds.txt").write_bytes(b"".join(b"\t".join(c) + b"\n" for c in cmds))
    r = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split(b"\n")[:-1]
    for line, kw in zip(out, (dict(window=100), dict(paths=[6, 1, 1, 2, 3], window=2, min_r2=0.1, min_count=0, all_strings=True))):
        w = ls.ld(eds, seds, **kw)
        pairs = "".join(",".join("%d" % v for v in p[:8] + tuple(bits(p[8:]))) + ";" for p in w["pairs"])
        alleles = "".join("%d,%d,%d,%d;" % a for a in w["alleles"])
        i = w["info"]
        assert w["pairs"] and line.decode() == "%s#%s#%d,%d,%d,%d" % (pairs, alleles, i["paths"], i["choice_symbols"], i["candidate_pairs"],
                                                                        i["undefined_pairs"])
    assert out[2] == b"invalid_argument:Path id 7 out of range (1..6)"
    assert out[3].startswith(b"invalid_argument:The LD window is 0")
