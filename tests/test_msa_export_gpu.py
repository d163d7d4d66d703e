"""GPU: edsx_paths_align / edsx_eds_msa (k_align_width / k_path_align) byte for byte against the Python restatement of the
specification (tests/msa_export_spec.py): the merge and VCF fixtures at the line widths around the 16-byte chunk, the
shapes at which the kernel takes another path (more symbols in a tile than the LDS holds, a symbol wider than several
tiles, zero-width symbols, missing strings), forced batches, errors, the round trip through msa2eds on the device, the
eds2msa tool and the edsparser::eds_to_msa shim."""
import os
import subprocess

import numpy as np
import pytest

import msa_export_spec as ms
import path_spec as ps
from test_paths_cpu import BUILD, HOST, INC, LIBDIR, ROOT, merge_fixture_inputs, vcf_fixture_outputs

pytestmark = pytest.mark.gpu

TILE = 16384                                                     # output bytes per workgroup step of k_path_align


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    return edsparser_amd.Context(0)


def _error(fn, *a, **kw):
    import edsparser_amd
    with pytest.raises(edsparser_amd.EdsxError) as ei:
        fn(*a, **kw)
    return ei.value.code, ei.value.message


def _enc(x):
    return x.encode() if isinstance(x, str) else x


def library(ctx, eds, seds, kw):
    """PathSession.align with the keywords of a case -> (fasta, [missing])"""
    with ctx.paths_open(eds, seds) as s:
        f, m = s.align(**kw)
    return f, [int(x) for x in m]


def spec(eds, seds, kw):
    return ms.align(eds, seds, kw.get("paths"), kw.get("line_width", 60), [_enc(x) for x in kw["names"]] if kw.get("names") else None,
                    _enc(kw.get("prefix") or "path"), _enc(kw.get("gap", "-")))


# ---- the shapes at which the kernel takes another path ------------------------------------------------------------------
def _rand(n, seed):
    rng = np.random.default_rng(seed)
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)])


def many_narrow(n=20000):
    """n symbols of width 1, every third a choice symbol, 3 paths: a tile covers more symbols than the LDS holds"""
    t = _rand(2 * n, 1)
    eds = b"".join(b"{%c,%c}" % (t[2 * i], b"ACGT"[(b"ACGT".index(t[2 * i]) + 1) % 4]) if i % 3 == 0 else b"{%c}" % t[2 * i] for i in range(n))
    seds = b"".join(b"{1}{2,3}" if i % 3 == 0 else b"{0}" for i in range(n))
    return eds, seds


def one_wide(n):
    """{<n chars>,}{A,C}: path 2 takes the empty string and gets n gap bytes across the tile edges"""
    return b"{" + _rand(n, n) + b",}{A,C}", b"{1}{2}{1}{2}"


def zero_widths(lead):
    """symbols whose only string is empty at the start, the end, in runs of three and behind `lead` characters"""
    eds = b"{}{}{}{" + _rand(lead, 5) + b"}{}{}{}{AC,G}{}{T}{}{,}{}{GGA,}{}{}{}"
    seds = b"{0}{0}{0}{0}{0}{0}{0}{1}{2}{0}{0}{0}{1}{2}{0}{1}{2}{0}{0}{0}"
    return eds, seds


def _boundary():
    out = []
    e, s = many_narrow()
    for lw in (0, 60):
        out.append(("narrow lw %d" % lw, e, s, dict(line_width=lw)))
    out.append(("narrow lw 16383 gap", e, s, dict(line_width=16383, gap=".", paths=[3, 1])))
    for n in (2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 40000):
        e, s = one_wide(n)
        out.append(("wide %d lw 0" % n, e, s, dict(line_width=0)))
        out.append(("wide %d lw 60" % n, e, s, dict(line_width=60, gap="N", prefix="s")))
    # with the header ">path1\n" in front, the string's end also meets the 16-byte chunks at every phase
    for n in range(TILE - 9, TILE + 9, 3):
        e, s = one_wide(n)
        out.append(("wide %d lw 17" % n, e, s, dict(line_width=17, paths=[2, 1, 2])))
    for lead in (5, TILE - 1, TILE, TILE + 1):
        e, s = zero_widths(lead)
        for lw in (0, 16):
            out.append(("zero widths %d lw %d" % (lead, lw), e, s, dict(line_width=lw, gap="*")))
    out.append(("missing", b"{AC}{G,TTTTTTTTTTTTTTTTTTTT}{A}{C,}", b"{0}{1}{3}{0}{1}{3}", dict(line_width=0)))
    out.append(("missing lw 5", b"{AC}{G,TTTTTTTTTTTTTTTTTTTT}{A}{C,}", b"{0}{1}{3}{0}{1}{3}", dict(line_width=5, paths=[2, 2, 3])))
    out.append(("one path", b"{AC}{GTT}", b"{0}{1}", dict(line_width=2)))
    out.append(("no column", b"{}{,}", b"{0}{1}{2}", dict(line_width=60)))
    out.append(("names", b"{ACGTAC}{A,ACA,}{CGTTTTT}{,T}{GG}{C,G}{TTTTTTTTTT}", b"{0}{1,3}{2}{4}{0}{1,2}{3,4}{0}{1,2,3}{4}{0}",
                dict(line_width=7, paths=[4, 1, 4, 2], names=["x", "row two|y", "z", "a b"])))
    return out


BOUNDARY = _boundary()


@pytest.mark.parametrize("case", BOUNDARY, ids=[c[0] for c in BOUNDARY])
def test_boundary_shapes(ctx, case):
    name, eds, seds, kw = case
    want = spec(eds, seds, kw)
    assert library(ctx, eds, seds, kw) == want
    f, m, info = ctx.eds_msa(eds, seds, **kw)
    assert (f, [int(x) for x in m]) == want and info == ms.info(eds, seds)


def test_shapes_are_what_they_claim(ctx):
    e, s = many_narrow()
    with ctx.paths_open(e, s) as ses:
        i = ses.align_info()
        assert i == ms.info(e, s) and i["n_columns"] == i["n_symbols"] == 20000 and i["widest_symbol"] == 1 and i["num_paths"] == 3
        assert ses.info["n_choice_symbols"] == 6667
    e, s = zero_widths(TILE)
    with ctx.paths_open(e, s) as ses:
        assert ses.align_info() == ms.info(e, s) and ses.align_info()["n_zero_width_symbols"] == 13
    e, s = one_wide(40000)
    f, m = library(ctx, e, s, dict(line_width=0, paths=[2]))
    assert f == b">path2\n" + b"-" * 40000 + b"C\n" and m == [0]


# ---- fixtures ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["merge", "vcf"])
def test_fixture_sets_line_widths_around_the_chunk(ctx, which):
    ran = 0
    for k, (eds, seds) in enumerate(merge_fixture_inputs() if which == "merge" else vcf_fixture_outputs()):
        try:
            syms, sets, P = ps.parse(eds, seds)
        except ValueError:
            continue
        W = sum(ms.widths(syms))
        with ctx.paths_open(eds, seds) as s:
            assert s.align_info() == ms.info(eds, seds)
            for lw in (0, 1, 15, 16, 17, 60, W + 5):
                want = ms.align(eds, seds, None, lw, gap=b".")
                f, m = s.align(None, lw, gap=".")
                assert f == want[0] and list(m) == want[1], (eds, seds, lw)
            assert s.align(None, 60)[0] == ms.align(eds, seds, None, 60)[0]          # the default gap
            assert s.align(None, 60, gap=0)[0] == ms.align(eds, seds, None, 60)[0]
            if k % 5 == 0 and P >= 1:
                req = [P, 1, P, (P + 1) // 2, 1]                # unordered, with duplicates
                names = [b"row %d|x" % i for i in range(len(req))]
                f, m = s.align(req, 7, names=names, gap="~")
                assert (f, list(m)) == ms.align(eds, seds, req, 7, names=names, gap=b"~")
                f, m = s.align(req, 16, prefix="s")
                assert (f, list(m)) == ms.align(eds, seds, req, 16, prefix=b"s")
                f, m, _ = ctx.eds_msa(eds, seds, req, 3, gap=b"\xff")
                assert (f, list(m)) == ms.align(eds, seds, req, 3, gap=b"\xff")
        ran += 1
    assert ran >= 100


def test_empty_eds(ctx):
    """An empty EDS has no string for a source set to belong to, and the tokenisers refuse both an empty .seds and one
    with a set: what edsx_paths_open says about it (tests/test_paths_gpu.py pins that), edsx_eds_msa says too.  No input
    is known that opens a session with n == 0, so the branch below that handles one, and with it the n == 0 path of
    align_open / align, is not run by this test; it is kept for the day the open takes such an input."""
    import edsparser_amd
    for seds in (b"", b"{0}"):
        try:
            s = ctx.paths_open(b"", seds)
        except edsparser_amd.EdsxError as ex:
            assert _error(ctx.eds_msa, b"", seds) == (ex.code, ex.message)
            continue
        with s:
            assert s.align_info() == dict(n_symbols=0, n_columns=0, n_zero_width_symbols=0, widest_symbol=0, num_paths=0)
            assert s.align()[0] == b"" and len(s.align()[1]) == 0
            assert _error(s.align, [1]) == (3, "Path id 1 out of range (1..0)")
        f, m, info = ctx.eds_msa(b"", seds)
        assert f == b"" and len(m) == 0 and info["n_columns"] == 0


# ---- batches, errors, sessions ------------------------------------------------------------------------------------------
def test_forced_batches_equal_one_batch(ctx):
    """EDSX_PATHS_BUDGET stands in for the free HBM: tables of one or two paths, outputs of one record per batch."""
    eds, seds, _ = ctx.genrandomeds(400_000, seed=11)
    req = [4, 1, 2, 3, 3, 1, 2]
    with ctx.paths_open(eds, seds) as s:
        nc = s.info["n_choice_symbols"]
        assert nc > 1000
        want = s.align(req, 60)
        assert (want[0], list(want[1])) == ms.align(eds, seds, req, 60)
        t = s.timing
        assert t["bytes_written"] == len(want[0]) and t["copy_ms"] > 0 and t["choose_ms"] > 0
        try:
            for budget in (1, 16 * nc + 64, 2 * (16 * nc + 64), 900_000):
                os.environ["EDSX_PATHS_BUDGET"] = str(budget)
                got = s.align(req, 60)
                assert got[0] == want[0] and list(got[1]) == list(want[1]), budget
        finally:
            del os.environ["EDSX_PATHS_BUDGET"]


def test_errors_leave_the_session_usable(ctx):
    eds, seds = b"{AC}{G,TTT,}{A}", b"{0}{1}{2}{3}{0}"
    assert _error(ctx.eds_msa, eds, None) == (3, "Path spelling needs sources (.seds)")
    other, oseds, _ = ctx.genrandomeds(200_000, seed=4)
    with ctx.paths_open(eds, seds) as s:
        good = ms.align(eds, seds, None, 0)
        for g in ms.BAD_GAPS:
            assert _error(s.align, None, 0, gap=bytes([g])) == (3, "Gap character is not usable in an alignment")
        assert _error(s.align, None, 0, gap=256) == (3, "Gap character is not usable in an alignment")
        assert _error(s.align, None, 0, gap=-1) == (3, "Gap character is not usable in an alignment")
        n = ms.size(eds, seds, None, 0)
        assert n == len(good[0])
        assert _error(s.align, None, 0, max_bytes=n - 1) == (3, "Alignment has %d bytes, above the limit of %d" % (n, n - 1))
        assert s.align(None, 0, max_bytes=n)[0] == good[0]
        n7 = ms.size(eds, seds, [3, 3], 2, names=[b"a", b"bcd"])
        assert _error(s.align, [3, 3], 2, names=["a", "bcd"], max_bytes=n7 - 1) == \
            (3, "Alignment has %d bytes, above the limit of %d" % (n7, n7 - 1))
        assert len(s.align([3, 3], 2, names=["a", "bcd"], max_bytes=n7)[0]) == n7
        assert _error(s.align, [1, 0]) == (3, "Path id 0 out of range (1..3)")
        assert _error(s.align, [4]) == (3, "Path id 4 out of range (1..3)")
        with pytest.raises(ValueError):
            s.align([1, 2], names=["a"])
        ctx.leds_merge(other, oseds, 8)                          # other calls on the context do not touch the session
        ctx.eds_stats(other, oseds)
        f, m = s.align(None, 0)
        assert (f, list(m)) == good
        assert s.spell(None, 0)[0] == ps.fasta(eds, seds, None, 0)[0]                # ... nor does align touch spell
        assert s.align([2], 4, gap=".")[0] == ms.align(eds, seds, [2], 4, gap=b".")[0]
    assert _error(ctx.eds_msa, eds, seds, None, 0, max_bytes=n - 1) == (3, "Alignment has %d bytes, above the limit of %d" % (n, n - 1))
    assert _error(ctx.eds_msa, eds, seds, [9]) == (3, "Path id 9 out of range (1..3)")


# ---- the round trip through msa2eds on the device -----------------------------------------------------------------------
def test_round_trip_through_msa_transform(ctx):
    """E from a 64-row x 20 000-column synthetic alignment: msa2eds(align(E)) keeps every path's sequence, and its own
    alignment is align(E) again (every string of an msa2eds result is taken by some path)."""
    import torch
    import edsparser_amd
    S, L = 64, 20000
    n = edsparser_amd.synth_size(S, L)
    buf = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    ctx.msa_synth_device(buf.data_ptr(), n, S, L)
    torch.cuda.synchronize()
    msa = bytes(buf.cpu().numpy())
    for l in (0, 3):
        eds, seds = ctx.msa_transform(msa, l)
        with ctx.paths_open(eds, seds) as s:
            assert s.info["num_paths"] == S
            a1, m1 = s.align(None, 0)
            seqs = s.spell(None, 0)[0]
        assert not m1.any()
        rows = ms.rows_of(a1)
        assert len(rows) == S and len({len(r) for _, r in rows}) == 1
        assert b"".join(b">%s\n%s\n" % (nm, r.replace(b"-", b"")) for nm, r in rows) == seqs
        eds2, seds2 = ctx.msa_transform(a1, 0)
        with ctx.paths_open(eds2, seds2) as s:
            assert s.spell(None, 0)[0] == seqs
            a2, m2 = s.align(None, 0)
        assert a2 == a1 and not m2.any()
    small, ssmall = ctx.msa_transform(b">a\nAC-GT\n>b\nACTG-\n>c\nA--GT\n", 0)
    assert library(ctx, small, ssmall, dict(line_width=0)) == ms.align(small, ssmall, None, 0)


# ---- the tool and the C++ shim ------------------------------------------------------------------------------------------
def _build_host():
    subprocess.run(["make", "-s", "-C", HOST], check=True)        # (libedsx.so itself comes from build())


def test_eds2msa_cli(ctx, tmp_path):
    _build_host()
    exe = os.path.join(BUILD, "eds2msa")
    eds, seds, _ = ctx.genrandomeds(1_500_000, seed=21)
    (tmp_path / "g.eds").write_bytes(eds)
    (tmp_path / "g.seds").write_bytes(seds)
    # a path without a string at some symbol: one warning per such path; names from a file
    (tmp_path / "m.eds").write_bytes(b"{AC}{G,T}{A}{C,}")
    (tmp_path / "m.seds").write_bytes(b"{0}{1}{3}{0}{1}{3}")
    (tmp_path / "names.txt").write_text("alpha\nbeta\ngamma one\n")
    g = ["-i", str(tmp_path / "g.eds")]
    runs = {"whole": g + ["--batch-mb", "4"],
            "a": g + ["-s", str(tmp_path / "g.seds"), "-o", str(tmp_path / "a.msa"), "-p", "1-2"],
            "b": g + ["-o", str(tmp_path / "b.msa"), "-p", "3-4"],
            "limit": g + ["-o", str(tmp_path / "l.msa"), "--max-mb", "2"],
            "range": g + ["-o", str(tmp_path / "r.msa"), "-p", "5"],
            "m": ["-i", str(tmp_path / "m.eds"), "--names", str(tmp_path / "names.txt"), "-w", "3", "--gap", ".", "--prefix", "hap"]}
    procs = {k: subprocess.Popen([exe] + v, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for k, v in runs.items()}
    res = {k: (p.communicate(), p.returncode) for k, p in procs.items()}           # the six tools run side by side
    with ctx.paths_open(eds, seds) as s:
        assert s.info["num_paths"] == 4
        whole = s.align([1, 2, 3, 4], 0, names=["s0", "s1", "s2", "s3"])[0]
        W = s.align_info()["n_columns"]
    assert 1_400_000 < W < 2_090_000                             # two rows per 4 MiB batch, not three
    (out, err), rc = res["whole"]
    assert rc == 0, err
    assert "EDS → MSA alignment export" in out and "Alignment complete!" in out, out
    assert "Rows written: 4 in 2 batches, %d bytes" % len(whole) in out and "columns: %d, paths: 4" % W in out
    assert "[Performance] Runtime:" in err
    assert (tmp_path / "g.msa").read_bytes() == whole             # two batches equal the one call
    assert res["a"][1] == 0 and res["b"][1] == 0, (res["a"], res["b"])
    assert "Rows written: 2 in 1 batch," in res["a"][0][0]
    assert (tmp_path / "a.msa").read_bytes() + (tmp_path / "b.msa").read_bytes() == whole      # -p 1-2, then -p 3-4: -p 1-4
    assert res["limit"][1] == 1 and "above the limit of 2 (--max-mb)" in res["limit"][0][1] and not (tmp_path / "l.msa").exists()
    assert res["range"][1] == 1 and "Error: Path id 5 out of range (1..4)" in res["range"][0][1] and not (tmp_path / "r.msa").exists()
    (out, err), rc = res["m"]
    assert rc == 0, err
    assert err.count("Warning:") == 1 and "Warning: path 2 has no string in 2 symbols" in err
    assert (tmp_path / "m.msa").read_bytes() == b">alpha\nACG\nAC\n>beta\nAC.\nA.\n>gamma one\nACT\nA.\n"
    r = subprocess.run([exe, "-i", str(tmp_path / "g.eds"), "--gap", ","], capture_output=True, text=True)      # (before any device work)
    assert r.returncode == 1 and "Error: Gap character is not usable in an alignment" in r.stderr


def test_eds_to_msa_cpp_shim(ctx, tmp_path):
    _build_host()
    exe = os.path.join(BUILD, "test_msa_export")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, os.path.join(ROOT, "tests", "cpp", "test_msa_export.cpp"),
                    os.path.join(BUILD, "libedsparser_lib.a"), "-L", LIBDIR, "-ledsx", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    eds, seds = b"{ACGTAC}{A,ACA,}{CGTTTTT}{,T}{GG}{C,G}{TTTTTTTTTT}{}", b"{0}{1,3}{2}{4}{0}{1,2}{3,4}{0}{1,2,3}{4}{0}{0}"
    n = ms.size(eds, seds, None, 7)
    cmds = [(b"M", eds, seds, b"7", b"-", b"-", b"path", b"-", b"0"), (b"M", eds, seds, b"0", b"4,1,4", b"-", b"s", b".", b"0"),
            (b"M", eds, seds, b"60", b"2,3", b"x,y z", b"path", b"-", b"0"), (b"M", eds, seds, b"60", b"5", b"-", b"path", b"-", b"0"),
            (b"M", eds, seds, b"60", b"1", b"-", b"path", b",", b"0"), (b"M", eds, seds, b"7", b"-", b"-", b"path", b"-", b"%d" % (n - 1)),
            (b"M", eds, seds, b"7", b"-", b"-", b"path", b"-", b"%d" % n)]
    (tmp_path / "cmds.txt").write_bytes(b"".join(b"\t".join(c) + b"\n" for c in cmds))
    r = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split(b"\n")[:-1]
    i = ms.info(eds, seds)
    tail = b"#%d,%d,%d,%d,%d" % (i["n_symbols"], i["n_columns"], i["n_zero_width_symbols"], i["widest_symbol"], i["num_paths"])
    assert out[0].replace(b"|", b"\n") == ms.align(eds, seds, None, 7)[0] + b"#0,0,0,0" + tail
    assert out[1].replace(b"|", b"\n") == ms.align(eds, seds, [4, 1, 4], 0, prefix=b"s", gap=b".")[0] + b"#0,0,0" + tail
    assert out[2].replace(b"|", b"\n") == ms.align(eds, seds, [2, 3], 60, names=[b"x", b"y z"])[0] + b"#0,0" + tail
    assert out[3] == b"invalid_argument:Path id 5 out of range (1..4)"
    assert out[4] == b"invalid_argument:Gap character is not usable in an alignment"
    assert out[5] == b"invalid_argument:Alignment has %d bytes, above the limit of %d" % (n, n - 1)
    assert out[6] == out[0]
