"""GPU: edsx_paths_* (k_path_choose / k_path_copy) against the Python restatement of the specification
(tests/path_spec.py): fixtures with every line width, names, prefixes, duplicate / unordered / empty requests, host
tokenised inputs, errors, sessions next to other calls, forced batches, round trips at size against the INPUT alignment
(64 x 10 Mb, and 5 x 10^9 so that the FASTA passes 4 GiB), a 10 Mbp genrandomeds EDS before and after the LINEAR merge, a
VCF of BASELINE configs[3]'s shape at 1/100, the eds2fasta tool and the edsparser::eds_to_fasta shim."""
import os
import subprocess

import numpy as np
import pytest

import path_spec as ps
from test_paths_cpu import BUILD, HOST, INC, LIBDIR, ROOT, merge_fixture_inputs, vcf_fixture_outputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    return edsparser_amd.Context(0)


def _parseable(inputs):
    out = []
    for e, s in inputs:
        try:
            ps.parse(e, s)
        except ValueError:
            continue
        out.append((e, s))
    return out


def _error(fn, *a, **kw):
    import edsparser_amd
    with pytest.raises(edsparser_amd.EdsxError) as ei:
        fn(*a, **kw)
    return ei.value.code, ei.value.message


# ---- fixtures ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["merge", "vcf"])
def test_fixture_sets_every_line_width(ctx, which):
    inputs = _parseable(merge_fixture_inputs() if which == "merge" else vcf_fixture_outputs())
    assert len(inputs) >= 100
    for k, (eds, seds) in enumerate(inputs):
        with ctx.paths_open(eds, seds) as s:
            syms, sets, P = ps.parse(eds, seds)
            info = s.info
            assert (info["n_symbols"], info["n_strings"], info["num_paths"]) == (len(syms), len(sets), P)
            assert info["n_chars"] == sum(len(x) for strings in syms for x in strings)
            for lw in (0, 1, 7, 60):
                want, miss = ps.fasta(eds, seds, None, lw)
                got, gm = s.spell(None, lw)
                assert got == want and list(gm) == miss, (eds, seds, lw)
            ln, ms = s.lengths()
            assert [(int(a), int(b)) for a, b in zip(ln, ms)] == [(len(q), m) for q, m in (ps.spell(syms, sets, p) for p in range(1, P + 1))]
            if k % 5 == 0 and P >= 1:
                req = [P, 1, P, (P + 1) // 2, 1]                # unordered, with duplicates
                names = [b"row %d|x" % i for i in range(len(req))]
                assert s.spell(req, 7, names=names) == tuple_of(ps.fasta(eds, seds, req, 7, names=names))
                assert s.spell(req, 60, prefix="sample_") == tuple_of(ps.fasta(eds, seds, req, 60, prefix=b"sample_"))
                assert s.spell([], 60)[0] == ps.fasta(eds, seds, None, 60)[0]      # an empty request: all paths
                assert ctx.eds_spell_paths(eds, seds, req, 3) == tuple_of(ps.fasta(eds, seds, req, 3))
                one_shot, om = ctx.eds_spell_paths(eds, seds)
                assert one_shot == ps.fasta(eds, seds)[0] and list(om) == ps.fasta(eds, seds)[1]


class tuple_of:
    """(fasta, missing list) comparable with (bytes, numpy array)"""

    def __init__(self, pair):
        self.pair = pair

    def __eq__(self, other):
        return other[0] == self.pair[0] and list(other[1]) == self.pair[1]


def test_inputs_for_the_host_tokeniser_give_equal_results(ctx):
    plain = (b"{ACGT}{A,ACA,}{CGTTTTT}{,T}{GG}{C,G}{TTTTTTTTTT}", b"{0}{1,3}{2}{4}{0}{1,2}{3,4}{0}{1,2,3}{4}{0}")
    odd = (b"{AC GT}{A,A CA,}\n{CGTTTTT}{,T}{GG}\t{C,G}{TTTTT TTTTT}\n", b"{0}{1, 3}{2}{4}\n{0}{1,2}{3,4}{0}{1,2,3}{4}{0}\n")
    with ctx.paths_open(*plain) as a, ctx.paths_open(*odd) as b:
        assert a.info["tokenised_on_device"] == 1 and b.info["tokenised_on_device"] == 0
        assert {k: v for k, v in a.info.items() if k != "tokenised_on_device"} == \
               {k: v for k, v in b.info.items() if k != "tokenised_on_device"}
        for lw in (0, 1, 7, 60):
            fa, ma = a.spell(None, lw)
            fb, mb = b.spell(None, lw)
            assert fa == fb == ps.fasta(*plain, None, lw)[0] and list(ma) == list(mb) == ps.fasta(*plain, None, lw)[1]
    compact = (b"ACGT{A,ACA,}CGTTTTT{,T}GG{C,G}TTTTTTTTTT", plain[1])                # the compact form: bare strings
    with ctx.paths_open(*compact) as c:
        assert c.spell(None, 60)[0] == ps.fasta(*plain, None, 60)[0]


def test_errors(ctx):
    import edsparser_amd
    eds, seds = b"{AC}{G,T}{A}", b"{0}{1}{2,3}{0}"
    assert _error(ctx.paths_open, eds, None) == (3, "Path spelling needs sources (.seds)")
    assert _error(ctx.eds_spell_paths, eds, None, [1]) == (3, "Path spelling needs sources (.seds)")
    with ctx.paths_open(eds, seds) as s:
        assert s.info["num_paths"] == 3
        assert _error(s.spell, [1, 0]) == (3, "Path id 0 out of range (1..3)")
        assert _error(s.spell, [4]) == (3, "Path id 4 out of range (1..3)")
        assert _error(s.lengths, [2, 2**40]) == (3, "Path id %d out of range (1..3)" % 2**40)
        assert s.spell([3], 0)[0] == b">path3\nACTA\n"             # ... and the session still answers
    assert _error(ctx.eds_spell_paths, eds, seds, [9]) == (3, "Path id 9 out of range (1..3)")
    # malformed texts: the codes and texts of edsx_leds_merge
    bad = [(b"{A,C}{G", b"{1}{2}{0}"), (b"{A,C}}{G}", b"{1}{2}{0}"), (b"{A,C}{G}", b"{1}{2}"), (b"{A,C}{G}", b"{1}{2}{0}{3}"),
           (b"{A,C}{G}", b"{1}{x}{0}"), (b"{A,C}{G}", b"{1}{}{0}"), (b"{A,C}{G}", b"{1}{2}{0"), (b"{A,C}{G}", b""),
           (b"{A,C}{G}", b" \n"), (b"{A,C}{{G}", b"{1}{2}{0}"), (b"{A,C}{G}", b"1}{2}{0}")]
    refused = 0
    for e, q in bad:
        try:
            ctx.leds_merge(e, q, 1)
        except edsparser_amd.EdsxError as ex:
            assert _error(ctx.paths_open, e, q) == (ex.code, ex.message), (e, q)
            refused += 1
        else:                                                    # what the merge's tokenisers take, these take too
            ctx.paths_open(e, q).close()
    assert refused >= 8
    # an empty EDS has no paths
    try:
        ctx.leds_merge(b"", b"{0}", 1)
        merge_ok = True
    except edsparser_amd.EdsxError as ex:
        merge_ok, want = False, (ex.code, ex.message)
    if merge_ok:
        with ctx.paths_open(b"", b"{0}") as s:
            assert s.info["num_paths"] == 0 and s.spell()[0] == b""
            assert _error(s.spell, [1]) == (3, "Path id 1 out of range (1..0)")
    else:
        assert _error(ctx.paths_open, b"", b"{0}") == want


def test_session_survives_other_calls_on_the_context(ctx):
    eds, seds, _ = ctx.genrandomeds(200_000, seed=3)
    other, oseds, _ = ctx.genrandomeds(300_000, seed=4)
    with ctx.paths_open(eds, seds) as s, ctx.paths_open(other, oseds) as t:
        first = s.spell(None, 60)
        ctx.leds_merge(other, oseds, 8)
        ctx.eds_stats(other, oseds)
        ctx.eds_genpatterns(other, 100, 20, 1)
        assert t.spell([2], 0)[0] == ps.fasta(other, oseds, [2], 0)[0]
        again = s.spell(None, 60)
        assert again[0] == first[0] == ps.fasta(eds, seds, None, 60)[0] and list(again[1]) == list(first[1])


def test_forced_batches_equal_one_batch(ctx):
    """EDSX_PATHS_BUDGET stands in for the free HBM: tables of one or two paths, outputs of one record per batch."""
    eds, seds, _ = ctx.genrandomeds(400_000, seed=11)
    req = [4, 1, 2, 3, 3, 1, 2]
    with ctx.paths_open(eds, seds) as s:
        nc = s.info["n_choice_symbols"]
        assert nc > 1000
        want = s.spell(req, 60)
        assert want[0] == ps.fasta(eds, seds, req, 60)[0]
        try:
            for budget in (1, 16 * nc + 64, 2 * (16 * nc + 64), 900_000):
                os.environ["EDSX_PATHS_BUDGET"] = str(budget)
                got = s.spell(req, 60)
                assert got[0] == want[0] and list(got[1]) == list(want[1]), budget
                ln, ms = s.lengths(req)
                assert list(ms) == list(want[1]) and [int(x) for x in ln] == [len(ps.spell(*ps.parse(eds, seds)[:2], p)[0]) for p in req]
        finally:
            del os.environ["EDSX_PATHS_BUDGET"]


# ---- round trips at size ----------------------------------------------------------------------------------------------
def _records(fa):
    """[(name, sequence as a numpy view)] of a FASTA with one line per sequence (numpy uint8)."""
    nl = np.flatnonzero(fa == 10)
    assert len(nl) % 2 == 0
    out, start = [], 0
    for k in range(0, len(nl), 2):
        assert fa[start] == ord(">")
        out.append((bytes(fa[start + 1:nl[k]]), fa[nl[k] + 1:nl[k + 1]]))
        start = nl[k + 1] + 1
    assert start == len(fa)
    return out


def _msa_round_trip(ctx, S, L, ls):
    import torch
    import edsparser_amd
    n = edsparser_amd.synth_size(S, L)
    buf = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    ctx.msa_synth_device(buf.data_ptr(), n, S, L)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    nl = np.flatnonzero(host == 10)                              # one header line and one row line per sequence
    assert len(nl) == 2 * S
    rows = []
    for r in range(S):
        row = host[nl[2 * r] + 1:nl[2 * r + 1]]
        assert len(row) == L
        rows.append(row[row != ord("-")])
    for l in ls:
        E, Q = ctx.msa_plan_device(buf.data_ptr(), n, l)
        d_eds = torch.empty(E + 16, dtype=torch.uint8, device="cuda:0")
        d_seds = torch.empty(Q + 16, dtype=torch.uint8, device="cuda:0")
        ctx.msa_emit_device(d_eds.data_ptr(), d_seds.data_ptr())
        torch.cuda.synchronize()
        eds, seds = d_eds[:E].cpu().numpy().tobytes(), d_seds[:Q].cpu().numpy().tobytes()
        del d_eds, d_seds
        with ctx.paths_open(eds, seds) as s:
            del eds, seds
            assert s.info["num_paths"] == S
            fa, miss = s.spell(None, 0, as_numpy=True)
            t = s.timing
            print("S=%d L=%d l=%d: %d FASTA bytes, tokenise %.1f choose %.2f scan %.2f copy %.2f download %.1f ms" %
                  (S, L, l, len(fa), t["tokenise_ms"], t["choose_ms"], t["scan_ms"], t["copy_ms"], t["download_ms"]))
        assert not miss.any()
        recs = _records(fa)
        assert len(recs) == S                                    # no row is skipped
        for r, (name, seq) in enumerate(recs):
            assert name == b"path%d" % (r + 1)
            assert len(seq) == len(rows[r]) and np.array_equal(seq, rows[r]), (l, r)
        del fa, recs
    return rows


def test_msa_round_trip_64_rows_10mb(ctx):
    """BASELINE configs[1]: every path of msa2eds(A), l = 0 and l = 10, is its row of A without gaps."""
    _msa_round_trip(ctx, 64, 10_000_000, (0, 10))


def test_msa_round_trip_above_4gib(ctx):
    """5 rows x 10^9 columns: the FASTA passes 2^32 bytes, so offsets above 4 GiB are written and checked."""
    rows = _msa_round_trip(ctx, 5, 1_000_000_000, (0, 10))
    assert sum(len(r) + 8 for r in rows) > 2**32


def test_genrandomeds_10mbp_and_merge_invariance(ctx):
    eds, seds, sites = ctx.genrandomeds(10_000_000, seed=5)
    syms, sets, P = ps.parse(eds, seds)
    assert P == 4 and sites > 100_000
    want = [ps.spell(syms, sets, p) for p in range(1, P + 1)]
    with ctx.paths_open(eds, seds) as s:
        fa, miss = s.spell(None, 60)
        assert list(miss) == [m for _, m in want]
        assert fa == b"".join(ps.record(b"path%d" % (p + 1), want[p][0], 60) for p in range(P))    # the whole text, not windows
        assert s.spell([3, 1], 0)[0] == b"".join(ps.record(b"path%d" % p, want[p - 1][0], 0) for p in (3, 1))
    leds, lseds = ctx.leds_merge(eds, seds, 32, compact=False)
    with ctx.paths_open(leds, lseds) as s:
        assert s.info["num_paths"] == P
        fa2, miss2 = s.spell(None, 0)
    recs = fa2.split(b"\n")
    left_out = 0
    for p in range(P):
        if want[p][1]:
            left_out += 1
            continue
        assert miss2[p] == 0 and recs[2 * p] == b">path%d" % (p + 1) and recs[2 * p + 1] == want[p][0], p
    print("merge invariance at 10 Mbp: %d of %d paths compared (%d with missing symbols left out)" % (P - left_out, P, left_out))
    assert left_out == sum(1 for _, m in want if m)


def test_genvcf_all_samples(ctx):
    """BASELINE configs[3]'s shape at 1/100: 10 Mb reference, 10^5 records, 8 diploid samples."""
    vcf, fasta = ctx.genvcf(10_000_000, 100_000, 8)
    eds, seds, _ = ctx.vcf_transform(vcf, fasta, 0)
    syms, sets, P = ps.parse(eds, seds)
    assert P >= 8
    with ctx.paths_open(eds, seds) as s:
        fa, miss = s.spell(None, 60)
    want = [ps.spell(syms, sets, p) for p in range(1, P + 1)]
    assert list(miss) == [m for _, m in want]
    assert fa == b"".join(ps.record(b"path%d" % (p + 1), want[p][0], 60) for p in range(P))


# ---- the tool and the C++ shim ----------------------------------------------------------------------------------------
def _build_host():
    subprocess.run(["make", "-s", "-C", HOST], check=True)        # (libedsx.so itself comes from build())


def test_eds2fasta_cli(ctx, tmp_path):
    _build_host()
    exe = os.path.join(BUILD, "eds2fasta")
    eds, seds, _ = ctx.genrandomeds(3_000_000, seed=21)
    (tmp_path / "g.eds").write_bytes(eds)
    (tmp_path / "g.seds").write_bytes(seds)
    with ctx.paths_open(eds, seds) as s:
        r = subprocess.run([exe, "-i", str(tmp_path / "g.eds")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert "EDS → FASTA path spelling" in r.stdout and "Spelling complete!" in r.stdout and "in 1 batch," in r.stdout
        assert "[Performance] Runtime:" in r.stderr
        assert (tmp_path / "g.fa").read_bytes() == s.spell(None, 60)[0]
        # small batches, ranges, another line width
        r = subprocess.run([exe, "-i", str(tmp_path / "g.eds"), "-s", str(tmp_path / "g.seds"), "-o", str(tmp_path / "b.fa"),
                            "-p", "4,1-3,2", "-w", "0", "--batch-mb", "1", "--prefix", "hap"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert "Paths spelled: 5 in 5 batches" in r.stdout
        assert (tmp_path / "b.fa").read_bytes() == s.spell([4, 1, 2, 3, 2], 0, prefix="hap")[0]
        (tmp_path / "names.txt").write_text("alpha\nbeta\ngamma one\ndelta\n")
        r = subprocess.run([exe, "-i", str(tmp_path / "g.eds"), "-o", str(tmp_path / "n.fa"), "-p", "3-4,1", "-w", "80",
                            "--names", str(tmp_path / "names.txt"), "--batch-mb", "5"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "n.fa").read_bytes() == s.spell([3, 4, 1], 80, names=["gamma one", "delta", "alpha"])[0]
    r = subprocess.run([exe, "-i", str(tmp_path / "g.eds"), "-p", "5"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: Path id 5 out of range (1..4)" in r.stderr
    # a path without a string at some symbol: one warning per such path
    (tmp_path / "m.eds").write_bytes(b"{AC}{G,T}{A}{C,}")
    (tmp_path / "m.seds").write_bytes(b"{0}{1}{3}{0}{1}{3}")
    r = subprocess.run([exe, "-i", str(tmp_path / "m.eds")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("Warning:") == 1 and "Warning: path 2 has no string in 2 symbols" in r.stderr
    assert (tmp_path / "m.fa").read_bytes() == b">path1\nACGAC\n>path2\nACA\n>path3\nACTA\n"


def test_eds_to_fasta_cpp_shim(ctx, tmp_path):
    _build_host()
    exe = os.path.join(BUILD, "test_paths")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, os.path.join(ROOT, "tests", "cpp", "test_paths.cpp"),
                    os.path.join(BUILD, "libedsparser_lib.a"), "-L", LIBDIR, "-ledsx", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    eds, seds = b"{ACGTAC}{A,ACA,}{CGTTTTT}{,T}{GG}{C,G}{TTTTTTTTTT}", b"{0}{1,3}{2}{4}{0}{1,2}{3,4}{0}{1,2,3}{4}{0}"
    cmds = [(b"F", eds, seds, b"7", b"-", b"-"), (b"F", eds, seds, b"0", b"4,1,4", b"-"), (b"F", eds, seds, b"60", b"2,3", b"x,y z"),
            (b"F", eds, seds, b"60", b"5", b"-")]
    (tmp_path / "cmds.txt").write_bytes(b"".join(b"\t".join(c) + b"\n" for c in cmds))
    r = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split(b"\n")[:-1]
    assert out[0].replace(b"|", b"\n") == ps.fasta(eds, seds, None, 7)[0] + b"#0,0,0,0"
    assert out[1].replace(b"|", b"\n") == ps.fasta(eds, seds, [4, 1, 4], 0)[0] + b"#0,0,0"
    assert out[2].replace(b"|", b"\n") == ps.fasta(eds, seds, [2, 3], 60, names=[b"x", b"y z"])[0] + b"#0,0"
    assert out[3] == b"invalid_argument:Path id 5 out of range (1..4)"
