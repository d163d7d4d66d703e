"""GPU: edsx_eds_vcf (vcf_export_device.hip) against the Python restatement of its specification
(tests/vcf_export_spec.py), byte for byte in VCF, FASTA, info and error text: hand-written cases and shapes at the kernels'
own boundaries; and against independent machinery: the rows of an alignment through msa2eds, and vcf2eds on its own input
with diploid genotypes and a tri-allelic site; the boundary's contract; the eds2vcf tool."""
import ctypes
import os
import random
import subprocess

import pytest

import path_spec as ps
import vcf_export_spec as vs
from test_paths_cpu import BUILD, HOST, ROOT
from test_subset_cpu import random_eds
from test_vcf_export_cpu import separated_eds

pytestmark = pytest.mark.gpu

T = vs.TILE_PATHS                        # path ids per workgroup of the cell kernels (csrc/vcf_text.hpp)


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    return edsparser_amd.Context(0)


def _text(syms, sets=None):
    eds = b"".join(b"{" + b",".join(s) + b"}" for s in syms)
    if sets is None:
        return eds, None
    return eds, b"".join(b"{" + b",".join(b"%d" % p for p in sorted(s)) + b"}" for s in sets)


INFO_KEYS = ("symbols", "strings", "paths", "records", "anchored", "overlapping", "ref_length", "header_bytes", "body_bytes")


def library(ctx, eds, seds, kw):
    """-> (vcf, fasta, info) or ("ERR", code, text)"""
    import edsparser_amd
    kw = {k: ([x.decode() for x in v] if k == "names" else v.decode() if isinstance(v, bytes) else v) for k, v in kw.items()}
    try:
        vcf, fa, info = ctx.eds_vcf(eds, seds, **kw)
    except edsparser_amd.EdsxError as ex:
        return ("ERR", ex.code, ex.message)
    return vcf, fa, {k: info[k] for k in INFO_KEYS}


def spec(eds, seds, kw):
    try:
        return vs.export(eds, seds, **kw)
    except ValueError as ex:
        text = str(ex)
        code = 2 if text.startswith("Symbol") else 4 if text.startswith("VCF body") else 3
        return ("ERR", code, text)


def check(ctx, eds, seds, **kw):
    want = spec(eds, seds, kw)
    got = library(ctx, eds, seds, kw)
    assert got == want, (eds[:200], seds and seds[:200], kw)
    return want


def word(rng, lo, hi=None):
    return bytes(rng.choice(b"ACGT") for _ in range(rng.randint(lo, lo if hi is None else hi)))


def wide_symbol(rng, k, P, everyone=False):
    """[common][k strings][common]: every path in all k strings, or every string with a random set (one with 0)"""
    strings = [word(rng, 0 if j == k // 2 else 1, 3) for j in range(k)]
    allp = set(range(1, P + 1))
    sets = [allp if everyone else ({0} if j == 1 and k > 2 else set(rng.sample(range(1, P + 1), rng.randint(1, min(P, 3))))) for j in range(k)]
    if not everyone:
        sets[-1] = sets[-1] | {P}
    return _text([[b"ACGTAC"], strings, [b"GT"]], [{0}] + sets + [{0}])


def pos_ladder():
    """SNPs at POS 9, 10, 11, 99, 100, 101 and 999 999, 1 000 000, 1 000 001"""
    syms, sets, at = [], [], 0
    for pos in (9, 10, 11, 99, 100, 101, 999_999, 1_000_000, 1_000_001):
        if pos - 1 > at:
            syms.append([b"A" * (pos - 1 - at)]); sets.append({0})
        syms.append([b"C", b"G"]); sets += [{1}, {2}]
        at = pos
    return _text(syms, sets)


def boundary_cases():
    """(name, eds, seds, keyword arguments): the shapes at which the kernels take another path"""
    out = []
    for P in (1, 62, 63, 64, 65, 127, 128, T - 1, T, T + 1, 2 * T + 1):
        rng = random.Random(1000 + P)
        eds, seds = random_eds(rng, P=P, n=200)
        out.append(("P = %d" % P, eds, seds, {}))
    for k in (2, 3, 64, 65, 300):
        out.append(("k = %d" % k,) + wide_symbol(random.Random(k), k, 5) + ({},))
    out.append(("65 strings hold all of %d paths" % (T + 1),) + wide_symbol(random.Random(65), 65, T + 1, everyone=True) + ({},))
    out.append(("one record",) + _text([[b"ACGT"], [b"A", b"CC"], [b"G"]], [{0}, {1}, {2}, {0}]) + ({},))
    out.append(("no record",) + _text([[b"ACGT"], [b"A"]], [{0}, {1, 2}]) + ({},))
    out.append(("empty EDS", b"", None, {}))                     # (an empty .seds is refused by the tokeniser)
    out.append(("empty string in the first symbol",) + _text([[b"", b"AC"], [b"GT"], [b"A", b"C"]], [{1}, {2}, {0}, {1}, {2}]) + ({},))
    out.append(("empty string in the last symbol",) + _text([[b"GT"], [b"A", b"C"], [b"T"], [b"AC", b""]], [{0}, {1}, {2}, {0}, {1}, {2}]) + ({},))
    out.append(("adjacent degenerate symbols",) + _text([[b"A"], [b"C", b""], [b"G", b"T"], [b"", b"TT"], [b"", b"A"], [b"C"]],
                                                        [{0}, {1}, {2}, {1}, {2}, {1}, {2}, {2}, {1}, {0}]) + ({},))
    out.append(("unanchorable",) + _text([[b"", b"A"], [b"", b"C"]], [{1}, {2}, {1}, {2}]) + ({},))
    out.append(("unanchorable, one symbol",) + _text([[b"ACG", b""]], [{1}, {2}]) + ({},))
    out.append(("POS ladder",) + pos_ladder() + ({},))
    for n in (15, 16, 17, 5000):
        rng = random.Random(n)
        for lead in (0, 7):
            syms = [[word(rng, 3 + lead)], [word(rng, n), b"", word(rng, n)], [b"T"], [word(rng, n), word(rng, n + 1)], [b"G"]]
            out.append(("alleles of %d, lead %d" % (n, lead),) + _text(syms, [{0}, {1}, {2}, {3}, {0}, {1, 3}, {2}, {0}]) + (dict(ref_path=lead and 2),))
    eds, seds = separated_eds(random.Random(5), 7)
    for rp in (0, 1, 7, 8):
        out.append(("ref_path %d" % rp, eds, seds, dict(ref_path=rp)))
    out.append(("ref_path takes no string",) + _text([[b"A"], [b"C", b"G"], [b"T"]], [{0}, {1}, {3}, {0}]) + (dict(ref_path=2),))
    for lw in (0, 1, 60):
        out.append(("line_width %d" % lw, eds, seds, dict(line_width=lw)))
    out.append(("without sources", eds, None, {}))
    out.append(("ref_path without sources", eds, None, dict(ref_path=1)))
    body = vs.export(eds, seds)[2]["body_bytes"]
    out.append(("max_bytes below", eds, seds, dict(max_bytes=body - 1)))
    out.append(("max_bytes exact", eds, seds, dict(max_bytes=body)))
    out.append(("names and chrom", eds, seds, dict(chrom=b"chr21", names=[b"s%c" % (65 + k) for k in range(7)])))
    out.append(("prefix", eds, seds, dict(prefix=b"hap_")))
    return out


BOUNDARY = boundary_cases()


# ---- (a) byte equality with the specification -----------------------------------------------------------------------------
def test_documented_example(ctx):
    vcf, fa, info = ctx.eds_vcf(b"{AGCT}{T,C}{AG}{G,}{TA}", b"{0}{1,2}{3}{0}{1}{2,3}{0}")
    assert vcf.split(b"\n")[4:] == [b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tpath1\tpath2\tpath3",
                                    b"eds\t5\t.\tT\tC\t.\t.\t.\tGT\t0\t0\t1", b"eds\t7\t.\tGG\tG\t.\t.\t.\tGT\t0\t1\t1", b""]
    assert fa == b">eds\nAGCTTAGGTA\n" and (info["records"], info["anchored"], info["paths"]) == (2, 1, 3)


@pytest.mark.parametrize("case", BOUNDARY, ids=[c[0] for c in BOUNDARY])
def test_boundary_shapes(ctx, case):
    name, eds, seds, kw = case
    want = check(ctx, eds, seds, **kw)
    if name.startswith("unanchorable"):
        assert want == ("ERR", 2, "Symbol 0 has an empty string and no reference base to anchor it")
    if name == "adjacent degenerate symbols":
        assert want[2]["overlapping"] > 0
    if name == "max_bytes below":
        assert want[0] == "ERR" and want[1] == 4
    if name.startswith("65 strings hold all"):
        assert want[2]["body_bytes"] > 2 * vs.STAGE                 # the tile's text does not fit the LDS stage
    if name == "without sources":
        assert all(len(l.split(b"\t")) == 8 for l in want[0].split(b"\n")[4:-1])


def test_random_texts(ctx):
    rng = random.Random(20250613)
    ok = 0
    for k in range(60):
        eds, seds = random_eds(rng) if k % 2 else separated_eds(rng, rng.randint(1, 7))
        P = ps.parse(eds, seds)[2]
        for kw in ({}, dict(ref_path=1), dict(ref_path=P, line_width=rng.choice([0, 1, 7]))):
            ok += check(ctx, eds, seds, **kw)[0] != "ERR"
        check(ctx, eds, None)
    assert ok >= 90


def test_errors_leave_the_context_usable(ctx):
    eds, seds = b"{AC}{G,T}{A}", b"{0}{1}{2,3}{0}"
    for kw in (dict(chrom=b""), dict(chrom=b"a b"), dict(chrom=b"a\tb"), dict(names=[b"x"]), dict(names=[b"x", b"", b"z"]),
               dict(names=[b"x", b"y\tq", b"z"]), dict(ref_path=4)):
        assert check(ctx, eds, seds, **kw)[:2] == ("ERR", 3), kw
    import edsparser_amd
    with pytest.raises(edsparser_amd.EdsxError) as a:
        ctx.eds_vcf(eds, b"{0}{1}{2,3}")
    with pytest.raises(edsparser_amd.EdsxError) as b:
        ctx.paths_open(eds, b"{0}{1}{2,3}")
    assert (a.value.code, a.value.message) == (b.value.code, b.value.message)
    assert check(ctx, eds, seds)[0].endswith(b"\neds\t3\t.\tG\tT\t.\t.\t.\tGT\t0\t1\t1\n")


def test_timing_names_the_kernels(ctx):
    ctx.set_timing(True)
    try:
        ctx.eds_vcf(b"{AC}{G,T}{A}", b"{0}{1}{2}{0}")
        names = {n: c for n, _, c in ctx.get_timing()}
    finally:
        ctx.set_timing(False)
    for k in ("k_vcf_or", "k_vcf_sym", "scan_symbols", "k_vcf_anchor", "k_vcf_fixedlen", "k_vcf_count", "scan_table", "k_vcf_fixed",
              "k_vcf_cells", "k_vcf_ref"):
        assert names.get(k) == 1, names


# ---- (b) against the input of msa2eds -------------------------------------------------------------------------------------
def alignment(rng, rows, cols):
    """Random rows with substitutions and gaps in which no two variant stretches touch and none lies at either end: between
    two stretches there are at least 3 columns that all rows share, so msa2eds emits no adjacent degenerate symbols (that
    is asserted below through info["overlapping"] == 0)."""
    base = [rng.choice("ACGT") for _ in range(cols)]
    out = [list(base) for _ in range(rows)]
    c = 4
    while c < cols - 12:
        w = rng.randint(1, 4)
        for r in range(1, rows):
            kind = rng.random()
            if kind < 0.25:
                for x in range(c, c + w):
                    out[r][x] = rng.choice("ACGT")
            elif kind < 0.45:
                g = rng.randint(1, w)
                a = c + rng.randint(0, w - g)
                out[r][a:a + g] = "-" * g
        if rng.random() < 0.3:                                   # a stretch where row 0 itself has gaps
            out[0][c:c + w] = "-" * w
            if all(out[r][x] == "-" for r in range(rows) for x in range(c, c + w)):
                out[rows - 1][c] = "A"
        c += w + rng.randint(3, 9)
    return ["".join(r) for r in out]


@pytest.mark.parametrize("shape", [(5, 400), (70, 200)], ids=["5x400", "70x200"])
def test_msa_rows_come_back_through_the_vcf(ctx, shape):
    rows = alignment(random.Random(shape[0]), *shape)
    msa = "".join(">s%d\n%s\n" % (i, r) for i, r in enumerate(rows)).encode()
    eds, seds = ctx.msa_transform(msa, 0)
    vcf, fa, info = ctx.eds_vcf(eds, seds, ref_path=1)
    assert info["overlapping"] == 0 and info["paths"] == shape[0] and info["records"] > 10 and info["anchored"] > 3
    ref = vs.fasta_sequence(fa)
    assert ref == rows[0].replace("-", "").encode()
    names, recs = vs.read(vcf)
    assert len(names) == shape[0] and len(recs) == info["records"]
    assert all(len(cell) == 1 for _, _, _, cells in recs for cell in cells)
    for s in range(shape[0]):
        assert vs.apply_sample(ref, recs, s) == rows[s].replace("-", "").encode(), s
    assert (vcf, fa) == vs.export(eds, seds, ref_path=1)[:2]


# ---- (c) round trip through vcf2eds -----------------------------------------------------------------------------------------
def roundtrip_vcf(rng, family):
    """(vcf, fasta): 3 to 5 diploid samples, phased and unphased, SNPs, multi-base substitutions, insertions written with a
    non-empty REF and one tri-allelic site, the records 3 bases and more apart; family 2 adds <DEL> records.  REF and every
    ALT are carried by some sample (vcf2eds writes no string for an allele nobody carries: the EDS would not hold what the
    VCF says, and there would be nothing to compare)."""
    ns = rng.randint(3, 5)
    ref = word(rng, 150)
    lines = [b"##fileformat=VCFv4.2", b"\t".join([b"#CHROM", b"POS", b"ID", b"REF", b"ALT", b"QUAL", b"FILTER", b"INFO", b"FORMAT"] +
                                                  [b"S%d" % k for k in range(ns)])]
    at, k = 3, 0
    while at < 135:
        kinds = ["snp", "mnp", "ins", "tri"] + (["del", "del"] if family == 2 else [])
        kind = "tri" if k == 2 else rng.choice(kinds)
        r = ref[at:at + (rng.randint(2, 3) if kind == "mnp" else 1)]
        other = lambda t: bytes(rng.choice([c for c in b"ACGT" if c != x]) for x in t)
        if kind == "snp":
            alts = [other(r)]
        elif kind == "mnp":
            alts = [other(r) + word(rng, 0, 1)]
        elif kind == "ins":
            alts = [r + word(rng, 1, 3)]
        elif kind == "tri":
            a = other(r)
            alts = [a, bytes(rng.choice([c for c in b"ACGT" if c not in (r[0], a[0])]) for _ in range(1)) + word(rng, 0, 2)]
        else:
            alts = [b"<DEL>"]
        na = len(alts) + 1
        gts = [[rng.randrange(na), rng.randrange(na)] for _ in range(ns)]
        for a in range(na):                                      # every allele is carried
            if not any(a in g for g in gts):
                gts[a % ns][a % 2] = a
        for a in range(na):
            assert any(a in g for g in gts)
        cells = [(b"|" if rng.random() < 0.5 else b"/").join(b"%d" % x for x in g) for g in gts]
        lines.append(b"\t".join([b"chr1", b"%d" % (at + 1), b".", r, b",".join(alts), b"99", b"PASS", b".", b"GT"] + cells))
        at += len(r) + rng.randint(3, 8)
        k += 1
    return b"\n".join(lines) + b"\n", b">chr1\n" + b"\n".join(ref[i:i + 60] for i in range(0, len(ref), 60)) + b"\n"


def spellings(ctx, eds, seds):
    fa, miss = ctx.eds_spell_paths(eds, seds, line_width=0)
    assert not any(miss)
    return fa


@pytest.mark.parametrize("family", [1, 2])
def test_round_trip_through_vcf2eds(ctx, family):
    inputs = [roundtrip_vcf(random.Random(10 * family + s), family) for s in range(4)]
    small = os.path.join(ROOT, "tests", "golden", "ref_data", "vcf", "small")
    if family == 2 and os.path.exists(small + ".vcf"):
        inputs.append((open(small + ".vcf", "rb").read(), open(small + ".fa", "rb").read()))
    empties = 0
    for V0, F0 in inputs:
        e0, s0, st0 = ctx.vcf_transform(V0, F0)
        assert st0["processed_variants"] == st0["total_variants"] >= 10
        V1, F1, info = ctx.eds_vcf(e0, s0)
        assert (V1, F1) == vs.export(e0, s0)[:2]
        assert vs.fasta_sequence(F1) == vs.fasta_sequence(F0)
        e1, s1, st1 = ctx.vcf_transform(V1, F1)
        assert st1["processed_variants"] == st1["total_variants"] == info["records"]
        if family == 1:
            assert info["anchored"] == 0 and (e1, s1) == (e0, s0)
        else:
            empties += info["anchored"]
        assert spellings(ctx, e1, s1) == spellings(ctx, e0, s0)
    assert family == 1 or empties > 0


# ---- (d) the boundary's contract, the tool ---------------------------------------------------------------------------------
def test_contract(ctx):
    """NULL handle, NULL outputs, outs cleared and info zeroed before anything can fail, ref_fasta optional."""
    from edsparser_amd._capi import VcfExportInfo, VcfExportOpts, _Buf
    lib, h = ctx._lib, ctx._h
    eds, seds = b"{AC}{G,T}{A}", b"{0}{1}{2,3}{0}"
    junk = ctypes.create_string_buffer(b"junk")

    def dirty():
        b = _Buf()
        b.data = ctypes.addressof(junk)
        b.size = 4
        return b
    info = VcfExportInfo()
    ctypes.memset(ctypes.byref(info), 0xAB, ctypes.sizeof(info))
    v, f = dirty(), dirty()
    assert lib.edsx_eds_vcf(None, eds, len(eds), seds, len(seds), None, ctypes.byref(v), ctypes.byref(f), ctypes.byref(info)) == 3
    assert (v.size, f.size, bool(v.data), bool(f.data)) == (0, 0, False, False) and info.symbols == 0 and info.tokenised_on_device == 0
    assert lib.edsx_eds_vcf(h, eds, len(eds), seds, len(seds), None, None, ctypes.byref(f), ctypes.byref(info)) == 3   # no vcf out
    assert lib.edsx_last_error(h).decode() == "null argument"
    v, f = dirty(), dirty()
    assert lib.edsx_eds_vcf(h, None, 5, None, 0, None, ctypes.byref(v), ctypes.byref(f), None) == 3
    assert (v.size, f.size, bool(v.data), bool(f.data)) == (0, 0, False, False)
    # a failing call clears the outs; the byte limit fills info in
    v, f = dirty(), dirty()
    opts = VcfExportOpts(None, 0, None, 0, None, 60, 5)
    assert lib.edsx_eds_vcf(h, eds, len(eds), seds, len(seds), ctypes.byref(opts), ctypes.byref(v), ctypes.byref(f), ctypes.byref(info)) == 4
    assert (v.size, f.size, bool(v.data), bool(f.data)) == (0, 0, False, False)
    assert (info.records, info.paths, info.body_bytes) == (1, 3, 27) and "27 bytes is above the limit of 5" in lib.edsx_last_error(h).decode()
    opts = VcfExportOpts(None, 0, None, 2, None, 60, 0)                  # names announced, none given
    assert lib.edsx_eds_vcf(h, eds, len(eds), seds, len(seds), ctypes.byref(opts), ctypes.byref(v), ctypes.byref(f), None) == 3
    # opts NULL = defaults; ref_fasta and info may be NULL
    v = _Buf()
    assert lib.edsx_eds_vcf(h, eds, len(eds), seds, len(seds), None, ctypes.byref(v), None, None) == 0
    want = vs.export(eds, seds)
    assert ctypes.string_at(v.data, v.size) == want[0]
    lib.edsx_buf_free(ctypes.byref(v))
    assert ctx.eds_vcf(eds, seds)[:2] == want[:2]


def test_eds2vcf_cli(ctx, tmp_path):
    subprocess.run(["make", "-s", "-C", HOST], check=True)        # (libedsx.so itself comes from build())
    exe = os.path.join(BUILD, "eds2vcf")
    run = lambda *a: subprocess.run([exe] + [str(x) for x in a], capture_output=True, text=True)
    eds, seds = [c for c in BOUNDARY if c[0] == "adjacent degenerate symbols"][0][1:3]
    g = tmp_path / "g.eds"
    g.write_bytes(eds)
    (tmp_path / "g.seds").write_bytes(seds)
    vcf, fa, info = ctx.eds_vcf(eds, seds)
    r = run("-i", g)                                              # the sources beside the input, the default output names
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "g.vcf").read_bytes() == vcf and (tmp_path / "g.ref.fa").read_bytes() == fa
    assert "Records: %d (%d anchored), samples: 2" % (info["records"], info["anchored"]) in r.stdout and "Export complete!" in r.stdout
    assert "[Performance] Runtime:" in r.stderr
    assert r.stderr.count("Warning") == 1 and "Warning: %d records overlap the record before" % info["overlapping"] in r.stderr
    (tmp_path / "names.txt").write_text("mother\nfather\n")
    r = run("-i", g, "-s", tmp_path / "g.seds", "--chrom", "chr2", "--ref-path", "2", "--names", tmp_path / "names.txt", "--line-width", "3",
            "-o", tmp_path / "x.vcf", "--ref-out", tmp_path / "x.fa")
    assert r.returncode == 0, r.stderr
    want = ctx.eds_vcf(eds, seds, chrom="chr2", ref_path=2, names=["mother", "father"], line_width=3)
    assert ((tmp_path / "x.vcf").read_bytes(), (tmp_path / "x.fa").read_bytes()) == want[:2]
    r = run("-i", g, "--no-samples", "--prefix", "h", "-o", tmp_path / "n.vcf")
    assert r.returncode == 0 and (tmp_path / "n.vcf").read_bytes() == ctx.eds_vcf(eds)[0] and "Sources" not in r.stdout
    r = run("-i", g, "--max-bytes", "10")
    assert r.returncode == 1 and "Error: VCF body of %d bytes is above the limit of 10" % info["body_bytes"] in r.stderr
    assert "[Performance] Runtime:" in r.stderr
    r = run("-i", g, "--ref-path", "9")
    assert r.returncode == 1 and "Error: Path id 9 out of range (1..2)" in r.stderr
    r = run("-i", g, "--no-samples", "--names", tmp_path / "names.txt")
    assert r.returncode == 1 and "--no-samples does not go with" in r.stderr
    r = run("-i", tmp_path / "none.eds")
    assert r.returncode == 1 and "Input file does not exist" in r.stderr
    r = run("--help")
    assert r.returncode == 0 and "--ref-path" in r.stdout and "edsparser-subset" in r.stdout and "not merged" in r.stdout
