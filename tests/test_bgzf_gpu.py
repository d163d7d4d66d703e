"""GPU: gzip / BGZF input (edsx_gz_inflate, edsx_vcf_transform_z, edsx_vcf_session_open_z, vcf2eds on .vcf.gz, edsx-zcat).
The compressed layer is checked against Python's zlib / gzip (tests/bgzf_spec.py), the transforms against the plain
calls on the inflated texts: texts, counters and error text."""
import gzip
import os
import subprocess
import time
import zlib

import pytest

import bgzf_spec as bz
import deflate_spec as ds
import contig_spec as cs
from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "edsparser_amd", "host", "build")
VCF2EDS = os.path.join(BUILD, "vcf2eds")
ZCAT = os.path.join(BUILD, "edsx-zcat")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    c = edsparser_amd.Context(0)
    yield c
    c.close()


def _res(fn):
    import edsparser_amd
    try:
        e, s, st = fn()
        return {"eds": e.decode(), "seds": s.decode(), "stats": st}
    except edsparser_amd.EdsxError as ex:
        return {"error": ex.message}


def _bgzf(text, level=6, payload=bz.MAX_PAYLOAD):
    return bz.write(text, level, payload=payload)[0]


# ---- 1. inflate parity ----------------------------------------------------------------------------------------------
def test_gz_inflate_equals_the_text_for_the_whole_corpus(ctx):
    for name, data, text, kind, table in bz.corpus():
        assert ctx.gz_inflate(data) == text, name
        info = ctx.gz_last_info(0)
        assert info["kind"] == kind and info["inflated_on_device"] == (1 if kind == 1 else 0), (name, info)
        assert info["text_bytes"] == len(text) and info["comp_bytes"] == len(data), (name, info)
        if kind == 1:
            assert info["blocks"] == len(table) and info["h2d_bytes"] == len(data) + 24 * len(table), (name, info)
    for name, text in bz.texts().items():                               # plain input: inflate(x) is x
        assert ctx.gz_inflate(text) == text
        assert ctx.gz_last_info(0)["kind"] == 0


def test_corrupted_streams_are_refused_as_the_host_decoder_refuses_them(ctx, tmp_path):
    """Every damaged input has passed the sanitized host build of the decoder core (bgzf_spec.host_refusals asserts it);
    the device decoder must give the same status and text, each case run once."""
    import edsparser_amd
    want, _ = bz.host_refusals(ROOT, str(tmp_path))
    cases = [(name, data) for name, data, _, _ in bz.damaged_cases()]
    data, flips = bz.flip_positions()
    cases += [("flip%d" % i, bz.flipped(data, at, bit)) for i, (at, bit) in enumerate(flips)]
    assert len(cases) == len(want)
    on_device = 0
    for name, bad in cases:
        with pytest.raises(edsparser_amd.EdsxError) as ex:
            ctx.gz_inflate(bad)
        assert ex.value.code == 2 and ex.value.message == want[name], name
        on_device += edsparser_amd.gz_probe(bad) == 1
    assert on_device >= 3000                                            # the bit flips leave the file BGZF: the device decides


# ---- 1b. streams zlib never writes (tests/deflate_spec.py; the reference is zlib) ---------------------------------------
def test_streams_zlib_never_writes_inflate_to_zlibs_text(ctx):
    """Directed, sized and random members, about 64 to a BGZF file, one call per file; compared member by member through
    the block table so that a failure names the case or the seed."""
    t0 = time.time()
    files = ds.accepted_files()
    cnt = ds.random_corpus()[1]
    t1 = time.time()
    members, bad = 0, []
    for data, table, names in files:
        out = ctx.gz_inflate(data)
        info = ctx.gz_last_info(0)
        assert info["kind"] == 1 and info["inflated_on_device"] == 1 and info["blocks"] == len(table), (names[0][0], info)
        assert info["text_bytes"] == len(out) == table[-1][1], (names[0][0], info)
        for (name, text), (_, off, _, isize) in zip(names, table):
            members += 1
            if out[off:off + isize] != text:
                first = next((i for i in range(min(isize, len(text))) if out[off + i] != text[i]), None)
                bad.append((name, isize, first))
    print("deflate_spec on the device: %d files, %d members, generated in %.1f s, inflated and compared in %.1f s; random corpus %s"
          % (len(files), members, t1 - t0, time.time() - t1, cnt))
    assert not bad, "%d members differ from zlib's text (name, size, first differing byte): %s" % (len(bad), bad[:20])
    assert members == len(ds.accepted_cases())


def test_streams_gzip_refuses_are_refused_as_the_host_decoder_refuses_them(ctx, tmp_path):
    """One fault per file, between two valid members; gzip.decompress raises on every faulty member (deflate_spec.refused
    asserts it).  The device gives the host decoder's status and text, and names block 1; each case runs once."""
    import edsparser_amd
    t0 = time.time()
    code, want, log = ds.host_run(ROOT, str(tmp_path), with_accepted=False)
    assert code == 0, log[-4000:]
    cases = ds.refused_files()
    assert sorted(want) == sorted(name for name, _, _ in cases)
    t1 = time.time()
    for name, bad, reason in cases:
        assert edsparser_amd.gz_probe(bad) == 1, name                       # BGZF: the device decides
        with pytest.raises(edsparser_amd.EdsxError) as ex:
            ctx.gz_inflate(bad)
        assert ex.value.code == 2 and ex.value.message == want[name], (name, ex.value.message, want[name])
        assert ex.value.message.startswith("Compressed input: block 1 at byte ") and ex.value.message.endswith(": " + reason), name
    print("refused streams: %d cases, host decoder %.1f s, device %.1f s" % (len(cases), t1 - t0, time.time() - t1))


def test_far_match_streams_through_the_compressed_transform(ctx):
    """A fixture's VCF and FASTA as one BGZF member each whose matches all reach back 32 507 bytes or more: the records
    stand 32 640 bytes in front of themselves as meta lines, the sequence is followed by unrelated lines and then by itself
    at that distance.  The compressed call must equal the plain one."""
    import random
    c = max(cs.load_fixtures(GOLDEN), key=lambda x: len(x["vcf"]) if "error" not in x["expect"] else 0)
    v, f = c["vcf"].encode(), c["fasta"].encode()
    rng, back = random.Random(5), 32640

    def lines(n, prefix, alphabet, width=60):
        """exactly n bytes of lines"""
        out = b""
        while len(out) < n:
            out += prefix + bytes(rng.choice(alphabet) for _ in range(width)) + b"\n"
        return out[:n - 1] + b"\n"

    records = [ln for ln in v.split(b"\n") if ln and not ln.startswith(b"#")]
    first = v.index(records[0])
    meta = b"".join(b"##" + ln[2:] + b"\n" for ln in records)            # as long as the record lines
    V = meta + lines(back - len(meta) - first, b"##pad=", b"ACGTacgt0123456789|") + v
    head, seq = f.rstrip(b"\n").split(b"\n", 1)
    F = head + b"\n" + seq + b"\n" + lines(back - len(seq) - 1, b"", b"ACGT", len(seq.split(b"\n")[0])) + seq + b"\n"
    files = []
    for text in (V, F):
        assert len(text) <= 65536
        toks = ds.far_lz77(text)
        far = [t for t in toks if not isinstance(t, int)]
        assert len(far) >= 5 and min(t[1] for t in far) > ds.FAR and sum(t[0] for t in far) >= 300, (len(far), len(text))
        blocks = [("dynamic", toks, ds.auto_codes(toks))]
        raw = ds.assemble(blocks)
        assert zlib.decompress(raw, -15) == text == ds.expand(blocks)
        files.append(ds.wrap(raw, text) + bz.EOF_BLOCK)
    plain = _res(lambda: ctx.vcf_transform(V, F, c["l"]))
    assert "error" not in plain, plain
    assert _res(lambda: ctx.vcf_transform(files[0], files[1], c["l"], compressed=True)) == plain
    for which, text in ((0, V), (1, F)):
        info = ctx.gz_last_info(which)
        assert info["kind"] == 1 and info["inflated_on_device"] == 1 and info["blocks"] == 2 and info["text_bytes"] == len(text), info


# ---- 2. the fixtures through the compressed calls ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["both_bgzf", "vcf_only", "fasta_only", "fasta_gzip"])
def test_fixtures_through_compressed_transform_equal_the_plain_call(ctx, shape):
    cases = cs.load_fixtures(GOLDEN)
    assert len(cases) == 366
    for c in cases:
        V, F = c["vcf"].encode(), c["fasta"].encode()
        zv = _bgzf(V, payload=4000) if shape in ("both_bgzf", "vcf_only") else V
        zf = _bgzf(F, payload=3000) if shape in ("both_bgzf", "fasta_only") else gzip.compress(F) if shape == "fasta_gzip" else F
        plain = _res(lambda: ctx.vcf_transform(V, F, c["l"]))
        assert _res(lambda: ctx.vcf_transform(zv, zf, c["l"], compressed=True)) == plain, (shape, c.get("name"))
        assert plain == c["expect"], c.get("name")


def test_compressed_layer_errors_name_the_input(ctx):
    import edsparser_amd
    V, F = b"#h\nchr1\t2\t.\tA\tC\t.\t.\t.\tGT\t0|1\n", b">chr1\nACGTACGT\n"
    bad = bytearray(_bgzf(V)); bad[20] ^= 0x40
    with pytest.raises(edsparser_amd.EdsxError) as ex:
        ctx.vcf_transform(bytes(bad), _bgzf(F), compressed=True)
    assert ex.value.code == 2 and ex.value.message.startswith("Compressed VCF: block 0 at byte 0: ")
    zf = bytearray(_bgzf(F)); zf[-36] ^= 1                              # the CRC in block 0's trailer (the EOF block follows)
    with pytest.raises(edsparser_amd.EdsxError) as ex:
        ctx.vcf_transform(_bgzf(V), bytes(zf), compressed=True)
    assert ex.value.code == 2 and ex.value.message == "Compressed FASTA: block 0 at byte 0: CRC mismatch"


# ---- 3. contig paths ------------------------------------------------------------------------------------------------
def test_composed_contigs_through_a_compressed_session(ctx):
    cases = cs.load_fixtures(GOLDEN)
    done = 0
    for V, F, parts, left in cs.compose(cases, 5):
        zv, zf = _bgzf(V, payload=5000), _bgzf(F, 1, payload=7000)
        with ctx.vcf_session(zv, zf, compressed=True) as ses, ctx.vcf_session(V, F) as plain:
            assert ses.contigs() == plain.contigs()
            assert ses.info()["classified_on_device"] == plain.info()["classified_on_device"]
            assert ses.unknown_contigs() == plain.unknown_contigs()
            for nm, c in parts:
                assert _res(lambda: ses.transform(nm, c["l"])) == c["expect"], (nm, c.get("name"))
                done += 1
        nm, c = parts[0]
        assert _res(lambda: ctx.vcf_transform(zv, F, c["l"], contig=nm, compressed=True)) == c["expect"]
    assert done == 366


def _multi_contig(ctx, n_contigs=3, ref_len=200000, records=4000):
    vs, fs, header = [], [], None
    for k in range(n_contigs):
        v, f = ctx.genvcf(ref_len + 1000 * k, records, 4, 100 + k)
        nm = b"chr%d" % (k + 1)
        lines = v.split(b"\n")
        header = header or [x for x in lines if x.startswith(b"#")]
        vs += [nm + x[x.index(b"\t"):] for x in lines if x and not x.startswith(b"#")]
        fs.append(b">" + nm + b"\n" + f.split(b"\n", 1)[1])
    return b"\n".join(header + vs) + b"\n", b"".join(x if x.endswith(b"\n") else x + b"\n" for x in fs)


def _run(args):
    return subprocess.run(args, capture_output=True, text=True)


def test_cli_on_compressed_files_writes_the_bytes_of_the_plain_run(ctx, tmp_path):
    import torch
    pd, zd = tmp_path / "plain", tmp_path / "z"
    pd.mkdir(); zd.mkdir()

    def put(V, F, ref):
        (pd / "in.vcf").write_bytes(V); (pd / "ref.fa").write_bytes(F)
        (zd / "in.vcf.gz").write_bytes(_bgzf(V))
        (zd / "ref.fa.gz").write_bytes(gzip.compress(F) if ref == "gzip" else _bgzf(F, 1))

    # (flags, contigs, reference): one contig for the runs that ignore CHROM, three for the contig flags; the reference as
    # plain gzip (inflated by the tool) or as BGZF (inflated on the device).  --gpus 1 takes the multi-GPU entry point,
    # in front of which BGZF inputs are inflated on GPU 0; --gpus 2 joins where two devices exist.
    modes = [([], 1, "gzip"), (["-l", "5"], 1, "gzip"), (["--gpus", "1"], 1, "gzip"), (["--gpus", "1"], 1, "bgzf"),
             (["--gpus", "1", "-l", "5"], 1, "bgzf"), ([], 1, "bgzf"),
             (["--chrom", "chr2"], 3, "gzip"), (["--all-chroms"], 3, "gzip"), (["--all-chroms"], 3, "bgzf")]
    if torch.cuda.device_count() >= 2:
        modes += [(["--gpus", "2"], 1, "gzip"), (["--gpus", "2"], 1, "bgzf")]
    state = None
    for extra, k, ref in modes:
        if (k, ref) != state:
            V, F = _multi_contig(ctx, k)
            put(V, F, ref)
            state = (k, ref)
        a = _run([VCF2EDS, "-i", str(pd / "in.vcf"), "-r", str(pd / "ref.fa")] + extra)
        b = _run([VCF2EDS, "-i", str(zd / "in.vcf.gz"), "-r", str(zd / "ref.fa.gz")] + extra)
        assert a.returncode == 0 and b.returncode == 0, (extra, ref, a.stderr, b.stderr)
        assert "Compression: VCF BGZF, " in b.stdout, b.stdout
        assert ("reference gzip (inflated on the host, one thread)" if ref == "gzip" else "reference BGZF, ") in b.stdout, b.stdout
        assert "Compression:" not in a.stdout
        outs = sorted(p.name for p in pd.iterdir() if p.suffix in (".eds", ".seds", ".leds"))
        assert outs and outs == sorted(p.name for p in zd.iterdir() if p.suffix in (".eds", ".seds", ".leds")), extra
        for name in outs:
            assert (pd / name).read_bytes() == (zd / name).read_bytes(), (extra, name)
            (pd / name).unlink(); (zd / name).unlink()
    # edsx-zcat: the text, and the block table
    r = _run([ZCAT, "-i", str(zd / "in.vcf.gz"), "-o", str(tmp_path / "out.vcf")])
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out.vcf").read_bytes() == V
    r = _run([ZCAT, "-i", str(zd / "in.vcf.gz"), "--index"])
    rows = [tuple(map(int, ln.split("\t"))) for ln in r.stdout.splitlines() if ln and not ln.startswith("#")]
    assert r.returncode == 0 and rows == bz.write(V)[1]


# ---- 4. full shape: the text stays in HBM ----------------------------------------------------------------------------
def test_full_shape_compressed_equals_plain_and_the_text_stays_on_the_device(ctx):
    V, F = ctx.genvcf(100_000_000, 1_000_000, 8, 42)                    # 1/10 of BASELINE configs[3]
    zv, tv = bz.write(V, 1)
    zf, tf = bz.write(F, 1)
    plain = ctx.vcf_transform(V, F)
    got = ctx.vcf_transform(zv, zf, compressed=True)
    assert got[2] == plain[2] and got[0] == plain[0] and got[1] == plain[1]
    for which, z, table, text in ((0, zv, tv, V), (1, zf, tf, F)):
        info = ctx.gz_last_info(which)
        print("input %d: %s" % (which, info))
        assert info["kind"] == 1 and info["inflated_on_device"] == 1 and info["blocks"] == len(table)
        assert info["text_bytes"] == len(text)
        assert info["text_d2h_bytes"] < (1 << 20)                       # the text never came back to the host
        assert info["h2d_bytes"] == len(z) + 24 * len(table)            # compressed bytes + block table


# ---- 5. offsets above 4 GiB -------------------------------------------------------------------------------------------
def test_text_beyond_4_gib(ctx):
    """BGZF blocks are independent: one 65280-byte block repeated until the text passes 4.5 GiB."""
    payload = bz.vcf_text(bz.MAX_PAYLOAD, seed=21)
    blk = bz.block(payload, 6)
    reps = (int(4.5 * (1 << 30)) // len(payload)) + 1
    data = blk * reps + bz.EOF_BLOCK
    text = ctx.gz_inflate(data)
    info = ctx.gz_last_info(0)
    assert info["blocks"] == reps + 1 and info["text_bytes"] == reps * len(payload) == len(text) and len(text) > 4.5 * (1 << 30)
    view = memoryview(text)
    chunk = payload * 256
    for off in range(0, len(text), len(chunk)):
        n = min(len(chunk), len(text) - off)
        assert view[off:off + n] == chunk[:n], off
    assert zlib.crc32(view[-len(payload):]) == zlib.crc32(payload)
