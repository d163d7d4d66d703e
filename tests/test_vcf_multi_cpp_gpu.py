"""The C++ multi-GPU path of vcf2eds (edsx_vcf_transform_multi, csrc/vcf_multi.hip): rank threads inside the library,
reference-position ranges, record lines moved between ranks, per-rank FASTA windows.  On the one-GPU box N ranks share
the device and exchange in process (RCCL does not run two ranks on one device); the RCCL exchange runs with one rank.
Expected: the reference's fixtures, the oracle, and the unpartitioned edsx_vcf_transform."""
import json
import os
import random
import subprocess
import sys

import pytest

import oracle_lib as o
from conftest import GOLDEN
from test_vcf_shard_cpu import _random_records, _vcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def multi():
    import edsparser_amd
    made = {}

    def get(n, rccl=False):
        if (n, rccl) not in made:
            made[(n, rccl)] = edsparser_amd.MultiGpu([0] * n, use_rccl=rccl)
        return made[(n, rccl)]
    yield get
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    c = edsparser_amd.Context(0)
    yield c
    c.close()


def _run(m, vcf, fasta, l):
    import edsparser_amd
    try:
        e, s, st = m.vcf_transform(vcf, fasta, l)
        return {"eds": e.decode(), "seds": s.decode(), "stats": st}
    except edsparser_amd.EdsxError as ex:
        return {"error": ex.message}


def _oracle(vcf, fasta, l=0):
    e, s, st = o.vcf(vcf, fasta, l)
    return e, s, st


@pytest.mark.parametrize("name", ["gen_vcf.json", "gen2_vcf.json"])
def test_reference_fixtures(multi, name):
    cases = json.load(open(os.path.join(GOLDEN, name)))["cases"]
    errors = 0
    for i, c in enumerate(cases):
        n = (2, 3, 5)[i % 3]
        got = _run(multi(n), c["vcf"].encode(), c["fasta"].encode(), c["l"])
        assert got == c["expect"], (name, i, n, c.get("name"))
        errors += "error" in c["expect"]
    assert len(cases) in (300, 66)
    if name == "gen_vcf.json":
        assert errors == 16


@pytest.mark.parametrize("seed", range(4))
def test_random_sorted_shuffled_duplicates(multi, seed):
    rng = random.Random(4000 + seed)
    ref = "".join(rng.choice("ACGT") for _ in range(rng.randint(2000, 6000)))
    for dup in (0.0, 0.3):
        recs = _random_records(rng, ref, rng.randint(150, 400), rng.choice([1, 3, 8]), dup_frac=dup)
        for shuffle in (None, rng):
            for lw in (60, 7):
                vcf, fasta = _vcf(ref, recs, len(recs[0][3]), lw=lw, shuffle=shuffle)
                want = _oracle(vcf, fasta)
                for n in (2, 4):
                    m = multi(n)
                    assert m.vcf_transform(vcf, fasta) == want, (seed, dup, shuffle is not None, lw, n)
                    info = m.last_vcf()
                    assert info["records_min"] >= 1
                    if shuffle is None and dup == 0.0:
                        assert info["partitioned"]


def test_degenerate_shapes(multi, ctx):
    rng = random.Random(9)
    ref = "".join(rng.choice("ACGT") for _ in range(600))
    fasta = (">c\n" + "\n".join(ref[i:i + 60] for i in range(0, len(ref), 60)) + "\n").encode()
    hdr = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS0\n"
    wrap = hdr + b"c\t0\t.\tA\tG\t.\t.\t.\tGT\t0|1\nc\t5\t.\tA\tC\t.\t.\t.\tGT\t1|1\nc\t90\t.\tA\tT\t.\t.\t.\tGT\t0|1\nc\t300\t.\tA\tG\t.\t.\t.\tGT\t1|0\n"
    few = hdr + b"c\t7\t.\tG\tT\t.\t.\t.\tGT\t0|1\nc\t400\t.\tA\tG\t.\t.\t.\tGT\t1|1\n"
    one_del = hdr + ("c\t2\t.\t%s\t%s\t.\t.\t.\tGT\t0|1\nc\t20\t.\t%s\tG\t.\t.\t.\tGT\t1|1\nc\t590\t.\t%s\tT\t.\t.\t.\tGT\t1|0\n"
                     % (ref[1:595], ref[1], ref[19], ref[589])).encode()
    spaces = hdr + b"c 7 . G T . . . GT 0|1\nc\t400\t.\tA\tG\t.\t.\t.\tGT\t1|1\nc\t500\t.\tA\t<INV>\t.\t.\t.\tGT\t1|1\nbadline\n"
    for vcf in (b"", hdr, wrap, few, one_del, spaces):
        want = _oracle(vcf, fasta)
        assert ctx.vcf_transform(vcf, fasta) == want
        for n in (2, 5):
            m = multi(n)
            assert m.vcf_transform(vcf, fasta) == want, (vcf[:200], n)
            info = m.last_vcf()
            if vcf is wrap:
                assert not info["partitioned"]
            if vcf in (b"", hdr, one_del):
                assert not info["partitioned"] and info["records_max"] <= 3
    for l in (1, 3):
        assert _run(multi(3), few, fasta, l) == _run(ctx, few, fasta, l)


def test_window_regular_and_irregular_fasta(multi, ctx):
    rng = random.Random(21)
    ref = "".join(rng.choice("ACGT") for _ in range(60000))
    recs = _random_records(rng, ref, 800, 2)
    vcf, fasta = _vcf(ref, recs, 2, lw=60)
    m = multi(8)
    want = _oracle(vcf, fasta)
    assert m.vcf_transform(vcf, fasta) == want
    info = m.last_vcf()
    assert info["partitioned"] and info["fasta_windowed"]
    assert info["fasta_h2d_bytes_max"] <= len(fasta) // 3, info
    # not regular: every rank copies the whole file, same bytes
    lines = [ref[i:i + 60] for i in range(0, len(ref), 60)]
    crlf = (">chr1 synthetic\r\n" + "\r\n".join(lines) + "\r\n").encode()
    blank = (">chr1 synthetic\n" + "\n".join(lines[:500]) + "\n\n" + "\n".join(lines[500:]) + "\n").encode()
    short = (">chr1 synthetic\n" + "\n".join(lines[:300]) + "\n" + lines[300][:41] + "\n" + lines[300][41:] + "\n" +
             "\n".join(lines[301:]) + "\n").encode()
    second = fasta + b">chr2\nACGTACGT\n"
    for fa in (crlf, blank, short, second):
        single = ctx.vcf_transform(vcf, fa)
        for l in (0, 2):
            assert _run(m, vcf, fa, l) == _run(ctx, vcf, fa, l)
        assert m.vcf_transform(vcf, fa) == single
        info = m.last_vcf()
        assert not info["fasta_windowed"], fa[:40]
        assert info["fasta_h2d_bytes_max"] >= len(fa)
    # a regular file whose last line is short, with and without the final newline
    for fa in (fasta[:-30], fasta[:-31] + b"\n"):
        assert m.vcf_transform(vcf, fa) == ctx.vcf_transform(vcf, fa)
        assert m.last_vcf()["fasta_windowed"]


def test_configs3_shape_at_one_hundredth(multi, ctx):
    vcf, fasta = ctx.genvcf(10_000_000, 100_000, 8)
    want = ctx.vcf_transform(vcf, fasta)
    m = multi(4)
    assert m.vcf_transform(vcf, fasta) == want
    info = m.last_vcf()
    assert info["partitioned"] and info["fasta_windowed"], info
    assert info["records_min"] > 100_000 // 5, info
    assert info["moved_line_bytes"] < len(vcf) // 100, info


def test_rccl_exchange_single_rank(multi, ctx):
    rng = random.Random(31)
    ref = "".join(rng.choice("ACGT") for _ in range(5000))
    recs = _random_records(rng, ref, 300, 3, dup_frac=0.2)
    vcf, fasta = _vcf(ref, recs, 3, lw=60, shuffle=rng)
    m = multi(1, rccl=True)
    for l in (0, 4):
        assert _run(m, vcf, fasta, l) == _run(ctx, vcf, fasta, l)


def test_vcf2eds_cli_gpus_option(tmp_path):
    from test_host_cpp import BUILD, _build_host
    _build_host()
    rng = random.Random(41)
    ref = "".join(rng.choice("ACGT") for _ in range(3000))
    vcf, fasta = _vcf(ref, _random_records(rng, ref, 120, 2), 2, lw=60)
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    (tmp_path / "ref.fa").write_bytes(fasta)
    outs = []
    for d, extra in (("a", []), ("b", ["--gpus", "1"])):
        (tmp_path / d / "x.vcf").write_bytes(vcf)
        r = subprocess.run([os.path.join(BUILD, "vcf2eds"), "-i", str(tmp_path / d / "x.vcf"), "-r", str(tmp_path / "ref.fa")] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        block = r.stdout[r.stdout.index("Variant Processing Statistics:"):].split("\n\n")[0]
        outs.append(((tmp_path / d / "x.eds").read_bytes(), (tmp_path / d / "x.seds").read_bytes(), block))
    assert outs[0] == outs[1]
    e, s, _ = _oracle(vcf, fasta)
    assert outs[0][:2] == (e, s)
    assert "Successfully processed:     120" in outs[0][2]
