"""GPU parity tests for VCF -> EDS / l-EDS (edsx_vcf_transform): the reference's data/vcf goldens,
SURVEY KATs, 300 fixtures generated from the real reference library, larger random cases vs the oracle."""
import json
import os
import random

import pytest

import oracle_lib as o
from conftest import GOLDEN
from vcf_cases import large_key_vcf, random_vcf as _random_vcf, single_damage_files, text_length_files

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    c = edsparser_amd.Context(0)
    yield c
    c.close()


def _run(ctx, vcf, fasta, l):
    import edsparser_amd
    try:
        e, s, st = ctx.vcf_transform(vcf, fasta, l)
        return {"eds": e.decode(), "seds": s.decode(), "stats": st}
    except edsparser_amd.EdsxError as ex:
        return {"error": ex.message}


def _rd(rel):
    return open(os.path.join(GOLDEN, rel), "rb").read()


def test_kat_and_reference_goldens(ctx):
    k = json.load(open(os.path.join(GOLDEN, "kat_vcf.json")))
    for c in k["cases"]:
        v = c["vcf"].encode() if "vcf" in c else _rd(c["vcf_file"])
        f = _rd(c["fasta_file"]) if "fasta_file" in c else k["fasta_default"].encode()
        ee = c["eds"].encode() if "eds" in c else _rd(c["eds_file"])
        ss = c["seds"].encode() if "seds" in c else _rd(c["seds_file"])
        got = _run(ctx, v, f, c["l"])
        assert got.get("eds", "").encode() == ee, c["name"]
        assert got.get("seds", "").encode() == ss, c["name"]


def test_generated_reference_fixtures(ctx):
    cases = json.load(open(os.path.join(GOLDEN, "gen_vcf.json")))["cases"]
    for c in cases:
        got = _run(ctx, c["vcf"].encode(), c["fasta"].encode(), c["l"])
        assert got == c["expect"], c


def test_generated_reference_fixtures_round2(ctx):
    """17..200 records with many equal POS (the reference's unstable std::sort decides their order, quirk 29) and the
    SURVEY quirk 22-27 shapes; expected text from the reference itself (tests/golden/make_golden2.py)."""
    cases = json.load(open(os.path.join(GOLDEN, "gen2_vcf.json")))["cases"]
    for c in cases:
        got = _run(ctx, c["vcf"].encode(), c["fasta"].encode(), c["l"])
        assert got == c["expect"], c["name"]


@pytest.mark.parametrize("L,nvar,ns,lw,l", [(5000, 300, 8, 60, 0), (20000, 1500, 3, 70, 0), (3000, 200, 70, 3000, 0),
                                            (4000, 150, 4, 60, 6)])
def test_random_larger_inputs_vs_oracle(ctx, L, nvar, ns, lw, l):
    rng = random.Random(L + nvar)
    vcf, fasta = _random_vcf(rng, L, nvar, ns, lw)
    try:
        e, s, st = o.vcf(vcf, fasta, l)
        want = {"eds": e.decode(), "seds": s.decode(), "stats": st}
    except o.OracleError as ex:
        want = {"error": str(ex)}
    assert _run(ctx, vcf, fasta, l) == want


def test_multithreaded_tokeniser_large_vcf(ctx):
    """VCF files of 4 MB and more are cut at line starts and tokenised by several host threads;
    records, counters and group order must still equal the oracle's (which reads line by line).
    The file also carries malformed lines and unsupported structural variants across the cuts."""
    rng = random.Random(99)
    vcf, fasta = _random_vcf(rng, 400000, 40000, 24, 60)
    lines = vcf.decode().split("\n")
    for i in range(200, len(lines) - 1, 997):
        lines.insert(i, "chr1\tnot_a_number" if i % 2 else "chr1\t%d\t.\tA\t<INV>\t.\tPASS\t." % (i % 4000 + 1))
    vcf = "\n".join(lines).encode()
    assert len(vcf) >= 4 << 20
    e, s, st = o.vcf(vcf, fasta, 0)
    assert _run(ctx, vcf, fasta, 0) == {"eds": e.decode(), "seds": s.decode(), "stats": st}


def test_multithreaded_tokeniser_fuzz(ctx):
    """Random damage to a large VCF (tabs turned into spaces, fields removed, junk lines, odd genotypes,
    symbolic alleles, CR line ends): records, counters and output must equal the oracle's."""
    rng = random.Random(4242)
    vcf0, fasta = _random_vcf(rng, 300000, 36000, 24, 60)
    lines0 = vcf0.decode().split("\n")
    assert len(vcf0) >= 4 << 20
    for it in range(8):
        lines = list(lines0)
        for _ in range(400):
            i = rng.randrange(2, len(lines) - 1)
            f = lines[i].split("\t")
            op = rng.randrange(9)
            if op == 0:
                lines[i] = lines[i].replace("\t", " ")
            elif op == 1 and len(f) > 6:
                lines[i] = "\t".join(f[:rng.randint(1, 6)])
            elif op == 2:
                lines[i] = rng.choice(["", "#junk", "chr1", "\t\t\t", "chr1\t12\t.\tA"])
            elif op == 3 and len(f) > 10:
                f[9 + rng.randrange(len(f) - 9)] = rng.choice(["./.", ".", "1", "0/1/2", "x|1", "1|", "|", "0|1:9:x", "", "99999999999|0"])
                lines[i] = "\t".join(f)
            elif op == 4 and len(f) > 5:
                f[4] = rng.choice(["<DEL>", "<INS>", "<INV>", "A,<DEL>", "<DUP>,C", ",", "A,,C", "C,", "<>", "<", "."])
                lines[i] = "\t".join(f)
            elif op == 5:
                lines[i] = lines[i] + "\r"
            elif op == 6 and len(f) > 2:
                f[1] = rng.choice(["0", "-5", "+7", " 12", "12abc", "abc", "", "99999999999999999999999", "300001"])
                lines[i] = "\t".join(f)
            elif op == 7:
                lines[i] = lines[i].replace("\t", "\t\t", 2)
            else:
                lines.insert(i, lines[rng.randrange(2, len(lines) - 1)])
        vcf = "\n".join(lines).encode()
        for l in ((0, 6) if it < 2 else (0,)):
            try:
                e, s, st = o.vcf(vcf, fasta, l)
                want = {"eds": e.decode(), "seds": s.decode(), "stats": st}
            except o.OracleError as ex:
                want = {"error": str(ex)}
            assert _run(ctx, vcf, fasta, l) == want, (it, l)


def test_randomized_campaign(ctx):
    """80 random VCF/FASTA pairs: reference length 30..30000, site density up to 0.4 (long overlap chains),
    0..70 samples, several FASTA line widths, shuffled record order, l in {0, 3, 10}; 900 cases of the same
    generator were run once on the MI355X box without a mismatch."""
    rng = random.Random(21)
    for it in range(80):
        L = rng.choice([30, 100, 1000, 5000, 30000])
        nvar = max(1, min(L - 12, int(L * rng.choice([0.01, 0.05, 0.2, 0.4]))))
        ns = rng.choice([0, 1, 2, 8, 63, 64, 65, 70])
        lw = rng.choice([60, 70, 7, L, 61])
        l = rng.choice([0, 0, 0, 3, 10]) if nvar <= 60 else 0
        vcf, fasta = _random_vcf(rng, L, nvar, ns, lw)
        if rng.random() < 0.3:
            lines = vcf.decode().split("\n")
            head, body = lines[:2], [x for x in lines[2:] if x]
            rng.shuffle(body)
            vcf = ("\n".join(head + body) + "\n").encode()
        try:
            e, s, st = o.vcf(vcf, fasta, l)
            want = {"eds": e.decode(), "seds": s.decode(), "stats": st}
        except o.OracleError as ex:
            want = {"error": str(ex)}
        assert _run(ctx, vcf, fasta, l) == want, (it, L, nvar, ns, lw, l)


def _want(vcf, fasta, l=0):
    try:
        e, s, st = o.vcf(vcf, fasta, l)
        return {"eds": e.decode(), "seds": s.decode(), "stats": st}
    except o.OracleError as ex:
        return {"error": str(ex)}


def test_device_tokeniser_single_damage_per_file(ctx):
    """One oddity per small file, every kind the device tokeniser must either place exactly or hand to the host
    tokeniser: the result must equal the oracle's either way (a wrongly accepted line would show here, where no
    second oddity in the same file can trigger the fallback for it)."""
    rng = random.Random(808)
    taken = {True: 0, False: 0}
    n = 0
    for kind, ch, ns, tail, line, v, fasta in single_damage_files(rng):
        got = _run(ctx, v, fasta, 0)
        assert got == _want(v, fasta), (kind, ch, ns, tail, line)
        taken[ctx.vcf_tokenised_on_device()] += 1
        n += 1
    assert n > 150 and taken[True] > 20 and taken[False] > 60, taken


def test_device_tokeniser_is_taken_and_equals_the_host_tokeniser(ctx):
    """Plain files go through the device tokeniser; EDSX_HOST_TOKENIZER=1 forces the host tokeniser: same bytes, same
    counters; shuffled files and duplicate positions included (the sort is the host's in both)."""
    rng = random.Random(909)
    for it in range(40):
        L = rng.choice([100, 1000, 5000, 30000])
        nvar = max(1, min(L - 12, int(L * rng.choice([0.01, 0.05, 0.2, 0.4]))))
        ns = rng.choice([0, 1, 2, 8, 64, 70])
        vcf, fasta = _random_vcf(rng, L, nvar, ns, rng.choice([60, 7, L]))
        lines = vcf.decode().split("\n")
        head, body = lines[:2], [x for x in lines[2:] if x]
        if it % 3 == 1:
            rng.shuffle(body)
        if it % 3 == 2:
            body += [rng.choice(body) for _ in range(len(body) // 2)]
            rng.shuffle(body)
        vcf = ("\n".join(head + body) + ("\n" if it % 2 else "")).encode()
        got = _run(ctx, vcf, fasta, 0)
        assert ctx.vcf_tokenised_on_device(), it
        os.environ["EDSX_HOST_TOKENIZER"] = "1"
        try:
            host = _run(ctx, vcf, fasta, 0)
            assert not ctx.vcf_tokenised_on_device()
        finally:
            del os.environ["EDSX_HOST_TOKENIZER"]
        assert got == host == _want(vcf, fasta), it


def test_large_outputs_every_size_remainder(ctx):
    """.eds of 17 MB and more (pinned-chunk download): reference lengths with every remainder modulo the copy threads
    and the 64-byte rounding, a handful of records, against the oracle."""
    import numpy as np
    rng = np.random.default_rng(3)
    base = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 17_825_800, dtype=np.uint8)].tobytes()
    hdr = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS0\tS1\n"
    for extra in range(0, 12):
        ref = base[:17_825_792 - 40 + extra]          # .eds = reference + a few braces: sizes step through all remainders
        fasta = b">c\n" + ref + b"\n"
        recs = [(1000, "0|1\t1|1"), (9_000_000, "1|0\t0|0"), (len(ref) - 5, "0|0\t0|1")]
        vcf = (hdr + "".join("c\t%d\t.\t%s\t%s\t.\t.\t.\tGT\t%s\n" % (p, chr(ref[p - 1]), "A" if chr(ref[p - 1]) != "A" else "C", g)
                             for p, g in recs)).encode()
        want = o.vcf(vcf, fasta, 0)
        got = ctx.vcf_transform(vcf, fasta, 0)
        assert len(got[0]) >= 16 << 20
        assert got == want, extra


def test_text_length_every_remainder_mod_8_with_and_without_final_newline(ctx):
    """The device tokeniser reads the text through aligned 8-byte words (ByteWindow, csrc/vcf_walk.hpp): the last line
    may end anywhere inside its word.  Text lengths 0..7 modulo 8 (a comment line of adjustable length in front), with
    and without the final newline, last record with a long ALT, an <INS> (copies REF) and a <DEL>; and a text whose
    length is just below / at / above multiples of 256 (the allocation granule of the text buffer)."""
    fasta, mod8, sized = text_length_files(random.Random(88))
    seen = set()
    for tail, pad, nl, vcf in mod8:
        seen.add((len(vcf) % 8, nl))
        got = _run(ctx, vcf, fasta, 0)
        assert ctx.vcf_tokenised_on_device()
        assert got == _want(vcf, fasta), (tail[:30], pad, nl)
    assert len(seen) == 16
    for target, vcf in sized:
        assert len(vcf) == target
        assert _run(ctx, vcf, fasta, 0) == _want(vcf, fasta), target


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097, 70000])
def test_device_sort_large_keys_and_tile_edges(ctx, n):
    """The device radix sort runs eight 8-bit passes over 64-bit keys, in tiles of 2048 records: shuffled files with
    pairwise distinct positions of one tile less one record, exactly one, one more, two and one more, and 35 tiles; a
    quarter of the positions have 8 to 19 digits (up to 9 * 10^18), so that every pass sees digits other than 0.
    (The oracle takes 0.5 s for the 70 000 records.)"""
    vcf, fasta = large_key_vcf(random.Random(n), n)
    pos = [int(x.split(b"\t")[1]) for x in vcf.split(b"\n")[2:] if x]
    assert len(set(pos)) == n == len(pos) and pos != sorted(pos)
    assert all(any((p >> (8 * k)) & 0xFF for p in pos) for k in range(8)) and max(pos) <= 9 * 10 ** 18
    want = _want(vcf, fasta)
    assert "error" not in want and want["stats"]["processed_variants"] == n
    assert _run(ctx, vcf, fasta, 0) == want
    assert ctx.vcf_tokenised_on_device()
