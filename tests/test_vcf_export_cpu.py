"""CPU: the VCF export specification (tests/vcf_export_spec.py) against hand-written expectations and against the path
spelling specification (tests/path_spec.py); and the functions of csrc/vcf_text.hpp, compiled for the host, against the
specification byte for byte.  The library is pinned to this specification in tests/test_vcf_export_gpu.py.

The documented example, {AGCT}{T,C}{AG}{G,}{TA} with the sets {0}{1,2}{3}{0}{1}{2,3}{0}: the reference is AGCTTAGGTA;
{T,C} lies at 0-based 4 and has no empty string, so POS = 5 and the alleles are verbatim; {G,} lies at 7 and has one, so it
is anchored with the base in front of it, G at 0-based 6: POS = 7, REF = GG, ALT = G.  Paths 1 and 2 take T, path 3 takes
C; path 1 takes G, paths 2 and 3 the empty string:
    eds  5  .  T   C  .  .  .  GT  0  0  1
    eds  7  .  GG  G  .  .  .  GT  0  1  1
"""
import os
import random
import subprocess

import pytest

import path_spec as ps
import vcf_export_spec as vs
from test_gfa_cpu import open_run_eds
from test_subset_cpu import random_eds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = b"##fileformat=VCFv4.2\n##source=eds2vcf\n##contig=<ID=%s,length=%d>\n"
GT = b"##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
COLS = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"


def rec(*fields):
    return b"\t".join(f if isinstance(f, bytes) else str(f).encode() for f in fields) + b"\n"


def test_documented_example():
    eds, seds = b"{AGCT}{T,C}{AG}{G,}{TA}", b"{0}{1,2}{3}{0}{1}{2,3}{0}"
    vcf, fa, info = vs.export(eds, seds)
    assert vcf == (HEAD % (b"eds", 10) + GT + COLS + b"\tFORMAT\tpath1\tpath2\tpath3\n" +
                   rec(b"eds", 5, b".", b"T", b"C", b".", b".", b".", b"GT", 0, 0, 1) +
                   rec(b"eds", 7, b".", b"GG", b"G", b".", b".", b".", b"GT", 0, 1, 1))
    assert fa == b">eds\nAGCTTAGGTA\n"
    assert info == dict(symbols=5, strings=7, paths=3, records=2, anchored=1, overlapping=0, ref_length=10,
                        header_bytes=len(vcf) - 55, body_bytes=27 + 28)
    # without sources: eight columns; another name, other sample names, line width
    vcf, fa, info = vs.export(eds, None, chrom=b"chr7", line_width=4)
    assert vcf == HEAD % (b"chr7", 10) + COLS + b"\n" + rec(b"chr7", 5, b".", b"T", b"C", b".", b".", b".") + \
        rec(b"chr7", 7, b".", b"GG", b"G", b".", b".", b".")
    assert fa == b">chr7\nAGCT\nTAGG\nTA\n" and info["paths"] == 0
    assert vs.export(eds, seds, names=[b"a", b"b", b"c"])[0].split(b"\n")[4].endswith(b"FORMAT\ta\tb\tc")
    assert vs.export(eds, seds, prefix=b"s")[0].split(b"\n")[4].endswith(b"FORMAT\ts1\ts2\ts3")
    # path 3 as the reference: C is allele 0 of {T,C}, the empty string that of {G,}
    vcf, fa, info = vs.export(eds, seds, ref_path=3)
    assert fa == b">eds\nAGCTCAGTA\n"
    assert vcf.split(b"\n")[5:] == [rec(b"eds", 5, b".", b"C", b"T", b".", b".", b".", b"GT", 1, 1, 0)[:-1],
                                    rec(b"eds", 7, b".", b"G", b"GG", b".", b".", b".", b"GT", 1, 0, 0)[:-1], b""]


def test_anchors_genotypes_and_errors():
    body = lambda *a, **k: vs.export(*a, **k)[0].split(b"\n")[5:-1]
    # an empty string in the first symbol: the base behind the reference string, POS 1
    assert body(b"{AC,}{GT}", b"{1}{2}{0}") == [rec(b"eds", 1, b".", b"ACG", b"G", b".", b".", b".", b"GT", 0, 1)[:-1]]
    assert body(b"{,AC}{GT}", b"{1}{2}{0}") == [rec(b"eds", 1, b".", b"G", b"ACG", b".", b".", b".", b"GT", 0, 1)[:-1]]
    # adjacent degenerate symbols: the second is anchored on the first one's reference base and overlaps it
    vcf, _, info = vs.export(b"{A}{C,}{G,T}{,TT}", b"{0}{1}{2}{1}{2}{1}{2}")
    assert vcf.split(b"\n")[5:-1] == [rec(b"eds", 1, b".", b"AC", b"A", b".", b".", b".", b"GT", 0, 1)[:-1],
                                      rec(b"eds", 3, b".", b"G", b"T", b".", b".", b".", b"GT", 0, 1)[:-1],
                                      rec(b"eds", 3, b".", b"G", b"GTT", b".", b".", b".", b"GT", 0, 1)[:-1]]
    assert (info["anchored"], info["overlapping"]) == (2, 1)
    # several alleles per cell, a universal string inside a degenerate symbol, a path in no string, equal texts not merged
    assert body(b"{A,C,A}", b"{1,2}{0}{2,4}") == [rec(b"eds", 1, b".", b"A", b"C,A", b".", b".", b".", b"GT", b"0/1", b"0/1/2", 1, b"1/2")[:-1]]
    assert body(b"{A,C}{G}", b"{1}{3}{0}") == [rec(b"eds", 1, b".", b"A", b"C", b".", b".", b".", b"GT", 0, b".", 1)[:-1]]
    # a one-string symbol gives no record, whatever its set
    assert body(b"{A}{C}", b"{1}{0}") == [] and vs.export(b"{A}{C}", b"{1}{0}")[2]["records"] == 0
    assert vs.export(b"", b"")[0] == HEAD % (b"eds", 0) + GT + COLS + b"\tFORMAT\n" and vs.export(b"", None)[1] == b">eds\n"
    for args, kw, text in [((b"{A,}", b"{1}{2}"), {}, "Symbol 0 has an empty string and no reference base to anchor it"),
                           ((b"{,A}{,C}", b"{1}{2}{1}{2}"), {}, "Symbol 0 has an empty string and no reference base to anchor it"),
                           ((b"{A}{C,G}", b"{0}{1}{2}"), dict(ref_path=3), "Path id 3 out of range (1..2)"),
                           ((b"{A}{C,G}{T}", b"{0}{1}{3}{0}"), dict(ref_path=2), "Path 2 takes no string of symbol 1"),
                           ((b"{A}{C,G}", None), dict(ref_path=1), "A reference path needs sources (.seds)"),
                           ((b"{A}", None), dict(chrom=b""), "Chromosome name is empty or holds whitespace"),
                           ((b"{A}", None), dict(chrom=b"a b"), "Chromosome name is empty or holds whitespace"),
                           ((b"{A,C}", b"{1}{2}"), dict(names=[b"x"]), "Expected 2 sample names, got 1"),
                           ((b"{A,C}", b"{1}{2}"), dict(names=[b"x", b"y\tz"]), "Sample name 1 is not a VCF sample name"),
                           ((b"{A,C}", b"{1}{2}"), dict(max_bytes=24), "VCF body of 25 bytes is above the limit of 24")]:
        with pytest.raises(ValueError) as ei:
            vs.export(*args, **kw)
        assert str(ei.value) == text
    assert vs.export(b"{A,C}", b"{1}{2}", max_bytes=25)[2]["body_bytes"] == 25


def separated_eds(rng, P):
    """A random (eds, seds) whose degenerate symbols are separated by common symbols and in which every path takes exactly
    one string of every symbol (the sets of a symbol partition the paths), with empty strings."""
    syms, sets = [[b"".join(rng.choice([b"A", b"C", b"G", b"T"]) for _ in range(rng.randint(1, 4)))]], [{0}]
    for _ in range(rng.randint(1, 12)):
        k = rng.randint(2, min(4, P)) if P > 1 else 1
        owner = [rng.randrange(k) for _ in range(P)]
        for j in range(k):
            if j not in owner:
                owner[rng.randrange(P)] = j
        used = sorted(set(owner))
        texts = set()
        while len(texts) < len(used):
            texts.add(b"".join(rng.choice([b"A", b"C", b"G", b"T"]) for _ in range(rng.randint(0, 4))))
        texts = list(texts)
        rng.shuffle(texts)
        syms.append(texts)
        sets += [{p + 1 for p in range(P) if owner[p] == j} for j in used]
        syms.append([b"".join(rng.choice([b"A", b"C", b"G", b"T"]) for _ in range(rng.randint(1, 4)))])
        sets.append({0})
    return (b"".join(b"{" + b",".join(s) + b"}" for s in syms),
            b"".join(b"{" + b",".join(b"%d" % p for p in sorted(s)) + b"}" for s in sets))


def test_samples_applied_to_the_reference_spell_the_paths():
    rng = random.Random(20250611)
    checked = anchored = 0
    for _ in range(200):
        P = rng.randint(1, 7)
        eds, seds = separated_eds(rng, P)
        syms, sets, P2 = ps.parse(eds, seds)
        for ref_path in (0, 1, P2):
            vcf, fa, info = vs.export(eds, seds, ref_path=ref_path, line_width=rng.choice([0, 1, 7, 60]))
            assert info["overlapping"] == 0
            ref = vs.fasta_sequence(fa)
            if ref_path:
                assert ref == ps.spell(syms, sets, ref_path)[0]
            names, recs = vs.read(vcf)
            assert len(names) == P2
            for p in range(1, P2 + 1):
                assert vs.apply_sample(ref, recs, p - 1) == ps.spell(syms, sets, p)[0], (eds, seds, ref_path, p)
                checked += 1
            anchored += info["anchored"]
    assert checked >= 1500 and anchored >= 300


# ---- csrc/vcf_text.hpp on the host ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def writer(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vcf_text") / "test_vcf_text")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "cpp", "test_vcf_text.cpp"), "-o", exe],
                   check=True)

    def run(jobs):
        """jobs: (eds, seds or None, ref_path, lead, chrom) -> the bodies"""
        inp = b"".join(e + b" " + (s if s is not None else b"-") + b" %d %d " % (rp, lead) + c + b"\n" for e, s, rp, lead, c in jobs)
        out = subprocess.run([exe], input=inp, capture_output=True, check=True).stdout
        texts, k = [], 0
        for _ in jobs:
            nl = out.index(b"\n", k)
            size = int(out[k:nl])
            texts.append(out[nl + 1:nl + 1 + size])
            k = nl + 1 + size
        assert k == len(out)
        return texts
    return run


def accepted(eds, seds, **kw):
    try:
        return vs.export(eds, seds, **kw)
    except ValueError:
        return None


def test_text_functions_against_the_spec(writer):
    rng = random.Random(20250612)
    jobs = []
    for k in range(400):
        eds, seds = (random_eds(rng) if k % 2 else open_run_eds(rng)) if k % 4 else separated_eds(rng, rng.randint(1, 7))
        P = ps.parse(eds, seds)[2]
        for rp, s in ((0, seds), (0, None), (1, seds), (P, seds)):
            if eds and accepted(eds, s, ref_path=rp) is not None:
                jobs.append((eds, s, rp, k % 16, rng.choice([b"eds", b"c", b"chr21_a_long_name"])))
    wide = lambda w, t: b"{" + b",".join(t(j) for j in range(w)) + b"}"
    sets = lambda ss: b"".join(b"{" + b",".join(b"%d" % p for p in sorted(s)) + b"}" for s in ss)
    # 65 and 300 strings, every path in all of them; alleles of 15, 16, 17 and 5000 characters; POS across 9/10 and 99/100
    for k, P in ((65, 70), (300, 3), (2, 257), (3, 513)):
        eds = b"{ACGTACGTA}" + wide(k, lambda j: b"ACGT"[j % 4:j % 4 + 1] * (1 + j % 3)) + b"{" + b"T" * 88 + b"}" + wide(2, lambda j: b"AC"[j:j + 1])
        allp = set(range(1, P + 1))
        jobs.append((eds, sets([{0}] + [allp] * k + [{0}] + [{1}, allp - {1}]), 0, 5, b"eds"))
        jobs.append((eds, sets([{0}] + [{1 + j % P} for j in range(k)] + [{0}] + [{P}, {1}]), 0, 11, b"eds"))
    for n in (15, 16, 17, 5000):
        jobs.append((b"{G}" + wide(3, lambda j: b"ACGT"[j:j + 1] * (n if j != 1 else 0)) + b"{T}", sets([{0}, {1}, {2}, {3}, {0}]), 2, 3, b"eds"))
    assert len(jobs) >= 600
    got = writer(jobs)
    for (eds, seds, rp, lead, chrom), text in zip(jobs, got):
        vcf, _, info = vs.export(eds, seds, chrom=chrom, ref_path=rp)
        assert text == vcf[info["header_bytes"]:], (eds[:200], seds and seds[:200], rp, lead)
