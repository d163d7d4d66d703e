"""CPU: path spelling.  EDS::path_sequence / EDS::max_path_id of the host container against the Python restatement of
the specification (tests/path_spec.py) on the merge and VCF fixtures, their errors, and the specification itself against
the oracle: an MSA round trip that compares with the INPUT alignment, a haploid VCF consensus, and the invariance of the
spelled paths under the LINEAR merge."""
import json
import os
import random
import subprocess

import pytest

import oracle_lib as o
import path_spec as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HOST = os.path.join(ROOT, "edsparser_amd", "host")
BUILD = os.path.join(HOST, "build")
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "edsparser_amd")


def _cases(fn):
    return json.load(open(os.path.join(GOLDEN, fn)))["cases"]


def merge_fixture_inputs():
    """(eds, seds) of every merge fixture case that has sources."""
    return [(c["eds"].encode(), c["seds"].encode()) for fn in ("gen_merge.json", "gen2_merge.json") for c in _cases(fn)
            if c.get("seds") is not None]


def vcf_fixture_outputs():
    """The expected (eds, seds) of every VCF fixture case with l = 0 that produced a text."""
    return [(c["expect"]["eds"].encode(), c["expect"]["seds"].encode()) for fn in ("gen_vcf.json", "gen2_vcf.json")
            for c in _cases(fn) if c["l"] == 0 and "eds" in c["expect"]]


@pytest.fixture(scope="module")
def runner(tmp_path_factory):
    subprocess.run(["make", "-s", "-C", HOST], check=True)        # (libedsx.so itself comes from build())
    exe = os.path.join(BUILD, "test_paths")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", INC, os.path.join(ROOT, "tests", "cpp", "test_paths.cpp"),
                    os.path.join(BUILD, "libedsparser_lib.a"), "-L", LIBDIR, "-ledsx", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    d = tmp_path_factory.mktemp("paths")

    def run(cmds):
        f = d / "cmds.txt"
        f.write_bytes(b"".join(b"\t".join(x if isinstance(x, bytes) else str(x).encode() for x in c) + b"\n" for c in cmds))
        r = subprocess.run([exe, str(f)], capture_output=True)
        assert r.returncode == 0, r.stderr
        out = r.stdout.split(b"\n")[:-1]
        assert len(out) == len(cmds)
        return out
    return run


def _one_line(t):
    return b"".join(t.split())


def _check_all_paths(runner, inputs):
    out = runner([("A", _one_line(e), _one_line(s)) for e, s in inputs])
    paths = 0
    for (e, s), line in zip(inputs, out):
        try:
            syms, sets, P = ps.parse(e, s)
        except ValueError:                                      # fixtures whose sources do not match: the container refuses too
            assert line.startswith(b"runtime_error:"), (e, s, line)
            continue
        want = [b"%d" % P]
        for p in range(1, P + 1):
            seq, miss = ps.spell(syms, sets, p)
            want.append(seq + b":%d" % miss)
        assert line == b"|".join(want), (e, s)
        paths += P
    return paths


def test_path_sequence_on_merge_fixtures(runner):
    inputs = merge_fixture_inputs()
    assert len(inputs) >= 100
    assert _check_all_paths(runner, inputs) >= 300


def test_path_sequence_on_vcf_fixture_outputs(runner):
    inputs = vcf_fixture_outputs()
    assert len(inputs) >= 100
    assert _check_all_paths(runner, inputs) >= 300


def test_path_sequence_errors(runner):
    eds, seds = b"{AC}{G,T}{A}", b"{0}{1}{2,3}{0}"
    out = runner([("P", eds, seds, 0), ("P", eds, seds, 4), ("P", eds, seds, -1), ("P", eds, b"-", 1), ("P", eds, seds, 3),
                  ("P", b"{AC}{G,T}", b"{0}{1}{4}", 2), ("A", b"", b"-")])
    assert out[0] == b"invalid_argument:Path id 0 out of range (1..3)"
    assert out[1] == b"invalid_argument:Path id 4 out of range (1..3)"
    assert out[2] == b"invalid_argument:Path id -1 out of range (1..3)"
    assert out[3] == b"invalid_argument:Path spelling needs sources (.seds)"
    assert out[4] == b"ACTA:0"
    assert out[5] == b"AC:1"                 # no string of {G,T} holds path 2
    assert out[6] == b"0"                    # an empty EDS has no paths


# ---- the specification against the oracle ---------------------------------------------------------------------------
def _random_msa(rng, wrap):
    S, L = rng.randint(2, 9), rng.randint(1, 120)
    rows = []
    base = [rng.choice("ACGT") for _ in range(L)]
    for _ in range(S):
        row = list(base)
        for c in range(L):
            r = rng.random()
            if r < 0.08:
                row[c] = rng.choice("ACGT")
            elif r < 0.16:
                row[c] = "-"
        rows.append("".join(row))
    # gap runs shared by several rows, so that empty strings and all-gap stretches of a row occur
    for _ in range(rng.randint(0, 3)):
        a = rng.randrange(L)
        b = min(L, a + rng.randint(1, 12))
        for r in rng.sample(range(S), rng.randint(1, S - 1)):
            rows[r] = rows[r][:a] + "-" * (b - a) + rows[r][b:]
    w = rng.choice([7, 10, 60]) if wrap else L
    text = "".join(">s%d\n" % i + "".join(row[k:k + w] + "\n" for k in range(0, L, w)) for i, row in enumerate(rows))
    return text.encode(), [r.replace("-", "").encode() for r in rows]


def test_msa_round_trip_against_the_input():
    """Path s + 1 of msa2eds(A) is row s of A without gaps and line feeds, for l = 0 and any l: compares against the
    input alignment, not against another implementation."""
    rng = random.Random(20240607)
    checked = 0
    for it in range(600):
        msa, rows = _random_msa(rng, wrap=it % 2 == 1)
        for l in (0, 1, 3, 8):
            eds, seds = o.msa(msa, l)
            syms, sets, P = ps.parse(eds, seds)
            assert P == len(rows), (msa, l)
            for s, row in enumerate(rows):
                assert ps.spell(syms, sets, s + 1) == (row, 0), (msa, l, s)
            checked += 1
    assert checked == 2400


def _haploid_vcf(rng):
    L, ns = rng.randint(30, 200), rng.randint(1, 6)
    ref = "".join(rng.choice("ACGT") for _ in range(L))
    lines = ["##fileformat=VCFv4.2", "\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] +
                                               ["S%d" % i for i in range(ns)])]
    cons = [[] for _ in range(ns)]
    cur = 0
    pos = rng.randint(2, 6)
    while pos + 12 < L:
        kind = rng.random()
        if kind < 0.6:
            refa = ref[pos - 1]
            alts = rng.sample([c for c in "ACGT" if c != refa], rng.randint(1, 2))
        elif kind < 0.8:
            refa = ref[pos - 1]
            alts = [refa + "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 4)))]
        else:
            refa = ref[pos - 1:pos - 1 + rng.randint(2, 5)]
            alts = [refa[0]]
        gts = [rng.randint(0, len(alts)) for _ in range(ns)]
        lines.append("\t".join(["chr1", str(pos), ".", refa, ",".join(alts), ".", "PASS", ".", "GT"] + [str(g) for g in gts]))
        for s in range(ns):
            cons[s].append(ref[cur:pos - 1] + ([refa] + alts)[gts[s]])
        cur = pos - 1 + len(refa)
        pos = cur + rng.randint(2, 15)                         # records never touch or overlap
    for s in range(ns):
        cons[s].append(ref[cur:])
    fasta = ">chr1\n" + "".join(ref[i:i + 60] + "\n" for i in range(0, L, 60))
    return ("\n".join(lines) + "\n").encode(), fasta.encode(), ["".join(c).encode() for c in cons]


def test_haploid_vcf_consensus():
    """With haploid genotypes and records that do not overlap, path s + 1 of vcf2eds is the reference with sample s's
    ALT alleles applied."""
    rng = random.Random(77)
    checked = 0
    for _ in range(500):
        vcf, fasta, cons = _haploid_vcf(rng)
        eds, seds, st = o.vcf(vcf, fasta, 0)
        syms, sets, P = ps.parse(eds, seds)
        used = sorted(set().union(*sets) - {0})
        assert P <= len(cons)
        for s, want in enumerate(cons):
            if s + 1 > P:                                      # trailing samples that carry no ALT: the reference path
                continue
            assert ps.spell(syms, sets, s + 1) == (want, 0), (vcf, fasta, s, used)
            checked += 1
    assert checked >= 1000


def _limit_memory():
    import resource
    resource.setrlimit(resource.RLIMIT_AS, (2 << 30, 2 << 30))


def _merge_job(job):
    eds, seds, l = job
    try:
        return o.merge(eds, seds, l, False)
    except (o.OracleError, MemoryError):
        return None


def test_merge_keeps_every_spelled_path():
    """The LINEAR merge I(a, b) holds p (or 0) exactly when both parts do, and products come in lexicographic order: the
    first matching string of a merged symbol is the concatenation of the first matching strings of its parts.  So
    eds2leds -s changes no path that has a string at every symbol.  compact = 0: a compact .leds drops '{}' of an
    empty single-string symbol and then no longer matches its .seds (a documented quirk of save(COMPACT)).
    The merges run in a child process with 2 GiB of address space: LINEAR products of diploid source sets can double
    per merge (one VCF fixture has a symbol of 52 strings), and a merge that runs out of memory there counts as one that
    throws.  At least half of all (case, l, path) triples must come through."""
    import multiprocessing as mp
    jobs, meta = [], []
    for inputs, ls in ((merge_fixture_inputs(), (1, 2, 3, 5)), (vcf_fixture_outputs(), (1, 2, 3))):
        for eds, seds in inputs:
            try:
                syms, sets, P = ps.parse(eds, seds)
            except ValueError:
                continue
            before = [ps.spell(syms, sets, p) for p in range(1, P + 1)]
            for l in ls:
                jobs.append((eds, seds, l))
                meta.append(before)
    with mp.get_context("fork").Pool(1, initializer=_limit_memory) as pool:
        merged = pool.map(_merge_job, jobs)
    triples = checked = 0
    for (eds, seds, l), before, res in zip(jobs, meta, merged):
        triples += len(before)
        if res is None:
            continue
        msyms, msets, MP = ps.parse(*res)
        for p, (seq, miss) in enumerate(before, 1):
            if miss:
                continue
            assert p <= MP and ps.spell(msyms, msets, p) == (seq, 0), (eds, seds, l, p)
            checked += 1
    print("merge invariance: %d of %d (case, l, path) triples checked" % (checked, triples))
    assert triples >= 3000 and 2 * checked >= triples


# ---- eds2fasta argument errors (before any device work) ---------------------------------------------------------------
def test_eds2fasta_argument_errors(tmp_path, runner):
    exe = os.path.join(BUILD, "eds2fasta")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1 and "the option '--input' is required but missing" in r.stderr and "[Performance] Runtime:" in r.stderr
    r = subprocess.run([exe, "-i", str(tmp_path / "none.eds")], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: Input file does not exist" in r.stderr
    (tmp_path / "x.eds").write_text("{A}")
    r = subprocess.run([exe, "-i", str(tmp_path / "x.eds")], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: Path spelling needs sources (.seds)" in r.stderr
    (tmp_path / "x.seds").write_text("{1}")
    r = subprocess.run([exe, "-i", str(tmp_path / "x.eds"), "-p", "1,x"], capture_output=True, text=True)
    assert r.returncode == 1 and "for option '--paths' is invalid" in r.stderr
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--line-width" in r.stdout and "--batch-mb" in r.stdout
