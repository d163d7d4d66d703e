"""GPU: contig selection (edsx_vcf_session_*, edsx_vcf_transform_contig, vcf2eds --chrom / --all-chroms) against the
specification in tests/contig_spec.py.  Every comparison is bytes + counters + error text."""
import os
import random
import subprocess

import pytest

import oracle_lib as o
from conftest import GOLDEN
import contig_spec as cs
from vcf_cases import gen_vcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "edsparser_amd", "host")
VCF2EDS = os.path.join(HOST, "build", "vcf2eds")
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


def _want(V, F, name, l):
    try:
        e, s, st = o.vcf(*cs.split(V, F, name), l)
        return {"eds": e.decode(), "seds": s.decode(), "stats": st}
    except Exception as ex:
        return {"error": str(ex)}


class _host_tokenizer:
    def __enter__(self):
        os.environ["EDSX_HOST_TOKENIZER"] = "1"

    def __exit__(self, *exc):
        del os.environ["EDSX_HOST_TOKENIZER"]


# ---- 1. composed fixtures -------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_composed_fixtures_every_contig_equals_its_fixture(ctx, seed):
    cases = cs.load_fixtures(GOLDEN)
    done = on_device = 0
    for V, F, parts, left in cs.compose(cases, seed):
        assert not left                                              # no fixture may be left out
        with ctx.vcf_session(V, F) as ses:
            for nm, c in parts:
                assert _res(lambda: ses.transform(nm, c["l"])) == c["expect"], (seed, nm, c.get("name"))
                done += 1
            on_device += ses.info()["classified_on_device"]
        nm, c = parts[seed % len(parts)]
        assert _res(lambda: ctx.vcf_transform(V, F, c["l"], contig=nm)) == c["expect"], (seed, nm, c.get("name"))
        with _host_tokenizer():
            with ctx.vcf_session(V, F) as ses:
                assert ses.info()["classified_on_device"] == 0
                for nm, c in parts:
                    assert _res(lambda: ses.transform(nm, c["l"])) == c["expect"], (seed, nm, c.get("name"), "host")
                    assert not ctx.vcf_tokenised_on_device()
    assert done == len(cases) == 366
    print("seed %d: %d combined inputs classified on the device" % (seed, on_device))


# ---- 2. + 5. random plain inputs, residency ---------------------------------------------------------------------
def _wrap(seq, w):
    return b"\n".join(seq[i:i + w] for i in range(0, len(seq), w))


def _plain_input(rng):
    """3..12 contigs out of gen_vcf parts: another line width per record, a contig without VCF records, record lines of
    a contig the FASTA lacks, a duplicate FASTA name, contigs not contiguous in the VCF, no final newline."""
    K = rng.randint(3, 12)
    names = [b"chr%d" % (k + 1) for k in range(K)]                   # chr1 is a prefix of chr10..chr12
    fa, chunks, header = [], [], None
    ns = rng.choice([1, 2, 3, 8])       # (gen_vcf with 0 samples ends every line with a tab: an empty field, not plain)
    empty = rng.randrange(K)
    for k, nm in enumerate(names):
        Lf = rng.randint(200, 6000)
        v, f = gen_vcf(Lf, rng.randint(1, max(1, Lf // 40)), ns, rng.randrange(1 << 30))
        lines = v.split(b"\n")
        header = header or [x for x in lines if x.startswith(b"#")]
        body = [nm + x[4:] for x in lines if x.startswith(b"chr1\t")]
        seq = b"".join(f.split(b"\n")[1:])
        desc = b" synthetic" if rng.random() < 0.5 else b""
        fa.append(b">" + nm + desc + b"\n" + _wrap(seq, rng.choice([1, 7, 60, 61, 80, 1024, 5000])) + b"\n")
        if k != empty:
            cut = sorted(rng.sample(range(len(body) + 1), min(len(body), rng.randint(0, 3))))
            for a, b in zip([0] + cut, cut + [len(body)]):
                if a < b:
                    chunks.append(body[a:b])
    ghost_v, _ = gen_vcf(300, 5, ns, 7)
    chunks.append([b"ghost" + x[4:] for x in ghost_v.split(b"\n") if x.startswith(b"chr1\t")])
    chunks.append([b"chr" + x[4:] for x in ghost_v.split(b"\n") if x.startswith(b"chr1\t")][:2])    # "chr": a prefix of every name
    rng.shuffle(chunks)
    dup = rng.randrange(K)
    fa.insert(rng.randint(dup + 1, K), b">" + names[dup] + b" again\n" + _wrap(bytes(rng.choices(b"ACGT", k=100)), 50) + b"\n")
    V = b"\n".join(header + [ln for ch in chunks for ln in ch])     # the last record has no final newline
    F = b"".join(fa)
    if rng.random() < 0.5:
        F = F[:-1]
    return V, F, names, empty


def test_random_plain_inputs_run_on_the_device_from_resident_texts(ctx):
    import edsparser_amd
    rng = random.Random(20261016)
    for it in range(40):
        V, F, names, empty = _plain_input(rng)
        l = 0 if it % 2 == 0 else rng.choice([1, 4, 9])
        with ctx.vcf_session(V, F) as ses:
            info = ses.info()
            assert info["classified_on_device"] == 1, it
            recs = ses.contigs()
            spec = cs.fasta_records(F)
            assert [(r["name"], r["rec_start"], r["rec_end"]) for r in recs] == spec
            seen = set()
            for i, r in enumerate(recs):
                assert r["duplicate"] == (1 if r["name"] in seen else 0)
                if r["duplicate"]:
                    assert r["vcf_records"] == 0
                    with pytest.raises(edsparser_amd.EdsxError):
                        ses.transform(i, l)
                seen.add(r["name"])
            lines = [ln for ln in V.split(b"\n") if cs.is_record_line(ln)]
            assert info["records_total"] == len(lines) and info["records_without_token"] == 0
            assert info["records_unknown_contig"] == 7 and dict(ses.unknown_contigs()) == {b"ghost": 5, b"chr": 2}
            for k, nm in enumerate(names):
                assert ses.find(nm) == [r["name"] for r in recs].index(nm)
                assert recs[ses.find(nm)]["vcf_records"] == sum(cs.first_token(ln) == nm for ln in lines)
                assert (recs[ses.find(nm)]["vcf_records"] == 0) == (k == empty)
                assert _res(lambda: ses.transform(nm, l)) == _want(V, F, nm, l), (it, nm, l)
                assert ctx.vcf_tokenised_on_device(), (it, nm)       # no silent fall-back to the host
            info = ses.info()
            assert info["vcf_h2d_bytes"] == len(V) and info["fasta_h2d_bytes"] == len(F), (it, info)   # the inputs travel once
            with pytest.raises(edsparser_amd.EdsxError) as ei:
                ses.find(b"ghost")
            assert ei.value.message == "Contig 'ghost' not found in reference FASTA"
        nm = names[it % len(names)]
        assert _res(lambda: ctx.vcf_transform(V, F, l, contig=nm)) == _want(V, F, nm, l)
        assert ctx.vcf_tokenised_on_device()
        with _host_tokenizer():
            assert _res(lambda: ctx.vcf_transform(V, F, l, contig=nm)) == _want(V, F, nm, l)
            assert not ctx.vcf_tokenised_on_device()
    with pytest.raises(edsparser_amd.EdsxError) as ei:
        ctx.vcf_transform(V, F, 0, contig="nope")
    assert ei.value.message == "Contig 'nope' not found in reference FASTA"
    with pytest.raises(edsparser_amd.EdsxError) as ei:
        ctx.vcf_session(V, b"ACGT\n")
    assert ei.value.message == "Invalid FASTA format: expected header line starting with '>'"


def test_many_contigs_take_two_radix_passes(ctx):
    """More than 255 FASTA records: the contig id needs two 8-bit passes of the stable sort."""
    rng = random.Random(5)
    K = 700
    seqs = [bytes(rng.choices(b"ACGT", k=rng.randint(20, 90))) for _ in range(K)]
    F = b"".join(b">s%d\n%s\n" % (k, _wrap(seqs[k], 30)) for k in range(K))
    lines = []
    for _ in range(6000):
        k = rng.randrange(K + 20)                                    # s700..s719: not in the FASTA
        p = rng.randint(1, 20)
        ref = seqs[k][p - 1:p] if k < K else b"A"
        lines.append(b"s%d\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT\t%d|%d" % (k, p, ref, b"ACGT".replace(ref, b"")[:1], rng.random() < .5, rng.random() < .5))
    V = b"##fileformat=VCFv4.2\n" + b"\n".join(lines) + b"\n"
    with ctx.vcf_session(V, F) as ses:
        assert ses.info()["classified_on_device"] == 1
        assert ses.info()["records_unknown_contig"] == sum(int(ln.split(b"\t")[0][1:]) >= K for ln in lines)
        for k in list(range(0, K, 37)) + [255, 256, 257, 511, 512, K - 1]:
            nm = b"s%d" % k
            assert _res(lambda: ses.transform(nm)) == _want(V, F, nm, 0), k
            assert ctx.vcf_tokenised_on_device()


# ---- 3. damage ----------------------------------------------------------------------------------------------------
def _seeded_input(seed):
    return _plain_input(random.Random(seed))


def test_damage_in_another_contig_leaves_the_selected_one_alone(ctx, capfd):
    V, F, names, empty = _seeded_input(11)
    sel = names[(empty + 1) % len(names)]
    other = names[(empty + 2) % len(names)]
    base = _want(V, F, sel, 0)
    lines = V.split(b"\n")
    victim = next(i for i, ln in enumerate(lines) if ln.startswith(other + b"\t"))
    f = lines[victim].split(b"\t")
    for what, bad in (("<INV>", b"\t".join(f[:4] + [b"<INV>"] + f[5:])), ("too few fields", b"\t".join(f[:3])),
                      ("junk POS", b"\t".join(f[:1] + [b"12x"] + f[2:]))):
        V2 = b"\n".join(lines[:victim] + [bad] + lines[victim + 1:])
        with ctx.vcf_session(V2, F) as ses:
            assert ses.info()["classified_on_device"] == 1, what
            capfd.readouterr()
            assert _res(lambda: ses.transform(sel)) == base, what
            assert ctx.vcf_tokenised_on_device(), what
            assert "Warning" not in capfd.readouterr().err, what
            assert _res(lambda: ses.transform(other)) == _want(V2, F, other, 0), what       # the damaged contig: host text
            assert not ctx.vcf_tokenised_on_device(), what
            assert _res(lambda: ses.transform(sel)) == base, what


def test_lines_the_device_cannot_classify_go_to_the_host_and_equal_the_spec(ctx):
    V, F, names, empty = _seeded_input(12)
    lines = V.split(b"\n")
    first = next(i for i, ln in enumerate(lines) if cs.is_record_line(ln))
    variants = {
        "leading tab": b"\n".join(lines[:first] + [b"\t" + lines[first]] + lines[first + 1:]),
        "spaces only": b"\n".join(ln if ln.startswith(b"#") else b" ".join(ln.split(b"\t")[:8]) for ln in lines),
        "one spaces-only line": b"\n".join(lines[:first] + [b"  " + b"   ".join(lines[first].split(b"\t"))] + lines[first + 1:]),
        "crlf": b"\r\n".join(lines) + b"\r\n",
        "no token": b"\n".join(lines[:first] + [b" \t "] + lines[first:]),
    }
    for what, V2 in variants.items():
        with ctx.vcf_session(V2, F) as ses:
            info = ses.info()
            assert info["classified_on_device"] == 0, what
            assert info["records_without_token"] == (1 if what == "no token" else 0)
            for nm in names:
                assert _res(lambda: ses.transform(nm)) == _want(V2, F, nm, 0), (what, nm)
            recs = {r["name"]: r for r in ses.contigs() if not r["duplicate"]}
            rl = [ln for ln in V2.split(b"\n") if cs.is_record_line(ln)]
            for nm in names:
                assert recs[nm]["vcf_records"] == sum(cs.first_token(ln) == nm for ln in rl), (what, nm)


# ---- 4. index -----------------------------------------------------------------------------------------------------
def _random_fasta(rng):
    eol = rng.choice([b"\n", b"\n", b"\r\n"])
    out = []
    n = rng.randint(1, 30)
    for k in range(n):
        name = rng.choice([b"chr%d" % rng.randint(1, 12), b"s" * rng.randint(1, 40), b"HLA-A*01:01", b"", b"x" * 1500])
        hdr = b">" + name + rng.choice([b"", b" desc", b"  two  spaces", b"\tTAB"])
        kind = rng.random()
        if kind < 0.15:
            out.append(hdr + eol)                                        # empty record
            continue
        L = rng.choice([1, 5, 59, 60, 61, 1023, 1024, 1025, 3000, 9000])
        w = rng.choice([1, 60, 70, 1024, 20000])
        seq = bytes(rng.choices(b"ACGTN", k=L))
        body = [seq[i:i + w] for i in range(0, L, w)]
        if rng.random() < 0.2:
            body.insert(rng.randint(0, len(body)), b"")                  # a blank line
        if rng.random() < 0.1:
            body.insert(1, b"AC>GT")                                     # '>' inside a line starts nothing
        out.append(hdr + eol + eol.join(body) + eol)
    f = b"".join(out)
    r = rng.random()
    if r < 0.2:
        f += b">last"                                                    # header-only last record, no newline
    elif r < 0.4:
        f += b">last tail" + eol
    elif r < 0.6:
        f = f[:-len(eol)]                                                # no final newline
    return f


def test_fasta_index_equals_the_spec(ctx):
    rng = random.Random(77)
    for it in range(120):
        F = _random_fasta(rng)
        V = b"" if it % 3 else b"chr1\t1\t.\tA\tC\n"
        with ctx.vcf_session(V, F) as ses:
            got = ses.contigs()
            spec = cs.fasta_records(F)
            assert len(got) == len(spec), it
            seen = set()
            for g, (nm, s, e) in zip(got, spec):
                ss, lw, size = cs.fasta_metadata(F, s, e)
                assert (g["name"], g["name_off"], g["rec_start"], g["rec_end"]) == (nm, s + 1, s, e), (it, nm)
                assert (g["seq_start"], g["line_width"], g["seq_size"]) == (ss, lw, size), (it, nm, s, e)
                assert g["duplicate"] == (1 if nm in seen else 0)
                seen.add(nm)
            assert ses.info()["fasta_h2d_bytes"] == len(F)
            if not V:
                assert ses.info()["records_total"] == 0 and ses.info()["vcf_h2d_bytes"] == 0


# ---- 6. full size ------------------------------------------------------------------------------------------------
def test_config3_cut_in_eight_contigs_full_size(ctx):
    """BASELINE configs[3] cut in eight: eight generator outputs (125 Mb reference, 1.25 M records, 8 samples each) as the
    contigs chr1..chr8 of one VCF (~665 MB) and one FASTA (~1 GB); contig k through one session == the oracle on generator
    output k as it came (the oracle ignores CHROM)."""
    import torch
    free, _ = torch.cuda.mem_get_info(0)
    assert free / 2**30 > 24, "needs an (almost) empty MI355X"
    from measure_vcf_contigs import config3_in_eight
    V, F, parts = config3_in_eight(ctx, keep_parts=True)
    want = []
    while parts:
        want.append(o.vcf(*parts.pop(0)))                             # (the generator outputs are dropped as we go)
    assert len(V) > 640e6 and len(F) > 1.0e9
    with ctx.vcf_session(V, F) as ses:
        info = ses.info()
        assert info["classified_on_device"] == 1 and info["records_total"] == 10_000_000 and info["records_unknown_contig"] == 0
        assert [(r["name"], r["vcf_records"], r["seq_size"]) for r in ses.contigs()] == [(b"chr%d" % k, 1_250_000, 125_000_000) for k in range(1, 9)]
        for k in range(1, 9):
            got = ses.transform(b"chr%d" % k)
            assert ctx.vcf_tokenised_on_device()
            assert got[2] == want[k - 1][2], k
            assert got[0] == want[k - 1][0] and got[1] == want[k - 1][1], k
        info = ses.info()
        assert info["vcf_h2d_bytes"] == len(V) and info["fasta_h2d_bytes"] == len(F)


# ---- 7. CLI ----------------------------------------------------------------------------------------------------------
def _cli(*args):
    import edsparser_amd.build as b
    b.build()
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    return subprocess.run([VCF2EDS] + list(args), capture_output=True, text=True)


def test_vcf2eds_chrom_and_all_chroms(ctx, tmp_path):
    V, F, names, empty = _seeded_input(21)
    F += b"\n>broken\n" if not F.endswith(b"\n") else b">broken\n"       # a record without a sequence line ...
    V += b"\nbroken\t1\t.\tA\tC\t.\tPASS\t."                              # ... that the VCF has a record for
    (tmp_path / "in.vcf").write_bytes(V)
    (tmp_path / "ref.fa").write_bytes(F)
    io = ["-i", str(tmp_path / "in.vcf"), "-r", str(tmp_path / "ref.fa")]
    sel = names[(empty + 1) % len(names)]
    # --chrom: naming as without it
    r = _cli(*io, "--chrom", sel.decode())
    assert r.returncode == 0, r.stderr
    assert "  Contig: " + sel.decode() in r.stdout
    w = _want(V, F, sel, 0)
    assert (tmp_path / "in.eds").read_bytes().decode() == w["eds"] and (tmp_path / "in.seds").read_bytes().decode() == w["seds"]
    assert "Total variants read:        %d" % w["stats"]["total_variants"] in r.stdout
    r = _cli(*io, "-c", sel.decode(), "-l", "4", "-o", str(tmp_path / "o.leds"))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "o.leds").read_bytes().decode() == _want(V, F, sel, 4)["eds"]
    r = _cli(*io, "--chrom", "nope")
    assert r.returncode == 1 and "Error: Contig 'nope' not found in reference FASTA" in r.stderr
    r = _cli(*io, "--chrom", "broken")
    assert r.returncode == 1 and "Error: FASTA file is empty" in r.stderr
    # --all-chroms: one pair of files per FASTA record with VCF records; the broken one fails alone
    out = tmp_path / "out"
    r = _cli(*io, "--all-chroms", "--output-dir", str(out))
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert "Error [broken]: FASTA file is empty" in r.stderr
    assert "contig 'ghost' has 5 VCF record line(s)" in r.stderr and "contig 'chr' has 2 VCF record line(s)" in r.stderr
    expect_files = set()
    for k, nm in enumerate(names):
        if k == empty:
            continue
        w = _want(V, F, nm, 0)
        assert (out / ("in.%s.eds" % nm.decode())).read_bytes().decode() == w["eds"], nm
        assert (out / ("in.%s.seds" % nm.decode())).read_bytes().decode() == w["seds"], nm
        expect_files |= {"in.%s.eds" % nm.decode(), "in.%s.seds" % nm.decode()}
        assert "Contig %s\n" % nm.decode() in r.stdout
    assert set(os.listdir(out)) == expect_files
    nrec = sum(cs.is_record_line(ln) for ln in V.split(b"\n"))
    assert "VCF record lines: %d total, 0 without a token, 7 of contigs the reference lacks" % nrec in r.stdout
    # l > 0 names, default directory = the input's
    (tmp_path / "ref2.fa").write_bytes(F[:F.rindex(b">broken")])
    r = _cli("-i", str(tmp_path / "in.vcf"), "-r", str(tmp_path / "ref2.fa"), "--all-chroms", "-l", "3")
    assert r.returncode == 0, r.stderr
    assert "contig 'broken' has 1 VCF record line(s)" in r.stderr
    w = _want(V, F, sel, 3)
    assert (tmp_path / ("in.%s_l3.leds" % sel.decode())).read_bytes().decode() == w["eds"]
    assert (tmp_path / ("in.%s_l3.seds" % sel.decode())).read_bytes().decode() == w["seds"]
