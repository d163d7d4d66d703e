"""CPU: the contig-selection specification (tests/contig_spec.py) against the reference-generated fixtures, the new C ABI
symbols, and the vcf2eds flags --chrom / --all-chroms / --output-dir with their conflicts (no device is touched)."""
import os
import re
import subprocess

import oracle_lib as o
from conftest import GOLDEN
import contig_spec as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "edsparser_amd", "host")
VCF2EDS = os.path.join(HOST, "build", "vcf2eds")


def _run(fn, v, f, l):
    try:
        e, s, st = fn(v, f, l)
        return {"eds": e.decode(), "seds": s.decode(), "stats": st}
    except Exception as ex:
        return {"error": str(ex)}


def test_spec_on_composed_fixtures_equals_the_reference_generated_answers():
    """All 366 fixtures, renamed to eight contig names with prefix relations, combined eight at a time, split again by the
    spec: the oracle (and the compiled reference, where it was built) on (V_c, F_c) gives the fixture's expect."""
    cases = cs.load_fixtures(GOLDEN)
    assert len(cases) == 366
    compared = 0
    for V, F, parts, left in cs.compose(cases, seed=1):
        assert not left, [c.get("name") for c in left]
        assert len({nm for nm, _ in parts}) == len(parts)
        for nm, c in parts:
            vc, fc = cs.split(V, F, nm)
            assert _run(o.vcf, vc, fc, c["l"]) == c["expect"], (nm, c.get("name"))
            if o.have_ref():
                assert _run(o.ref_vcf, vc, fc, c["l"]) == c["expect"], (nm, c.get("name"))
            compared += 1
    assert compared == 366


def test_spec_helpers():
    f = b">a desc\nACGT\nAC\n>b\n\n>a\nTT\n>c"
    recs = cs.fasta_records(f)
    assert [r[0] for r in recs] == [b"a", b"b", b"a", b"c"]
    assert cs.fasta_metadata(f, *recs[0][1:]) == (8, 4, 6)
    assert cs.fasta_metadata(f, *recs[1][1:]) == (19, 0, 0)
    assert cs.fasta_metadata(f, *recs[3][1:]) == (len(f), 0, 0)
    v = b"#h\nchr1\t1\nchr10\t2\n\n \t\n  chr1 3\n"
    assert cs.split(v, b">chr1\nA\n", b"chr1")[0] == b"#h\nchr1\t1\n\n  chr1 3\n"


def test_library_exports_the_session_entry_points():
    import edsparser_amd.build as b
    lib = b.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (edsx_[a-z_]+)", out))
    want = {"edsx_vcf_session_open", "edsx_vcf_session_contigs", "edsx_vcf_session_find", "edsx_vcf_session_transform",
            "edsx_vcf_session_info", "edsx_vcf_session_unknown_contigs", "edsx_vcf_session_close", "edsx_vcf_transform_contig"}
    assert want <= exported, sorted(want - exported)
    hdr = open(os.path.join(ROOT, "include", "edsx.h")).read()
    assert want <= set(re.findall(r"\b(edsx_[a-z_]+)\s*\(", hdr))


def _vcf2eds(*args):
    import edsparser_amd.build as b
    b.build()
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    return subprocess.run([VCF2EDS] + list(args), capture_output=True, text=True)


def test_vcf2eds_help_lists_the_contig_flags():
    r = _vcf2eds("--help")
    assert r.returncode == 0
    for flag in ("--chrom", "--all-chroms", "--output-dir"):
        assert flag in r.stdout, flag


def test_vcf2eds_flag_conflicts_exit_1_before_any_device_work(tmp_path):
    (tmp_path / "a.vcf").write_bytes(b"chr1\t1\t.\tA\tC\n")
    (tmp_path / "a.fa").write_bytes(b">chr1\nACGT\n")
    io = ["-i", str(tmp_path / "a.vcf"), "-r", str(tmp_path / "a.fa")]
    for extra, what in ((["--chrom", "chr1", "--all-chroms"], "--chrom and --all-chroms exclude each other"),
                        (["--all-chroms", "-o", str(tmp_path / "x.eds")], "--output-dir, not -o / -s"),
                        (["--all-chroms", "-s", str(tmp_path / "x.seds")], "--output-dir, not -o / -s"),
                        (["--all-chroms", "--gpus", "2"], "cannot be combined with --gpus"),
                        (["--chrom", "chr1", "--gpus", "1"], "cannot be combined with --gpus"),
                        (["--output-dir", str(tmp_path)], "--output-dir needs --all-chroms")):
        r = _vcf2eds(*(io + extra))
        assert r.returncode == 1, (extra, r.stdout, r.stderr)
        assert what in r.stderr, (extra, r.stderr)
        assert "hip" not in r.stderr.lower() and "device" not in r.stderr.lower(), r.stderr
        assert not list(tmp_path.glob("*.eds")) and not list(tmp_path.glob("*.seds"))
