"""GPU: the directed inputs of tests/contig_walk_cases.py through ctx.vcf_session against tests/contig_spec.py and the
oracle (tests/contig_walk_expect.py): every field of every FASTA record, the counters of the session, the contigs the
FASTA lacks, the verdict "classified on the device" case by case, and the picked contigs' texts, counters and error
texts.  Which tokeniser a contig's lines went through must be what the host program says - the same source on the CPU,
built here without sanitizers (tests/cpp/test_contig_walk.cpp)."""
import pytest

import contig_walk_cases as w
import contig_walk_expect as x

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    c = edsparser_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def families():
    return w.families()


@pytest.fixture(scope="module")
def program(tmp_path_factory, families):
    """{case name: the host program's run under one fill}, from one run of a plain build: verdicts only"""
    d = tmp_path_factory.mktemp("contig_walk")
    exe = w.build_test_contig_walk(w.ROOT, str(d / "test_contig_walk"), sanitize=False)
    cases = [dict(c, fills=(0x0A,)) for fam in families.values() for c in fam]
    res = w.run_program(exe, str(d), cases, x.records_of, "gpu_cases")
    return {name: runs[0] for name, runs in res.items()}


def _transform(ses, name):
    import edsparser_amd
    try:
        e, s, st = ses.transform(name, 0)
        return {"eds": e, "seds": s, "stats": st}
    except edsparser_amd.EdsxError as ex:
        return {"error": ex.message}


def _check(ctx, program, cases):
    """every case of one family; returns (cases run, sessions classified on the device, contigs transformed)"""
    ran = on_device = transformed = 0
    for case in cases:
        V, F, tag = case["V"], case["F"], case["name"]
        e = x.expected(case)
        twin = program[tag]
        assert twin["status"] == w.OK, tag
        with ctx.vcf_session(V, F) as ses:
            info = ses.info()
            assert info["classified_on_device"] == (0 if e["host"] else 1), tag
            assert (info["records_total"], info["records_without_token"], info["records_unknown_contig"]) == (e["nr"], e["without_token"], e["unknown"]), tag
            assert ses.unknown_contigs() == e["unknown_names"], tag
            got = ses.contigs()
            assert len(got) == e["K"], tag
            for i, g in enumerate(got):
                want = tuple(int(v) for v in e["recs"][i]) + (int(e["counts"][i]), int(e["duplicate"][i]))
                assert tuple(g[f] for f in w.REC_FIELDS) == want and g["name"] == e["names"][i], (tag, i, g)
            for nm, tc in zip(case["pick"], twin["contigs"]):
                want = x.expected_texts(case, nm)
                assert _transform(ses, nm) == want, (tag, nm)
                if "error" not in want:
                    assert ctx.vcf_tokenised_on_device() == (not tc["host_tokeniser"]), (tag, nm)
                transformed += 1
            on_device += info["classified_on_device"]
        ran += 1
    return ran, on_device, transformed


def test_fasta_index_shift_sweep(ctx, program, families):
    cases = families["shift"]
    ran, on_device, _ = _check(ctx, program, cases)
    assert ran == on_device == len(cases) >= 60


def test_fasta_index_ends_edges_and_long_walks(ctx, program, families):
    cases = families["ends"] + families["walks"]
    ran, on_device, _ = _check(ctx, program, cases)
    assert ran == on_device == len(cases) == len(w.END_TARGETS) * 5 + 4 + 22


def test_fasta_index_two_scan_tiles(ctx, program, families):
    ran, on_device, transformed = _check(ctx, program, families["tile"])
    assert (ran, on_device, transformed) == (1, 1, 6)


def test_classification_names(ctx, program, families):
    cases = families["names"]
    ran, on_device, _ = _check(ctx, program, cases)
    assert ran == on_device == len(cases) == 25


def test_classification_host_bound(ctx, program, families):
    cases = families["hostbound"]
    ran, on_device, _ = _check(ctx, program, cases)
    assert (ran, on_device) == (len(cases), 0) and len(cases) == 7


def test_record_count_switches(ctx, program, families):
    cases = families["counts"]
    assert [x.expected(c)["K"] for c in cases] == [255, 256, 65535, 65536, 256, 256, 256]
    ran, on_device, _ = _check(ctx, program, cases)
    assert ran == on_device == len(cases)
