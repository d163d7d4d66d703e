"""GPU: the directed and random inputs of the host twin that are new to the suite (tests/vcf_walk_cases.py) through
ctx.vcf_transform against the oracle, and the way each call went: the device tokeniser must have taken a file exactly
where the twin's count pass - the same source, on the CPU, built here without sanitizers - accepts it.  (The 10 Mb call
is in test_vcf_shard_gpu.py.)"""
import random

import pytest

import oracle_lib as o
import vcf_walk_cases as w

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    c = edsparser_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    """{name: the twin's count-pass verdict} of every case of this file, from one run of the program"""
    d = tmp_path_factory.mktemp("vcf_walk")
    exe = w.build_test_vcf_walk(w.ROOT, str(d / "test_vcf_walk"), sanitize=False)      # plain build: verdicts only
    res = w.run_twin(exe, str(d), [(w.COUNT, (0x0A,), n, v, f) for n, v, f in _cases()], "gpu_cases")
    return {name: runs[0][1] for name, runs in res.items()}


_CASES = None


def _cases():
    global _CASES
    if _CASES is None:
        rng = random.Random(5151)
        _CASES = w.sized_texts(rng) + w.open_ended_texts(rng) + w.random_families()
    return _CASES


def _check(ctx, verdicts, named):
    on_device = 0
    for name, vcf, fasta in named:
        want = o.vcf(vcf, fasta, 0)
        assert ctx.vcf_transform(vcf, fasta, 0) == want, name
        assert verdicts[name] in (w.ACCEPTED, w.NOT_PLAIN), (name, verdicts[name])
        assert ctx.vcf_tokenised_on_device() == (verdicts[name] == w.ACCEPTED), name
        on_device += ctx.vcf_tokenised_on_device()
    return on_device


def test_text_lengths_and_open_last_lines(ctx, verdicts):
    named = [c for c in _cases() if c[0].startswith(("sized/", "open/"))]
    assert len(named) == 30 + 64
    assert _check(ctx, verdicts, named) == len(named) - 16          # (a last line ending in a tab has an empty field)


def test_random_families(ctx, verdicts):
    named = [c for c in _cases() if c[0].startswith("random/")]
    assert len(named) == len(w.SAMPLES) * len(w.WIDTHS) * 6
    assert _check(ctx, verdicts, named) * 100 >= 95 * len(named)
