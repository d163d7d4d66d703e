"""CPU: the per-thread device code of the VCF transform (csrc/vcf_walk.hpp) as host code under the address and
undefined-behaviour sanitizers (tests/cpp/test_vcf_walk.cpp, a stand-alone program), on buffers of exactly the sizes the
library allocates, filled with NUL, line feeds, 0xFF or tabs.  Every load and store of that source is checked there, the
masked ones the guard build cannot see included; the texts must equal the oracle's under every fill.  Equal positions
change only the record order, through the host's unstable sort: no case compared in full has them."""
import random
import time

import pytest

import oracle_lib as o
import vcf_cases as vc
import vcf_walk_cases as w


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    d = tmp_path_factory.mktemp("vcf_walk")
    return w.build_test_vcf_walk(w.ROOT, str(d / "test_vcf_walk")), str(d)


def _oracle(vcf, fasta):
    try:
        e, s, _ = o.vcf(vcf, fasta, 0)
        return e, s
    except o.OracleError:
        return None


def _compare(twin, named, tag, fills=w.FILLS):
    """named: (name, vcf, fasta) with pairwise distinct positions.  The whole transform under every fill: where the count
    pass accepts the file the texts must be the oracle's, otherwise only the verdict and the clean exit are asserted.
    Returns the number of cases compared in full."""
    exe, workdir = twin
    for name, vcf, _ in named:
        assert w.distinct_positions(vcf), name
    res = w.run_twin(exe, workdir, [(w.FULL, fills, name, vcf, fasta) for name, vcf, fasta in named], tag)
    full = 0
    for name, vcf, fasta in named:
        runs = res[name]
        assert [r[0] for r in runs] == list(fills), name
        verdicts = {r[1] for r in runs}
        assert len(verdicts) == 1, (name, runs)                # the verdict does not depend on the fill
        verdict = verdicts.pop()
        assert verdict in (w.ACCEPTED, w.NOT_PLAIN, w.REFUSED), (name, verdict, runs[0][2])
        if verdict == w.ACCEPTED:
            want = _oracle(vcf, fasta)
            assert want is not None, name
            for fill, _, _, eds, seds in runs:
                assert (eds, seds) == want, (name, fill)
            full += 1
    return full


def test_reference_fixtures(twin):
    """Every input of gen_vcf.json and of the round-2 set.  Files with equal positions (the round-2 set is built around
    them) go through the count pass only - what the device runs on them before the order is the host sort's."""
    exe, workdir = twin
    cases = w.fixture_cases()
    distinct = [c for c in cases if w.distinct_positions(c[1])]
    equal = [c for c in cases if not w.distinct_positions(c[1])]
    assert len(cases) > 40 and len(distinct) > 20
    full = _compare(twin, distinct, "fixtures")
    res = w.run_twin(exe, workdir, [(w.COUNT, w.FILLS, n, v, f) for n, v, f in equal], "fixtures_count")
    for name, _, _ in equal:
        assert len({r[1] for r in res[name]}) == 1 and res[name][0][1] in (w.ACCEPTED, w.NOT_PLAIN), name
    print("fixtures: %d compared in full, %d with distinct positions, %d count pass only" % (full, len(distinct), len(equal)))
    assert full > 10


def test_existing_edge_files(twin):
    """vcf_cases.text_length_files in full; vcf_cases.single_damage_files (one oddity per file) through the count pass,
    which reads every such file on the device before the host tokeniser gets it."""
    exe, workdir = twin
    fasta, mod8, sized = vc.text_length_files(random.Random(88))
    named = [("mod8/%d" % i, vcf, fasta) for i, (_, _, _, vcf) in enumerate(mod8)] + [("sized256/%d" % t, vcf, fasta) for t, vcf in sized]
    assert _compare(twin, named, "edge_lengths") == len(named)
    damaged = [("damage/%d/%s" % (i, kind), v, f) for i, (kind, ch, ns, tail, line, v, f) in enumerate(vc.single_damage_files(random.Random(808)))]
    assert len(damaged) > 150
    res = w.run_twin(exe, workdir, [(w.COUNT, w.FILLS, n, v, f) for n, v, f in damaged], "edge_damage")
    taken = {w.ACCEPTED: 0, w.NOT_PLAIN: 0}
    for name, _, _ in damaged:
        verdicts = {r[1] for r in res[name]}
        assert len(verdicts) == 1 and verdicts <= set(taken), (name, res[name])
        taken[verdicts.pop()] += 1
    assert taken[w.ACCEPTED] > 20 and taken[w.NOT_PLAIN] > 60, taken


def test_text_lengths_and_open_last_lines(twin):
    rng = random.Random(5151)
    sized, opened = w.sized_texts(rng), w.open_ended_texts(rng)
    assert _compare(twin, sized, "sized") == len(sized)
    full = _compare(twin, opened, "open")
    # a last line that ends in a tab has an empty field: not plain; the other three endings are
    assert full == len(opened) - 16, full


def test_random_families(twin):
    named = w.random_families()
    t0 = time.time()
    full = _compare(twin, named, "random")
    print("random families: %d cases, %d compared in full, %.1f s" % (len(named), full, time.time() - t0))
    assert len(named) == len(w.SAMPLES) * len(w.WIDTHS) * 6
    assert full * 100 >= 95 * len(named), (full, len(named))
    for feat in w.FEATURES:                                   # (the names list the features a file really shows)
        shown = sum(feat in n.rsplit("/", 1)[1].split("+") for n, _, _ in named)
        print(feat, shown)
        assert shown >= 20, feat


def test_fa_cpos_windows(twin):
    """fa_cpos alone over every file offset of a window, against a byte-by-byte count: windows starting at every residue
    modulo 256 with lengths of every residue modulo 8, and windows that end at or one byte before the end of the file."""
    exe, workdir = twin
    cases = w.cpos_windows(random.Random(77))
    res = w.run_twin(exe, workdir, [(mode, w.FILLS, name, b"", fasta, up0, up1) for mode, name, fasta, up0, up1 in cases], "cpos")
    assert len(cases) >= 256 * 10
    for _, name, _, _, _ in cases:
        for fill, verdict, detail, _, _ in res[name]:
            assert verdict == w.ACCEPTED, (name, fill, verdict, detail)


def test_the_call_on_record(twin):
    """The input of test_larger_sharded_equals_unpartitioned (seed 11, 10 Mb reference, 10^5 records, 8 samples), the call
    in which the device tokeniser faulted in rounds 2 and 3: one case, under every fill."""
    vcf, fasta = w.call_on_record()
    t0 = time.time()
    assert _compare(twin, [("call_on_record", vcf, fasta)], "record") == 1
    print("the call on record under the sanitizers: %.1f s" % (time.time() - t0))
