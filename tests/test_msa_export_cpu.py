"""CPU: the alignment export specification itself (tests/msa_export_spec.py) against the oracle's msa2eds: the rows of
align(msa2eds(A)) are the rows of A, align is a fixed point of msa2eds o align on every EDS that came from msa2eds, and on
the merge and VCF fixtures every path of msa2eds(align(E)) spells what it spelled in E."""
import random

import msa_export_spec as ms
import oracle_lib as o
import path_spec as ps
from test_paths_cpu import _random_msa, merge_fixture_inputs, vcf_fixture_outputs


def _alignments(count, seed):
    """(alignment text, its rows without gaps) with at least two rows of which two differ (else the EDS has no path)"""
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        msa, rows = _random_msa(rng, wrap=len(out) % 2 == 1)
        if len(set(rows)) >= 2 and any(rows):
            out.append((msa, rows))
    return out


def test_rows_without_gaps_are_the_input_rows():
    checked = 0
    for msa, rows in _alignments(150, 20260101):
        for l in (0, 3):
            eds, seds = o.msa(msa, l)
            syms, sets, P = ps.parse(eds, seds)
            assert P == len(rows)
            got = ms.rows_of(ms.align(eds, seds, None, 0, prefix=b"s")[0])
            assert [n for n, _ in got] == [b"s%d" % (k + 1) for k in range(P)]
            assert len({len(r) for _, r in got}) == 1 and len(got[0][1]) == ms.info(eds, seds)["n_columns"]
            assert [r.replace(b"-", b"") for _, r in got] == rows, (msa, l)
            for lw in (1, 7, 60):                                # wrapping changes the line feeds alone
                assert ms.rows_of(ms.align(eds, seds, None, lw, prefix=b"s")[0]) == got
            checked += 1
    assert checked == 300


def test_align_is_a_fixed_point_on_msa2eds_results():
    """Every string of msa2eds(A) is taken by some path, so align leaves no all-gap column and msa2eds (l = 0) of the
    alignment gives back an EDS with the same alignment, byte for byte."""
    checked = 0
    for msa, rows in _alignments(150, 7):
        for l in (0, 3):
            eds, seds = o.msa(msa, l)
            a1, m1 = ms.align(eds, seds, None, 0)
            assert ms.info(eds, seds)["n_columns"] >= 1 and ps.parse(eds, seds)[2] >= 2 and m1 == [0] * len(rows)
            eds2, seds2 = o.msa(a1, 0)
            assert ms.align(eds2, seds2, None, 0) == (a1, m1), (msa, l)
            checked += 1
    assert checked == 300


def test_one_row_and_equal_rows():
    """What bounds the inputs above: the oracle refuses one row, and rows that do not differ give an EDS without paths."""
    try:
        o.msa(b">a\nACGT\n", 0)
        assert False
    except o.OracleError as ex:
        assert "MSA needs >= 2 sequences" in str(ex)
    eds, seds = o.msa(b">a\nACGT\n>b\nACGT\n", 0)
    assert ps.parse(eds, seds)[2] == 0 and ms.align(eds, seds) == (b"", [])


def test_fixture_paths_survive_the_round_trip():
    """Strings no path takes leave all-gap columns, so the fixed point is not claimed here: every path of
    msa2eds(align(E)) spells what it spelled in E."""
    ran = skipped = 0
    for eds, seds in merge_fixture_inputs() + vcf_fixture_outputs():
        try:
            syms, sets, P = ps.parse(eds, seds)
        except ValueError:                                       # fixtures whose sources do not match their text
            skipped += 1
            continue
        if P < 2 or sum(ms.widths(syms)) < 1:                    # the oracle needs two rows and a column
            skipped += 1
            continue
        a, miss = ms.align(eds, seds, None, 0)
        assert all(len(r) == sum(ms.widths(syms)) for _, r in ms.rows_of(a))
        eds2, seds2 = o.msa(a, 0)
        syms2, sets2, _ = ps.parse(eds2, seds2)
        for p in range(1, P + 1):
            assert ps.spell(syms2, sets2, p)[0] == ps.spell(syms, sets, p)[0], (eds, seds, p)
        ran += 1
    print("fixture cases: ran %d, skipped %d" % (ran, skipped))
    assert ran >= 250


def test_gap_bytes_and_limit():
    eds, seds = b"{AC}{G,TTT,}{A}", b"{0}{1}{2}{3}{0}"
    assert ms.align(eds, seds, None, 0, gap=b".")[0] == b">path1\nACG..A\n>path2\nACTTTA\n>path3\nAC...A\n"
    assert ms.align(eds, seds, [2, 1], 4, names=[b"x", b"y"])[0] == b">x\nACTT\nTA\n>y\nACG-\n-A\n"
    assert ms.align(b"{AC}{G,T}", b"{0}{1}{3}", [2], 0) == (b">path2\nAC-\n", [1])
    for g in ms.BAD_GAPS:
        try:
            ms.align(eds, seds, gap=bytes([g]))
            assert False
        except ValueError as ex:
            assert str(ex) == "Gap character is not usable in an alignment"
    n = ms.size(eds, seds, None, 0)
    assert n == len(ms.align(eds, seds, None, 0, max_bytes=n)[0])
    try:
        ms.align(eds, seds, None, 0, max_bytes=n - 1)
        assert False
    except ValueError as ex:
        assert str(ex) == "Alignment has %d bytes, above the limit of %d" % (n, n - 1)
