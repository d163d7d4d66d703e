"""CPU tests: the MSA oracle (oracle/msa_oracle.cpp, a transliteration of the reference's stream code) against the
column-wise specification (tests/msa_spec.py, written from the meaning of the operation).  Two restatements made by
different methods have to agree byte for byte on both texts: on the known-answer vectors, on EVERY local pattern of
common and variant runs (all masks of 1..12 columns, l = 0..5, one-line and wrapped rows), on every alignment over
{A, C, -} of 2 x 5 and 3 x 3, and on the random families the GPU tests use.  The oracle's outputs also pass three
checks that know neither restatement: every row comes back as its path, the source sets partition the rows, and the
l-EDS passes is_leds (pinned to the compiled reference by tests/golden/gen2_stats.json)."""
import itertools
import json
import os
import random

import pytest

import msa_spec as spec
import oracle_lib as o
from conftest import GOLDEN
from msa_cases import campaign_msa, random_msa, wide_msa


class Tally:
    def __init__(self):
        self.cases = self.checked = self.leds_seen = self.leds_premise = 0

    def __str__(self):
        return ("%d cases byte-equal, closure + partition on %d, is_leds premise held on %d of %d l > 0 cases"
                % (self.cases, self.checked, self.leds_premise, self.leds_seen))


def _fasta(rows, lw=None, final_newline=True):
    out = []
    for i, r in enumerate(rows):
        out.append(b">r%d" % i)
        w = lw or len(r)
        out.extend(r[k:k + w] for k in range(0, len(r), w))
    return b"\n".join(out) + (b"\n" if final_newline else b"")


def _equal(al, msa, l, t, want=None):
    """The oracle's output for the text `msa`, after it was found equal to the specification's for its alignment
    (`want`, where the caller has it from another text of the same alignment)."""
    got = o.msa(msa, l)
    assert got == (want or al.transform(l)), (l, msa)
    t.cases += 1
    return got


def _checkers(al, l, out, t):
    """closure, partition and (l > 0, under its premise) is_leds on the oracle's output of a NUL-free input."""
    eds, seds = out
    spec.closure_rows(al.rows, eds, seds)
    spec.partition(eds, seds, len(al.rows))
    t.checked += 1
    if l > 0:
        t.leds_seen += 1
        if spec.every_segment_has_two_strings(eds):
            t.leds_premise += 1
            assert o.eds_stats(eds, seds, l)["is_leds"] == 1, (l, al.rows, eds)


# ---- the known-answer vectors, against the specification directly ----

@pytest.mark.parametrize("case", json.load(open(os.path.join(GOLDEN, "kat_msa.json")))["cases"], ids=lambda c: c["name"])
def test_known_answer_vectors(case):
    msa = case["msa"].encode() if "msa" in case else open(os.path.join(GOLDEN, case["msa_file"]), "rb").read()
    eds, seds = spec.transform(msa, case["l"])
    assert eds.decode() == case["eds"]
    assert seds.decode() == case["seds"]


# ---- every mask of 1..12 columns ----

def _mask_rows(n, mask, gaps):
    """Two rows of n columns; row 2 differs from row 1 exactly on the columns of `mask`: by another letter or, with
    `gaps`, by a gap on every third column."""
    ref = bytes(b"ACGT"[c & 3] for c in range(n))
    alt = bytes((0x2D if gaps and c % 3 == 0 else b"CGTA"[c & 3]) if mask >> c & 1 else ref[c] for c in range(n))
    return [ref, alt]


def test_every_mask_of_1_to_12_columns():
    t = Tally()
    for n in range(1, 13):
        for mask in range(1 << n):
            rows = _mask_rows(n, mask, gaps=True)
            one, wrapped = _fasta(rows), _fasta(rows, lw=3)
            assert spec.rows(one) == spec.rows(wrapped) == rows        # the specification reads one alignment from both
            al = spec.Alignment(rows)
            for l in range(6):
                out = _equal(al, one, l, t)
                _equal(al, wrapped, l, t, want=out)
                _checkers(al, l, out, t)
    print("\nmasks of 1..12 columns: %s" % t)
    assert t.cases == 98_280 and t.checked == t.cases // 2


def test_substitution_only_masks_are_l_eds():
    """Without gaps two rows never spell one string in a variant segment, so the premise of the is_leds check holds
    for every mask and every l: the oracle's l-EDS of each passes the check the compiled reference pins."""
    t = Tally()
    for n in range(1, 13):
        for mask in range(1 << n):
            rows = _mask_rows(n, mask, gaps=False)
            msa = _fasta(rows)
            al = spec.Alignment(spec.rows(msa))
            for l in range(1, 6):
                _checkers(al, l, _equal(al, msa, l, t), t)
    print("\nsubstitution-only masks: %s" % t)
    assert t.leds_premise == t.leds_seen == 40_950


# ---- every alignment over {A, C, -} of 2 x 5 and of 3 x 3 ----

@pytest.mark.parametrize("S,L", [(2, 5), (3, 3)])
def test_every_alignment_over_A_C_gap(S, L):
    """Includes columns that are all gaps, gaps in the reference row, rows that spell one string with their gaps placed
    differently, and alignments without a variant column."""
    t = Tally()
    for cells in itertools.product(b"AC-", repeat=S * L):
        rows = [bytes(cells[r * L:(r + 1) * L]) for r in range(S)]
        one, wrapped = _fasta(rows), _fasta(rows, lw=2, final_newline=False)
        assert spec.rows(one) == spec.rows(wrapped) == rows        # the specification reads one alignment from both
        al = spec.Alignment(rows)
        for l in range(4):
            out = _equal(al, one, l, t)
            _equal(al, wrapped, l, t, want=out)
            _checkers(al, l, out, t)
    print("\n{A, C, -} alignments of %d x %d: %s" % (S, L, t))
    assert t.cases == 3 ** (S * L) * 8


# ---- the random families of the GPU parity tests ----

def test_random_alignments():
    t = Tally()
    rng = random.Random(20)
    for i in range(3000):
        msa = random_msa(rng, trailing_newline=(i % 3 != 0))
        al = spec.Alignment(spec.rows(msa))
        for l in (0, 1, 2, 3, 5, 8, 32):
            _checkers(al, l, _equal(al, msa, l, t), t)
    print("\nrandom_msa: %s" % t)
    assert t.cases == 21_000
    assert 2 * t.leds_premise >= t.leds_seen


def test_wide_segments_and_nul_bytes():
    t = Tally()
    rng = random.Random(21)
    for i in range(150):
        nul = i % 2 == 1
        msa = wide_msa(rng, nul=nul)
        al = spec.Alignment(spec.rows(msa))
        for l in (0, 3, 10):
            out = _equal(al, msa, l, t)
            if b"\0" not in msa:
                _checkers(al, l, out, t)
    print("\nwide_msa: %s" % t)
    assert t.cases == 450 and t.checked >= 225


def test_campaign_alignments():
    """The generator of the randomized GPU campaign (row counts around every kernel switch, five alphabets, site and
    gap densities from 0 to 1, lines of one column, doubled final newline), capped at 200 000 cells."""
    t = Tally()
    rng = random.Random(22)
    for _ in range(60):
        msa, desc = campaign_msa(rng, max_cells=200_000)
        al = spec.Alignment(spec.rows(msa))
        for l in (0, rng.choice([1, 2, 5, 9, 33])):
            _checkers(al, l, _equal(al, msa, l, t), t)
    print("\ncampaign_msa: %s" % t)


# ---- the masks of the GPU tests ----

@pytest.mark.parametrize("n", [8, 10, 12])
def test_the_gpu_masks_hold_every_window_at_every_phase(n):
    """B(2, n) is a de Bruijn sequence, and the mask built from it has every n-column window at each of the 64 column
    phases of the device's boundary words."""
    from msa_spec_cases import check_mask
    check_mask(n)


# ---- the checkers themselves ----

def test_spell_all_is_path_spec_spell():
    """closure() spells all paths in one walk; it is path_spec.spell, path by path."""
    import path_spec
    rng = random.Random(23)
    for _ in range(200):
        msa = random_msa(rng, p_var=0.3)
        S = len(spec.rows(msa))
        for l in (0, 3):
            eds, seds = spec.transform(msa, l)
            syms, sets, _ = path_spec.parse(eds, seds)
            assert spec.spell_all(eds, seds, S) == [path_spec.spell(syms, sets, p)[0] for p in range(1, S + 1)]


def test_checkers_refuse_wrong_texts():
    msa = b">a\nACGTA\n>b\nAC-TA\n>c\nACCTA\n"
    eds, seds = spec.transform(msa, 0)
    assert (eds, seds) == (b"{AC}{G,,C}{TA}", b"{0}{1}{2}{3}{0}")
    spec.closure(msa, eds, seds)
    spec.partition(eds, seds, 3)
    with pytest.raises(AssertionError):
        spec.closure(msa, b"{AC}{G,,C}{T}", b"{0}{1}{2}{3}{0}")                 # a column lost
    with pytest.raises(AssertionError):
        spec.closure(msa, eds, b"{0}{1}{3}{2}{0}")                              # two rows exchanged
    for bad_eds, bad_seds in [(eds, b"{0}{1}{2}{2,3}{0}"),                      # an id twice
                              (eds, b"{0}{1}{2}{4}{0}"),                        # an id outside 1..S
                              (eds, b"{0}{2}{1}{3}{0}"),                        # not in order of first appearance
                              (b"{AC}{G,G,C}{TA}", seds),                       # one string twice
                              (b"{AC}{G,C}{TA}", b"{0}{1}{3,2}{0}")]:           # a set that does not ascend
        with pytest.raises(AssertionError):
            spec.partition(bad_eds, bad_seds, 3)
    assert spec.every_segment_has_two_strings(eds)
    assert not spec.every_segment_has_two_strings(b"{AC}{G}{TA}")


def test_inputs_outside_the_domain_raise():
    for bad in [b"", b"ACGT\n", b">a\nACGT\n", b">a\nACGT\n>b\nAC\n", b">a\nACGT\n>b\nACGTA\n", b">a\n>b\n"]:
        with pytest.raises(ValueError):
            spec.transform(bad, 0)
