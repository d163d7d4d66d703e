"""GPU tests: the MSA -> EDS / l-EDS kernels against the column-wise specification (tests/msa_spec.py), never against
the oracle.  The l-EDS boundaries are computed on the device from 64-column words with a carry bit across word edges
(k_runstart_words, k_seg_flags, k_write_segs): here EVERY local pattern of common and variant runs meets every one of
the 64 column phases of those words, every short alignment decides the "starts at column 0" / "ends at the last
column" exemptions, and merged segments sit on the limits of the staging and row-loop kernels."""
import functools
import re

import numpy as np
import pytest

import msa_spec as spec
from msa_spec_cases import DNA, A65, alignment, alphabet, chain, chains, check_mask, fasta

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    c = edsparser_amd.Context(0)
    yield c
    c.close()


def same(got, want, what):
    """Byte equality of both texts, with a short report (the texts are megabytes long)."""
    for name, g, w in zip((".eds", ".seds"), got, want):
        if g != w:
            n = min(len(g), len(w))
            d = next((i for i in range(n) if g[i] != w[i]), n)
            raise AssertionError("%s: %s differs at byte %d of %d / %d: got %r, specified %r"
                                 % (what, name, d, len(g), len(w), g[max(0, d - 30):d + 30], w[max(0, d - 30):d + 30]))


@functools.lru_cache(maxsize=1)
def case(rows, layouts):
    """-> (the texts of the alignment, its specification): built once for the tests that differ in l only."""
    rows = list(rows)
    texts = [fasta(rows, lw) for lw in layouts]
    al = spec.Alignment(spec.rows(texts[0]))
    assert al.rows == rows and all(spec.rows(t) == rows for t in texts[1:])
    return texts, al


def check(ctx, rows, l, layouts, what):
    """The library on every text of the alignment: equal to the specification, every row comes back as its path, and
    for l > 0 the device's own is_leds holds (its premise is a property of these alignments: asserted)."""
    texts, al = case(tuple(rows), layouts)
    want = al.transform(l)
    for lw, text in zip(layouts, texts):
        got = ctx.msa_transform(text, l)
        same(got, want, "%s l=%d line width %s" % (what, l, lw))
    spec.closure_rows(rows, *got)
    if l > 0:
        assert spec.every_segment_has_two_strings(got[0])
        assert ctx.eds_stats(got[0], got[1], l)["is_leds"] == 1, (what, l)


# ---- every window at every word phase ----

@functools.lru_cache(maxsize=1)
def phase_rows(S, k):
    return alignment(check_mask(10), S, k, alphabet(k), seed=100 * S + k)


@pytest.mark.parametrize("l", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("S,k", [(S, k) for S in (2, 5, 9, 17, 65) for k in (2, 5, 9, 17, 65) if k <= S])
def test_every_window_at_every_word_phase(ctx, S, k, l):
    """65 609 columns, one-line rows and rows wrapped at 60.  S rows copy k <= S haplotypes; k strings in every variant
    segment: 2 the lean emitter, 5 / 9 / 17 the three wide ones, 65 the generic kernels."""
    check(ctx, phase_rows(S, k), l, (None, 60), "B(2,10) S=%d k=%d" % (S, k))


def test_longer_windows_for_longer_contexts(ctx):
    """l = 5 and 6 need windows of up to 8 columns around a run; B(2, 12) has every window of 12."""
    rows = alignment(check_mask(12), 2, 2, DNA, seed=12)
    for l in (5, 6):
        check(ctx, rows, l, (None, 60), "B(2,12) S=2")


# ---- the ends of the alignment ----

@pytest.mark.parametrize("l", [1, 2, 3, 4])
@pytest.mark.parametrize("S", [2, 65])
def test_every_mask_of_1_to_8_columns_as_a_whole_alignment(ctx, S, l):
    """Where 'starts at column 0' and 'ends at the last column' decide: 510 alignments per case."""
    for n in range(1, 9):
        for m in range(1 << n):
            mask = np.array([m >> c & 1 for c in range(n)])
            rows = alignment(mask, S, S, alphabet(S), seed=m, gaps=(m % 2 == 0))
            text = fasta(rows)
            want = spec.transform(text, l)
            got = ctx.msa_transform(text, l)
            assert got == want, (S, l, n, m, rows[:3])
            spec.closure_rows(rows, *got)
            assert spec.every_segment_has_two_strings(got[0])
            assert ctx.eds_stats(got[0], got[1], l)["is_leds"] == 1, (S, l, n, m)


# ---- merged segments at the kernels' limits ----

@pytest.mark.parametrize("k", [3, 70])
@pytest.mark.parametrize("l", [2, 8])
def test_merged_segments_at_the_kernels_limits(ctx, l, k):
    cs = chains(l)
    assert sorted({len(c) for c in cs} & {511, 512, 513}) == [511, 512, 513]
    assert {sum(c) for c in cs} >= {15, 16, 17, 63, 64, 65}
    mask = [0] * 5
    for i, c in enumerate(cs):
        mask += c + [0] * (l + i % 3)                    # a common run that stands alone: l, l + 1, l + 2 columns
    rows = alignment(mask, 100, k, DNA, seed=7 * l + k)
    text = fasta(rows)
    want = spec.transform(text, l)
    # the specification made one segment of k strings of every chain
    segs = [s for s in spec.segments(spec.common_columns(rows), l) if not s[2]]
    assert [b - a for a, b, _ in segs] == [len(c) for c in cs]
    commas = [g.count(b",") for g in re.findall(rb"\{([^{}]*)\}", want[0])]
    assert commas[0::2] == [0] * (len(cs) + 1) and commas[1::2] == [k - 1] * len(cs)
    check(ctx, rows, l, (None, 60), "chains l=%d k=%d" % (l, k))


@pytest.mark.parametrize("k", [3, 70])
@pytest.mark.parametrize("l", [2, 8])
@pytest.mark.parametrize("width", [511, 512, 513])
def test_the_whole_alignment_is_one_segment(ctx, width, l, k):
    rows = alignment(chain(width, 300, l), 100, k, DNA, seed=width + l + k)
    want = spec.transform(fasta(rows), l)
    assert want[0].count(b"{") == 1 and want[0].count(b",") == k - 1
    check(ctx, rows, l, (None, 60), "one segment of %d columns l=%d k=%d" % (width, l, k))


# ---- many rows ----

def test_many_rows(ctx):
    """1025 rows (more than the wave-per-segment kernels take) x 16 455 columns, every window of 8 at every phase."""
    rows = alignment(check_mask(8), 1025, 9, A65, seed=1025)
    for l in (0, 3):
        check(ctx, rows, l, (None,), "B(2,8) S=1025")
