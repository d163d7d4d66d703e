"""The tile path of the column scan (csrc/msa_scan_kernels.hpp: k_scan_extract) against the CPU oracle, byte for byte:
the hand-off of the variant-column slots (one atomic per tile whose result is looked at late), the overflow retry, the
batched extraction, every instantiation that shares the code, and the accumulation / wave reduction of the column masks.

Every case runs for l = 0 and l = 3.  Alignments under 1 MB go through the host call, which keeps such a FASTA image as
it is (rows at odd offsets); the few larger ones go through the device-resident calls, which keep any image as it is.
"""
import os
import re

import numpy as np
import pytest

import oracle_lib as o

pytestmark = pytest.mark.gpu

LS = (0, 3)
_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "edsparser_amd", "csrc")


def _source_constant(file, pattern):
    m = re.search(pattern, open(os.path.join(_CSRC, file)).read())
    assert m, (file, pattern)
    return int(m.group(1))


# read from the source, so that a changed limit moves the cases with it (or fails here)
LDS_ROWS = _source_constant("msa_device.hpp", r"LDS_ROWS\s*=\s*(\d+)\s*;")        # more rows take the BIG instantiation
HOLD_ROWS = _source_constant("msa_device.hip", r"S > 2048 && S <= (\d+)\)")         # more rows are walked in a loop
COLBUF_KB = _source_constant("msa_device.hip", r"\? (\d+) \* 1024 : 64 \* 1024;")    # LDS image of the tile's variant columns


def fused_cols(S):
    """variant columns of S rows that the LDS image holds (pitch: vc_pitch); denser tiles take the batched path"""
    return COLBUF_KB * 1024 // ((S + 15) // 16 * 16 + 16)


ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    c = edsparser_amd.Context(0)
    yield c
    c.close()


def _fasta(rows):
    return b"".join(b">s%d\n" % i + rows[i].tobytes() + b"\n" for i in range(rows.shape[0]))


def _reference_rows(rng, S, L):
    return np.tile(ACGT[rng.integers(0, 4, size=L)], (S, 1))


def _other_letter(rng, letters):
    """a letter of ACGT that differs from each of `letters`"""
    idx = np.searchsorted(ACGT, letters)
    return ACGT[(idx + rng.integers(1, 4, size=letters.shape)) % 4]


def _scatter_variants(rng, rows, cols, p_row=0.3):
    """Rows 1.. deviate in the columns `cols` with probability p_row each; row 1 always does, so that every one of
    them is a variant column."""
    S = rows.shape[0]
    for c in cols:
        pick = rng.random(S) < p_row
        pick[0] = False
        pick[1] = True
        rows[pick, c] = _other_letter(rng, rows[pick, c])


def _transform(ctx, msa, l):
    if len(msa) < (1 << 20):
        return ctx.msa_transform(msa, l)
    import torch
    buf = torch.frombuffer(bytearray(msa), dtype=torch.uint8).to("cuda:0")
    E, Q = ctx.msa_plan_device(buf.data_ptr(), len(msa), l)
    d_eds = torch.empty(E, dtype=torch.uint8, device="cuda:0")
    d_seds = torch.empty(Q, dtype=torch.uint8, device="cuda:0")
    ctx.msa_emit_device(d_eds.data_ptr(), d_seds.data_ptr())
    torch.cuda.synchronize()
    return bytes(d_eds.cpu().numpy()), bytes(d_seds.cpu().numpy())


def _check(ctx, msa, what):
    for l in LS:
        assert _transform(ctx, msa, l) == o.msa(msa, l), (what, l)


def _variant_columns_sparse(rows, L):
    """the same for a large alignment, in slices (no S x L temporary)"""
    return np.concatenate([c0 + _variant_columns(rows[:, c0:c0 + 8192]) for c0 in range(0, L, 8192)])


def _variant_columns(rows):
    return np.flatnonzero((rows != rows[0]).any(axis=0) | (rows[0] == ord("-")))


# ---- slot hand-off ---------------------------------------------------------------------------------------------

def _racing_40(rng):
    rows = _reference_rows(rng, 40, 300_000)
    _scatter_variants(rng, rows, np.flatnonzero(rng.random(300_000) < 0.03))
    return rows


def _racing_bench_instantiation(rng):
    # 40 rows take 2048-column tiles, 147 of them.  More than 2000 tiles need the 128-column tiles of 513 .. 1024
    # rows - the instantiation the benchmark runs: 513 rows x (2001 tiles + 5 columns), 131 MB.  Two variant columns
    # per tile on average with a deviating row or two each: every tile but a few still asks for slots, and the .seds
    # text stays small (7 MB).  The case takes 2.5 s, 1.6 s of it the oracle's two passes over the 131 MB
    L = 2001 * 128 + 5
    rows = _reference_rows(rng, 513, L)
    _scatter_variants(rng, rows, np.flatnonzero(rng.random(L) < 0.015), p_row=0.002)
    v = _variant_columns_sparse(rows, L)
    assert np.unique(v // 128).size > 1500
    return rows


def _quiet_ends(rng):
    L = 6 * 128
    rows = _reference_rows(rng, 1000, L)
    cols = 128 + np.flatnonzero(rng.random(4 * 128) < 0.05)
    _scatter_variants(rng, rows, cols)
    v = _variant_columns(rows)
    assert v.size and v.min() >= 128 and v.max() < L - 128
    return rows


def _no_variant(rng):
    rows = _reference_rows(rng, 1000, 700)
    assert _variant_columns(rows).size == 0
    return rows


@pytest.mark.parametrize("make", [_racing_40, _racing_bench_instantiation, _quiet_ends, _no_variant],
                         ids=lambda f: f.__name__.strip("_"))
def test_slot_hand_off(ctx, make):
    """The tiles take their variant-column slots off one counter and look at the answer only after the extraction and
    the run registration: thousands of tiles that race for it, first and last tiles that never ask, and an alignment
    in which no tile asks."""
    rows = make(np.random.default_rng(101))
    _check(ctx, _fasta(rows), make.__name__)


# ---- overflow retry --------------------------------------------------------------------------------------------

def test_overflow_retry():
    """Every column variant and more of them than the first guess of the column store (4096): the tiles' slots run
    past the capacity, the plan reports it, and the second plan - on a counter that was reset - gives the text."""
    import edsparser_amd
    rng = np.random.default_rng(102)
    S, L = 20, 6000
    rows = ACGT[rng.integers(0, 4, size=(S, L))]
    rows[1] = _other_letter(rng, rows[0])
    assert _variant_columns(rows).size == L > 4096
    msa = _fasta(rows)
    for l in LS:
        fresh = edsparser_amd.Context(0)                       # a context whose column store has not grown yet
        try:
            assert fresh.msa_transform(msa, l) == o.msa(msa, l), l
        finally:
            fresh.close()


# ---- batched path ----------------------------------------------------------------------------------------------

def test_batched_path(ctx):
    """1000 rows x 512 columns, half of them variant: every tile has more variant columns than its LDS image holds
    and extracts them in batches."""
    rng = np.random.default_rng(103)
    rows = _reference_rows(rng, 1000, 512)
    _scatter_variants(rng, rows, np.flatnonzero(rng.random(512) < 0.5))
    per_tile = np.bincount(_variant_columns(rows) // 128, minlength=4)
    assert per_tile.min() > fused_cols(1000)
    _check(ctx, _fasta(rows), "batched")


# ---- every instantiation that shares the changed code ----------------------------------------------------------------

@pytest.mark.parametrize("S", [3, 64, 65, 1000, 1024, 1025, 2049, HOLD_ROWS + 1, LDS_ROWS + 1])
def test_every_instantiation(ctx, S):
    """One row per lane (S <= 64), sixteen rows per lane in wide tiles (65) and in the eight-chunk tiles of the
    benchmark (1000, 1024), 64-column tiles (1025), the 1024-thread workgroup (2049), the row loop (more than 4096 rows) and the row loop with
    its tables in HBM (more than LDS_ROWS rows), each on alignments of one column, less than a chunk, one tile minus / exactly /
    plus a column, and several tiles with a partial last one."""
    rng = np.random.default_rng(104 + S)
    for L in (1, 15, 127, 128, 129, 300):
        rows = _reference_rows(rng, S, L)
        cols = np.flatnonzero(rng.random(L) < 0.15)
        if L == 1:
            cols = np.array([0])
        _scatter_variants(rng, rows, cols)
        gaps = rng.random(rows.shape) < 0.002                  # a few gaps, in the first row too
        rows[gaps] = ord("-")
        _check(ctx, _fasta(rows), (S, L))


# ---- accumulate and reduce -----------------------------------------------------------------------------------------

def _single_row_sites(rng, S, pairs):
    """1000 or 1024 rows x 512 columns, 38 variant columns per 128-column tile (the fused path takes them); each owes
    its variation to one row.  pairs: None - a random reference letter and another letter in that row; else
    (reference byte, deviating byte) pairs taken in turn."""
    L, G = 512, (S + 15) // 16
    rows = _reference_rows(rng, S, L)
    cols = np.concatenate([128 * t + np.sort(rng.choice(128, size=38, replace=False)) for t in range(4)])
    owners = []
    for k, c in enumerate(cols):
        g, pos = k % G, (k + 1 + k // G) % 16
        if 16 * g + pos >= S:
            pos %= S - 16 * g
        r = 16 * g + pos
        assert 0 < r < S
        owners.append(r)
        if pairs is None:
            rows[r, c] = _other_letter(rng, rows[r:r + 1, c])[0]
        else:
            rows[:, c], rows[r, c] = pairs[k % len(pairs)][0], pairs[k % len(pairs)][1]
    # the owners visit all sixteen register positions of a thread and every group of sixteen rows (64 of them for 1024 rows)
    assert {r % 16 for r in owners} == set(range(16)) and {r // 16 for r in owners} == set(range(G))
    v = _variant_columns(rows)
    assert np.array_equal(v, np.sort(cols)) and np.bincount(v // 128, minlength=4).max() <= min(39, fused_cols(S))
    assert all(int((rows[:, c] != rows[0, c]).sum()) == 1 for c in cols)
    return rows


BIT_PAIRS = [(ord("A"), ord("C")), (ord("C"), ord("A")), (ord("-"), ord("m")), (ord("m"), ord("-")), (0x20, 0x60), (0x60, 0x20)]


@pytest.mark.parametrize("S", [1000, 1024])
@pytest.mark.parametrize("kind", ["one_row", "bit_subsets"])
def test_accumulate_and_reduce(ctx, S, kind):
    """acc |= row ^ ref as one three-input boolean per dword, and the OR of the chunk masks over the lanes of a wave.
    one_row: a single deviating row per variant column, at every register position and in every row group - a mask bit
    lost by the accumulation or by a lane exchange drops the column.  bit_subsets: the deviating byte is a bit-subset
    or a bit-superset of the reference byte (A/C, '-'/m, 0x20/0x60, both ways round), so that a truth table that
    computes acc | (row & ref), acc | (row & ~ref) or acc | (~row & ref) loses columns."""
    for a, b in BIT_PAIRS:
        assert a != b and ((a & b) == a or (a & b) == b)
    rng = np.random.default_rng(105 + S)
    rows = _single_row_sites(rng, S, None if kind == "one_row" else BIT_PAIRS)
    _check(ctx, _fasta(rows), (kind, S))
