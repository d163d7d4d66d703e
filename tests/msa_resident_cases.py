"""Constructed alignments for the device-resident MSA calls on caller-owned buffers (tests/test_msa_resident_gpu.py),
with the premise every case is named after (tests/test_msa_resident_cpu.py checks the premises with the oracle alone).

OUTPUT SIDE (constructed_cases): small alignments whose FIRST and LAST segment are of a chosen kind - the last
segment's tail is where an emitter can store behind the output, the first segment's head is where one could store in
front of it.  A case of kind X is  X | 3 common | 1 variant column | 3 common | X  (variant X) or
X | 1 variant column | X  (common X), so both ends are of kind X.  Kinds:

  c<n>        common run of n columns: 15/16/17 straddle the single-store / multi-store switch of k_emit_common_seg,
              512/513 the switch to k_emit_common_long (LONG_COMMON)
  huge        one common run of more than HUGE_COMMON (2^20) columns, two rows, at the end / at the start
  a<n>        n columns, no variant column at all (k_seg_meta's nvs == 0 branch)
  v<k>        variant segment of k = 1..4 strings                (main emitter)
  w<k>        ... of 5..8 strings (wide8 list), 9..16 strings (wide16 list), 17..64 strings (wide16 list, 8-bit ids)
  gstrings    ... of more than 64 strings                        (generic k_emit_variant)
  gcols       ... of 70 columns                                  (generic k_emit_variant)
  nul         ... with a NUL byte                                (generic k_emit_variant)

Rows: 2, 70, 999, 1000 (from 1000 on ids of five bytes exist: HAS5), and 1025 (k_rl_emit) and 8193 (tables in HBM).  A
segment has at most as many strings as the alignment has rows, so kinds that need more strings than rows do not exist
for that row count (v3, v4 and everything wider at 2 rows); IMPOSSIBLE counts them, nothing else is left out.
Layouts: one line per row, and wrapped rows (mv.lw != 0: the byte-wise common path, raw positions through k_vmap).  The
line width is 60 where the alignment is wider than that, else 7, else 2 (wrap_width): every wrapped case really has
more than one line per row, so no wrapped case repeats the text of a one-line case.  One column (a1) cannot wrap.
Context lengths 3 and 10 for a subset (MIXED_KINDS, with 2 common columns between the pieces, so that a variant first
and last segment absorb their neighbours and become mixed; a common run at either end stands alone at any length
(msa_transforms.cpp:153), so the common kinds get  X | site | 2 common | site | X  and it is the middle that merges).

INPUT SIDE (input_cases): seeded random alignments over L x S x line width x how the text ends (final newline, none,
blank lines, a partial last wrapped line with no newline), a seeded sample of the product."""
import itertools
import random

import numpy as np

LONG_COMMON = 512
HUGE_COMMON = 1 << 20
COMMON_RUNS = [1, 2, 14, 15, 16, 17, 31, 32, 33, 511, 512, 513, 1100]
NVS0_LENGTHS = [1, 16, 600]
ROWS = [2, 70, 999, 1000]
ROUTE_ROWS = [1025, 8193]
LAYOUTS = [False, True]                # one line per row / wrapped rows (line width: wrap_width)
VARIANT_KINDS = ["v1", "v2", "v3", "v4", "w5", "w8", "w9", "w16", "w17", "w64", "gstrings", "gcols", "nul"]
KINDS = ["c%d" % n for n in COMMON_RUNS] + ["a%d" % n for n in NVS0_LENGTHS] + VARIANT_KINDS
MIXED_KINDS = ["c1", "c2", "v2", "w5", "w16", "gcols", "nul"]
MIXED_ROWS = [2, 999, 1000, 1025]
MIXED_L = [3, 10]
GENERIC_KINDS = ("gstrings", "gcols", "nul")

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def min_rows(kind):
    """Fewest rows at which a segment of this kind exists."""
    if kind == "gstrings":
        return 65
    if kind[0] in "vw":
        return max(2, int(kind[1:]))
    return 2


def wrap_width(width):
    """Line width of the wrapped layout for an alignment of `width` columns (None: one column cannot wrap)."""
    return 60 if width > 60 else 7 if width > 7 else 2 if width > 2 else None


def _common(rng, S, w):
    return np.tile(_ACGT[rng.integers(0, 4, size=w)], (S, 1))


def _site(rng, S):
    """One variant column of two strings (odd rows differ from row 0)."""
    ref = int(rng.integers(0, 4))
    col = np.full((S, 1), _ACGT[ref], dtype=np.uint8)
    col[1::2, 0] = _ACGT[(ref + 1) % 4]
    return col


def _variant(kind, S):
    """-> (S x w bytes, number of strings or None where only the oracle knows)."""
    r = np.arange(S)
    if kind == "v1":                                   # "-A" / "A-": two columns, every row spells "A"
        a = np.empty((S, 2), dtype=np.uint8)
        a[:, 0] = ord("A"); a[:, 1] = ord("-")
        a[0] = (ord("-"), ord("A"))
        return a, 1
    if kind[0] in "vw":                                # k strings: the digits of (row % k) in base 4 as letters
        k = int(kind[1:])
        w = 1 if k <= 4 else 2 if k <= 16 else 3
        i = r % k
        return np.stack([_ACGT[(i >> (2 * j)) & 3] for j in range(w)], axis=1), k
    if kind == "gstrings":                             # up to 100 strings of two letters
        v = r % 100
        return np.stack([65 + v // 10, 97 + v % 10], axis=1).astype(np.uint8), min(S, 100)
    if kind == "gcols":                                # 70 columns, two strings
        a = np.full((S, 70), ord("G"), dtype=np.uint8)
        a[1::2] = ord("T")
        return a, 2
    if kind == "nul":                                  # a NUL ends the row's string
        a = np.full((S, 1), ord("A"), dtype=np.uint8)
        a[1::2, 0] = ord("C")
        a[1, 0] = 0
        return a, None
    raise ValueError(kind)


def fasta(rows, lw=None, ending="\n", header=lambda i: b">s%d" % i):
    """S x L bytes -> FASTA text; rows wrapped at lw columns when 0 < lw < L."""
    S, L = rows.shape
    if lw and lw < L:
        nl = (L + lw - 1) // lw
        pad = np.zeros((S, nl * lw), dtype=np.uint8)
        pad[:, :L] = rows
        pad = np.concatenate([pad.reshape(S, nl, lw), np.full((S, nl, 1), 10, dtype=np.uint8)], axis=2).reshape(S, nl * (lw + 1))
        rows = pad[:, :L + nl - 1]
    text = b"\n".join(header(i) + b"\n" + rows[i].tobytes() for i in range(S))
    return text + ending.encode()


class Case:
    """kind, S, lw, l; build() -> (text, rows); expectations of the first and the last segment at l = 0:
    variant (bool), cols, strings (None: ask the oracle); slow: segments for the generic kernels at l = 0."""

    def __init__(self, kind, S, wrapped, l=0, where="both"):
        self.kind, self.S, self.l, self.where = kind, S, l, where
        lw = self.lw = wrap_width(self.width()) if wrapped else None
        assert not wrapped or lw
        self.id = "%s%s-S%d-%s-l%d" % (kind, "" if where == "both" else "_" + where, S, "lw%d" % lw if lw else "oneline", l)
        self.slow = 2 if kind in GENERIC_KINDS else 0

    def pieces(self):
        """-> list of (S x w bytes, variant, strings)"""
        kind, S = self.kind, self.S
        rng = np.random.default_rng(sum(map(ord, kind)) * 7919 + S)
        gap = 2 if self.l else 3
        site = (_site(rng, S), True, 2)
        if kind == "huge":
            run = (_common(rng, S, HUGE_COMMON + 5), False, 1)
            small = [site, (_common(rng, S, gap), False, 1), site]
            return small + [run] if self.where == "last" else [run] + small
        if kind[0] == "a":
            return [(_common(rng, S, int(kind[1:])), False, 1)]
        if kind[0] == "c":
            n = int(kind[1:])
            if self.l:             # a common run at either end stands alone whatever its length: the middle is what merges
                return [(_common(rng, S, n), False, 1), site, (_common(rng, S, gap), False, 1), site, (_common(rng, S, n), False, 1)]
            return [(_common(rng, S, n), False, 1), site, (_common(rng, S, n), False, 1)]
        a, k = _variant(kind, S)
        return [(a, True, k), (_common(rng, S, gap), False, 1), site, (_common(rng, S, gap), False, 1), (a.copy(), True, k)]

    def build(self):
        p = self.pieces()
        rows = np.concatenate([x[0] for x in p], axis=1)
        self.first, self.last = p[0][1:] + (p[0][0].shape[1],), p[-1][1:] + (p[-1][0].shape[1],)     # (variant, strings, cols)
        return fasta(rows, self.lw), rows

    def routes(self):
        """Emitter routes this case is there for (first/last segment; l = 0 cases only)."""
        S, kind, out = self.S, self.kind, set()
        if S > 8192:
            out.add("big")
        if kind == "huge" or kind[0] in "ca":
            n = HUGE_COMMON + 5 if kind == "huge" else int(kind[1:])
            if kind[0] == "a":
                out.add("nvs0" if S <= 1024 else "nvs0_rowloop")
            if self.lw:
                out.add("common_bytewise_long" if n > LONG_COMMON else "common_bytewise")
            elif n > HUGE_COMMON:
                out.add("common_huge")
            elif n > LONG_COMMON:
                out.add("common_long")
            else:
                out.add("common_single_store" if n < 16 else "common_multi_store")
        elif kind in GENERIC_KINDS:
            out.add(("generic" if S <= 1024 else "generic_rowloop") + ("_wrapped" if self.lw else ""))
        elif S > 1024:
            out.add("rowloop")
        else:
            k = int(kind[1:])
            out.add(("main" if k <= 4 else "wide8" if k <= 8 else "wide16" if k <= 16 else "wide64") + ("_wrapped" if self.lw else ""))
            if S >= 1000:
                out.add("has5_wrapped" if self.lw else "has5")
        return out

    def width(self):
        """Columns of the whole alignment."""
        kind, gap = self.kind, 2 if self.l else 3
        if kind == "huge":
            return HUGE_COMMON + 5 + gap + 2
        if kind[0] == "a":
            return int(kind[1:])
        if kind[0] == "c":
            return 2 * int(kind[1:]) + (2 + gap if self.l else 1)
        return 2 * _variant(kind, 2)[0].shape[1] + 2 * gap + 1


ALL_ROUTES = {"big", "nvs0", "nvs0_rowloop", "common_bytewise", "common_bytewise_long", "common_huge", "common_long",
              "common_single_store", "common_multi_store", "generic", "generic_rowloop", "rowloop", "main", "wide8",
              "wide16", "wide64", "has5", "generic_wrapped", "main_wrapped", "wide8_wrapped", "wide16_wrapped",
              "wide64_wrapped", "has5_wrapped"}


def constructed_cases():
    """-> (cases, impossible): every kind x row count x layout at l = 0, the two huge runs, the mixed subset; impossible
    lists the (kind, S, wrapped) triples that cannot exist (more strings than rows; one column does not wrap)."""
    cases, impossible = [], []
    for S in ROWS + ROUTE_ROWS:
        for kind in KINDS:
            for wrapped in LAYOUTS if S in ROWS else [False]:
                if S < min_rows(kind) or (wrapped and kind == "a1"):
                    impossible.append((kind, S, wrapped))
                    continue
                cases.append(Case(kind, S, wrapped))
    for where in ("last", "first"):
        for lw in LAYOUTS:
            cases.append(Case("huge", 2, lw, where=where))
    for S in MIXED_ROWS:
        for kind in MIXED_KINDS:
            for l in MIXED_L:
                for wrapped in LAYOUTS:
                    if S < min_rows(kind):
                        impossible.append((kind, S, wrapped))
                        continue
                    cases.append(Case(kind, S, wrapped, l=l))
    return cases, impossible


# the counts the CPU and the GPU tests both assert (6 row counts x 29 kinds, less what cannot exist at 2 rows and the
# wrapped a1 of the four row counts that have both layouts)
N_IMPOSSIBLE_L0 = len([k for k in KINDS if min_rows(k) > 2])
N_L0 = (len(KINDS) * len(ROWS) - N_IMPOSSIBLE_L0) * len(LAYOUTS) - len(ROWS) + len(KINDS) * len(ROUTE_ROWS)
N_HUGE = 4
N_IMPOSSIBLE_MIXED = len([k for k in MIXED_KINDS if min_rows(k) > 2])
N_MIXED = (len(MIXED_KINDS) * len(MIXED_ROWS) - N_IMPOSSIBLE_MIXED) * len(MIXED_L) * len(LAYOUTS)
N_CONSTRUCTED = N_L0 + N_HUGE + N_MIXED


def one_per_route():
    """A small subset for the tests that vary something else (pointer offsets, streams): for every route the first case
    that has it, the huge runs excepted (2 MB each: the containment test has them)."""
    cases, _ = constructed_cases()
    seen, out = set(), []
    for c in cases:
        if c.l or c.kind == "huge":
            continue
        new = c.routes() - seen
        if new:
            seen |= new
            out.append(c)
    assert seen == ALL_ROUTES - {"common_huge"}, ALL_ROUTES - seen
    return out


# ---- input side ------------------------------------------------------------------------------------------------
IN_L = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4099]
IN_S = [2, 3, 17, 64, 65, 257, 1025]
IN_LW = [None, 7, 60]
ENDINGS = {"newline": "\n", "none": "", "blank": "\n\n\n", "partial": ""}
N_INPUT = 240


class InputCase:
    def __init__(self, i, L, S, lw, ending):
        self.L, self.S, self.lw, self.ending = L, S, lw, ending
        self.l = 0 if i % 2 == 0 else 5
        self.seed = 5000 + i
        self.id = "L%d-S%d-%s-%s-l%d" % (L, S, "lw%d" % lw if lw else "oneline", ending, self.l)

    def build(self):
        rng = np.random.default_rng(self.seed)
        S, L = self.S, self.L
        ref = _ACGT[rng.integers(0, 4, size=L)].copy()
        ref[rng.random(L) < 0.02] = ord("-")
        rows = np.tile(ref, (S, 1))
        sites = np.flatnonzero(rng.random(L) < 0.08)
        alph = np.frombuffer(b"ACGT-acgtN", dtype=np.uint8)
        for c in sites:
            pick = rng.random(S) < 0.5
            rows[pick, c] = alph[rng.integers(0, len(alph), size=int(pick.sum()))]
        return fasta(rows, self.lw, ENDINGS[self.ending], header=lambda i: b">s%d%s" % (i, b" x" * (i % 3)))


def input_cases():
    """A seeded sample of N_INPUT from L x S x line width x ending ("partial": wrapped rows whose last line is shorter
    than the others, text ending without a newline - only where L is no multiple of the line width)."""
    prod = [(L, S, lw, e) for L, S, lw, e in itertools.product(IN_L, IN_S, IN_LW, ENDINGS)
            if e != "partial" or (lw and lw < L and L % lw)]
    picked = random.Random(2026).sample(prod, N_INPUT)
    return [InputCase(i, *p) for i, p in enumerate(picked)]


# a ragged last row (and the other format errors of test_msa_gpu.py::test_format_errors)
FORMAT_ERRORS = [b"", b"ACGT\n", b">a\nACGT\n", b">a\nACGT\n>b\nAC\n", b">a\nACGT\n>b\nACGTA\n", b">a\nAC\nGT\n>b\nACG\nT\n"]
