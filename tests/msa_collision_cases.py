"""Directed alignments for the hash-then-compare sites of the MSA grouping (csrc/msa_fast_kernels.hpp: the one-row-per-lane
branch of fast_group and the root join of refine_groups; csrc/msa_generic_kernels.hpp: the hashed keys of group_segment).

With full-width hashes the byte compares behind them are never asked to say "no".  libedsx_weakhash.so keeps ONE bit of
every such hash, so of any three distinct strings two share it, whatever the hash function is: a segment with three
distinct strings (of one length where the site also compares the length) guarantees its collision by pigeonhole, and this
module never restates a hash.

A case is built column by column: runs of variant columns between SEP common columns (one-line rows), optionally glued
by fewer than L_POS common columns so that they become one mixed segment at l = L_POS.  Everything a test expects comes
from the columns: the segments at l = 0 and at l = L_POS, their distinct raw rows and gap-stripped strings in the order
of first appearance, the .eds / .seds text, and the route the geometry implies (`slow`, `heavy`).  tests/
test_msa_weakhash_cpu.py asserts the premises and that the oracle writes the same text; tests/test_msa_weakhash_gpu.py
runs the cases on the device."""

SEP = 4              # common columns between the runs: >= L_POS, so l = L_POS leaves the unglued runs as they are
L_POS = 3
PROT = "DEFHIKLMPQRSVWY"      # letters outside the exact DNA keys {A,C,G,T,N,-}
DNA = "ACGT"

FAMILIES = ("lane", "rootjoin", "rootjoin_mixed", "generic_table", "generic_iterative", "generic_mixed")


def spell(s, w, i):
    """the letters of s in w columns: the gaps as one block in front of letter i (i = len(s): behind the last one);
    i = "spread": the gaps spread between the letters"""
    g = w - len(s)
    assert g >= 0, (s, w)
    if i == "spread":
        out, used = [], 0
        for j, ch in enumerate(s):
            want = g * (j + 1) // (len(s) + 1)
            out.append("-" * (want - used) + ch)
            used = want
        return "".join(out) + "-" * (g - used)
    i = min(i, len(s))
    return s[:i] + "-" * g + s[i:]


def strip(row):
    """a row's string: up to the first NUL, without gaps (msa_transforms.cpp:282-283)"""
    return row.split("\0")[0].replace("-", "")


def word(alph, n, seed):
    """n letters, no two neighbours equal (so that every placement of the gap block is another raw row)"""
    out, x = [], seed
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7fffffff
        ch = alph[(x >> 16) % len(alph)]
        if out and out[-1] == ch:
            ch = alph[(alph.index(ch) + 1) % len(alph)]
        out.append(ch)
    return "".join(out)


def swap(s, p, alph, step):
    """s with the letter at p replaced by another one of alph (step = 1, 2: two different replacements)"""
    return s[:p] + alph[(alph.index(s[p]) + step) % len(alph)] + s[p + 1:]


def fill(first, pool, S):
    """S rows: `first`, then the rows of `pool` in a fixed scattered order (byte-identical rows far apart)"""
    rows = list(first[:S])
    r = len(rows)
    while len(rows) < S:
        rows.append(pool[(7 * r + 3) % len(pool)])
        r += 1
    return rows


class Segment:
    """w columns of S rows (str, latin-1; '-' gap, '\\0' ends the row's string); mixed: common columns inside"""

    def __init__(self, rows, mixed=False, note=""):
        self.rows, self.w, self.mixed, self.note = rows, len(rows[0]), mixed, note
        assert all(len(r) == self.w for r in rows)

    def raw_rows(self):
        return list(dict.fromkeys(self.rows))

    def strings(self):
        return list(dict.fromkeys(strip(r) for r in self.rows))

    def per_length(self):
        out = {}
        for s in self.strings():
            out[len(s)] = out.get(len(s), 0) + 1
        return out

    def has_nul(self):
        return any("\0" in r for r in self.rows)

    def alphabet(self):
        return set("".join(self.rows)) - {"-"}

    def dna_only(self):
        return self.alphabet() <= set("ACGTN")

    def column_is_variant(self, c):
        col = [r[c] for r in self.rows]
        return any(x != col[0] or x == "-" for x in col[1:])

    # ---- the route the geometry implies (fast = wave per segment up to 1024 rows; row-loop kernels above)
    def slow(self, S):
        """does the segment go to the generic kernels?"""
        if S <= 1024:
            return self.w > 64 or self.has_nul() or len(self.raw_rows()) > 64
        return self.mixed or self.w > 16 or self.has_nul() or len(self.strings()) > 64

    def heavy(self, S):
        """is it on the heavy work list of the wave-per-segment grouping (no fused grouping: l > 0)?"""
        return S <= 1024 and self.w <= 64 and (self.mixed or self.w >= 11)

    def site(self, S):
        """the hash-then-compare site that groups it: 1 one row per lane, 2 root join, 3 generic keys, 0 none of them"""
        if self.slow(S):
            return 3 if self.w > 8 else 0
        if S > 1024 or self.w < 2 or (not self.mixed and self.w <= 20 and self.dna_only()):
            return 0
        return 1 if S <= 64 and not self.mixed else 2


class Case:
    """runs: the variant runs; glue: {i: letters} - fewer than L_POS common columns between run i and run i + 1"""

    def __init__(self, family, name, S, runs, glue=None):
        self.family, self.id, self.S, self.runs, self.glue = family, "%s/%s/S%d" % (family, name, S), S, runs, glue or {}
        assert all(len(r.rows) == S for r in runs) and all(0 < len(g) < L_POS for g in self.glue.values())

    def pieces(self, l):
        """[("common", letters) | ("variant", Segment)] in column order, as the transform with context length l sees them"""
        out = [("common", word(DNA, SEP, 1))]
        i = 0
        while i < len(self.runs):
            seg = self.runs[i]
            while l and i in self.glue:
                g = self.glue[i]
                seg = Segment([a + g + b for a, b in zip(seg.rows, self.runs[i + 1].rows)], mixed=True, note=seg.note)
                i += 1
            out.append(("variant", seg))
            if i in self.glue:
                out.append(("common", self.glue[i]))
            else:
                out.append(("common", word(DNA, SEP, 2 + i)))
            i += 1
        return out

    def segments(self, l):
        return [p for kind, p in self.pieces(l) if kind == "variant"]

    def build(self):
        cols = [p if kind == "common" else None for kind, p in self.pieces(0)]
        segs = self.segments(0)
        out = []
        for r in range(self.S):
            it = iter(segs)
            out.append(">r%d\n%s\n" % (r, "".join(c if c is not None else next(it).rows[r] for c in cols)))
        return "".join(out).encode("latin-1")

    def cells(self):
        return self.S * sum(len(p) if kind == "common" else p.w for kind, p in self.pieces(0))

    def expected(self, l):
        """(.eds, .seds) from the columns alone (msa_transforms.cpp:245-317)"""
        eds, seds = [], []
        for kind, p in self.pieces(l):
            if kind == "common":
                eds.append("{%s}" % p)
                seds.append("{0}")
                continue
            ids = {}
            for r, row in enumerate(p.rows):
                ids.setdefault(strip(row), []).append(str(r + 1))
            eds.append("{%s}" % ",".join(ids))
            seds.append("".join("{%s}" % ",".join(v) for v in ids.values()))
        return "".join(eds).encode("latin-1"), "".join(seds).encode("latin-1")

    def n_slow(self, l):
        return sum(1 for s in self.segments(l) if s.slow(self.S))

    def n_heavy(self, l):
        return sum(1 for s in self.segments(l) if s.heavy(self.S))


# ---- one row per lane (S <= 64) -------------------------------------------------------------------------------------------

LANE_ROWS = (3, 5, 17, 63, 64)
LANE_LENGTHS = (1, 3, 4, 5, 8, 12, 13, 63, 64)
KINDS = ("first", "last", "partial")


def diff_position(n, kind):
    """where the strings of one kind differ: the first byte, the last byte, a byte of the last partial dword (the
    middle one of its bytes; a string of 4 k letters has no partial dword: the middle of its last dword)"""
    if kind == "first":
        return 0
    if kind == "last":
        return n - 1
    lo = 4 * ((n - 1) // 4)
    return (lo + n - 1) // 2


def lane_run(S, n, si, w=None):
    """one run whose strings of length n differ in one byte only"""
    wide = n > 10
    alph = DNA if wide else PROT
    if S == 3:                                     # no room for an all-gap first row: the columns are variant because
        w = 2 if n == 1 else 11 if n <= 5 else 21 if n <= 8 else 63          # row 1 is right-aligned in w >= 2 n columns
        assert 2 * n <= w
    elif w is None:
        w = 2 if n == 1 else 11 if n <= 5 else 21 if n <= 13 else n
    base = word(alph, n, 100 + n)
    trios = []
    for kind in KINDS:
        p = diff_position(n, kind)
        trios.append([base, swap(base, p, alph, 1), swap(base, p, alph, 2)])
    if S == 3:
        a, b, c = trios[si % 3]
        return Segment([spell(a, w, n), spell(b, w, 0), spell(c, w, "spread")], note="len %d %s" % (n, KINDS[si % 3]))
    if S == 5:
        a, b, c = trios[si % 3]
        return Segment(["-" * w, spell(a, w, n), spell(b, w, 0), spell(c, w, "spread"), spell(a, w, n // 2)],
                       note="len %d %s" % (n, KINDS[si % 3]))
    strings = list(dict.fromkeys(s for t in trios for s in t))
    first = ["-" * w] + [spell(s, w, (j * 5) % (n + 1)) for j, s in enumerate(strings)]
    again = [spell(s, w, (j * 5 + n // 2 + 1) % (n + 1)) for j, s in enumerate(strings)]
    return Segment(fill(first + again, first + again, S), note="len %d all kinds" % n)


def lane_cases():
    out = []
    for S in LANE_ROWS:
        lens = [n for n in LANE_LENGTHS if S > 3 or n <= 13]
        runs = [lane_run(S, n, si) for si, n in enumerate(lens)]
        if S == 3:                                 # the all-gap row and one string spelt twice, where three rows allow it
            s = word(PROT, 5, 7)
            runs.append(Segment(["-" * 11, spell(s, 11, 0), spell(s, 11, 3)], note="all-gap row, one string twice"))
        else:
            runs.append(lane_run(S, 63, len(lens), w=64))      # 63 letters in 64 columns: one gap, in another place per row
        out.append(Case("lane", "lengths", S, runs))
    return out


# ---- root join of refine_groups (65 .. 1024 rows, runs of 11 .. 64 columns) --------------------------------------------

ROOT_ROWS = (65, 100, 256, 257, 1000, 1024)


def abc_run(S, w, alph, placements):
    """first rows: the all-gap row, A, B, C (three strings of one length), then A, B, C again per further placement of
    the gap block; two more strings of another length"""
    n = w - 3
    base = word(alph, n, 300 + w)
    abc = [base, swap(base, n - 1, alph, 1), swap(base, 0, alph, 1)]
    de = [word(alph, n - 2, 400 + w), word(alph, n - 2, 500 + w)]
    first = ["-" * w]
    for i in placements:
        first += [spell(s, w, i) for s in abc]
    first += [spell(s, w, 0) for s in de] + [spell(s, w, 2) for s in de]
    return Segment(fill(first, first, S), note="A B C x %d placements" % len(placements))


def rootjoin_cases():
    out = []
    for S in ROOT_ROWS:
        out.append(Case("rootjoin", "abc16", S, [abc_run(S, 11, PROT, (0, 8, 4)), abc_run(S, 33, DNA, (0, 30, 15)),
                                                 abc_run(S, 64, DNA, (0, 61, 7))]))
        out.append(Case("rootjoin", "abc64", S, [abc_run(S, 11, PROT, range(0, 9)), abc_run(S, 40, DNA, range(0, 36, 2)),
                                                 abc_run(S, 64, DNA, range(1, 61, 4))]))
        # about 60 roots of one length: the last ones walk a long list of candidates
        base = word(PROT, 12, 77)
        many = [base[:3] + p + base[4:8] + q + base[9:] for p in PROT for q in "DEFH"]
        assert len(set(many)) == 60
        first = ["-" * 24] + [spell(s, 24, 0) for s in many] + [spell(s, 24, 6) for s in many[-3:]]
        out.append(Case("rootjoin", "roots60", S, [Segment(fill(first, first, S), note="60 roots of length 12")]))
        # 65 raw groups and more: the wave gives up, the generic kernels group the segment
        some = [word(DNA, 24, 900 + j) for j in range(13)]
        first = [spell(s, 30, i) for i in (0, 5, 11, 17, 24) for s in some] + ["-" * 30]
        out.append(Case("rootjoin", "raw65", S, [Segment(fill(first, first, S), note="65+ raw groups, 13 strings")]))
    return out


MIXED_ROWS = (17, 65, 1000)


def glued_runs(S, w1, w2, alph, seed):
    """two runs whose rows spell A, B, C (one length over both runs), then the same with other gaps, in either run"""
    n1, n2 = w1 - 4, w2 - 5
    a1, a2 = word(alph, n1, seed), word(alph, n2, seed + 1)
    parts = [(a1, a2), (swap(a1, 0, alph, 1), a2), (a1, swap(a2, n2 - 1, alph, 1)), (a1[:-2], a2), (a1, a2[2:])]
    first = [("-" * w1, "-" * w2)]
    for i1, i2 in ((0, 0), (n1, 0), (0, n2 // 2), (3, 3)):
        first += [(spell(x, w1, i1), spell(y, w2, i2)) for x, y in parts[:3]]
    first += [(spell(x, w1, 1), spell(y, w2, 1)) for x, y in parts[3:]]
    rows = fill(first, first, S)
    return Segment([r[0] for r in rows], note="part 1"), Segment([r[1] for r in rows], note="part 2")


def rootjoin_mixed_cases():
    out = []
    for S in MIXED_ROWS:
        r1, r2 = glued_runs(S, 21, 30, DNA, 31)
        r3, r4 = glued_runs(S, 11, 40, PROT, 41)
        out.append(Case("rootjoin_mixed", "glued", S, [r1, r2, r3, r4], glue={0: "KL", 2: "W"}))
    return out


# ---- generic kernels ----------------------------------------------------------------------------------------------------

TABLE_ROWS = (3, 64, 65, 128, 129, 1024, 1025, 2049, 4096)
ITER_ROWS = (4097, 8192, 8193)


def generic_run(S, w, nul=False, many=False, two=False, seed=0):
    alph = PROT if w < 21 else DNA
    if S == 3:
        n = min((w - 1) // 2, 20)
        base = word(alph, n, 600 + w + seed)
        a, b, c = base, swap(base, n - 1, alph, 1), (swap(base, 0, alph, 1) if seed % 2 == 0 else base[:-1])
        if two:
            return Segment([spell(a, w, n), spell(b, w, 0), spell(a, w, 1)], note="two strings")
        if nul:
            a = a + "\0" + word(alph, 2, 9)                  # the NUL ends row 0's string; the letters behind it are not part of it
        return Segment([spell(a, w, len(a)), spell(b, w, 0), spell(c, w, "spread")], note="nul" if nul else "plain")
    n = w - 3
    base = word(alph, n, 600 + w + seed)
    if two:                                                  # exactly two strings; row 0 spells one of them left-aligned in
        m = (w - 1) // 2                                     # less than half of the columns, the other one stands to the right
        p, q = word(alph, m, 640 + w), word(alph, m - 4, 650 + w)
        first = [spell(p, w, m), spell(q, w, 0), spell(p, w, m // 2), spell(q, w, 2)]
        return Segment(fill(first, first, S), note="two strings")
    abc = [base, swap(base, n - 1, alph, 1), swap(base, 0, alph, 1)]
    de = [base[:-2], swap(base[:-2], 1, alph, 1)]
    first = ["-" * w] + [spell(s, w, 0) for s in abc + de] + [spell(s, w, len(s) // 2) for s in abc + de]
    if nul:                                                  # two different rows that a NUL cuts down to one string, which a third
        k = n // 2                                           # row spells with gaps
        x = base[:k]
        first += [x + "\0" + word(alph, w - k - 1, 11), spell(x + "\0" + word(alph, 1, 12), w, 1), spell(x, w, 2),
                  spell(abc[1] + "\0", w, n + 1)]            # and a NUL behind a whole string: the same string as without it
    if many:                                                 # more than 64 distinct strings (and raw rows)
        extra = [base[:2] + p + base[3:6] + q + base[7:] for p in PROT for q in "DEFHI"][:70]
        assert len(set(extra)) == 70
        first = first[:1] + [spell(s, w, (j % 3) * 2) for j, s in enumerate(extra)] + first[1:]
    return Segment(fill(first, first, S), note="nul" if nul else "many" if many else "plain")


def generic_runs(S, with_two):
    runs = [generic_run(S, 9, nul=True), generic_run(S, 20, many=S >= 65, nul=S < 65), generic_run(S, 64, nul=True, seed=1),
            generic_run(S, 65), generic_run(S, 200, seed=1)]
    if with_two:
        runs.append(generic_run(S, 65, two=True))
    return runs


def generic_table_cases():
    return [Case("generic_table", "segments", S, generic_runs(S, True)) for S in TABLE_ROWS]


def generic_iterative_cases():
    return [Case("generic_iterative", "segments", S, generic_runs(S, False)) for S in ITER_ROWS]


def generic_mixed_cases():
    out = []
    for S in (100, 1025):
        r1, r2 = glued_runs(S, 40, 40, DNA, 51)
        out.append(Case("generic_mixed", "glued", S, [r1, r2], glue={0: "KL"}))
    return out


_BUILDERS = {"lane": lane_cases, "rootjoin": rootjoin_cases, "rootjoin_mixed": rootjoin_mixed_cases,
             "generic_table": generic_table_cases, "generic_iterative": generic_iterative_cases,
             "generic_mixed": generic_mixed_cases}
_CACHE = {}


def cases(family):
    if family not in _CACHE:
        _CACHE[family] = _BUILDERS[family]()
    return _CACHE[family]
