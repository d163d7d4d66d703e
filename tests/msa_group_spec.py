"""Reference of the MSA transform's grouping of ONE variant segment, and the directed segments of
tests/test_msa_group_cpu.py / tests/test_msa_group_gpu.py.  TEST INFRASTRUCTURE: plain Python and
numpy, no kernel logic restated, never imported by edsparser_amd/.

A segment is an S x ncol matrix of bytes.  A row's string is its bytes without '-' and '\\n'; the groups are the distinct
strings in the order of their first rows.  The routing (`route`) is the return code that the comments of fast_group
(csrc/msa_fast_kernels.hpp) promise for the segment, as a table over what the segment IS (columns, alphabet, numbers of
strings and of distinct raw rows) - not over how the kernel finds that out."""
import numpy as np

D = b"ACGTN-"                     # the alphabet of the exact-key paths
KCAP = 64                         # distinct strings (or raw classes) a wave groups
REC_TEXT_MAX = 64                 # bytes of .eds text in a fused record
CNT_SCATTER, CNT_MIXED = 1 << 63, 1 << 62
TILE_W = 64                       # columns per tile in the worlds of the GPU test
SIZES = (2, 15, 16, 17, 63, 64, 65, 66, 127, 128, 129, 1008, 1023, 1024)
# bytes outside D that an alignment's text can carry as they are (no NUL, no line ends, no '>')
NOND = bytes(b for b in range(1, 256) if b not in D and b not in b"\n\r>")
_D_SET = np.zeros(256, dtype=bool)
_D_SET[list(D)] = True


def vc_pitch(S):
    return (S + 15) // 16 * 16 + 16


def strip(row):
    return bytes(row).replace(b"-", b"").replace(b"\n", b"")


class Groups:
    """gid[row], rep[g] (first row of group g), strings[g], k, sumlen of a segment"""

    def __init__(self, M):
        seen, self.rep, self.strings = {}, [], []
        self.gid = np.zeros(M.shape[0], dtype=np.int64)
        for r in range(M.shape[0]):
            s = strip(M[r].tobytes())
            g = seen.get(s)
            if g is None:
                g = seen[s] = len(self.rep)
                self.rep.append(r)
                self.strings.append(s)
            self.gid[r] = g
        self.k = len(self.rep)
        self.sumlen = sum(len(s) for s in self.strings)

    def text(self):
        return b"{" + b",".join(self.strings) + b"}"

    def id_sets(self):
        """the segment's part of the .seds text: per string the ascending 1-based ids of its rows"""
        return b"".join(b"{" + b",".join(b"%d" % (r + 1) for r in np.flatnonzero(self.gid == g)) + b"}" for g in range(self.k))


def pack_ids(gid, bits):
    """64 lanes x (1 or 2) u32: `bits` bits per row, lane l = rows 16 l .. 16 l + 15, rows that do not exist 0
    (pack_gid2 / pack_gid4 of csrc/msa_wave.hpp: bits = 4 puts rows 0..7 of the lane in the first dword)"""
    ids = np.zeros(1024, dtype=np.uint64)
    ids[:len(gid)] = gid
    assert ids.max() < (1 << bits)
    per = 32 // bits                                           # rows per dword
    w = ids.reshape(-1, per) << (np.arange(per, dtype=np.uint64) * np.uint64(bits))
    return w.sum(axis=1).astype(np.uint32).reshape(64, 16 // per)


class Seg:
    """One segment.  place: None - consecutive slots; ("two", nA) - CNT_SCATTER, one-line rows, a tile edge behind its first
    nA columns; ("lw",) - CNT_SCATTER in a world of wrapped rows; ("mixed", common) - CNT_MIXED, common[c] says which columns
    are common ones (every row holds the reference byte there).  premise: what the case claims about itself, asserted by
    tests/test_msa_group_cpu.py from the bytes."""

    def __init__(self, name, M, place=None, **premise):
        self.name, self.M, self.place, self.premise = name, np.ascontiguousarray(M, dtype=np.uint8), place, premise
        self.S, self.ncol = self.M.shape
        assert 1 <= self.ncol <= 64
        self.mixed = place is not None and place[0] == "mixed"
        self.variant = ~np.asarray(place[1], dtype=bool) if self.mixed else np.ones(self.ncol, dtype=bool)
        if self.mixed:
            assert self.ncol >= 2 and self.variant.any() and not self.variant.all()
            C = self.M[:, ~self.variant]
            assert (C == C[0]).all() and (C != 0x2D).all()
        self._g = None

    @property
    def groups(self):
        if self._g is None:
            self._g = Groups(self.M)
        return self._g

    def all_dna(self):
        return bool(_D_SET[self.M].all())

    def has(self, byte):
        return bool((self.M[:, self.variant] == byte).any())

    def raw_classes(self):
        """distinct rows as bytes over the variant columns"""
        return len({r.tobytes() for r in self.M[:, self.variant]})

    def route(self, heavy):
        """the return code of fast_group<_, heavy>: 1 grouped, 0 generic kernels, 2 the heavy pass"""
        S, ncol = self.S, self.ncol
        if ncol == 1:
            if self.all_dna():
                return 1
            if self.has(0):
                return 0
            return 1 if self.groups.k <= KCAP else 0          # ('-' and '\n' are one string: the empty one)
        general = 0 if self.has(0) else 1 if (S <= 64 and not self.mixed) or self.raw_classes() <= KCAP else 0
        if self.mixed:
            return general if heavy else 2
        if self.all_dna() and (ncol <= 10 or (heavy and ncol <= 20)):
            return 1 if self.groups.k <= KCAP else 0
        return general if heavy else 2

    def saw_nl(self):
        return 1 if self.has(0x0A) else 0

    def fused_ok(self):
        """does the column scan write a record for this run (else its columns go to vc)?"""
        g = self.groups
        return self.all_dna() and g.k <= 16 and 1 + g.k + g.sumlen <= REC_TEXT_MAX


# ================================================================================================================
# the directed segments
# ================================================================================================================
def _mat(rows):
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), len(rows[0]))


def _rng(S, tag):
    return np.random.default_rng([S, sum(tag.encode()) * 131 + len(tag)])


def _spread(pool, S, rng, shuffle=False):
    """S rows from the pool: every pool row once (while there are rows), in pool order or shuffled, then random repeats"""
    pool = list(pool)
    if shuffle:
        pool = [pool[i] for i in rng.permutation(len(pool))]
    rows = pool[:S] + [pool[i] for i in rng.integers(0, len(pool), max(0, S - len(pool)))]
    return _mat(rows)


def _distinct_rows(n, ncol, alphabet, rng):
    """n distinct rows of ncol bytes over the alphabet"""
    out, seen = [], set()
    assert n <= len(set(alphabet)) ** ncol
    while len(out) < n:
        r = bytes(rng.choice(list(alphabet), ncol).astype(np.uint8))
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


def _gapped(s, ncol, rng):
    """the string s spelt over ncol columns with gaps at random places"""
    at = np.sort(rng.choice(ncol, len(s), replace=False))
    row = bytearray(b"-" * ncol)
    for p, c in zip(at, s):
        row[p] = c
    return bytes(row)


def one_column(S):
    out = []
    rng = _rng(S, "one")
    for mask in range(1, 64):                                  # every subset of D as the column's alphabet
        sub = bytes(D[i] for i in range(6) if (mask >> i) & 1)
        if len(sub) <= S:
            out.append(Seg("one/subset%02d" % mask, _spread([bytes([c]) for c in sub], S, rng, shuffle=True), strings=len(sub), dna=True))
    for r in sorted({63, 64, 79, 80, S - 1}):                  # a class whose first row is r, all earlier rows one letter
        if 1 <= r < S:
            col = bytearray(b"A" * r + b"T" + bytes(b"AT"[i & 1] for i in range(S - r - 1)))
            out.append(Seg("one/late%d" % r, _mat([bytes([c]) for c in col]), first_row={ord("T"): r}, strings=2, dna=True))
            if r + 2 < S:                                      # two more late classes: the next row and the last one
                col[r + 1] = ord("-")
                col[S - 1] = ord("G")
                out.append(Seg("one/late%d+2" % r, _mat([bytes([c]) for c in col]), first_row={ord("T"): r, ord("-"): r + 1, ord("G"): S - 1},
                               strings=4, dna=True))
    for name, pool in (("lower", b"acA-"), ("iupac", b"RYAN"), ("high", b"\x80\xff\xc1A-"), ("newline", b"A\n-C")):
        if S >= 2:
            out.append(Seg("one/" + name, _spread([bytes([c]) for c in pool], S, rng), dna=False, strings=min(S, len(pool)) - (name == "newline" and S >= 3)))
    out.append(Seg("one/nul_first", _mat([b"\0"] + [b"AC"[i & 1:][:1] for i in range(S - 1)]), nul=True))
    out.append(Seg("one/nul_last", _mat([b"AC"[i & 1:][:1] for i in range(S - 1)] + [b"\0"]), nul=True))
    for i, pool in enumerate((NOND[100:164], NOND[100:165], NOND[7:70] + b"-", NOND[7:70] + b"-\n", NOND[7:71] + b"-")):
        if S >= len(pool):
            strings = len(pool) - (b"\n" in pool)             # ('-' and '\n' are one string)
            out.append(Seg("one/bytes%d_strings%d_%d" % (len(pool), strings, i), _spread([bytes([c]) for c in pool], S, rng, shuffle=True),
                           dna=False, strings=strings, distinct_bytes=len(pool)))
    return out


DNA_NCOLS = (2, 9, 10, 11, 19, 20)


def dna_keys(S):
    out = []
    for ncol in DNA_NCOLS:
        rng = _rng(S, "dna%d" % ncol)
        base = bytes(rng.choice(list(b"ACGTN"), ncol).astype(np.uint8))
        for j in sorted({0, 9, 10, ncol - 1}):                 # rows that differ in column j only
            if j < ncol:
                pool = [base[:j] + bytes([c]) + base[j + 1:] for c in D]
                out.append(Seg("dna/w%d/differ_at%d" % (ncol, j), _spread(pool, S, rng, shuffle=True), dna=True, strings=min(S, 6),
                               differ_only_at=j))
        # stripped lengths on both sides of the ten-letter seam of the string keys; every string twice with other gaps
        pool = []
        lengths = sorted({n for n in (0, 1, 9, 10, 11, 20, ncol) if n <= ncol})
        for n in lengths:
            if n <= ncol:
                for s in sorted({bytes(rng.choice(list(b"ACGTN"), n).astype(np.uint8)) for _ in range(2)} | {b"ACGTNACGTNACGTNACGTN"[:n]}):
                    pool += [_gapped(s, ncol, rng), _gapped(s, ncol, rng)]
                if 0 < n < ncol:                               # equal up to the last letter
                    pool += [_gapped(b"ACGTNACGTNACGTNACGTN"[:n - 1] + b"A", ncol, rng)]
        out.append(Seg("dna/w%d/lengths" % ncol, _spread(pool, S, rng, shuffle=True), dna=True,
                       lengths=lengths if S >= len(pool) else None))
        if ncol == 2:                                          # equal after stripping, not as raw rows
            out.append(Seg("dna/w2/gap_shift", _spread([b"A-", b"-A", b"--", b"AA", b"C-", b"-C"], S, rng), dna=True,
                           raw=min(S, 6), joins=True))
        if ncol >= 9:
            for n in (64, 65):                                 # 64 and 65 strings
                if S >= n:
                    out.append(Seg("dna/w%d/strings%d" % (ncol, n), _spread(_distinct_rows(n, ncol, b"ACGTN", rng), S, rng, shuffle=True),
                                   dna=True, strings=n))
            if S >= 65:                                        # 65 raw rows that spell 64 strings
                rows = _distinct_rows(64, ncol - 1, b"ACGTN", rng)
                out.append(Seg("dna/w%d/raw65_strings64" % ncol, _spread([r + b"-" for r in rows] + [b"-" + rows[0]], S, rng, shuffle=True),
                               dna=True, strings=64, raw=65))
        rows = [bytes(r) for r in _spread(_distinct_rows(min(S, 5), ncol, D, rng), S, rng)]
        rows[-1] = rows[-1][:-1] + b"a"                        # one byte outside D: last row, last column
        out.append(Seg("dna/w%d/one_foreign_byte" % ncol, _mat(rows), dna=False, foreign_at=(S - 1, ncol - 1)))
    return out


def lane_rows(S):
    """the one-row-per-lane branch (S <= 64, heavy): more than 20 columns, or another alphabet"""
    out = []
    if S > 64:
        return out
    for ncol, alpha in ((21, b"ACGT"), (64, b"ACGT"), (2, b"ac"), (21, b"acgRY\xc1")):
        rng = _rng(S, "lane%d%d" % (ncol, len(alpha)))
        a = alpha * 16
        pool = [b"-" * ncol]
        for n in (3, 4, 5, 64):
            if n <= ncol:                                      # strings of n letters that are equal up to the last byte
                for last in alpha[:3]:
                    s = a[:n - 1] + bytes([last])
                    pool += [_gapped(s, ncol, rng), _gapped(s, ncol, rng)]
        pool += [_gapped(a[:min(ncol, 7)], ncol, rng)]
        if ncol == 2:
            pool += [b"a-", b"-a", b"c-", b"ca", b"cc"]
        out.append(Seg("lane/w%d/%s" % (ncol, "dna" if alpha == b"ACGT" else "other%d" % len(alpha)), _spread(pool, S, rng, shuffle=True),
                       dna=alpha == b"ACGT", lane_path=True))
    rows = [bytes(r) for r in _spread([b"-" * 21, b"A" * 21, b"AC" + b"-" * 19], S, _rng(S, "lanenul"))]
    rows[S // 2] = rows[S // 2][:20] + b"\0"
    out.append(Seg("lane/w21/nul", _mat(rows), nul=True))
    rows[S // 2] = rows[S // 2][:20] + b"\n"
    out.append(Seg("lane/w21/newline", _mat(rows), dna=False, lane_path=True))
    return out


REFINE_ALPHA = b"acgtnRYKM"                                    # nine letters outside D: 81 rows of two columns


def refine(S):
    """refine_groups (S >= 65, heavy; with up to 64 rows the same segments take the one-row-per-lane branch)"""
    out = []
    for ncol in (2, 21, 63, 64):
        rng = _rng(S, "refine%d" % ncol)
        for R in (8, 9, 16, 17, 32, 33, 64, 65):               # raw classes at the table sizes of lutN and at KCAP
            if S >= R:
                pool = _distinct_rows(R, ncol, REFINE_ALPHA, rng)
                out.append(Seg("refine/w%d/raw%d" % (ncol, R), _spread(pool, S, rng, shuffle=True), dna=False, raw=R, strings=R))
        # raw classes that join to fewer strings: every string spelt with gaps in three different places
        strings = [bytes(rng.choice(list(REFINE_ALPHA), max(1, ncol // 2)).astype(np.uint8)) for _ in range(6)]
        strings += [strings[0][:-1] + b"Z", b""]
        pool = [_gapped(s, ncol, rng) for s in strings for _ in range(3)]
        M = _spread(pool, S, rng, shuffle=True)
        out.append(Seg("refine/w%d/join" % ncol, M, dna=False, joins=S >= 2 * len(pool)))
        rows = [pool[0]] * S                                   # one class but for the last row's last column
        rows[-1] = rows[-1][:-1] + (b"Q" if rows[-1][-1:] != b"Q" else b"W")
        out.append(Seg("refine/w%d/last_row_splits" % ncol, _mat(rows), dna=False, raw=2, strings=2))
        rows = [bytes(r) for r in M]
        rows[S - 1] = rows[S - 1][:ncol // 2] + b"\0" + rows[S - 1][ncol // 2 + 1:]
        out.append(Seg("refine/w%d/nul" % ncol, _mat(rows), nul=True))
        rows[S - 1] = rows[S - 1][:ncol // 2] + b"\n" + rows[S - 1][ncol // 2 + 1:]
        out.append(Seg("refine/w%d/newline" % ncol, _mat(rows), dna=False))
    return out


def descriptors(S):
    """the same kinds of segment behind the other column descriptors: a tile edge inside, wrapped rows, common columns inside"""
    out = []
    rng = _rng(S, "desc")
    bodies = []
    for ncol, alpha in ((10, D), (20, D), (21, D), (64, REFINE_ALPHA + b"-"), (3, REFINE_ALPHA)):
        pool = _distinct_rows(min(S, 12), ncol, alpha, rng)
        bodies.append(("w%d%s" % (ncol, "dna" if alpha == D else "other"), _spread(pool, S, rng, shuffle=True), alpha == D))
    for name, M, dna in bodies:
        ncol = M.shape[1]
        for nA in sorted({1, 2, ncol - 1}):
            if 1 <= nA < ncol:
                out.append(Seg("desc/two/%s/edge%d" % (name, nA), M, ("two", nA), dna=dna))
        out.append(Seg("desc/lw/%s" % name, M, ("lw",), dna=dna))
    # common columns first, last and between the variant runs ('G' / 'T' / 'c' in every row)
    for name, layout in (("first", "CVVVV"), ("last", "VVVVC"), ("between", "VVCVV"), ("runs", "VCCVVVVVVVVVVCVVVVVVVVVVVVVVCV"),
                         ("wide", "V" * 31 + "C" + "V" * 31 + "C")):
        for alpha in (D, REFINE_ALPHA + b"-"):
            ncol = len(layout)
            nv = layout.count("V")
            pool = _distinct_rows(min(S, 9), nv, alpha, rng)
            if nv > 1:
                pool += [b"-" * nv, pool[0][:-1] + (b"-" if pool[0][-1:] != b"-" else b"A")]
            V = _spread(pool, S, rng, shuffle=True)
            M = np.zeros((S, ncol), dtype=np.uint8)
            common = np.array([c == "C" for c in layout])
            M[:, ~common] = V
            M[:, common] = np.frombuffer((b"GTc" * ncol)[:int(common.sum())], dtype=np.uint8)
            out.append(Seg("desc/mixed/%s/%s" % (name, "dna" if alpha == D else "other"), M, ("mixed", common), mixed=True))
    if S >= 65:
        common = np.array([c == "C" for c in "VVCVV"])
        for R in (64, 65):
            M = np.full((S, 5), ord("G"), dtype=np.uint8)
            M[:, ~common] = _spread(_distinct_rows(R, 4, REFINE_ALPHA, rng), S, rng, shuffle=True)
            out.append(Seg("desc/mixed/raw%d" % R, M, ("mixed", common), mixed=True, raw=R))
    M = np.full((S, 5), ord("G"), dtype=np.uint8)
    M[:, ~np.array([False, False, True, False, False])] = _spread([b"A\0GT", b"AC-T", b"ACGT"], S, rng)
    out.append(Seg("desc/mixed/nul", M, ("mixed", np.array([False, False, True, False, False])), nul=True, mixed=True))
    return out


def random_sweep(S):
    """a seeded sweep per route: a few strings over random widths and alphabets"""
    out = []
    rng = _rng(S, "sweep")
    for i in range(24):
        ncol = int(rng.choice([1, 1, 2, 3, 5, 7, 10, 11, 13, 20, 21, 40, 64]))
        alpha = [D, D, b"ACGT-", REFINE_ALPHA + b"-", bytes(range(0x41, 0x61)) + b"-\n"][int(rng.integers(0, 5))]
        npool = int(rng.choice([1, 2, 3, 4, 5, 8, 16, 17, 40, 70]))
        pool = _distinct_rows(min(npool, len(set(alpha)) ** ncol), ncol, alpha, rng)
        place = None
        if ncol >= 2 and i % 4 == 3:
            place = ("two", int(rng.integers(1, ncol)))
        out.append(Seg("sweep/%d/w%d" % (i, ncol), _spread(pool, S, rng, shuffle=True), place))
    return out


_CASES = {}


def cases(S):
    """every segment of S rows, built once"""
    if S not in _CASES:
        segs = one_column(S) + dna_keys(S) + lane_rows(S) + refine(S) + descriptors(S) + random_sweep(S)
        assert len({s.name for s in segs}) == len(segs)
        _CASES[S] = segs
    return _CASES[S]


# ---- runs of the column scan's own grouping (fused_group_run): S x w, w <= 10 (one row per lane: <= 20)
def fused_runs(S, rows64):
    out = []
    rng = _rng(S, "fused%d" % rows64)
    wmax = 20 if rows64 else 10
    for w in range(1, wmax + 1):
        for k in (1, 4, 5, 16, 17):
            if k <= S and k <= min(6 ** w, 5 ** w + 1):
                pool = _distinct_rows(k, w, b"ACGTN", rng) if w > 1 else [bytes([c]) for c in D[:k]]
                if w > 1 and k > 1:
                    pool[int(rng.integers(0, k))] = b"-" * w
                out.append(Seg("fused/w%d/k%d" % (w, k), _spread(pool, S, rng, shuffle=True), strings=k))
    # text of 64 and of 65 bytes: 1 + k + sumlen
    for name, lens in (("text64", (10, 10, 10, 10, 10, 7)), ("text65", (10, 10, 10, 10, 10, 8))) if not rows64 else \
            (("text64", (20, 20, 20)), ("text65", (20, 20, 20, 0)), ("text64b", (20, 11, 10, 9, 7, 0)), ("text65b", (20, 11, 10, 9, 8, 0))):
        if S >= len(lens):
            pool = []
            for i, n in enumerate(lens):
                pool.append(_gapped(bytes(rng.choice(list(b"ACGTN"), n).astype(np.uint8))[:-1] + b"ACGTNA"[i:i + 1] if n else b"", wmax, rng))
            out.append(Seg("fused/" + name, _spread(pool, S, rng, shuffle=True), textlen=1 + len(lens) + sum(lens)))
    # the empty string first, in the middle and last (in the order of first rows)
    for name, pool in (("empty_first", [b"---", b"A-C", b"-G-"]), ("empty_middle", [b"A-C", b"---", b"-G-"]), ("empty_last", [b"A-C", b"-G-", b"---"])):
        if S >= 3:
            out.append(Seg("fused/" + name, _spread(pool, S, rng), strings=3))
    out.append(Seg("fused/empty_only", _mat([b"--"] * S), strings=1))
    for w in (1, 2, wmax):                                     # a byte outside D: the columns go to vc
        rows = [bytes(r) for r in _spread(_distinct_rows(min(S, 3, 5 ** w), w, b"ACGTN", rng), S, rng)]
        rows[S - 1] = rows[S - 1][:-1] + b"a"
        out.append(Seg("fused/w%d/foreign_last" % w, _mat(rows), dna=False))
        rows[0] = b"\n" + rows[0][1:]
        out.append(Seg("fused/w%d/foreign_first" % w, _mat(rows), dna=False))
    if S >= 65 and not rows64:                                 # more strings than a wave keeps
        out.append(Seg("fused/w10/strings65", _spread(_distinct_rows(65, 10, b"ACGTN", rng), S, rng, shuffle=True), strings=65))
    for i in range(12):                                        # seeded sweep
        w = int(rng.integers(1, wmax + 1))
        alpha = [D, b"ACGT-", b"AC-"][i % 3]
        pool = _distinct_rows(min(int(rng.choice([1, 2, 3, 4, 5, 9, 16, 17])), len(alpha) ** w), w, alpha, rng)
        out.append(Seg("fused/sweep%d/w%d" % (i, w), _spread(pool, S, rng, shuffle=True)))
    assert len({s.name for s in out}) == len(out)
    return out


# ================================================================================================================
# one alignment of many segments, for the comparison with the specifications the project already trusts
# ================================================================================================================
WRAP_L = 67                       # context length of the wrapped alignment: longer than any common run inside a segment


def wrappable(seg):
    """an alignment's text cannot carry NUL (it ends a row's string in the reference) or a line end inside a row"""
    return not (seg.M == 0).any() and not (seg.M == 0x0A).any() and not (seg.M == 0x0D).any()


def wrap(segs):
    """-> (FASTA text, expected eds, expected seds): flank, then per segment an all-gap column, the segment, an all-gap
    column and a flank.  An all-gap column is a variant column that adds nothing to any string, and a flank of WRAP_L
    common columns stands alone at context length WRAP_L, so every segment is one symbol whatever its own columns are."""
    S = segs[0].S
    flank = np.full((S, WRAP_L), ord("C"), dtype=np.uint8)
    gap = np.full((S, 1), ord("-"), dtype=np.uint8)
    parts, eds, seds = [flank], [b"{" + b"C" * WRAP_L + b"}"], [b"{0}"]
    for s in segs:
        parts += [gap, s.M, gap, flank]
        eds += [s.groups.text(), b"{" + b"C" * WRAP_L + b"}"]
        seds += [s.groups.id_sets(), b"{0}"]
    A = np.concatenate(parts, axis=1)
    text = b"".join(b">r%d\n" % i + A[i].tobytes() + b"\n" for i in range(S))
    return text, b"".join(eds), b"".join(seds)


# ================================================================================================================
# the world a launch of mg_group sees: vc, V, Vraw, word_slot, the reference row (numpy only)
# ================================================================================================================
BAND = 3                          # poison columns in front of the slots of every word
POISON_COL = 0xEE                 # what columns that belong to no segment hold (not in D, not NUL, not a gap)


class World:
    """vc and the column maps of a list of segments of one S.  lw == 0: one-line rows; lw > 0: rows wrapped at lw columns
    (raw column of c = c + c // lw).  fill: what the padding rows S .. Spad-1 of every column hold."""

    def __init__(self, S, segs, fill, lw=0):
        self.S, self.Spad, self.lw, self.segs = S, vc_pitch(S), lw, segs
        raw = (lambda c: c + c // lw) if lw else (lambda c: c)
        placed = [s for s in segs if s.place is not None]
        # columns of the placed segments: three tiles each
        self.seg_a = {}
        tile = 1
        for s in placed:
            if s.place[0] == "two":
                assert lw == 0
                self.seg_a[s.name] = TILE_W * (tile + 1) - s.place[1]
            else:
                self.seg_a[s.name] = TILE_W * tile + 40
            tile += 3
        self.L = TILE_W * (tile + 1)
        nraw = raw(self.L) + 64
        Vb = np.zeros(self.L, dtype=bool)
        file = np.full(nraw + 8, POISON_COL, dtype=np.uint8)
        self.row0 = 5                                          # where the reference row starts in `file`
        for s in placed:
            a = self.seg_a[s.name]
            Vb[a:a + s.ncol] = s.variant
            for c in np.flatnonzero(~s.variant):
                file[self.row0 + raw(a + c)] = s.M[0, c]
        Vrawb = np.zeros((nraw + 63) // 64 * 64, dtype=bool)
        Vrawb[[raw(c) for c in np.flatnonzero(Vb)]] = True
        # slots: per word of raw columns a band of poison columns, then the word's variant columns
        counts = Vrawb.reshape(-1, 64).sum(axis=1)
        self.word_slot = np.zeros(len(counts), dtype=np.uint64)
        nslot = 1
        for w, n in enumerate(counts):
            nslot += BAND if n else 0
            self.word_slot[w] = nslot
            nslot += int(n)
        below = np.cumsum(Vrawb.reshape(-1, 64), axis=1) - Vrawb.reshape(-1, 64)

        def slot(c):
            q = raw(c)
            return int(self.word_slot[q >> 6]) + int(below[q >> 6, q & 63])

        cols = {}                                              # slot -> column bytes
        self.cmeta, self.seg_a_list = [], []
        for s in segs:
            if s.place is None:
                nslot += 1                                     # a poison column between two segments
                s0 = nslot
                for c in range(s.ncol):
                    cols[s0 + c] = s.M[:, c]
                nslot += s.ncol
                self.cmeta.append((s.ncol << 48) | s0)
                self.seg_a_list.append(0)
            else:
                a = self.seg_a[s.name]
                for c in np.flatnonzero(s.variant):
                    cols[slot(a + c)] = s.M[:, c]
                self.cmeta.append((s.ncol << 48) | slot(a) | (CNT_MIXED if s.mixed else CNT_SCATTER))
                self.seg_a_list.append(a)
        self.nslot = nslot + 2
        self.vc = np.full((self.nslot, self.Spad), POISON_COL, dtype=np.uint8)
        for sl, col in cols.items():
            self.vc[sl, :S] = col
            self.vc[sl, S:] = fill
        pack = lambda bits: np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1)
        self.Vraw = pack(Vrawb)
        Vpad = np.zeros((self.L + 63) // 64 * 64 + 64, dtype=bool)
        Vpad[:self.L] = Vb
        self.V = pack(Vpad)
        self.file = file
        self.cmeta = np.array(self.cmeta, dtype=np.uint64)
        self.seg_a_list = np.array(self.seg_a_list, dtype=np.uint64)


def split_launches(segs):
    """-> [(lw, segments)]: the segments placed in wrapped rows need a view of their own"""
    main = [s for s in segs if not (s.place and s.place[0] == "lw")]
    lw = [s for s in segs if s.place and s.place[0] == "lw"]
    return [(0, main)] + ([(60, lw)] if lw else [])
