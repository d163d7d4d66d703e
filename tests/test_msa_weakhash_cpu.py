"""Premises of the directed collision cases (tests/msa_collision_cases.py), asserted from the columns themselves and from the
oracle's text - never from the code under test.  The GPU tests (tests/test_msa_weakhash_gpu.py) rely on them: with one bit
of hash, three distinct strings (of one length, where the site compares lengths first) hold a colliding pair by pigeonhole,
so every segment named here makes its site's byte compare say "no" at least once."""
import pytest

import msa_collision_cases as mc
import oracle_lib as o

LS = (0, mc.L_POS)
_ORACLE = {}


def _oracle(c, l):
    """computed once per case and context length, shared by the tests"""
    if (c.id, l) not in _ORACLE:
        _ORACLE[(c.id, l)] = o.msa(c.build(), l)
    return _ORACLE[(c.id, l)]


def _all_cases():
    return [c for f in mc.FAMILIES for c in mc.cases(f)]


def _one_length_trio(seg):
    """a length with at least three distinct strings: two of them share one bit of (hash, length)"""
    return max(seg.per_length().values()) >= 3


def _differ_only_at(strings, n, p):
    """three strings of length n that differ in byte p only?"""
    groups = {}
    for s in strings:
        if len(s) == n:
            groups.setdefault(s[:p] + s[p + 1:], set()).add(s[p])
    return any(len(v) >= 3 for v in groups.values())


@pytest.mark.parametrize("family", mc.FAMILIES)
def test_oracle_accepts_and_writes_the_text_of_the_columns(family):
    """The expected text is spelt from the columns (Case.expected); the oracle, given the file, writes the same - so the
    strings per segment, their order of first appearance and the path lists are facts of the case, at l = 0 and l = 3."""
    assert mc.cases(family)
    for c in mc.cases(family):
        assert c.cells() <= 3_200_000, (c.id, c.cells())
        for l in LS:
            assert _oracle(c, l) == c.expected(l), (c.id, l)


def test_every_run_is_one_variant_segment():
    """every column of a run is variant (row 0 has a gap there or another row differs), the separators are at least L_POS
    wide and the glue is narrower: the segments are the runs at l = 0 and the glued runs at l = L_POS"""
    assert mc.SEP >= mc.L_POS
    for c in _all_cases():
        for seg in c.runs:
            assert len(seg.rows) == c.S and all(seg.column_is_variant(i) for i in range(seg.w)), (c.id, seg.note)
        assert len(c.segments(0)) == len(c.runs) and len(c.segments(mc.L_POS)) == len(c.runs) - len(c.glue)
        for seg in c.segments(mc.L_POS):
            assert seg.mixed == (seg.w not in [r.w for r in c.runs]) or not c.glue
        # the route is decided by the geometry alone: where the DNA keys could take a segment of up to 20 columns, strings
        # and raw rows are on the same side of 64; above 1024 rows likewise
        for l in LS:
            for seg in c.segments(l):
                if c.S > 1024 or (seg.w <= 20 and seg.dna_only() and not seg.mixed):
                    assert (len(seg.strings()) > 64) == (len(seg.raw_rows()) > 64), (c.id, seg.note)


def test_lane_family():
    """one row per lane: S <= 64, pure segments, no NUL, not for the exact DNA keys; three strings of every tested length
    that differ in the first byte only, in the last byte only, in a byte of the last partial dword only"""
    assert [c.S for c in mc.cases("lane")] == list(mc.LANE_ROWS) == [3, 5, 17, 63, 64]
    for c in mc.cases("lane"):
        kinds_seen = set()
        for l in LS:
            assert c.n_slow(l) == 0
            for seg in c.segments(l):
                assert seg.site(c.S) == 1 and not seg.has_nul() and not seg.mixed, (c.id, seg.note)
                assert seg.w in (2, 11) and not seg.dna_only() or seg.w in (21, 63, 64), (c.id, seg.w)
        assert {s.w for s in c.runs} >= ({2, 11, 21, 63} if c.S == 3 else {2, 11, 21, 63, 64})
        lengths = [n for n in mc.LANE_LENGTHS if c.S > 3 or n <= 13]
        for n in lengths:
            segs = [s for s in c.runs if s.per_length().get(n, 0) >= 3]
            assert segs, (c.id, n)
            for kind in mc.KINDS:
                if any(_differ_only_at(s.strings(), n, mc.diff_position(n, kind)) for s in segs):
                    kinds_seen.add((n, kind))
        if c.S >= 17:                                     # every kind at every length
            assert kinds_seen == {(n, k) for n in lengths for k in mc.KINDS}, c.id
        else:                                             # three or five rows: a kind per segment, all kinds over the case
            assert {k for _, k in kinds_seen} == set(mc.KINDS) and {n for n, _ in kinds_seen} == set(lengths), c.id
        assert any("" in s.strings() for s in c.runs), c.id                      # an all-gap row
        assert any(len(s.raw_rows()) > len(s.strings()) for s in c.runs), c.id   # one string, gaps in different places
    for n, kind, p in ((13, "partial", 12), (12, "partial", 9), (5, "partial", 4), (3, "partial", 1), (63, "partial", 61), (64, "last", 63)):
        assert mc.diff_position(n, kind) == p and p // 4 == (n - 1) // 4


def _abc_pattern(seg):
    """A, B, C: three distinct strings of one length whose first rows come before any second spelling of them, and each
    of them is spelt again later with other gaps.  Whatever pair of them shares the hash bit, the later one of the pair
    meets the earlier one's root - a failing candidate - before its own."""
    strings = seg.strings()
    for i in range(len(strings) - 2):
        abc = strings[i:i + 3]
        if len({len(s) for s in abc}) != 1 or not abc[0]:
            continue
        raws = {s: [r for r in seg.raw_rows() if mc.strip(r) == s] for s in abc}
        if any(len(v) < 2 for v in raws.values()):
            continue
        first = max(seg.rows.index(v[0]) for v in raws.values())
        if all(seg.rows.index(v[1]) > first for v in raws.values()):
            return True
    return False


def test_rootjoin_family():
    assert sorted({c.S for c in mc.cases("rootjoin")}) == list(mc.ROOT_ROWS) == [65, 100, 256, 257, 1000, 1024]
    names = set()
    for c in mc.cases("rootjoin"):
        name = c.id.split("/")[1]
        names.add(name)
        for l in LS:
            for seg in c.segments(l):
                raw = len(seg.raw_rows())
                assert 11 <= seg.w <= 64 and not seg.has_nul() and not seg.mixed
                if name == "raw65":
                    assert raw >= 65 and seg.site(c.S) == 3 and c.n_slow(l) == 1 and len(seg.strings()) >= 3
                    assert seg.w > 20                      # (not for the DNA keys: the raw groups decide)
                    continue
                assert seg.site(c.S) == 2 and c.n_slow(l) == 0, (c.id, seg.note)
                assert _abc_pattern(seg) and _one_length_trio(seg), (c.id, seg.note)
                if name == "abc16":
                    assert raw <= 16
                elif name == "abc64":
                    assert 17 <= raw <= 64
                else:
                    assert name == "roots60" and max(seg.per_length().values()) >= 60 and 17 <= raw <= 64
    assert names == {"abc16", "abc64", "roots60", "raw65"}


def test_rootjoin_mixed_family():
    assert [c.S for c in mc.cases("rootjoin_mixed")] == list(mc.MIXED_ROWS)
    for c in mc.cases("rootjoin_mixed"):
        segs = c.segments(mc.L_POS)
        assert len(segs) == 2 and c.n_slow(mc.L_POS) == 0 and c.n_heavy(mc.L_POS) == 2
        for seg, glue in zip(segs, c.glue.values()):
            assert seg.mixed and seg.w <= 64 and seg.site(c.S) == 2 and len(glue) < mc.L_POS
            assert all(glue in s and not s.startswith(glue) and not s.endswith(glue) for s in seg.strings() if s != glue)
            assert glue in seg.strings()                   # (the all-gap row spells the common letters alone)
            assert _abc_pattern(seg) and _one_length_trio(seg)
        for seg in c.segments(0):                          # apart, the runs are pure segments of the fast kernels
            assert not seg.mixed and seg.site(c.S) in (1, 2)


def _generic_segment_premises(c, seg, two):
    S = c.S
    assert seg.site(S) == 3 and seg.slow(S), (c.id, seg.note)
    strings = seg.strings()
    if two:
        assert len(strings) == 2 and len(seg.raw_rows()) > 2
        return
    assert len(strings) >= 3, (c.id, seg.note)             # two of them share the key's one bit
    if S > 3:
        lens = seg.per_length()
        assert max(lens.values()) >= 3 and len(lens) >= 2   # equal and different lengths
        assert len(seg.rows) > len(seg.raw_rows()) > len(strings) or len(strings) > 64   # identical rows; one string, other gaps
    if seg.has_nul() and S > 3:
        cut = [r for r in seg.raw_rows() if "\0" in r]
        assert any(a != b and mc.strip(a) == mc.strip(b) and a.split("\0")[1].replace("-", "") and b.split("\0")[1].replace("-", "")
                   for a in cut for b in cut), (c.id, seg.note)      # a NUL cuts two different rows down to one string
        assert any("\0" not in r and mc.strip(r) == mc.strip(cut[0]) for r in seg.raw_rows())


@pytest.mark.parametrize("family,rows,nseg", [("generic_table", (3, 64, 65, 128, 129, 1024, 1025, 2049, 4096), 6),
                                              ("generic_iterative", (4097, 8192, 8193), 5)])
def test_generic_families(family, rows, nseg):
    from_table = family == "generic_table"
    assert [c.S for c in mc.cases(family)] == list(rows)
    for c in mc.cases(family):
        assert [s.w for s in c.runs][:5] == [9, 20, 64, 65, 200]
        for l in LS:
            segs = c.segments(l)
            assert len(segs) == nseg and c.n_slow(l) == nseg
            for i, seg in enumerate(segs):
                _generic_segment_premises(c, seg, two=from_table and i == 5)
            # the three ways to the generic kernels: a NUL byte, more than 64 strings, more than 64 columns
            assert segs[0].has_nul() and segs[0].w <= 64 and segs[2].has_nul() and segs[2].w == 64
            assert (len(segs[1].strings()) > 64) if c.S >= 65 else segs[1].has_nul()
            assert not segs[3].has_nul() and not segs[4].has_nul() and segs[3].w > 64
    # the switches the rows are chosen for (csrc/msa_generic_kernels.hpp: ht_size_of, the R = 1, 2, 4 forms of make_keys,
    # HT_MAX_ROWS; csrc/msa_device.hpp: LDS_ROWS) - restated here as numbers, not read from the code
    if from_table:
        assert max(rows) == 4096 and {r for r in rows if r <= 128} and {r for r in rows if 128 < r <= 512} and \
            {r for r in rows if 512 < r <= 1024} and {r for r in rows if r > 1024}
    else:
        assert min(rows) == 4097 and 8192 in rows and max(rows) == 8193


def test_generic_mixed_family():
    got = {c.S: c for c in mc.cases("generic_mixed")}
    assert sorted(got) == [100, 1025]
    for S, c in got.items():
        (seg,) = c.segments(mc.L_POS)
        assert seg.mixed and seg.site(S) == 3 and c.n_slow(mc.L_POS) == 1 and len(seg.strings()) >= 3
        assert (seg.w > 64) if S <= 1024 else True
    assert got[100].n_slow(0) == 0 and got[1025].n_slow(0) == 2
