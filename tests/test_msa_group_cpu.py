"""The directed segments of tests/msa_group_spec.py, before a GPU is involved.

1. The reference of one segment (msa_group_spec.Groups) is pinned to what the project already trusts: every segment that an
   alignment's text can carry (no NUL, no line end inside a row) is wrapped, all segments of one S in one FASTA alignment,
   and the texts that the reference spells must equal those of msa_spec.transform and of the oracle (oracle_lib.msa).
2. The premises of the cases are asserted from the bytes - string counts, raw-class counts, first rows - and the routing
   table (msa_group_spec.Seg.route) is shown to be exercised on both sides of every limit."""
import numpy as np
import pytest

import msa_group_spec as spec
import msa_spec
import oracle_lib as o


@pytest.mark.parametrize("S", spec.SIZES)
def test_reference_equals_the_trusted_specifications(S):
    segs = [s for s in spec.cases(S) + spec.fused_runs(S, False) + (spec.fused_runs(S, True) if S <= 64 else []) if spec.wrappable(s)]
    assert len(segs) > 100
    text, eds, seds = spec.wrap(segs)
    assert msa_spec.transform(text, spec.WRAP_L) == (eds, seds)
    assert o.msa(text, spec.WRAP_L) == (eds, seds)


def test_wrapped_out_cases_are_the_nul_and_newline_ones():
    for S in spec.SIZES:
        for s in spec.cases(S):
            if not spec.wrappable(s):
                assert s.has(0) or s.has(0x0A), s.name
                if s.has(0):                                   # a NUL: only the return code is compared, and it is 0
                    assert s.route(True) == 0 and s.route(False) in (0, 2), s.name


@pytest.mark.parametrize("S", spec.SIZES)
def test_premises(S):
    for s in spec.cases(S) + spec.fused_runs(S, False) + (spec.fused_runs(S, True) if S <= 64 else []):
        p, g = s.premise, s.groups
        rows = [r.tobytes() for r in s.M]
        assert s.S == S and g.k == len({spec.strip(r) for r in rows}) and g.sumlen == sum(len(x) for x in {spec.strip(r) for r in rows})
        assert [rows.index(next(r for r in rows if spec.strip(r) == x)) for x in g.strings] == g.rep == sorted(g.rep), s.name
        if "strings" in p:
            assert g.k == p["strings"], (s.name, g.k)
        if "raw" in p:
            assert s.raw_classes() == p["raw"], (s.name, s.raw_classes())
        if "dna" in p:
            assert s.all_dna() == p["dna"], s.name
        if p.get("joins"):
            assert s.raw_classes() > g.k, s.name
        if p.get("nul"):
            assert s.has(0), s.name
        if "distinct_bytes" in p:
            assert len(set(s.M[:, 0].tolist())) == p["distinct_bytes"], s.name
        for byte, r in p.get("first_row", {}).items():
            col = s.M[:, 0].tolist()
            assert col.index(byte) == r and set(col[:min(r, min(p["first_row"].values()))]) == {ord("A")}, s.name
        if "differ_only_at" in p:
            j = p["differ_only_at"]
            assert len({r[:j] + r[j + 1:] for r in rows}) == 1 and len({r[j] for r in rows}) == min(S, 6), s.name
        if p.get("lengths"):
            assert {len(x) for x in g.strings} >= set(p["lengths"]) and (s.raw_classes() > g.k or s.ncol == 2), s.name
        if "foreign_at" in p:
            bad = np.argwhere(~spec._D_SET[s.M])
            assert bad.tolist() == [list(p["foreign_at"])], s.name
        if "textlen" in p:
            assert len(g.text()) == p["textlen"] == 1 + g.k + g.sumlen and s.all_dna(), s.name
        if p.get("lane_path"):
            assert S <= 64 and s.route(True) == 1 and s.route(False) == 2 and (s.ncol > 20 or not s.all_dna()), s.name


def _have(S, name):
    return [s for s in spec.cases(S) if s.name == name]


def test_routing_table_is_exercised_on_both_sides_of_every_limit():
    route = lambda S, name: [(s.route(False), s.route(True)) for s in _have(S, name)]
    for S in spec.SIZES:
        names = {s.name for s in spec.cases(S)}
        # one column: DNA, another alphabet, NUL first and last
        assert route(S, "one/subset01") == [(1, 1)] and route(S, "one/lower") == [(1, 1)]
        assert route(S, "one/nul_first") == [(0, 0)] and route(S, "one/nul_last") == [(0, 0)]
        # 10 against 11 letters in a key; a foreign byte
        assert route(S, "dna/w10/lengths") == [(1, 1)] and route(S, "dna/w11/lengths") == [(2, 1)]
        assert route(S, "dna/w20/lengths") == [(2, 1)]
        assert route(S, "dna/w10/one_foreign_byte") == [(2, 1)] and route(S, "dna/w20/one_foreign_byte") == [(2, 1)]
        assert route(S, "desc/mixed/between/dna") == [(2, 1)] and route(S, "desc/mixed/nul") == [(2, 0)]
        if S >= 65:
            # exactly 64 or 65 distinct strings, on each exact-key path
            for i, k in ((0, 64), (1, 65), (2, 64), (3, 64), (4, 65)):
                (s,) = [s for s in spec.cases(S) if s.name.startswith("one/bytes") and s.name.endswith("_%d" % i)]
                assert s.groups.k == k and (s.route(False), s.route(True)) == ((1, 1) if k == 64 else (0, 0)), s.name
            for w in (9, 10):
                assert route(S, "dna/w%d/strings64" % w) == [(1, 1)] and route(S, "dna/w%d/strings65" % w) == [(0, 0)]
                assert route(S, "dna/w%d/raw65_strings64" % w) == [(1, 1)]
            for w in (11, 19, 20):
                assert route(S, "dna/w%d/strings64" % w) == [(2, 1)] and route(S, "dna/w%d/strings65" % w) == [(2, 0)]
                assert route(S, "dna/w%d/raw65_strings64" % w) == [(2, 1)]
            # 16 against 17, 64 against 65 raw groups; a class that first appears in row 64 or later
            for w in (2, 21, 63, 64):
                for R in (8, 9, 16, 17, 32, 33, 64):
                    assert route(S, "refine/w%d/raw%d" % (w, R)) == [(2, 1)]
                assert route(S, "refine/w%d/raw65" % w) == [(2, 0)] and route(S, "refine/w%d/nul" % w) == [(2, 0)]
            assert route(S, "desc/mixed/raw64") == [(2, 1)] and route(S, "desc/mixed/raw65") == [(2, 0)]
            assert {"one/late63", "one/late64"} <= names and ("one/late%d" % (S - 1)) in names
            if S > 81:
                assert {"one/late79", "one/late80", "one/late80+2"} <= names
            assert any(s.place and s.place[0] == "two" and s.place[1] in (1, s.ncol - 1) for s in spec.cases(S))
        else:
            assert "lane/w21/dna" in names and route(S, "lane/w21/nul") == [(2, 0)]
            if S == 64:
                assert route(S, "dna/w10/strings64") == [(1, 1)] and route(S, "dna/w20/strings64") == [(2, 1)]


def test_fused_runs_sit_on_both_sides_of_the_record_limits():
    for S in spec.SIZES:
        for rows64 in ((False, True) if S <= 64 else (False,)):
            runs = {r.name: r for r in spec.fused_runs(S, rows64)}
            ok = {n: r.fused_ok() for n, r in runs.items()}
            assert {r.ncol for r in runs.values()} >= set(range(1, 21 if rows64 else 11))
            if S >= 17:
                assert ok["fused/w2/k16"] and not ok["fused/w2/k17"] and ok["fused/w2/k4"] and ok["fused/w2/k5"]
                assert runs["fused/w2/k16"].groups.k == 16 and runs["fused/w2/k17"].all_dna()
            if S >= 6:
                assert ok["fused/text64"] and not ok["fused/text65"] and runs["fused/text65"].groups.k <= 16
            if S >= 3:
                assert [runs["fused/empty_" + n].groups.strings.index(b"") for n in ("first", "middle", "last")] == [0, 1, 2]
            assert not ok["fused/w1/foreign_last"] and not ok["fused/w2/foreign_first"]
