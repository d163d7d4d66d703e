"""CPU: the path subsetting specification (tests/subset_spec.py) against the path spelling specification
(tests/path_spec.py) on seeded random EDS + sEDS, its own algebra (keep_ids, subsetting twice), and hand-written cases
with literal expected texts.  The library is pinned to this specification byte for byte in tests/test_subset_gpu.py."""
import random
import re

import pytest

import path_spec as ps
import subset_spec as ss


def random_eds(rng, P=None, n=None, disjoint=False):
    """A random (eds, seds): degenerate symbols with explicit sets, universal strings, one-string symbols with explicit
    sets, empty strings, paths that are missing at a symbol.  disjoint: no path has two strings to choose from in a
    symbol (no universal string and no overlapping sets inside a degenerate symbol)."""
    P = P or rng.randint(1, 9)
    syms, sets = [], []
    for _ in range(n or rng.randint(1, 14)):
        kind = rng.random()
        text = lambda lo=0: "".join(rng.choice("ACGT") for _ in range(rng.randint(lo, 5))).encode()
        if kind < 0.35:
            syms.append([text(1)]); sets.append({0})
        elif kind < 0.55:                                          # one string with an explicit set (sometimes all paths)
            syms.append([text()])
            sets.append(set(range(1, P + 1)) if rng.random() < 0.4 else set(rng.sample(range(1, P + 1), rng.randint(1, P))))
        else:
            k = rng.randint(2, 4)
            syms.append([text() for _ in range(k)])
            owner = [rng.randrange(k + 1) for _ in range(P)]       # k: the path has no string here
            for j in range(k):
                s = {p + 1 for p in range(P) if owner[p] == j}
                if disjoint:
                    pass
                elif rng.random() < 0.15:
                    s = {0}
                elif rng.random() < 0.2:
                    s |= set(rng.sample(range(1, P + 1), rng.randint(1, P)))   # overlapping sets: the first string wins
                sets.append(s or ({owner.index(k) + 1} if disjoint and k in owner else {rng.randint(1, P)}))
    if max(max(s) for s in sets) < P:
        sets[-1] = (sets[-1] - {0}) | {P} if sets[-1] != {0} else sets[-1]
    eds = b"".join(b"{" + b",".join(s) + b"}" for s in syms)
    seds = b"".join(b"{" + b",".join(b"%d" % p for p in sorted(s)) + b"}" for s in sets)
    return eds, seds


def random_cases(seed, count):
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        eds, seds = random_eds(rng)
        P = ps.parse(eds, seds)[2]
        if P == 0:
            continue
        out.append((eds, seds, sorted(rng.sample(range(1, P + 1), rng.randint(1, P)))))
    return out


CASES = random_cases(20250101, 400)


def test_every_kept_path_spells_what_it_spelled():
    checked = 0
    for eds, seds, K in CASES:
        syms, sets, P = ps.parse(eds, seds)
        oe, os_, info = ss.subset(eds, seds, K)
        osyms, osets, OP = ps.parse(oe, os_)                       # parse checks the cardinality of the pair
        assert oe.endswith(b"\n") and os_.endswith(b"\n") and OP <= len(K)
        for r, p in enumerate(K):
            seq, miss = ps.spell(syms, sets, p)
            oseq, omiss = ps.spell(osyms, osets, r + 1)
            assert oseq == seq and omiss <= miss, (eds, seds, K, p)
            checked += 1
        assert info["symbols_out"] == len(osyms) and info["strings_out"] == len(osets)
        assert info["chars_out"] == sum(len(t) for s in osyms for t in s)
        assert (info["symbols_in"], info["strings_in"], info["paths_in"], info["paths_out"]) == (len(syms), len(sets), P, len(K))
    assert checked >= 1000


def test_no_adjacent_commons_and_no_empty_common():
    for eds, seds, K in CASES:
        osyms, osets, _ = ps.parse(*ss.subset(eds, seds, K)[:2])
        sid, prev = 0, False
        for strings in osyms:
            common = len(strings) == 1 and osets[sid] == {0}
            assert not (common and prev), (eds, seds, K)
            assert not (common and strings[0] == b""), (eds, seds, K)
            prev = common
            sid += len(strings)


def test_keep_ids_differs_only_in_the_id_digits():
    for eds, seds, K in CASES:
        a = ss.subset(eds, seds, K)
        b = ss.subset(eds, seds, K, keep_ids=True)
        assert a[0] == b[0] and {k: v for k, v in a[2].items()} == b[2]
        back = {r + 1: p for r, p in enumerate(K)}
        back[0] = 0
        mapped = re.sub(rb"\d+", lambda m: b"%d" % back[int(m.group())], a[1])
        assert mapped == b[1], (eds, seds, K)


def test_subsetting_twice_is_subsetting_once():
    rng = random.Random(5)
    for eds, seds, K in CASES:
        K2 = sorted(rng.sample(K, rng.randint(1, len(K))))
        first = ss.subset(eds, seds, K)
        rank = {p: r + 1 for r, p in enumerate(K)}
        P1 = ps.parse(first[0], first[1])[2]
        ids = [rank[p] for p in K2]
        if any(i > P1 for i in ids):                               # a kept path that no string names: ids above P are refused
            continue
        second = ss.subset(first[0], first[1], ids)
        direct = ss.subset(eds, seds, K2)
        assert second[:2] == direct[:2], (eds, seds, K, K2)


# ---- hand-written cases: (name, eds, seds, K, keep_ids, expected eds, expected seds) --------------------------------------
HAND = [
    ("a symbol removed between two commons, which then fuse",
     b"{AC}{G,T}{TT}{A,C}", b"{0}{2}{4}{0}{1}{3}", [1, 3], False, b"{ACTT}{A,C}\n", b"{0}{1}{2}\n"),
    ("the same with an id that keeps the middle symbol: one kept string that covers K is common too",
     b"{AC}{G,T}{TT}{A}", b"{0}{1}{2}{0}{1,2,3}", [2], False, b"{ACTTTA}\n", b"{0}\n"),
    ("a one-string symbol whose set does not cover K stays explicit and does not fuse",
     b"{AC}{G}{TT}", b"{0}{1,3}{0}", [1, 2], False, b"{AC}{G}{TT}\n", b"{0}{1}{0}\n"),
    ("its ids are renumbered, or kept",
     b"{AC}{G}{TT}", b"{0}{2,3}{0}", [2, 3, 1], True, b"{AC}{G}{TT}\n", b"{0}{2,3}{0}\n"),
    ("a one-string empty symbol with set K becomes common, is empty, and its run is dropped",
     b"{}{A,C}", b"{1,2,3}{1}{2,3}", [1, 2, 3], False, b"{A,C}\n", b"{1}{2,3}\n"),
    ("an empty common between two commons neither breaks the run nor shows",
     b"{AC}{}{GT}{A,C}", b"{0}{1,2}{0}{1}{2}", [1, 2], False, b"{ACGT}{A,C}\n", b"{0}{1}{2}\n"),
    ("a universal string inside a degenerate symbol is kept and stays {0}",
     b"{A,C,G}{T}", b"{1}{0}{2}{0}", [2], False, b"{C,G}{T}\n", b"{0}{1}{0}\n"),
    ("sets inside a degenerate symbol are never rewritten to {0}, not even when they equal K",
     b"{A,C}", b"{1,2}{2}", [1, 2], False, b"{A,C}\n", b"{1,2}{2}\n"),
    ("K = {p} where p is missing at some symbol",
     b"{AC}{G,T}{A,C}{TT}", b"{0}{1}{2}{1,3}{2}{0}", [3], False, b"{ACATT}\n", b"{0}\n"),
    ("everything dropped: no string names the kept path",
     b"{A,C}{G}", b"{1}{2}{1,4}", [3], False, b"\n", b"\n"),
    ("equal texts are not deduplicated, file order stays, empty strings keep their place",
     b"{A,,A,C}{T}", b"{1}{2}{3}{4}{0}", [1, 2, 3], False, b"{A,,A}{T}\n", b"{1}{2}{3}{0}\n"),
    ("ranks with two digits",
     b"{A,C}{G}", b"{3,5,7,9,11,13,15,17,19,21,23}{2,4}{0}", [3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 2], False,
     b"{A,C}{G}\n", b"{2,3,4,5,6,7,8,9,10,11,12}{1}{0}\n"),
]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_written(case):
    _, eds, seds, K, keep, want_eds, want_seds = case
    got = ss.subset(eds, seds, K, keep)
    assert got[:2] == (want_eds, want_seds)


def test_hand_written_info():
    info = ss.subset(b"{AC}{G,T}{TT}{}{A,C}", b"{0}{1}{2}{0}{3}{1}{2,3}", [3])[2]
    assert info == {"symbols_in": 5, "symbols_out": 1, "strings_in": 7, "strings_out": 1, "chars_in": 8, "chars_out": 5,
                    "paths_in": 3, "paths_out": 1, "symbols_removed": 1, "common_runs_merged": 1}


def test_exclude_is_the_complement():
    eds, seds = b"{AC}{G,T,A}{TT}", b"{0}{1,4}{2}{3}{0}"
    assert ss.complement([2, 3], 4) == [1, 4]
    assert ss.subset(eds, seds, ss.complement([2, 3], 4))[:2] == (b"{ACGTT}\n", b"{0}\n")
    assert ss.subset(eds, seds, ss.complement([1, 4], 4))[:2] == (b"{AC}{T,A}{TT}\n", b"{0}{1}{2}{0}\n")
    assert ss.complement([], 3) == [1, 2, 3]
    with pytest.raises(ValueError, match="No paths selected"):
        ss.subset(eds, seds, ss.complement([1, 2, 3, 4], 4))


def test_errors():
    eds, seds = b"{AC}{G,T}", b"{0}{1}{2,3}"
    for ids, text in (([], "No paths selected"), ([0], r"Path id 0 out of range \(1..3\)"), ([2, 4], r"Path id 4 out of range \(1..3\)"),
                      ([2, 1, 2], "Path id 2 given twice")):
        with pytest.raises(ValueError, match=text):
            ss.subset(eds, seds, ids)
