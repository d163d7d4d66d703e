"""Python restatement of the linkage disequilibrium specification (edsx_paths_ld / edsparser-ld), for well formed texts:
brute force over tests/path_spec.py's parse with python sets, no bit tricks.  TEST INFRASTRUCTURE: the comparator of
tests/test_ld_*.py, never imported by edsparser_amd/."""
from fractions import Fraction

import path_spec as ps

PAIR_FIELDS = ("symbol_a", "string_a", "symbol_b", "string_b", "n_ab", "n_a", "n_b", "n", "r2")
ALLELE_FIELDS = ("symbol", "string", "count", "present")


def requested(P, paths):
    """the set M; ValueError with the library's text for an id outside 1..P"""
    paths = list(paths) if paths else list(range(1, P + 1))
    for p in paths:
        if p < 1 or p > P:
            raise ValueError("Path id %d out of range (1..%d)" % (p, P))
    return set(paths)


def carriers(syms, sets, M):
    """per choice symbol - one that is not a single universal string - in file order: (its index among all symbols, T: per
    string the paths of M that take it, U: the paths of M present).  A path takes the first string whose set holds it or 0."""
    out, sid = [], 0
    for i, strings in enumerate(syms):
        q = sets[sid:sid + len(strings)]
        sid += len(strings)
        if len(strings) == 1 and 0 in q[0]:
            continue
        T = [set() for _ in strings]
        for p in M:
            j = next((j for j in range(len(strings)) if p in q[j] or 0 in q[j]), None)
            if j is not None:
                T[j].add(p)
        out.append((i, T, set().union(*T)))
    return out


def counts(x, y):
    """(n_ab, n_a, n_b, n) of the alleles x = (T, U) and y, over the paths present at both symbols"""
    (Tx, Ux), (Ty, Uy) = x, y
    return len(Tx & Ty), len(Tx & Uy), len(Ty & Ux), len(Ux & Uy)


def r2_of(n_ab, n_a, n_b, n, exact=False):
    """None when undefined; the three operations of ld::r2 on doubles, or the exact fraction"""
    da, db, D = n_a * (n - n_a), n_b * (n - n_b), n * n_ab - n_a * n_b
    if da * db == 0:
        return None
    if exact:
        return Fraction(D, da) * Fraction(D, db)
    return (D / da) * (D / db)


def ld(eds, seds, paths=None, window=100, min_r2=0.0, min_count=1, all_strings=False):
    """-> dict: pairs (tuples in PAIR_FIELDS order, in (x, y) order), alleles (ALLELE_FIELDS), info (paths,
    choice_symbols, alleles, candidate_pairs, undefined_pairs, pairs), and for the tests below_pairs and candidates: every
    candidate pair as (symbol_a, string_a, symbol_b, string_b, n_ab, n_a, n_b, n) whatever its r2"""
    if window < 1:
        raise ValueError("window")
    if not 0.0 <= min_r2 <= 1.0:
        raise ValueError("min_r2")
    syms, sets, P = ps.parse(eds, seds)
    M = requested(P, paths)
    cs = carriers(syms, sets, M)
    listed = []                                                  # (r, symbol, j, T, U)
    for r, (i, T, U) in enumerate(cs):
        for j in range(len(T)):
            if (j >= 1 or all_strings) and min_count <= len(T[j]) <= len(U) - min_count:
                listed.append((r, i, j, T[j], U))
    pairs, cand, undefined, below = [], [], 0, 0
    for a, (r, i, j, T, U) in enumerate(listed):
        for (r2_, i2, j2, T2, U2) in listed[a + 1:]:
            if not r < r2_ <= r + window:
                continue
            c = counts((T, U), (T2, U2))
            cand.append((i, j, i2, j2) + c)
            v = r2_of(*c)
            if v is None:
                undefined += 1
            elif v >= min_r2:
                pairs.append((i, j, i2, j2) + c + (v,))
            else:
                below += 1
    info = {"paths": len(M), "choice_symbols": len(cs), "alleles": len(listed), "candidate_pairs": len(cand),
            "undefined_pairs": undefined, "pairs": len(pairs)}
    return {"pairs": pairs, "alleles": [(i, j, len(T), len(U)) for _, i, j, T, U in listed], "info": info, "below_pairs": below,
            "candidates": cand}


def pair_text(pairs):
    """what edsparser-ld writes: the header and one tab separated line per pair, r2 as %.6g"""
    return ("\t".join(PAIR_FIELDS) + "\n" + "".join("\t".join("%d" % v for v in p[:8]) + "\t%.6g\n" % p[8] for p in pairs)).encode()


def freq_text(alleles):
    """what edsparser-ld --freq writes: symbol string count present freq, freq = count / present as %.6g (0 for 0 / 0)"""
    return ("symbol\tstring\tcount\tpresent\tfreq\n" +
            "".join("%d\t%d\t%d\t%d\t%.6g\n" % (a + ((a[2] / a[3]) if a[3] else 0.0,)) for a in alleles)).encode()
