"""Python restatement of the diversity specification (edsx_paths_diversity / edsparser-diversity), for well formed texts:
brute force over tests/path_spec.py's parse - diff and comp are counted path pair by path pair from the chosen string
indices, never from the closed forms - and the derived statistics in the operation order of edsparser_amd/host/div_stats.hpp.
TEST INFRASTRUCTURE: the comparator of tests/test_div_*.py, never imported by edsparser_amd/."""
import math

import numpy as np

import ld_spec as ls
import path_spec as ps

MAX_GROUPS = 16
WINDOW_FIELDS = ("start", "end", "rank_first", "rank_end")
GROUP_FIELDS = ("segregating", "present")
PAIR_FIELDS = ("diff", "comp")


def group_sets(P, groups):
    """the sets M_g; ValueError with the library's text for what it refuses"""
    if groups is None or len(groups) == 0:
        return [set(range(1, P + 1))]
    if len(groups) > MAX_GROUPS:
        raise ValueError("Diversity has %d groups, above the limit of %d" % (len(groups), MAX_GROUPS))
    for g in groups:
        for p in g:
            if p < 1 or p > P:
                raise ValueError("Path id %d out of range (1..%d)" % (p, P))
    for k, g in enumerate(groups):
        if len(g) == 0:
            raise ValueError("Group %d is empty" % k)
    sets = [set(g) for g in groups]
    for p in range(1, P + 1):
        owners = [k for k, s in enumerate(sets) if p in s]
        if len(owners) > 1:
            raise ValueError("Path id %d is in groups %d and %d" % (p, owners[0], owners[1]))
    return sets


def chosen_indices(syms, sets, P):
    """per choice symbol: (symbol index, array over paths 1..P of the string index the path takes, -1 without one, strings)"""
    out = []
    for i, T, _ in ls.carriers(syms, sets, set(range(1, P + 1))):
        idx = np.full(P + 1, -1, dtype=np.int64)
        for j, t in enumerate(T):
            for p in t:
                idx[p] = j
        out.append((i, idx, len(T)))
    return out


def site(idx, n_strings, M):
    """one choice symbol: per group (seg, present, counts per string), per pair g <= h (diff, comp), by enumeration"""
    members = [np.array(sorted(m), dtype=np.int64) for m in M]
    per_group, per_pair = [], []
    for m in members:
        a = idx[m]
        counts = [int((a == j).sum()) for j in range(n_strings)]
        per_group.append((1 if sum(1 for c in counts if c) >= 2 else 0, int((a >= 0).sum()), counts))
    for g in range(len(M)):
        for h in range(g, len(M)):
            a, b = idx[members[g]], idx[members[h]]
            both = (a[:, None] >= 0) & (b[None, :] >= 0)         # every pair (p, q) of the two groups
            differ = both & (a[:, None] != b[None, :])
            if g == h:                                           # unordered, p != q
                both, differ = np.triu(both, 1), np.triu(differ, 1)
            per_pair.append((int(differ.sum()), int(both.sum())))
    return per_group, per_pair


def extent_and_coordinates(syms, choice, unit):
    if unit == "symbols":
        return len(choice), list(range(len(choice)))
    col, at = [], 0
    for s in syms:
        col.append(at)
        at += max(len(t) for t in s)
    E = max(at, 1)
    return E, [min(col[i], E - 1) for i, _, _ in choice]


def window_list(E, size, step):
    if E == 0:
        return []
    if size == 0:
        return [(0, E)]
    step = step or size
    return [(k * step, min(k * step + size, E)) for k in range((E + step - 1) // step)]


def diversity(eds, seds, groups=None, unit="symbols", size=0, step=0, sfs=False, max_windows=0):
    """-> dict: windows (tuples in WINDOW_FIELDS order), groups [window][g] (GROUP_FIELDS), pairs [window][q] (PAIR_FIELDS),
    sfs (per group a list of K_g + 1 counts, or None), K (per group), info"""
    syms, sets, P = ps.parse(eds, seds)
    M = group_sets(P, groups)
    G, NP = len(M), len(M) * (len(M) + 1) // 2
    choice = chosen_indices(syms, sets, P)
    nc = len(choice)
    E, coord = extent_and_coordinates(syms, choice, unit)
    info = {"groups": G, "paths": sum(len(m) for m in M), "choice_symbols": nc, "windows": 0, "pairs": NP, "row_words": (P + 63) // 64,
            "extent": E}
    K = [len(m) for m in M]
    if nc == 0:
        return {"windows": [], "groups": [], "pairs": [], "sfs": [[] for _ in M] if sfs else None, "K": K, "info": info}
    wins = window_list(E, size, step)
    info["windows"] = len(wins)
    if max_windows and len(wins) > max_windows:
        raise ValueError("Diversity has %d windows, above the limit of %d" % (len(wins), max_windows))
    sites = [site(idx, n, M) for _, idx, n in choice]
    spectra = [[0] * (k + 1) for k in K] if sfs else None
    if sfs:
        for per_group, _ in sites:
            for g, (_, present, counts) in enumerate(per_group):
                if present == K[g]:
                    for c in counts[1:]:
                        spectra[g][c] += 1
    out_w, out_g, out_p = [], [], []
    for start, end in wins:
        rs = [r for r in range(nc) if start <= coord[r] < end]
        r0 = sum(1 for r in range(nc) if coord[r] < start)
        assert rs == list(range(r0, r0 + len(rs)))               # coordinates do not decrease
        out_w.append((start, end, r0, r0 + len(rs)))
        out_g.append([(sum(sites[r][0][g][0] for r in rs), sum(sites[r][0][g][1] for r in rs)) for g in range(G)])
        out_p.append([(sum(sites[r][1][q][0] for r in rs), sum(sites[r][1][q][1] for r in rs)) for q in range(NP)])
    return {"windows": out_w, "groups": out_g, "pairs": out_p, "sfs": spectra, "K": K, "info": info}


def pair_index(G, g, h):
    return g * G - g * (g + 1) // 2 + h


# ---- the derived statistics: IEEE doubles in the operation order of div_stats.hpp; None where a denominator is zero
def ratio(diff, comp):
    return None if comp == 0 else float(diff) / float(comp)


def fst(pi_g, pi_h, dxy):
    if pi_g is None or pi_h is None or dxy is None or dxy == 0.0:
        return None
    return 1.0 - ((pi_g + pi_h) * 0.5) / dxy


def harmonic(K):
    a1 = a2 = 0.0
    for i in range(1, K):
        a1 += 1.0 / float(i)
        a2 += 1.0 / (float(i) * float(i))
    return a1, a2


def theta_w(seg, K):
    a1, _ = harmonic(K)
    return None if a1 == 0.0 else float(seg) / a1


def tajima_d(K, seg, diff, present, n_sites):
    if K < 2 or seg == 0 or present != n_sites * K:
        return None
    a1, a2 = harmonic(K)
    n = float(K)
    b1 = (n + 1.0) / (3.0 * (n - 1.0))
    b2 = (2.0 * (n * n + n + 3.0)) / (9.0 * n * (n - 1.0))
    c1 = b1 - 1.0 / a1
    c2 = b2 - (n + 2.0) / (a1 * n) + a2 / (a1 * a1)
    e1 = c1 / a1
    e2 = c2 / (a1 * a1 + a2)
    S = float(seg)
    k = float(diff) / float(K * (K - 1) // 2)
    var = e1 * S + e2 * S * (S - 1.0)
    if not var > 0.0:
        return None
    return (k - S / a1) / math.sqrt(var)


def fmt(v):
    return "NA" if v is None else "%.6g" % v


GROUP_HEADER = "start\tend\tsites\tgroup\tpaths\tsegregating\tpresent\tdiff\tcomp\tpi\ttheta_w\ttajima_d\n"
PAIR_HEADER = "start\tend\tsites\tgroup_a\tgroup_b\tdiff\tcomp\tdxy\tfst\n"


def group_text(res, names=None):
    """what edsparser-diversity writes to its output: one line per (window, group)"""
    K, G = res["K"], len(res["K"])
    names = names or (["all"] if G == 1 else ["g%d" % g for g in range(G)])
    out = [GROUP_HEADER]
    for w, (start, end, r0, r1) in enumerate(res["windows"]):
        for g in range(G):
            seg, present = res["groups"][w][g]
            diff, comp = res["pairs"][w][pair_index(G, g, g)]
            out.append("%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%s\t%s\t%s\n" % (
                start, end, r1 - r0, names[g], K[g], seg, present, diff, comp, fmt(ratio(diff, comp)), fmt(theta_w(seg, K[g])),
                fmt(tajima_d(K[g], seg, diff, present, r1 - r0))))
    return "".join(out).encode()


def pair_text(res, names=None):
    """<out>.pairs: one line per (window, g < h)"""
    G = len(res["K"])
    names = names or ["g%d" % g for g in range(G)]
    out = [PAIR_HEADER]
    for w, (start, end, r0, r1) in enumerate(res["windows"]):
        pr = res["pairs"][w]
        for g in range(G):
            for h in range(g + 1, G):
                diff, comp = pr[pair_index(G, g, h)]
                dxy = ratio(diff, comp)
                f = fst(ratio(*pr[pair_index(G, g, g)]), ratio(*pr[pair_index(G, h, h)]), dxy)
                out.append("%d\t%d\t%d\t%s\t%s\t%d\t%d\t%s\t%s\n" % (start, end, r1 - r0, names[g], names[h], diff, comp, fmt(dxy), fmt(f)))
    return "".join(out).encode()


def sfs_text(res, names=None):
    """--sfs: group, count, sites - one line per bin"""
    G = len(res["K"])
    names = names or (["all"] if G == 1 else ["g%d" % g for g in range(G)])
    return ("group\tcount\tsites\n" + "".join("%s\t%d\t%d\n" % (names[g], c, v) for g in range(G) for c, v in enumerate(res["sfs"][g]))).encode()
