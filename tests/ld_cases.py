"""Inputs of the linkage disequilibrium tests (tests/test_ld_cpu.py, test_ld_gpu.py, ld_guard_child.py): panels whose
symbols split the paths among their strings, with overlapping sets, paths left out and universal strings; and the boundary
shapes of the kernels - row words on both sides of a word, a second LDS stage, allele counts around the 64-allele tile, a
symbol whose alleles straddle a tile edge, windows around nc.  TEST INFRASTRUCTURE, never imported by edsparser_amd/."""
import random

from dist_cases import random_eds, render  # noqa: F401  (random_eds: the small random EDSs of the CPU tests)


def panel_eds(rng, P, n_symbols, p_missing=0.0, p_overlap=0.1, universal=None, sizes=(2, 2, 3, 4), fixed_every=4):
    """n_symbols choice symbols over P paths: every path takes one string of a symbol or, with p_missing, none; with
    p_overlap it stands in a second set as well (the first in file order counts).  universal: None, or "first" / "middle" /
    "last" - in every third symbol that string's set is {0}.  Fixed symbols in between; the last symbol names path P."""
    syms, sets = [], []
    for s in range(n_symbols):
        if fixed_every and s % fixed_every == fixed_every - 1:
            syms.append([b"ACGT"]); sets.append({0})
        k = rng.choice(sizes)
        part = [set() for _ in range(k)]
        for p in range(1, P + 1):
            if rng.random() >= p_missing:
                part[rng.randrange(k)].add(p)
            if rng.random() < p_overlap:
                part[rng.randrange(k)].add(p)
        for q in part:
            if not q:
                q.add(rng.randint(1, P))
        if universal and s % 3 == 1:
            part[{"first": 0, "middle": k // 2, "last": k - 1}[universal]] = {0}
        syms.append([b"ACGT"[j % 4:j % 4 + 1] * (1 + j // 4) for j in range(k)]); sets += part
    syms.append([b"A", b"C"]); sets += [{P}, {1} if P > 1 else {P}]
    return render(syms, sets)


def biallelic_eds(rng, n_symbols, P=6, dead=0):
    """n_symbols symbols {A,C} that split the P paths in two non-empty halves: one listed allele each by default; `dead` more
    symbols whose second string no path takes (its set lies inside the first): choice symbols without a listed allele"""
    syms, sets = [], []
    for s in range(n_symbols + dead):
        half = set(rng.sample(range(1, P + 1), rng.randint(1, P - 1)))
        syms.append([b"A", b"C"])
        sets += ([set(range(1, P + 1)), half] if s >= n_symbols else [half, set(range(1, P + 1)) - half])
    return render(syms, sets)


def wide_symbol_eds(rng, strings=70, P=80):
    """a symbol of `strings` strings, string j taken by path j + 1 alone and the last by all the others, between biallelic
    symbols: its alleles straddle a tile edge"""
    e1, s1 = biallelic_eds(rng, 30, P)
    e2, s2 = biallelic_eds(rng, 40, P)
    wide = [b"%c%c" % (65 + j % 26, 97 + j // 26) for j in range(strings)]
    wsets = [{j + 1} for j in range(strings - 1)] + [set(range(strings, P + 1))]
    we, ws = render([wide], wsets)
    return e1 + we + e2, s1 + ws + s2


def _req(**kw):
    return kw


def boundary_shapes():
    """name -> (eds, seds, requests): a request is the keyword arguments of PathSession.ld / ld_spec.ld"""
    rng = random.Random(20)
    both = [_req(window=3), _req(window=3, all_strings=True, min_count=0), _req(window=2, min_count=2, all_strings=True)]
    shapes = {}
    for P in (1, 2, 63, 64, 65, 127, 128, 129):                  # at 64, W = 2 but WP = 1
        shapes["paths%d" % P] = panel_eds(rng, P, 12, p_missing=0.1 if P > 2 else 0.0) + (both,)
    shapes["paths2049"] = panel_eds(rng, 2049, 5, p_missing=0.02, fixed_every=0) + ([_req(window=2), _req(window=6, all_strings=True)],)
    for A in (0, 1, 63, 64, 65, 129, 200):
        shapes["alleles%d" % A] = biallelic_eds(rng, A, dead=3 if A in (0, 64) else 0) + ([_req(window=5), _req(window=300)],)
    shapes["wide70"] = wide_symbol_eds(rng) + ([_req(window=4), _req(window=40, all_strings=True), _req(window=200, min_count=0)],)
    eds, seds = panel_eds(rng, 20, 9, fixed_every=0)             # nc = 10
    shapes["windows"] = (eds, seds, [_req(window=w, all_strings=True) for w in (1, 2, 9, 10, 15)])
    for where in ("first", "middle", "last"):
        shapes["universal_" + where] = panel_eds(rng, 70, 12, p_missing=0.15, universal=where) + (both,)
    # symbols that leave paths of M out next to ones that do not: both epilogue paths in one tile
    e1, s1 = panel_eds(rng, 40, 6, p_missing=0.0, p_overlap=0.0, fixed_every=0)
    e2, s2 = panel_eds(rng, 40, 6, p_missing=0.3, fixed_every=0)
    shapes["missing"] = (e1 + e2 + e1, s1 + s2 + s1, both + [_req(window=30, paths=[3, 40, 7, 7, 12, 13, 14, 21, 22, 30, 31])])
    shapes["subset"] = panel_eds(rng, 130, 10, p_missing=0.05) + ([_req(window=4, paths=list(range(1, 131, 3)) + [1, 4]),
                                                                    _req(window=4, paths=[64, 65, 128, 129, 130, 1, 2]),
                                                                    _req(window=9, paths=[5], min_count=0)],)
    shapes["fixed"] = (b"{ACGT}{GG}{}", b"{0,3}{0}{0,1}", [_req(window=1)])      # no choice symbol, three paths
    return shapes
