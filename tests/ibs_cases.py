"""Inputs of the shared-segment tests (tests/test_ibs_cpu.py, test_ibs_gpu.py, ibs_guard_child.py): the boundary shapes of
k_ibs_scan and k_ibs_stitch, each a few hundred symbols (the chunk shapes: two thousand) and a handful of paths, or 130
paths and 41 symbols.  A request is the keyword arguments of tests/ibs_spec.py's ibs and of PathSession.ibs.  TEST
INFRASTRUCTURE, never imported by edsparser_amd/."""
import random

import dist_cases as dc
import ibs_spec as isp

CHUNK_COLUMNS = dc.CHUNK_COLUMNS
EVERY = dict(min_sites=0, min_columns=0)


def seam_eds(c, rng, P=5):
    """exactly c class columns (c >= 8) over P paths, none of which ever lacks a string: a symbol of three strings first,
    so that the two or three columns of the symbols behind it lie across every multiple of 64; then symbols of two
    strings (and one more of three when c is even), with fixed symbols {TT} and zero-width fixed symbols {} strewn in.
    Most symbols single out path P, so the pairs among the others share long segments, over word and chunk seams; a symbol
    whose columns lie across a multiple of 64 splits the paths {1,2} | {3..P}, so its two bits are set in two words, or
    in two chunks, for the pairs (1,3), (2,3), ..."""
    sizes = [3] + [2] * ((c - 3) // 2) if c % 2 else [3] + [2] * ((c - 6) // 2) + [3]
    assert sum(sizes) == c
    everyone = set(range(1, P + 1))
    syms, sets, at = [], [], 0
    for k in sizes:
        across = any((at + j) % 64 == 63 for j in range(k - 1))
        if across:
            part = [{1, 2}, everyone - {1, 2}] if k == 2 else [{1, 2}, everyone - {1, 2, P}, {P}]
        else:
            q = P if rng.random() < 0.7 else rng.randint(1, P)
            if k == 2:
                part = [everyone - {q}, {q}]
            else:
                q2 = rng.choice(sorted(everyone - {q}))
                part = [everyone - {q, q2}, {q}, {q2}]
            rng.shuffle(part)
        syms.append([b"A", b"CG", b""][:k])
        sets += part
        at += k
        r = rng.random()
        if r < 0.25:
            syms.append([b"TT"]); sets.append({0})
        elif r < 0.35:
            syms.append([b""]); sets.append({0})
    return dc.render(syms, sets)


# by hand.  ENDS: the pair (1, 2) differs at the first and at the last symbol and shares the fixed symbol between them
# (sites 0: reported only with min_sites 0); path 3 goes with path 1 throughout: one segment, the whole EDS
ENDS = (b"{A,C}{TT}{G,T}", b"{1,3}{2}{0}{1,3}{2}")
# two adjacent differing symbols and nothing else: the pair has no segment at all
ADJACENT = (b"{A,C}{A,C}", b"{1}{2}{1}{2}")
# symbol 1 leaves the paths 3 and 4 without a string: (3, 4) agree there, (1, 3) and (2, 4) differ; symbol 3 is zero width
# and lies inside segments; symbol 5 tells 4 from the rest, so P = 4
NONE = (b"{A}{C,G}{T}{}{GG}{A,C}{T}", b"{0}{1}{2}{0}{0}{0}{1,2,3}{4}{0}")
# choice symbols 0, 3 and 6 with fixed and zero-width symbols between; equal texts in symbol 3 are different strings
GAPS = (b"{A,C}{TT}{}{G,G}{}{}{A,CCC,}{T}", b"{1,2}{3,4}{0}{0}{1,3}{2,4}{0}{0}{1}{2,3}{4}{0}")
FIXED = (b"{ACGT}{GG}{}", b"{0,3}{0}{0,1}")                     # no choice symbol, three paths: every pair shares [0, 2]


def thresholds(eds, seds, paths=None):
    """requests with the thresholds exactly at the sites and the columns of a segment of the shape, and one above"""
    segs = isp.ibs(eds, seds, paths, 0, 0)["segments"]
    s = sorted(segs, key=lambda r: (r[4], r[6] - r[5]))[len(segs) // 2]
    sites, cols = s[4], s[6] - s[5]
    kw = dict(paths=paths) if paths else {}
    return [dict(kw, min_sites=sites, min_columns=0), dict(kw, min_sites=sites + 1, min_columns=0), dict(kw, min_sites=0, min_columns=cols),
            dict(kw, min_sites=0, min_columns=cols + 1), dict(kw, min_sites=sites, min_columns=cols)]


def boundary_shapes():
    """name -> (eds, seds, requests)"""
    rng = random.Random(14)
    wide = dc.wide_eds(rng)
    shapes = {
        "wide": wide + ([dict(paths=list(range(1, K + 1))) for K in (1, 2, 63, 64, 65, 130)] +
                        [dict(EVERY, paths=list(range(130, 0, -1))), dict(EVERY, paths=[130, 1, 64, 64, 65, 1]), dict(paths=[7, 7])],),
        "fixed": FIXED + ([EVERY, {}, dict(EVERY, paths=[3, 3, 1]), dict(EVERY, paths=[2])],),
        "edge": dc.EDGE + ([EVERY, dict(paths=[66, 66, 1]), dict(EVERY, paths=[67, 65, 66, 2, 1])],),
        "ends": ENDS + ([EVERY, {}, dict(EVERY, paths=[2, 1, 3, 1])],),
        "adjacent": ADJACENT + ([EVERY, {}],),
        "none": NONE + ([EVERY, {}, dict(min_sites=0, min_columns=3)],),
        "gaps": GAPS + ([EVERY, {}] + thresholds(*GAPS),),
    }
    for c in (63, 64, 65, CHUNK_COLUMNS - 1, CHUNK_COLUMNS, CHUNK_COLUMNS + 1):
        e, s = seam_eds(c, rng)
        shapes["columns%d" % c] = (e, s, [EVERY, {}] + thresholds(e, s)[:4])
    return shapes
