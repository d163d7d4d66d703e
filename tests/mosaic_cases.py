"""Inputs of the mosaic tests (tests/test_mosaic_cpu.py, test_mosaic_gpu.py, mosaic_guard_child.py): the shapes of
tests/ibs_cases.py and tests/dist_cases.py at the word seams of the march of k_mosaic, 130 and 300 paths for the donors of
one lane, of one wave, of one workgroup and of more than one pass over its lanes, a planted recombinant, ties, duplicates,
the target among its donors and the target as its only donor.  A request is the keyword arguments of tests/mosaic_spec.py's
mosaic and of PathSession.mosaic.  TEST INFRASTRUCTURE, never imported by edsparser_amd/."""
import random

import dist_cases as dc
import ibs_cases as ic

CHUNK_COLUMNS = dc.CHUNK_COLUMNS
ALL = {}

# paths 1, 2, 3 start alike and 4 differs; at symbol 1 path 1 leaves 2 and 3 and joins 4: for target 1 the donors 2 and 3
# reach equally far, and the smaller request position wins
TIE = (b"{A,C}{G,T}{A}", b"{1,2,3}{4}{1,4}{2,3}{0}")

# the planted recombinant: 2 class columns per symbol, so symbol 32 starts word 1 and symbol 2048 starts column 4096
PLANTED_BREAKS = (32, CHUNK_COLUMNS // 2)
PLANTED_SYMBOLS = CHUNK_COLUMNS // 2 + 60


def planted_eds(rng):
    """paths 1, 2, 3 are the parents a, b, c; path 4 copies a up to the first break, b up to the second, c to the end;
    paths 5 and 6 take the first and the second string throughout, so that no string is without a path.  Every symbol is
    {A,C}; at a break the parent that ends differs from the one that begins, and at symbol 0 only a goes with the target"""
    n, (b1, b2) = PLANTED_SYMBOLS, PLANTED_BREAKS
    a = [rng.randrange(2) for _ in range(n)]
    b = [rng.randrange(2) for _ in range(n)]
    c = [rng.randrange(2) for _ in range(n)]
    b[0] = c[0] = 1 - a[0]
    b[b1] = 1 - a[b1]
    c[b1] = a[b1]
    c[b2] = 1 - b[b2]
    t = a[:b1] + b[b1:b2] + c[b2:]
    syms, sets = [], []
    for i in range(n):
        syms.append([b"A", b"C"])
        for v in (0, 1):
            sets.append({p + 1 for p, row in enumerate((a, b, c, t)) if row[i] == v} | {5 + v})
    return dc.render(syms, sets)


def shapes():
    """name -> (eds, seds, requests)"""
    rng = random.Random(15)
    wide = dc.wide_eds(rng)
    crowd = dc.wide_eds(rng, P=300, n_symbols=40)
    out = {
        "wide": wide + ([dict(targets=[1, 64, 65, 130], donors=list(range(1, D + 1))) for D in (1, 2, 63, 64, 65, 130)] +
                        [ALL, dict(targets=[130, 7, 7], donors=list(range(130, 0, -1)))],),
        "crowd": crowd + ([ALL, dict(targets=[1, 256, 257, 300], donors=list(range(300, 0, -1)) + [5, 5]),
                           dict(targets=[300], donors=list(range(1, 258)))],),
        "planted": planted_eds(rng) + ([dict(targets=[4], donors=[1, 2, 3]), dict(targets=[4], donors=[3, 2, 1, 2]), ALL,
                                        dict(targets=[4, 4, 1], donors=[6, 5, 4, 3, 2, 1])],),
        "tie": TIE + ([ALL, dict(targets=[1], donors=[3, 2, 4]), dict(targets=[1], donors=[2, 2, 3, 3])],),
        "fixed": ic.FIXED + ([ALL, dict(targets=[1], donors=[1]), dict(targets=[3, 3, 1], donors=[2]), dict(targets=[2])],),
        "edge": dc.EDGE + ([ALL, dict(targets=[66, 66, 1], donors=[1, 66, 2]), dict(targets=[67, 65, 66, 2, 1], donors=[66])],),
        "ends": ic.ENDS + ([ALL, dict(targets=[2, 1, 3, 1], donors=[3, 3, 1]), dict(targets=[2], donors=[2]),
                            dict(targets=[2], donors=[2, 2])],),
        "adjacent": ic.ADJACENT + ([ALL, dict(targets=[1], donors=[2, 1])],),
        "none": ic.NONE + ([ALL, dict(targets=[3], donors=[4, 1]), dict(donors=[4])],),
        "gaps": ic.GAPS + ([ALL, dict(targets=[4, 1], donors=[1, 2, 3]), dict(donors=[3, 3])],),
    }
    for c in (63, 64, 65, CHUNK_COLUMNS - 1, CHUNK_COLUMNS, CHUNK_COLUMNS + 1):
        e, s = ic.seam_eds(c, rng)
        out["columns%d" % c] = (e, s, [ALL, dict(targets=[1, 3], donors=[2, 3, 4, 1]), dict(targets=[5], donors=[1, 2])])
    return out
