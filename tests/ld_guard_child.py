"""Child program of tests/test_ld_guard_gpu.py: `python ld_guard_child.py ld` with EDSX_LIB=libedsx_guard.so.  The boundary
shapes of the linkage disequilibrium (tests/ld_cases.py, what tests/test_ld_gpu.py runs) through the guard library, as
tests/dist_guard_child.py runs the path distances: a fresh context per fill byte, the result equal to the specification's
under every fill, no zone dirty after the call or after close.  Every buffer of the feature is sized from scanned counts:
k_ld_rows writes an allele's row behind afirst, k_ld_pairs one counter per (allele, column tile) behind tstart and one
pair behind its scanned counter: a count that disagrees with the fill, a row past A or a pair past the last lands in a zone;
a fill of 0xff reads as a carrier wherever a padding bit, a counter or a mask was taken for zero without being written."""
import struct
import sys

from guard_child import EDS_FILLS, Guard                                  # (puts the repository and tests/ on sys.path)

import ld_cases as lc  # noqa: E402
import ld_spec as ls  # noqa: E402

INFO = ("paths", "choice_symbols", "alleles", "candidate_pairs", "undefined_pairs", "pairs")


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def library(ctx, eds, seds, requests):
    out = []
    with ctx.paths_open(eds, seds) as s:
        for kw in requests:
            for t in (0.0, 0.3):
                pairs, alleles, info = s.ld(min_r2=t, **kw)
                out.append(([tuple(p)[:8] + (_bits(p[8]),) for p in pairs.tolist()], [tuple(a) for a in alleles.tolist()],
                            [info[k] for k in INFO]))
    return out


def spec(eds, seds, requests):
    out = []
    for kw in requests:
        for t in (0.0, 0.3):
            w = ls.ld(eds, seds, min_r2=t, **kw)
            out.append(([p[:8] + (_bits(p[8]),) for p in w["pairs"]], w["alleles"], [w["info"][k] for k in INFO]))
    return out


def ld():
    g = Guard()
    shapes = lc.boundary_shapes()
    for name in sorted(shapes):
        eds, seds, requests = shapes[name]
        g.case(name, lambda ctx: library(ctx, eds, seds, requests), spec(eds, seds, requests), EDS_FILLS)
    g.finish("ld", len(shapes))


if __name__ == "__main__":
    {"ld": ld}[sys.argv[1]]()
