"""Child program of tests/test_ibs_guard_gpu.py: `python ibs_guard_child.py ibs` with EDSX_LIB=libedsx_guard.so.  The
boundary shapes of the shared segments (tests/ibs_cases.py, what tests/test_ibs_gpu.py runs) through the guard library, as
tests/dist_guard_child.py runs the distances: a fresh context per fill byte, the result equal to the specification's under
every fill, no zone dirty after the call or after close.  k_ibs_scan writes three words per (pair, chunk) and, in its FILL
pass, records behind the scanned offset less the chunk's count; k_ibs_stitch writes chunks + 1 counts per pair, the seam
records and pair_off: a pair index past the last, a count that disagrees with the fill or a record past the total lands in
a zone; a fill of 0xff shows as a wrong count or rank wherever a slot was taken for written without being so."""
import sys

from guard_child import EDS_FILLS, Guard                                  # (puts the repository and tests/ on sys.path)

import ibs_cases as ic  # noqa: E402
import ibs_spec as isp  # noqa: E402


def library(ctx, eds, seds, requests):
    out = []
    with ctx.paths_open(eds, seds) as s:
        for kw in requests:
            segs, off, info = s.ibs(**kw)
            out.append(([tuple(r) for r in segs.tolist()], off.tolist(), info["candidate_segments"]))
    return out


def spec(eds, seds, requests):
    out = []
    for kw in requests:
        w = isp.ibs(eds, seds, **kw)
        out.append((w["segments"], w["pair_off"], w["info"]["candidate_segments"]))
    return out


def ibs():
    g = Guard()
    shapes = ic.boundary_shapes()
    for name in sorted(shapes):
        eds, seds, requests = shapes[name]
        g.case(name, lambda ctx: library(ctx, eds, seds, requests), spec(eds, seds, requests), EDS_FILLS)
    g.finish("ibs", len(shapes))


if __name__ == "__main__":
    {"ibs": ibs}[sys.argv[1]]()
