"""Child program of tests/test_dist_guard_gpu.py: `python dist_guard_child.py dist` with EDSX_LIB=libedsx_guard.so.  The
boundary shapes of the path distances (tests/dist_cases.py, what tests/test_dist_gpu.py runs) through the guard library, as
tests/msa_export_guard_child.py runs the alignment export: a fresh context per fill byte, the result equal to the
specification's under every fill, no zone dirty after the call or after close.  k_dist_fill writes a unit's descriptors
behind its scanned offset, k_dist_rows one word per (path, 64 class columns), k_dist_pairs and k_dist_finish K x K sums: a
class count that disagrees with the fill, a row word past the last or a pair past K lands in a zone; a fill of 0xff reads
as a set bit wherever a padding bit or a sum was taken for zero without being written."""
import sys

from guard_child import EDS_FILLS, Guard                                  # (puts the repository and tests/ on sys.path)

import dist_cases as dc  # noqa: E402
import dist_spec as ds  # noqa: E402


def library(ctx, eds, seds, requests):
    out = []
    with ctx.paths_open(eds, seds) as s:
        for metric in ds.METRICS:
            for req in requests:
                D, miss, info = s.distances(req, metric)
                out.append((D.tolist(), miss.tolist(), info["units"]))
    return out


def spec(eds, seds, requests):
    return [ds.matrix(eds, seds, req, metric) for metric in ds.METRICS for req in requests]


def dist():
    g = Guard()
    shapes = dc.boundary_shapes()
    for name in sorted(shapes):
        eds, seds, requests = shapes[name]
        g.case(name, lambda ctx: library(ctx, eds, seds, requests), spec(eds, seds, requests), EDS_FILLS)
    g.finish("dist", len(shapes))


if __name__ == "__main__":
    {"dist": dist}[sys.argv[1]]()
