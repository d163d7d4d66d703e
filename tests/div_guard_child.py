"""Child program of tests/test_div_guard_gpu.py: `python div_guard_child.py div` with EDSX_LIB=libedsx_guard.so.  The boundary
shapes of the diversity (tests/div_cases.py, what tests/test_div_gpu.py runs) through the guard library, as
tests/ld_guard_child.py runs the linkage disequilibrium: a fresh context per fill byte, the result equal to the
specification's under every fill, no zone dirty after the call or after close.  k_div_sites writes NA numbers per choice
symbol with a stride of nc + 1 and, above 128 row words, a walk row per lane group; k_div_windows reads two prefixes per
record at ranks up to nc: an array, a row or a record past its end lands in a zone; a fill of 0xff shows wherever entry nc
of an array, a spectrum bin or a walk row was taken for zero without being written."""
import sys

from guard_child import EDS_FILLS, Guard                                  # (puts the repository and tests/ on sys.path)

import div_cases as dc  # noqa: E402
import div_spec as ds  # noqa: E402


def library(ctx, eds, seds, requests):
    out = []
    with ctx.paths_open(eds, seds) as s:
        for kw in requests:
            windows, groups, pairs, sfs, info = s.diversity(**kw)
            out.append(([tuple(w) for w in windows.tolist()], [[tuple(x) for x in row] for row in groups.tolist()],
                        [[tuple(x) for x in row] for row in pairs.tolist()], [v.tolist() for v in sfs] if sfs is not None else None, info))
    return out


def spec(eds, seds, requests):
    out = []
    for kw in requests:
        w = ds.diversity(eds, seds, **kw)
        out.append((w["windows"], w["groups"], w["pairs"], w["sfs"], w["info"]))
    return out


def div():
    g = Guard()
    shapes = dc.boundary_shapes()
    for name in sorted(shapes):
        eds, seds, requests = shapes[name]
        g.case(name, lambda ctx: library(ctx, eds, seds, requests), spec(eds, seds, requests), EDS_FILLS)
    g.finish("div", len(shapes))


if __name__ == "__main__":
    {"div": div}[sys.argv[1]]()
