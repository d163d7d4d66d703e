"""Child program of tests/test_mosaic_guard_gpu.py: `python mosaic_guard_child.py mosaic` with EDSX_LIB=libedsx_guard.so.
The shapes of the mosaics (tests/mosaic_cases.py, what tests/test_mosaic_gpu.py runs) through the guard library, as
tests/ibs_guard_child.py runs the shared segments: a fresh context per fill byte, the result equal to the specification's
under every fill, no zone dirty after the call or after close.  k_mosaic_donors writes D words per class word; k_mosaic
writes a lane's alive words 256 apart per target, one count per target and, in its FILL pass, records behind the scanned
offset: a donor past the last, an alive word past the last target's or a record past the total lands in a zone; a fill of
0xff shows as donors nobody listed wherever an alive word was taken for written without being so."""
import sys

from guard_child import EDS_FILLS, Guard                                  # (puts the repository and tests/ on sys.path)

import mosaic_cases as mc  # noqa: E402
import mosaic_spec as msp  # noqa: E402


def library(ctx, eds, seds, requests):
    out = []
    with ctx.paths_open(eds, seds) as s:
        for kw in requests:
            segs, off, info = s.mosaic(**kw)
            out.append(([tuple(r) for r in segs.tolist()], off.tolist(), info["private_symbols"]))
    return out


def spec(eds, seds, requests):
    out = []
    for kw in requests:
        w = msp.mosaic(eds, seds, **kw)
        out.append((w["segments"], w["target_off"], w["info"]["private_symbols"]))
    return out


def mosaic():
    g = Guard()
    shapes = mc.shapes()
    for name in sorted(shapes):
        eds, seds, requests = shapes[name]
        g.case(name, lambda ctx: library(ctx, eds, seds, requests), spec(eds, seds, requests), EDS_FILLS)
    g.finish("mosaic", len(shapes))


if __name__ == "__main__":
    {"mosaic": mosaic}[sys.argv[1]]()
