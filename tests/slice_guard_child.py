"""Child program of tests/test_slice_guard_gpu.py: `python slice_guard_child.py slice` with EDSX_LIB=libedsx_guard.so.  The
region slice's boundary shapes (tests/test_slice_gpu.py) through the guard library, as tests/lift_guard_child.py runs the
lift: a fresh context per fill byte, the result equal to the specification's under every fill, no zone dirty after the call
or after close.  Both texts are sized exactly from the counts and every string's place is worked out from scanned tables:
a brace, a comma, a 16-byte chunk or an id one past a region lands in the next region or in a zone, and a byte nobody
wrote shows under some fill (0x04 is RANGE, '}' and '0' are what the .seds kernel writes first)."""
import sys

from guard_child import EDS_FILLS, Guard                                  # (puts the repository and tests/ on sys.path)

import slice_spec as ss  # noqa: E402
from test_slice_gpu import SHAPES  # noqa: E402

SLICE_FILLS = EDS_FILLS + (0x04, ord("}"), ord("0"))


def run(eds, seds, regions):
    def call(ctx):
        with ctx.paths_open(eds, seds) as s:
            e, q, reg = s.slice(*regions)
        return (bytes(e), bytes(q), reg["status"].tobytes()) + tuple(reg[f].tobytes() for f in ss.FIELDS)
    return call


def want(eds, seds, regions):
    import numpy as np
    e, q, reg, st = ss.Model(eds, seds).slice(*[[int(x) for x in c] for c in regions])
    return (e, q, np.array(st, dtype=np.uint8).tobytes()) + tuple(np.array(reg[f], dtype=np.uint64).tobytes() for f in ss.FIELDS)


def slice_():
    g = Guard()
    cases = 0
    for name, make, _ in SHAPES:
        eds, seds, regions = make()
        g.case(name, run(eds, seds, regions), want(eds, seds, regions), SLICE_FILLS)
        cases += 1
    g.finish("slice", cases)


if __name__ == "__main__":
    {"slice": slice_}[sys.argv[1]]()
