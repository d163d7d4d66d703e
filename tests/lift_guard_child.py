"""Child program of tests/test_lift_guard_gpu.py: `python lift_guard_child.py lift` with EDSX_LIB=libedsx_guard.so.  The
coordinate lift's boundary shapes (tests/test_lift_gpu.py) through the guard library, as tests/msa_export_guard_child.py
runs the alignment export: a fresh context per fill byte, the result equal to the specification's under every fill, no
zone dirty after the call or after close.  The lift's buffers are sized per query and per distinct path: a slot, a site
or a status one past the chunk lands in a zone, and a status or position nobody wrote shows under some fill (0x04 is
RANGE, 0x00 is SAME)."""
import os
import sys

from guard_child import EDS_FILLS, Guard                                  # (puts the repository and tests/ on sys.path)

import lift_spec as ls  # noqa: E402
from test_lift_gpu import SHAPES, all_queries, expected  # noqa: E402

LIFT_FILLS = EDS_FILLS + (0x04,)


def run(eds, seds, q, budget=None):
    def call(ctx):
        if budget is not None:
            os.environ["EDSX_PATHS_BUDGET"] = str(budget)
        try:
            with ctx.paths_open(eds, seds) as s:
                pos, st, sites = s.lift(*q, with_sites=True)
                sites2, st2 = s.lift_sites(q[0], q[1])
                ok = st2 == 0
                pos3, st3 = s.lift_place(sites2["symbol"][ok], sites2["string"][ok], sites2["offset"][ok], q[2][ok])
        finally:
            os.environ.pop("EDSX_PATHS_BUDGET", None)
        return pos.tobytes(), st.tobytes(), sites.tobytes(), sites2.tobytes(), pos3.tobytes(), st3.tobytes()
    return call


def want(m, q):
    pos, st, sites = expected(m, *q)
    ok = sites["symbol"] != sites["symbol"].dtype.type(ls.U64_MAX)
    return pos.tobytes(), st.tobytes(), sites.tobytes(), sites.tobytes(), pos[ok].tobytes(), st[ok].tobytes()


def lift():
    g = Guard()
    cases = 0
    for name, make in SHAPES:
        eds, seds = make()
        m = ls.Model(eds, seds)
        q = all_queries(m, extra=7)
        w = want(m, q)
        g.case(name, run(eds, seds, q), w, LIFT_FILLS)
        cases += 1
        if name in ("narrow 4097", "empty path", "zero widths 5"):        # tables of one path: src and dst in different batches
            g.case(name + ", one path per table", run(eds, seds, q, 1), w, LIFT_FILLS)
            cases += 1
    g.finish("lift", cases)


if __name__ == "__main__":
    {"lift": lift}[sys.argv[1]]()
