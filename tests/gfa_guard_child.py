"""Child program of tests/test_gfa_guard_gpu.py: `python gfa_guard_child.py gfa` with EDSX_LIB=libedsx_guard.so.  The GFA
export's hand-written cases and boundary shapes (tests/test_gfa_gpu.py) through the guard library, as tests/guard_child.py
runs the other entry points: a fresh context per fill byte, the result equal to the specification's under every fill, no
zone dirty after the call or after close.  The emitters store aligned 16-byte chunks: a chunk past the end of a section,
or in front of the text, lands in a zone."""
import os
import random
import sys

from guard_child import EDS_FILLS, Guard                                  # (puts the repository and tests/ on sys.path)

import gfa_spec as gs  # noqa: E402
import path_spec as ps  # noqa: E402
from test_gfa_cpu import open_run_eds  # noqa: E402
from test_gfa_gpu import BLOCK, GFA_TILE, HAND, SCAN_TILE, _text  # noqa: E402
from test_subset_cpu import random_eds  # noqa: E402

GFA_FILLS = EDS_FILLS + (ord("\t"), ord("+"))


def _graph(g, name, eds):
    want = gs.graph(eds)

    def call(ctx):
        text, info = ctx.eds_gfa_graph(eds)
        return text, {k: info[k] for k in gs.INFO_KEYS}
    g.case(name, call, want, GFA_FILLS)


def _walks(g, name, eds, seds, paths=None):
    want = (gs.gfa(eds, seds)[0],) + gs.walks(eds, seds, paths)

    def call(ctx):
        whole = ctx.eds_gfa(eds, seds)[0]
        with ctx.paths_open(eds, seds) as s:
            lines, miss, steps = s.gfa_walks(paths)
        return whole, lines, [int(x) for x in miss], [int(x) for x in steps]
    g.case(name, call, want, GFA_FILLS)


def gfa():
    g = Guard()
    for name, eds, _ in HAND:
        _graph(g, "hand " + name, eds)
    _walks(g, "hand walks", b"{A}{C}{G,T}", b"{0}{1}{1}{2}")
    _walks(g, "hand empty walk", b"{,A}{C,}", b"{1}{2}{2}{1}")
    for M in (9, 10, 99, 100, 999, 1000, 9999, 10_000):
        rng = random.Random(M)
        _graph(g, "segments %d" % M, _text([[rng.choice("ACGT").encode()] + ([b""] if k % 3 == 1 else []) for k in range(M)]))
    for n in (1, BLOCK - 1, BLOCK, BLOCK + 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1):
        _walks(g, "symbols %d" % n, *open_run_eds(random.Random(n), P=3, n=n))
    for end in (GFA_TILE - 1, GFA_TILE, GFA_TILE + 1):
        _graph(g, "S lines end at %d" % end, b"{" + b"A" * (end - len(gs.HEADER) - 5 - 6) + b"}{C}{G,T}")
    rng = random.Random(300)
    word = lambda lo, hi: bytes(rng.choice(b"ACGT") for _ in range(rng.randint(lo, hi)))
    _graph(g, "300 x 300", _text([[b"ACGT"], [word(1, 4) for _ in range(300)], [word(1, 4) for _ in range(300)], [b"T"]]))
    run = [[b"", word(1, 1), word(2, 2)] for _ in range(64)]
    for where, syms in (("middle", [[b"AC"]] + run + [[b"GT"]]), ("start", run + [[b"GT"]]), ("end", [[b"AC"]] + run)):
        sets = []
        for s in syms:
            sets += [{0}] if len(s) == 1 else [{1}, {2}, {3}]
        _walks(g, "64 open symbols at the " + where, *_text(syms, sets))
    _graph(g, "100 000 characters", b"{AC}{" + word(100_000, 100_000) + b",G}{T}")
    for lead in range(16):
        syms = [[word(lead, lead)], [word(15, 15), word(16, 16), word(17, 17)], [word(17, 17), word(16, 16), word(15, 15)],
                [word(33, 33), b"", word(16, 16)]]
        _graph(g, "pool residue %d" % lead, _text(syms))
    for P in (63, 64, 65, 129):
        eds, seds = random_eds(random.Random(P), P=P, n=40)
        _walks(g, "P = %d" % P, eds, seds)
        _walks(g, "P = %d, four of them" % P, eds, seds, [P, 1, P // 2, P])
    # three table batches, P lines of several stretches
    rng = random.Random(6000)
    syms = [[rng.choice("AC").encode(), rng.choice("GT").encode() * 2] if k % 4 else [b"ACGT"] for k in range(8000)]
    sets = []
    for s in syms:
        if len(s) == 1:
            sets.append({0})
        else:
            a = set(rng.sample(range(1, 6), rng.randint(1, 4)))
            sets += [a, set(range(1, 6)) - a]
    eds, seds = _text(syms, sets)
    os.environ["EDSX_PATHS_BUDGET"] = str(2 * (24 * 6000 + 64) + 100)
    try:
        _walks(g, "three table batches", eds, seds)
    finally:
        del os.environ["EDSX_PATHS_BUDGET"]
    g.finish("gfa", 55)


if __name__ == "__main__":
    {"gfa": gfa}[sys.argv[1]]()
