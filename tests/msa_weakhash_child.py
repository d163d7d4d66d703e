"""Child program of tests/test_msa_weakhash_gpu.py: `python msa_weakhash_child.py <family>` with
EDSX_LIB=libedsx_weakhash.so (csrc/msa_device.hip with -DEDSX_MSA_HASH_BITS=1: one bit of every hash of the grouping's
hash-then-compare sites, csrc/msa_wave.hpp).  A family is one of tests/msa_collision_cases.py or one of the seeded
generators of tests/msa_cases.py.  run_family() is also what the parent runs on the product library in its own context,
so the two sides differ in the library alone.

Every case is one stderr marker line (in front of the EDSX_COUNTS line the library prints for it) and two transforms,
l = 0 and l = L_POS, compared byte for byte with the oracle; the route is checked through msa_info()["n_slow_segments"]."""
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import msa_collision_cases as mc  # noqa: E402
import oracle_lib as o  # noqa: E402

GENERATORS = ("wide", "wide_nul", "campaign")
WEAK = "libedsx_weakhash.so"


def _first_difference(got, want):
    n = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return "sizes %d / %d, first difference at %d: got %r, want %r" % (len(got), len(want), n, got[max(0, n - 30):n + 30],
                                                                    want[max(0, n - 30):n + 30])


def _compare(name, got, want):
    for what, g, w in zip((".eds", ".seds"), got, want):
        assert g == w, "%s: %s differs from the oracle: %s" % (name, what, _first_difference(g, w))


def run_family(ctx, family, log=sys.stderr):
    """-> (cases, transforms)"""
    runs = 0
    for c in mc.cases(family):
        m = c.build()
        for l in (0, mc.L_POS):
            log.write("weakhash-case %s l=%d rows=%d slow=%d heavy=%d\n" % (c.id, l, c.S, c.n_slow(l), c.n_heavy(l)))
            log.flush()
            got = ctx.msa_transform(m, l)
            _compare("%s l=%d" % (c.id, l), got, o.msa(m, l))
            slow = ctx.msa_info()["n_slow_segments"]
            assert slow == c.n_slow(l), "%s l=%d: %d segments went to the generic kernels, the geometry says %d" % (c.id, l, slow, c.n_slow(l))
            runs += 1
    return len(mc.cases(family)), runs


def generator_inputs(name):
    """[(description, alignment, l)] - sized so that a run of all of them stays within a few seconds"""
    from msa_cases import campaign_msa, wide_msa
    out = []
    if name in ("wide", "wide_nul"):
        rng = random.Random(20 if name == "wide" else 21)
        for it in range(48):
            m = wide_msa(rng, nul=name == "wide_nul")
            out.append(("%s %d" % (name, it), m, (0, rng.choice([1, 4, 12]))[it % 2]))
    else:
        rng = random.Random(3)
        for it in range(48):
            m, desc = campaign_msa(rng, max_cells=200_000)
            out.append(("campaign %d %r" % (it, desc), m, (0, rng.choice([1, 2, 5, 9, 33]))[it % 2]))
    return out


def run_generator(ctx, name):
    import edsparser_amd
    runs = 0
    for desc, m, l in generator_inputs(name):
        try:
            want = o.msa(m, l)
        except o.OracleError as ex:
            want = ("ERR", str(ex))
        try:
            got = ctx.msa_transform(m, l)
        except edsparser_amd.EdsxError as ex:
            got = ("ERR", ex.message)
        if want[0] == "ERR" or got[0] == "ERR":
            assert (want[0] == "ERR") == (got[0] == "ERR"), (desc, l, got[:2] if got[0] == "ERR" else "text", want[:2] if want[0] == "ERR" else "text")
        else:
            _compare("%s l=%d" % (desc, l), got, want)
        runs += 1
    return runs, runs


def main(name):
    import edsparser_amd
    edsparser_amd.load_library()
    assert os.path.basename(edsparser_amd._capi.lib_path()) == WEAK, edsparser_amd._capi.lib_path()
    t0 = time.time()
    ctx = edsparser_amd.Context(0)
    try:
        cases, runs = run_generator(ctx, name) if name in GENERATORS else run_family(ctx, name)
    finally:
        ctx.close()
    print("weakhash %s: cases %d runs %d seconds %.1f" % (name, cases, runs, time.time() - t0))


if __name__ == "__main__":
    main(sys.argv[1])
