"""Measurement (not a test): the shared segments of msa2eds results of synthetic alignments, one session per shape.
Shapes: 64 rows x 10 Mb and 1000 rows x 1 Mb (rows x columns of the alignment; l = 0), as tests/measure_dist.py.  Per shape:
C and the chunk geometry, pairs, candidate and reported segments, the device-event time of every kernel (edsx_set_timing)
and of the steps (edsx_paths_last_timing) and the wall clock of the call, median [min, max] of the repetitions after a
warm-up; k_ibs_scan (COUNT and FILL together) as xor pair-words per second - (tiles of 64 x 64 pairs with tile row <= tile
column) x 4096 pairs x words per row x 2 passes.  A shape whose rows, scratch or records do not fit the budget is reported
with the library's text instead.  Beside it what users do today at the same shape: PathSession.align and a numpy
run-length pass per pair over the rows, on the first `base_rows` paths only (quadratic in the rows, linear in the columns),
against ibs() of the same paths with thresholds 0, 0, as a measured ratio of wall clocks; the number of maximal equal runs
of columns is not the number of segments (a symbol may span several columns), so only the covered columns are compared.
Usage: python tests/measure_ibs.py [reps] [base_rows] [min_sites] [shape ...]   with shape = ROWSxCOLUMNS (JSON lines)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from measure_dist import mmm, synthetic_eds  # noqa: E402


def measure(ctx, s, shape, min_sites, reps):
    import edsparser_amd
    walls, kernels, steps = [], [], []
    for it in range(reps + 1):
        ctx.set_timing(True)                                     # (clears the accumulators)
        t0 = time.perf_counter()
        try:
            segs, off, info = s.ibs(None, min_sites, 0)
        except edsparser_amd.EdsxError as ex:
            ctx.set_timing(False)
            print(json.dumps({"shape": shape, "min_sites": min_sites, "does_not_fit": ex.message, **getattr(ex, "info", {})}), flush=True)
            return
        wall = (time.perf_counter() - t0) * 1e3
        k = {n: ms for n, ms, _ in ctx.get_timing() if n.startswith("k_ibs_") or n in ("scan_segments", "k_dist_rows", "k_path_choose")}
        ctx.set_timing(False)
        if it:                                                   # the first one warms up and makes the class list
            walls.append(wall)
            kernels.append(k)
            steps.append(s.timing)
    tiles = (info["paths"] + 63) // 64
    words = (info["class_columns"] + 63) // 64
    pair_words = tiles * (tiles + 1) // 2 * 4096 * words * 2
    scan_ms = statistics.median([k["k_ibs_scan"] for k in kernels])
    print(json.dumps({
        "shape": shape, "min_sites": min_sites, "reps": reps, **info,
        "kernel_ms": {n: mmm([k[n] for k in kernels]) for n in kernels[0]},
        "choose_ms": mmm([t["choose_ms"] for t in steps]), "scan_ms": mmm([t["scan_ms"] for t in steps]),
        "copy_ms": mmm([t["copy_ms"] for t in steps]), "download_ms": mmm([t["download_ms"] for t in steps]),
        "scan_pair_words_both_passes": pair_words, "scan_pair_words_per_s": float("%.4g" % (pair_words / (scan_ms * 1e-3))),
        "record_bytes": int(segs.nbytes), "call_wall_ms": mmm(walls, 1)}), flush=True)


def baseline(s, shape, base_rows):
    """what users do today: the alignment rows, then a run-length pass per pair on the host"""
    import numpy as np
    import edsparser_amd
    K = min(base_rows, s.info["num_paths"])
    ids = list(range(1, K + 1))
    t0 = time.perf_counter()
    text, _ = s.align(ids, 0, gap="-", as_numpy=True)
    W = s.align_info()["n_columns"]
    rows, at = [], 0
    for k in range(K):
        at = at + int(np.argmax(text[at:at + 64] == 10)) + 1
        rows.append(text[at:at + W])
        at += W + 1
    covered = runs = 0
    for a in range(K):
        for b in range(a + 1, K):
            eq = np.concatenate(([False], rows[a] == rows[b], [False]))
            edge = np.flatnonzero(eq[1:] != eq[:-1])             # starts and ends of the equal runs, alternating
            runs += len(edge) // 2
            covered += int((edge[1::2] - edge[0::2]).sum())
    today = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    try:
        segs = s.ibs(ids, 0, 0)[0]
    except edsparser_amd.EdsxError as ex:
        print(json.dumps({"shape": shape, "baseline_does_not_fit": ex.message}), flush=True)
        return
    ours = (time.perf_counter() - t0) * 1e3
    # a symbol at which two paths differ may still hold equal columns: the segments cover no more than the equal runs
    ours_cov = int((segs["column_end"] - segs["column_first"]).sum())
    assert ours_cov <= covered
    print(json.dumps({"shape": shape, "baseline": "PathSession.align + numpy run-length pass per pair", "paths": K, "columns": W,
                      "equal_runs": runs, "equal_columns": covered, "segments": len(segs), "segment_columns": ours_cov,
                      "align_and_loop_wall_ms": round(today, 1), "ibs_wall_ms": round(ours, 1), "ratio": round(today / ours, 1)}), flush=True)


def main():
    import edsparser_amd
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    base_rows = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    min_sites = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    shapes = [tuple(int(x) for x in a.split("x")) for a in sys.argv[4:]] or [(64, 10_000_000), (1000, 1_000_000)]
    ctx = edsparser_amd.Context(0)
    for rows, cols in shapes:
        shape = "%d rows x %d columns" % (rows, cols)
        eds, seds = synthetic_eds(ctx, rows, cols)
        with ctx.paths_open(eds, seds) as s:
            i = s.info
            print(json.dumps({"shape": shape, "symbols": i["n_symbols"], "choice_symbols": i["n_choice_symbols"], "strings": i["n_strings"],
                              "paths": i["num_paths"], "eds_bytes": len(eds), "tokenise_ms": round(s.timing["tokenise_ms"], 1)}), flush=True)
            del eds, seds
            measure(ctx, s, shape, min_sites, reps)
            baseline(s, shape, base_rows)


if __name__ == "__main__":
    main()
