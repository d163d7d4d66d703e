"""Measurement (not a test): pairwise path distances of msa2eds results of synthetic alignments, one session per shape.
Shapes: 64 rows x 10 Mb and 1000 rows x 1 Mb (rows x columns of the alignment; l = 0).  Per shape and metric: C, V and the
chunk geometry, the device-event time of every kernel (edsx_set_timing) and of the three steps (edsx_paths_last_timing),
the wall clock of the call, median [min, max] of the repetitions after a warm-up; k_dist_pairs as pair-words per second -
(tiles of 64 x 64 pairs with tile row <= tile column) x 4096 pairs x words per row - next to the VALU bound DERIVED from
four vector instructions per pair-word (two v_and_b32, two v_bcnt_u32_b32 that add): 256 CUs x 4 SIMDs x 32 lanes per
cycle x 2.4 GHz / 4.  Beside it what users do today at the same shape: PathSession.align and a numpy Hamming loop over
the rows, on the first `base_rows` paths only (the loop is quadratic in the rows and linear in the columns), against
distances() of the same paths, as a measured ratio of wall clocks.
Usage: python tests/measure_dist.py [reps] [base_rows] [shape ...]   with shape = ROWSxCOLUMNS (one JSON line per shape and metric)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_BOUND_PAIR_WORDS_PER_S = 256 * 4 * 32 * 2.4e9 / 4           # derived, not measured


def mmm(xs, nd=3):
    return [round(statistics.median(xs), nd), round(min(xs), nd), round(max(xs), nd)]


def synthetic_eds(ctx, rows, cols):
    import torch
    import edsparser_amd
    n = edsparser_amd.synth_size(rows, cols)
    buf = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    ctx.msa_synth_device(buf.data_ptr(), n, rows, cols)
    torch.cuda.synchronize()
    msa = buf.cpu().numpy()
    del buf
    return ctx.msa_transform(msa, 0)


def measure(ctx, s, shape, metric, reps):
    walls, kernels, steps = [], [], []
    for it in range(reps + 1):
        ctx.set_timing(True)                                     # (clears the accumulators)
        t0 = time.perf_counter()
        D, miss, info = s.distances(None, metric)
        wall = (time.perf_counter() - t0) * 1e3
        k = {n: ms for n, ms, _ in ctx.get_timing() if n.startswith("k_dist_") or n == "scan_classes"}
        ctx.set_timing(False)
        if it:                                                   # the first one warms up and makes the class list
            walls.append(wall)
            kernels.append(k)
            steps.append(s.timing)
        else:
            first = dict(k)
    K = len(D)
    tiles = (K + 63) // 64
    words = (info["class_columns"] + 63) // 64
    pair_words = tiles * (tiles + 1) // 2 * 4096 * words
    pairs_ms = statistics.median([k["k_dist_pairs"] for k in kernels])
    rate = pair_words / (pairs_ms * 1e-3)
    print(json.dumps({
        "shape": shape, "metric": metric, "paths": K, "reps": reps, **info,
        "class_list_ms_first_call": {n: round(first.get(n, 0.0), 3) for n in ("k_dist_count", "scan_classes", "k_dist_fill")},
        "kernel_ms": {n: mmm([k[n] for k in kernels]) for n in kernels[0]},
        "choose_ms": mmm([t["choose_ms"] for t in steps]), "scan_ms": mmm([t["scan_ms"] for t in steps]),
        "copy_ms": mmm([t["copy_ms"] for t in steps]), "download_ms": mmm([t["download_ms"] for t in steps]),
        "pair_words": pair_words, "pair_words_per_s": float("%.4g" % rate),
        "valu_bound_pair_words_per_s_derived": VALU_BOUND_PAIR_WORDS_PER_S,
        "fraction_of_derived_bound": round(rate / VALU_BOUND_PAIR_WORDS_PER_S, 4),
        "distinct_pairs_differing": int((D > 0).sum() // 2), "call_wall_ms": mmm(walls, 1)}), flush=True)


def baseline(s, shape, base_rows):
    """what users do today: the alignment rows, then a Hamming loop on the host"""
    import numpy as np
    K = min(base_rows, s.info["num_paths"])
    ids = list(range(1, K + 1))
    t0 = time.perf_counter()
    text, _ = s.align(ids, 0, gap="-", as_numpy=True)
    W = s.align_info()["n_columns"]
    rec = len(text) // K                                         # the names differ in length: find every row by its header
    rows, at = [], 0
    for k in range(K):
        at = at + int(np.argmax(text[at:at + 64] == 10)) + 1
        rows.append(text[at:at + W])
        at += W + 1
    H = np.zeros((K, K), dtype=np.uint64)
    for a in range(K):
        for b in range(a + 1, K):
            H[a, b] = H[b, a] = np.count_nonzero(rows[a] != rows[b])
    today = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    D = s.distances(ids, "columns")[0]
    ours = (time.perf_counter() - t0) * 1e3
    assert rec and (D == H).all()                                # (no path of an msa2eds result lacks a string: the gap is "no character")
    print(json.dumps({"shape": shape, "baseline": "PathSession.align + numpy Hamming loop", "paths": K, "columns": W,
                      "align_and_loop_wall_ms": round(today, 1), "distances_wall_ms": round(ours, 1),
                      "ratio": round(today / ours, 1)}), flush=True)


def main():
    import edsparser_amd
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    base_rows = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    shapes = [tuple(int(x) for x in a.split("x")) for a in sys.argv[3:]] or [(64, 10_000_000), (1000, 1_000_000)]
    ctx = edsparser_amd.Context(0)
    for rows, cols in shapes:
        shape = "%d rows x %d columns" % (rows, cols)
        eds, seds = synthetic_eds(ctx, rows, cols)
        with ctx.paths_open(eds, seds) as s:
            i = s.info
            print(json.dumps({"shape": shape, "symbols": i["n_symbols"], "choice_symbols": i["n_choice_symbols"], "strings": i["n_strings"],
                              "paths": i["num_paths"], "eds_bytes": len(eds), "tokenise_ms": round(s.timing["tokenise_ms"], 1)}), flush=True)
            del eds, seds
            for metric in ("columns", "strings"):
                measure(ctx, s, shape, metric, reps)
            baseline(s, shape, base_rows)


if __name__ == "__main__":
    main()
