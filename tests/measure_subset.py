"""Measurement (not a test): path subsetting on a 100 Mbp genrandomeds EDS with sources.  Subsets: half of the paths, one
path, all paths.  Per subset: the device-event time of every kernel (edsx_set_timing) and the wall clock of the whole
call, median of the repetitions after a warm-up; the bytes the subset kernels read at least (bitsets + characters) and
write (both texts) against the 8 TB/s HBM roofline; the tokeniser's share of the call (the call minus the subset kernels
and the download is upload + tokenising, which edsx_eds_stats on the same texts pays as well and is timed beside it).
Usage: python tests/measure_subset.py [reps] [genrandomeds bp]   (one JSON line per subset on stdout)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOFLINE_GBPS = 8000.0


def measure(ctx, name, eds, seds, K, reps, stats_ms):
    walls, kernels = [], []
    info = None
    for it in range(reps + 1):
        ctx.set_timing(True)                                     # (clears the accumulators)
        t0 = time.perf_counter()
        oe, os_, info = ctx.eds_subset(eds, seds, K)
        wall = (time.perf_counter() - t0) * 1e3
        t = {n: ms for n, ms, _ in ctx.get_timing()}
        ctx.set_timing(False)
        if it:                                                   # the first one warms up
            walls.append(wall)
            kernels.append(t)
        out_bytes = len(oe) + len(os_)
        del oe, os_
    med = {k: statistics.median(r[k] for r in kernels) for k in kernels[0]}
    dev = sum(med.values())
    W = info["paths_in"] // 64 + 1
    read = info["strings_in"] * W * 8 + info["chars_in"]
    print(json.dumps({
        "subset": name, "paths_in": info["paths_in"], "paths_out": info["paths_out"], "reps": reps,
        "symbols_in": info["symbols_in"], "symbols_out": info["symbols_out"], "strings_in": info["strings_in"],
        "strings_out": info["strings_out"], "chars_in": info["chars_in"], "chars_out": info["chars_out"],
        "kernel_ms": {k: round(v, 3) for k, v in med.items()}, "kernels_total_ms": round(dev, 3),
        "bytes_read_min": read, "bytes_written": out_bytes,
        "gbps_over_kernels": round((read + out_bytes) / (dev * 1e6), 1),
        "fraction_of_roofline": round((read + out_bytes) / (dev * 1e6) / ROOFLINE_GBPS, 4),
        "copy_gbps": round((info["chars_in"] + info["chars_out"]) / (med["k_sub_copy"] * 1e6), 1) if med.get("k_sub_copy") else None,
        "call_wall_ms": round(statistics.median(walls), 1), "call_wall_ms_min_max": [round(min(walls), 1), round(max(walls), 1)],
        "eds_stats_wall_ms": round(stats_ms, 1),
        "tokeniser_share": round(min(1.0, stats_ms / statistics.median(walls)), 3)}), flush=True)


def main():
    import edsparser_amd
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    bp = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    ctx = edsparser_amd.Context(0)
    eds, seds, _ = ctx.genrandomeds(bp, seed=5)
    with ctx.paths_open(eds, seds) as s:                          # (the statistics' num_paths counts id 0 as well)
        P = s.info["num_paths"]
    ts = []
    for _ in range(3):                                           # upload + tokenise + a few reductions: the tokeniser's cost
        t0 = time.perf_counter()
        ctx.eds_stats(eds, seds)
        ts.append((time.perf_counter() - t0) * 1e3)
    stats_ms = statistics.median(ts[1:])
    for name, K in (("half", list(range(1, P + 1, 2))), ("one", [1]), ("all", list(range(1, P + 1)))):
        measure(ctx, name, eds, seds, K, reps, stats_ms)


if __name__ == "__main__":
    main()
