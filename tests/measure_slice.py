"""Measurement (not a test): region slices of a 100 Mbp genrandomeds EDS with sources, one session.  Shapes: one region
of a whole path; 20 000 regions of 5 kb; 10^6 regions of 100 bp (random paths and starts).  Per shape: the device-event
time of every kernel (edsx_set_timing) and of the two steps (edsx_paths_last_timing), the wall clock of the whole call,
median [min, max] of the repetitions after a warm-up; the bytes the kernels read at least (the kept characters, the
bitsets of the slices' strings and 24 bytes of the scanned tables per string) and write (both texts) against the 8 TB/s
HBM roofline.
Usage: python tests/measure_slice.py [reps] [genrandomeds bp]   (one JSON line per shape on stdout)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOFLINE_GBPS = 8000.0


def mmm(xs, nd=3):
    return [round(statistics.median(xs), nd), round(min(xs), nd), round(max(xs), nd)]


def measure(ctx, s, name, path, start, end, reps, W):
    walls, kernels, steps = [], [], []
    for it in range(reps + 1):
        ctx.set_timing(True)                                     # (clears the accumulators)
        t0 = time.perf_counter()
        e, q, reg = s.slice(path, start, end)
        wall = (time.perf_counter() - t0) * 1e3
        k = {n: ms for n, ms, _ in ctx.get_timing()}
        ctx.set_timing(False)
        t = s.timing
        if it:                                                   # the first one warms up
            walls.append(wall)
            kernels.append(k)
            steps.append(t)
        written = len(e) + len(q)
        del e, q
    ok = reg["status"] == 0
    strings, chars = int(reg["strings"][ok].sum()), int(reg["chars"][ok].sum())
    read = chars + strings * (8 * W + 24)
    fill = [t["copy_ms"] for t in steps]
    dev = [t["copy_ms"] + t["scan_ms"] + t["choose_ms"] for t in steps]
    copy = [k.get("k_slice_copy", 0.0) for k in kernels]
    print(json.dumps({
        "shape": name, "regions": len(path), "regions_ok": int(ok.sum()), "reps": reps, "strings": strings, "chars": chars,
        "kernel_ms": {n: mmm([k[n] for k in kernels]) for n in kernels[0]},
        "resolve_count_scan_ms": mmm([t["scan_ms"] + t["choose_ms"] for t in steps]), "fill_ms": mmm(fill), "device_ms": mmm(dev),
        "download_ms": mmm([t["download_ms"] for t in steps]),
        "bytes_read_min": read, "bytes_written": written,
        "fill_gbps": round((read + written) / (statistics.median(fill) * 1e6), 1),
        "fill_fraction_of_roofline": round((read + written) / (statistics.median(fill) * 1e6) / ROOFLINE_GBPS, 4),
        "copy_gbps": round(2 * chars / (statistics.median(copy) * 1e6), 1) if statistics.median(copy) else None,
        "call_wall_ms": mmm(walls, 1)}), flush=True)


def main():
    import numpy as np
    import edsparser_amd
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    bp = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    ctx = edsparser_amd.Context(0)
    eds, seds, _ = ctx.genrandomeds(bp, seed=5)
    rng = np.random.default_rng(1)
    with ctx.paths_open(eds, seds) as s:
        info = s.info
        P, W = info["num_paths"], info["num_paths"] // 64 + 1
        lens = s.lengths()[0].astype(np.int64)
        print(json.dumps({"bp": bp, "symbols": info["n_symbols"], "strings": info["n_strings"], "chars": info["n_chars"], "paths": P,
                          "tokenise_ms": round(s.timing["tokenise_ms"], 1)}), flush=True)
        measure(ctx, s, "one region of a whole path", [1], [0], [int(lens[0])], reps, W)
        for name, n, w in (("20 000 regions of 5 kb", 20_000, 5_000), ("10^6 regions of 100 bp", 1_000_000, 100)):
            path = rng.integers(1, P + 1, n)
            start = (rng.random(n) * (lens[path - 1] - w)).astype(np.int64)
            measure(ctx, s, name, path, start, start + w, reps, W)


if __name__ == "__main__":
    main()
