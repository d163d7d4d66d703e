"""Measurement (not a test): the GFA export of a 100 Mbp genrandomeds EDS with sources (P = 4).  The graph call: the
device-event time of every kernel and scan (edsx_set_timing) and the wall clock of the whole call, median of the
repetitions after a warm-up; per emitter the bytes it writes and its rate against the 8 TB/s HBM roofline; the tokeniser's
share of the call (edsx_eds_stats on the same text pays upload + tokenising as well and is timed beside it) and the
download's (the call minus the kernels minus that).  The walks of all paths on a session: the device events of
edsx_paths_last_timing (choose, both scans, the walk kernel), the download on the host clock, bytes written and rate.
Usage: python tests/measure_gfa.py [reps] [genrandomeds bp]   (one JSON line for the graph, one for the walks)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOFLINE_GBPS = 8000.0


def _spread(xs):
    return [round(statistics.median(xs), 3), round(min(xs), 3), round(max(xs), 3)]


def graph(ctx, eds, reps, stats_ms):
    walls, kernels, info = [], [], None
    for it in range(reps + 1):
        ctx.set_timing(True)                                     # (clears the accumulators)
        t0 = time.perf_counter()
        text, info = ctx.eds_gfa_graph(eds)
        wall = (time.perf_counter() - t0) * 1e3
        t = {n: ms for n, ms, _ in ctx.get_timing()}
        ctx.set_timing(False)
        if it:                                                   # the first one warms up
            walls.append(wall)
            kernels.append(t)
        del text
    med = {k: _spread([r[k] for r in kernels]) for k in kernels[0]}
    dev = sum(v[0] for v in med.values())
    wall = statistics.median(walls)
    rate = lambda b, ms: round(b / (ms * 1e6), 1) if ms else None
    s_ms, l_ms = med["k_gfa_segments"][0], med["k_gfa_links"][0]
    print(json.dumps({
        "what": "graph", "reps": reps, "info": info, "kernel_ms_median_min_max": med, "kernels_total_ms": round(dev, 3),
        "segments_gbps": rate(info["segment_bytes"], s_ms), "segments_of_roofline": round(rate(info["segment_bytes"], s_ms) / ROOFLINE_GBPS, 4),
        "links_gbps": rate(info["link_bytes"], l_ms), "links_of_roofline": round(rate(info["link_bytes"], l_ms) / ROOFLINE_GBPS, 4),
        "call_wall_ms": _spread(walls), "eds_stats_wall_ms": round(stats_ms, 1),
        "tokeniser_share": round(min(1.0, stats_ms / wall), 3),
        "download_share": round(max(0.0, wall - dev - stats_ms) / wall, 3)}), flush=True)


def walks(ctx, eds, seds, reps):
    with ctx.paths_open(eds, seds) as s:
        rows, size, steps = [], 0, None
        for it in range(reps + 1):
            t0 = time.perf_counter()
            lines, miss, steps = s.gfa_walks()
            wall = (time.perf_counter() - t0) * 1e3
            size = len(lines)
            del lines
            if it:
                rows.append(dict(s.timing, wall_ms=wall))
        med = {k: _spread([r[k] for r in rows]) for k in ("choose_ms", "scan_ms", "copy_ms", "download_ms", "wall_ms")}
        print(json.dumps({
            "what": "walks", "reps": reps, "paths": int(s.info["num_paths"]), "n_choice_symbols": int(s.info["n_choice_symbols"]),
            "steps": [int(x) for x in steps], "bytes_written": size, "ms_median_min_max": med,
            "walk_gbps": round(size / (med["copy_ms"][0] * 1e6), 1),
            "walk_of_roofline": round(size / (med["copy_ms"][0] * 1e6) / ROOFLINE_GBPS, 4),
            "download_share": round(med["download_ms"][0] / med["wall_ms"][0], 3)}), flush=True)


def main():
    import edsparser_amd
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    bp = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    ctx = edsparser_amd.Context(0)
    eds, seds, _ = ctx.genrandomeds(bp, seed=5)
    ts = []
    for _ in range(3):                                           # upload + tokenise + a few reductions: the tokeniser's cost
        t0 = time.perf_counter()
        ctx.eds_stats(eds)
        ts.append((time.perf_counter() - t0) * 1e3)
    graph(ctx, eds, reps, statistics.median(ts[1:]))
    walks(ctx, eds, seds, reps)


if __name__ == "__main__":
    main()
