"""Measurement (not a test): windowed diversity of msa2eds results of synthetic alignments, one session per shape.
Shapes: 64 rows x 10 Mb and 1000 rows x 1 Mb (rows x columns of the alignment; l = 0).  Per shape and G = 1, 2 and 8 equal
groups, windows of 1000 choice symbols every 500: the info of the call, the device-event time of every kernel
(edsx_set_timing) and of the steps (edsx_paths_last_timing), the wall clock of the call, median [min, max] of the
repetitions after a warm-up; k_div_sites as bytes of source-set rows per second next to the 8 TB/s HBM roofline.  The byte
count is DERIVED, not counted: the strings of the choice symbols (all strings less one per fixed symbol) x row words x 8
bytes, once per launch of the kernel (one launch up to 4 groups, three at 8).
Beside it what users do today, on a column prefix of the EDS cut with PathSession.slice so that both routes see the same
input: Context.eds_vcf, the genotypes parsed on the host, a numpy pi / d_xy per window of records; against
Context.eds_diversity of the prefix, as a measured ratio of wall clocks.
Usage: python tests/measure_div.py [reps] [prefix_columns] [shape ...]   with shape = ROWSxCOLUMNS (one JSON line per run)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from measure_ld import mmm, synthetic_eds  # noqa: E402

HBM_BYTES_PER_S = 8e12                                           # the roofline, not measured
WINDOW, STEP = 1000, 500


def equal_groups(P, G):
    return None if G == 1 else [list(range(1 + P * g // G, 1 + P * (g + 1) // G)) for g in range(G)]


def measure(ctx, s, shape, G, reps):
    i = s.info
    groups = equal_groups(i["num_paths"], G)
    walls, kernels, steps, launches, info = [], [], [], {}, None
    for it in range(reps + 1):
        ctx.set_timing(True)                                     # (clears the accumulators)
        t0 = time.perf_counter()
        *_, info = s.diversity(groups=groups, size=WINDOW, step=STEP, sfs=True)
        wall = (time.perf_counter() - t0) * 1e3
        got = ctx.get_timing()
        ctx.set_timing(False)
        if it:                                                   # the first one warms up
            walls.append(wall)
            kernels.append({n: ms for n, ms, _ in got if n.startswith("k_div_") or n == "scan_div"})
            launches = {n: c for n, _, c in got}
            steps.append(s.timing)
    strings = i["n_strings"] - (i["n_symbols"] - i["n_choice_symbols"])
    row_bytes = strings * info["row_words"] * 8 * launches.get("k_div_sites", 0)
    sites_ms = statistics.median([k.get("k_div_sites", 0.0) for k in kernels])
    out = {"shape": shape, "G": G, "window": WINDOW, "step": STEP, "reps": reps, **info, "kernel_ms": {n: mmm([k[n] for k in kernels]) for n in kernels[0]},
           "k_div_sites_launches": launches.get("k_div_sites", 0), "scan_ms": mmm([t["scan_ms"] for t in steps]),
           "copy_ms": mmm([t["copy_ms"] for t in steps]), "download_ms": mmm([t["download_ms"] for t in steps]),
           "source_row_bytes_derived": row_bytes, "call_wall_ms": mmm(walls, 1)}
    if sites_ms > 0:
        rate = row_bytes / (sites_ms * 1e-3)
        out.update({"source_row_bytes_per_s_derived": float("%.4g" % rate), "fraction_of_8TBps_roofline": round(rate / HBM_BYTES_PER_S, 4)})
    print(json.dumps(out), flush=True)


def host_route(ctx, eds, seds, groups):
    """what users do today: eds2vcf, the genotype text parsed on the host, numpy pi / d_xy per window of records"""
    import numpy as np
    t0 = time.perf_counter()
    vcf, _, _ = ctx.eds_vcf(eds, seds)
    geno = []
    for line in vcf.split(b"\n"):
        if not line or line[:1] == b"#":
            continue
        f = line.split(b"\t")
        geno.append([int(g.split(b"/")[0]) if g != b"." else -1 for g in f[9:]])
    Gm = np.array(geno, dtype=np.int16)                          # records x paths
    members = [np.array(g) - 1 for g in groups]
    total = 0
    for a0 in range(0, len(Gm), STEP):
        block = Gm[a0:a0 + WINDOW]
        for x, gx in enumerate(members):
            for gy in members[x:]:
                a, b = block[:, gx], block[:, gy]
                both = (a[:, :, None] >= 0) & (b[:, None, :] >= 0)
                total += int((both & (a[:, :, None] != b[:, None, :])).sum())
    return (time.perf_counter() - t0) * 1e3, len(geno), total


def baseline(ctx, s, shape, prefix_columns, G):
    W = s.align_info()["n_columns"]
    cols = min(prefix_columns, W)
    e, q, reg = s.slice([0], [0], [cols])
    assert not reg["status"].any()
    groups = equal_groups(s.info["num_paths"], G) or [list(range(1, s.info["num_paths"] + 1))]
    today, records, _ = host_route(ctx, e, q, groups)
    t0 = time.perf_counter()
    *_, info = ctx.eds_diversity(e, q, groups=groups, size=WINDOW, step=STEP)
    ours = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"shape": shape, "baseline": "Context.eds_vcf + genotype parse + numpy pi / d_xy per window", "G": G, "prefix_columns": cols,
                      "of_columns": W, "records": records, "choice_symbols": info["choice_symbols"], "windows": info["windows"],
                      "vcf_parse_and_numpy_wall_ms": round(today, 1), "eds_diversity_wall_ms": round(ours, 1), "ratio": round(today / ours, 1)}),
          flush=True)


def main():
    import edsparser_amd
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    prefix = int(sys.argv[2]) if len(sys.argv) > 2 else 200_000
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
            for G in (1, 2, 8):
                measure(ctx, s, shape, G, reps)
            baseline(ctx, s, shape, prefix, 2)


if __name__ == "__main__":
    main()
