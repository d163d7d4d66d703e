"""Measurement (not a test): linkage disequilibrium of msa2eds results of synthetic alignments, one session per shape.
Shapes: 64 rows x 10 Mb and 1000 rows x 1 Mb (rows x columns of the alignment; l = 0).  Per shape, window (100, 1000 choice
symbols) and threshold (min_r2 0 and 0.2): the info of the call, the device-event time of every kernel (edsx_set_timing)
and of the steps (edsx_paths_last_timing), the wall clock of the call, median [min, max] of the repetitions after a
warm-up; k_ld_pairs as pair-words per second - tiles x 4096 pairs x row words, per pass - next to the VALU bound DERIVED
from four vector instructions per pair-word (two v_and_b32, two v_bcnt_u32_b32 that add): 256 CUs x 4 SIMDs x 32 lanes per
cycle x 2.4 GHz / 4; and the share of the FILL pass in the two passes.  A call that would report more than MAX_PAIRS pairs
is refused by max_pairs behind its COUNT pass: its line says so and holds that pass alone.
Beside it what users do today, on a column prefix of the EDS cut with PathSession.slice so that both routes see the same
input: Context.eds_vcf, the genotypes parsed on the host, a numpy correlation over the same window of records and the same
threshold; against Context.eds_ld of the prefix, as a measured ratio of wall clocks.
Usage: python tests/measure_ld.py [reps] [prefix_columns] [shape ...]   with shape = ROWSxCOLUMNS (one JSON line per run)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_BOUND_PAIR_WORDS_PER_S = 256 * 4 * 32 * 2.4e9 / 4           # derived, not measured
MAX_PAIRS = 50_000_000                                           # 3.6 GB of pair records


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


def measure(ctx, s, shape, window, min_r2, reps):
    import edsparser_amd
    walls, kernels, steps, launches = [], [], [], {}
    info, refused = None, False
    for it in range(reps + 1):
        ctx.set_timing(True)                                     # (clears the accumulators)
        t0 = time.perf_counter()
        try:
            pairs, alleles, info = s.ld(None, window=window, min_r2=min_r2, max_pairs=MAX_PAIRS)
            del pairs, alleles
        except edsparser_amd.EdsxError as ex:
            if "above the limit" not in ex.message:
                raise
            info, refused = ex.info, True
        wall = (time.perf_counter() - t0) * 1e3
        got = ctx.get_timing()
        ctx.set_timing(False)
        if it:                                                   # the first one warms up
            walls.append(wall)
            kernels.append({n: ms for n, ms, _ in got if n.startswith("k_ld_") or n.startswith("scan_")})
            launches = {n: c for n, _, c in got}
            steps.append(s.timing)
    passes = launches.get("k_ld_pairs", 0)
    pair_words = info["tiles"] * 4096 * info["row_words"]
    pairs_ms = statistics.median([k.get("k_ld_pairs", 0.0) for k in kernels])
    out = {"shape": shape, "window": window, "min_r2": min_r2, "reps": reps, **info, "refused_by_max_pairs": refused,
           "kernel_ms": {n: mmm([k[n] for k in kernels]) for n in kernels[0]}, "k_ld_pairs_launches": passes,
           "scan_ms": mmm([t["scan_ms"] for t in steps]), "copy_ms": mmm([t["copy_ms"] for t in steps]),
           "download_ms": mmm([t["download_ms"] for t in steps]), "pair_words_per_pass": pair_words, "call_wall_ms": mmm(walls, 1)}
    if passes and pairs_ms > 0:
        # FILL runs only the tiles with a reported pair: the rate below takes both passes as full ones, a lower bound
        rate = pair_words * passes / (pairs_ms * 1e-3)
        out.update({"pair_words_per_s": float("%.4g" % rate), "valu_bound_pair_words_per_s_derived": VALU_BOUND_PAIR_WORDS_PER_S,
                    "fraction_of_derived_bound": round(rate / VALU_BOUND_PAIR_WORDS_PER_S, 4)})
    print(json.dumps(out), flush=True)
    return out


def fill_share(ctx, s, shape, window, min_r2, reps):
    """the FILL pass alone: a call refused behind COUNT (max_pairs = 1) against the whole call"""
    import edsparser_amd
    both, count = [], []
    for it in range(reps + 1):
        for limit, sink in ((MAX_PAIRS, both), (1, count)):
            ctx.set_timing(True)
            try:
                s.ld(None, window=window, min_r2=min_r2, max_pairs=limit)
            except edsparser_amd.EdsxError as ex:
                if "above the limit" not in ex.message:
                    raise
                if limit != 1:                                   # no FILL pass to measure at this shape
                    ctx.set_timing(False)
                    print(json.dumps({"shape": shape, "window": window, "min_r2": min_r2, "fill_share_of_both": None,
                                      "refused_by_max_pairs": True}), flush=True)
                    return
            ms = dict((n, t) for n, t, _ in ctx.get_timing()).get("k_ld_pairs", 0.0)
            ctx.set_timing(False)
            if it:
                sink.append(ms)
    b, c = statistics.median(both), statistics.median(count)
    print(json.dumps({"shape": shape, "window": window, "min_r2": min_r2, "k_ld_pairs_both_passes_ms": mmm(both),
                      "k_ld_pairs_count_pass_ms": mmm(count), "fill_share_of_both": round((b - c) / b, 4) if b else None}), flush=True)


def host_route(ctx, eds, seds, window, min_r2):
    """what users do today: eds2vcf, the genotype text parsed on the host, a numpy correlation over the window"""
    import numpy as np
    t0 = time.perf_counter()
    vcf, _, _ = ctx.eds_vcf(eds, seds)
    geno = []
    for line in vcf.split(b"\n"):
        if not line or line[:1] == b"#":
            continue
        f = line.split(b"\t")
        geno.append(([int(g.split(b"/")[0]) if g != b"." else -1 for g in f[9:]], f[4].count(b",") + 1))
    G = np.array([g for g, _ in geno], dtype=np.int16)           # records x paths
    rec, rows = [], []
    for r, (_, alts) in enumerate(geno):
        for j in range(1, alts + 1):
            x = (G[r] == j).astype(np.float64)
            c = x.sum()
            if 1 <= c <= len(x) - 1:                             # min_count 1
                rec.append(r); rows.append(x)
    rec = np.array(rec)
    X = np.array(rows)
    Z = X - X.mean(axis=1, keepdims=True)
    Z /= np.sqrt((Z * Z).sum(axis=1, keepdims=True))
    reported, near, step = 0, 0, 512
    for a0 in range(0, len(Z), step):
        a1 = min(len(Z), a0 + step)
        b1 = int(np.searchsorted(rec, rec[a1 - 1] + window, side="right"))
        C = (Z[a0:a1] @ Z[a0:b1].T) ** 2
        d = rec[None, a0:b1] - rec[a0:a1, None]
        band = (d >= 1) & (d <= window)
        reported += int((band & (C >= min_r2)).sum())
        near += int((band & (C >= min_r2 - 1e-9)).sum())         # (a pair at the threshold: the rounding of this route decides)
    return (time.perf_counter() - t0) * 1e3, len(geno), len(Z), reported, near


def baseline(ctx, s, shape, prefix_columns, window, min_r2):
    W = s.align_info()["n_columns"]
    cols = min(prefix_columns, W)
    e, q, reg = s.slice([0], [0], [cols])
    assert not reg["status"].any()
    today, records, alleles, reported, near = host_route(ctx, e, q, window, min_r2)
    t0 = time.perf_counter()
    pairs, al, info = ctx.eds_ld(e, q, window=window, min_r2=min_r2)
    ours = (time.perf_counter() - t0) * 1e3
    # (the host route standardises in floating point: a pair at the threshold may fall on either side of it)
    print(json.dumps({"shape": shape, "baseline": "Context.eds_vcf + genotype parse + numpy correlation", "prefix_columns": cols,
                      "of_columns": W, "window": window, "min_r2": min_r2, "records": records, "host_alleles": alleles,
                      "host_reported": reported, "host_reported_within_1e-9": near, "alleles": info["alleles"], "reported": info["pairs"],
                      "vcf_parse_and_numpy_wall_ms": round(today, 1), "eds_ld_wall_ms": round(ours, 1), "ratio": round(today / ours, 1)}),
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
            for window in (100, 1000):
                for min_r2 in (0.0, 0.2):
                    measure(ctx, s, shape, window, min_r2, reps)
                fill_share(ctx, s, shape, window, 0.2, reps)
            baseline(ctx, s, shape, prefix, 100, 0.2)


if __name__ == "__main__":
    main()
