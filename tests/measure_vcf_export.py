"""Measurement (not a test): the VCF export (edsx_eds_vcf) of BASELINE configs[1]'s EDS (msa2eds of 64 rows x 10 Mb,
ref_path = 1) and of a 100 Mbp genrandomeds EDS with sources (the first strings as the reference).  Per shape: the
device-event time of every kernel and scan (edsx_set_timing) and the wall clock of the whole call, median [min, max] of
the repetitions after a warm-up; the bytes the three emitters write (fixed parts and cells together are the body) and
their rates against the 8 TB/s HBM roofline.
Usage: python tests/measure_vcf_export.py [reps] [genrandomeds bp]   (one JSON line per shape)"""
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


def measure(ctx, name, eds, seds, reps, **kw):
    walls, kernels, info, sizes = [], [], None, None
    for it in range(reps + 1):
        ctx.set_timing(True)                                     # (clears the accumulators)
        t0 = time.perf_counter()
        vcf, fa, info = ctx.eds_vcf(eds, seds, **kw)
        wall = (time.perf_counter() - t0) * 1e3
        t = {n: ms for n, ms, _ in ctx.get_timing()}
        ctx.set_timing(False)
        sizes = (len(vcf), len(fa))
        del vcf, fa
        if it:                                                   # the first one warms up
            walls.append(wall)
            kernels.append(t)
    med = {k: _spread([r[k] for r in kernels]) for k in kernels[0]}
    dev = sum(v[0] for v in med.values())
    rate = lambda b, ms: round(b / (ms * 1e6), 1) if ms else None
    body_ms = med["k_vcf_fixed"][0] + med.get("k_vcf_cells", [0])[0]
    cells = info["records"] * info["paths"]
    print(json.dumps({
        "shape": name, "reps": reps, "info": info, "vcf_bytes": sizes[0], "fasta_bytes": sizes[1], "cells": cells,
        "body_bytes_per_cell": round(info["body_bytes"] / cells, 2) if cells else None,
        "kernel_ms_median_min_max": med, "kernels_total_ms": round(dev, 3),
        "body_gbps": rate(info["body_bytes"], body_ms), "body_of_roofline": round(rate(info["body_bytes"], body_ms) / ROOFLINE_GBPS, 4),
        "ref_gbps": rate(sizes[1], med["k_vcf_ref"][0]), "call_wall_ms": _spread(walls)}), flush=True)


def main():
    import torch
    import edsparser_amd
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    gen_bp = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    ctx = edsparser_amd.Context(0)
    S, L = 64, 10_000_000
    n = edsparser_amd.synth_size(S, L)
    buf = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    ctx.msa_synth_device(buf.data_ptr(), n, S, L)
    E, Q = ctx.msa_plan_device(buf.data_ptr(), n, 0)
    d_eds = torch.empty(E + 16, dtype=torch.uint8, device="cuda:0")
    d_seds = torch.empty(Q + 16, dtype=torch.uint8, device="cuda:0")
    ctx.msa_emit_device(d_eds.data_ptr(), d_seds.data_ptr())
    torch.cuda.synchronize()
    eds, seds = d_eds[:E].cpu().numpy().tobytes(), d_seds[:Q].cpu().numpy().tobytes()
    del buf, d_eds, d_seds
    measure(ctx, "configs[1] msa2eds output, 64 x 10 Mb, ref_path 1", eds, seds, reps, ref_path=1)
    eds, seds, _ = ctx.genrandomeds(gen_bp, seed=5)
    measure(ctx, "genrandomeds %d bp" % gen_bp, eds, seds, reps)


if __name__ == "__main__":
    main()
