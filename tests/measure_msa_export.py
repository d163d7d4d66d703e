"""Measurement (not a test): the alignment export on BASELINE configs[1]'s EDS (64 paths x 10 Mb) and on a 100 Mbp
genrandomeds EDS, in the style of tests/measure_paths.py.  Per shape: the device times of edsx_paths_last_timing for
PathSession.align over several repetitions after a warm-up (median and spread), k_path_align's rate bytes_written /
copy_ms, and beside it - on the same session in the same run, the repetitions taken in turn - the same figures of
PathSession.spell (k_path_copy), the yardstick: the same pool and the same tables written at the same store width.
Usage: python tests/measure_msa_export.py [reps] [genrandomeds bp]   (one JSON line per shape on stdout)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _summary(rows, nbytes):
    copy = [r["copy_ms"] for r in rows]
    rate = [nbytes / (c * 1e6) for c in copy]
    med = {k: statistics.median(r[k] for r in rows) for k in rows[0]}
    return {"bytes": nbytes, "choose_ms": round(med["choose_ms"], 3), "scan_ms": round(med["scan_ms"], 3),
            "copy_ms": round(med["copy_ms"], 3), "copy_ms_min_max": [round(min(copy), 3), round(max(copy), 3)],
            "download_ms": round(med["download_ms"], 2), "gbps": round(statistics.median(rate), 1),
            "gbps_min_max": [round(min(rate), 1), round(max(rate), 1)]}


def measure(ctx, name, eds, seds, reps, line_width=60):
    s = ctx.paths_open(eds, seds)
    info, ainfo = s.info, s.align_info()
    al, sp = [], []
    for it in range(reps + 1):                                   # the first round warms up; align and spell in turn
        a, _ = s.align(None, line_width, as_numpy=True)
        ta, na = s.timing, len(a)
        del a
        f, _ = s.spell(None, line_width, as_numpy=True)
        ts, nf = s.timing, len(f)
        del f
        if it:
            al.append(ta)
            sp.append(ts)
    s.close()
    A, F = _summary(al, na), _summary(sp, nf)
    print(json.dumps({"shape": name, "paths": info["num_paths"], "n_symbols": info["n_symbols"],
                      "n_choice_symbols": info["n_choice_symbols"], "n_chars": info["n_chars"], "n_columns": ainfo["n_columns"],
                      "widest_symbol": ainfo["widest_symbol"], "line_width": line_width, "reps": reps, "align": A, "spell": F,
                      "align_over_spell_gbps": round(A["gbps"] / F["gbps"], 3)}), flush=True)


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
    measure(ctx, "configs[1] msa2eds output, 64 x 10 Mb", eds, seds, reps)
    eds, seds, _ = ctx.genrandomeds(gen_bp, seed=5)
    measure(ctx, "genrandomeds %d bp" % gen_bp, eds, seds, reps)


if __name__ == "__main__":
    main()
