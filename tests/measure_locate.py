"""Measure the pattern search on the GPU (not a test): edsx_eds_locate on a genrandomeds EDS of 100 Mbp with 1 000 and
10 000 patterns of lengths 16 and 32 sampled from it (edsx_eds_genpatterns).

Per configuration, median of 5 timed runs after one warm-up: the device-event time of the locate kernels and scans
(kernel_ms of edsx_query_last_info), character-pattern pairs per second, the HBM read rate that implies (every chunk of
64 patterns reads the character pool once: pool bytes x chunks / kernel time, against the 8 TB/s roofline), the whole
call with the tokeniser's share, and the returned common-start hits through edsx_eds_check_positions (all true).

    python tests/measure_locate.py [--mbp 100] [--runs 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK = 64                                                   # LCHUNK of csrc/locate_device.hip
ROOFLINE = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=int, default=100)
    ap.add_argument("--counts", default="1000,10000")
    ap.add_argument("--lengths", default="16,32")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import edsparser_amd
    ctx = edsparser_amd.Context(0)
    eds, _, sites = ctx.genrandomeds(a.mbp * 1_000_000, seed=21)
    res = {"eds_bytes": len(eds), "sites": sites, "runs": a.runs, "configs": []}
    for count in (int(x) for x in a.counts.split(",")):
        for length in (int(x) for x in a.lengths.split(",")):
            pats = ctx.eds_genpatterns(eds, count, length, 7).split(b"\n")[:-1]
            out = ctx.eds_locate(eds, pats, max_hits=4096)               # warm-up
            kern, wall, tok = [], [], []
            for _ in range(a.runs):
                t0 = time.perf_counter()
                out = ctx.eds_locate(eds, pats, max_hits=4096)
                wall.append((time.perf_counter() - t0) * 1e3)
                info = ctx.query_last_info()
                kern.append(info["kernel_ms"])
                tok.append(info["tokenise_ms"])
            hit_off, hits, choice_off, choices, totals, flags = out
            k = statistics.median(kern) / 1e3
            chunks = (count + CHUNK - 1) // CHUNK
            c = {"patterns": count, "length": length, "n_chars": int(info["n_chars"]), "hits": int(hit_off[-1]),
                 "flagged_patterns": int((flags != 0).sum()), "kernel_ms_median": k * 1e3, "kernel_ms_all": kern,
                 "pairs_per_s": int(info["n_chars"]) * count / k,
                 "implied_hbm_read_GB_per_s": int(info["n_chars"]) * chunks / k / 1e9,
                 "call_ms_median": statistics.median(wall), "tokenise_ms_median": statistics.median(tok)}
            c["implied_hbm_share_of_roofline"] = c["implied_hbm_read_GB_per_s"] * 1e9 / ROOFLINE
            common = np.flatnonzero(hits["common_pos"] != np.uint64(2 ** 64 - 1))
            owner = np.repeat(np.arange(count), np.diff(hit_off).astype(np.int64))[common]
            klen = np.diff(choice_off).astype(np.int64)
            coff = np.zeros(len(common) + 1, dtype=np.uint64)
            coff[1:] = np.cumsum(klen[common])
            keep = np.repeat(hits["common_pos"] != np.uint64(2 ** 64 - 1), klen)
            st = ctx.eds_check_positions(eds, hits["common_pos"][common], coff, choices[keep],
                                         np.arange(len(common) + 1, dtype=np.uint64) * np.uint64(length),
                                         b"".join(pats[q] for q in owner))
            c["checked"] = int(len(common))
            c["check_all_true"] = bool((st == 1).all())
            res["configs"].append(c)
            print(json.dumps(c), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
