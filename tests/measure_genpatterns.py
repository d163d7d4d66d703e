"""Measure the query kernels on the GPU (not a test): 10**7 patterns of length 32 sampled from a genrandomeds EDS of
about 1 GB (edsx_eds_genpatterns), the checking of their 10**7 witnesses (edsx_eds_check_positions), and the
container's seeded EDS::generate_patterns on the same EDS for comparison.

Every call tokenises its .eds text again (DeviceEds::load); the kernel times below are device events around
k_pat_sample / k_pat_check only, on tables already in HBM.  Median of 5 timed runs after one warm-up.

    python tests/measure_genpatterns.py [--mb 1000] [--count 10000000] [--host-count 100000] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HOST = os.path.join(ROOT, "edsparser_amd", "host")
BUILD = os.path.join(HOST, "build")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1000)
    ap.add_argument("--count", type=int, default=10_000_000)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--host-count", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default=None, help="directory for the container run's files (default: a temporary one)")
    a = ap.parse_args()
    import edsparser_amd
    ctx = edsparser_amd.Context(0)
    eds, _, sites = ctx.genrandomeds(a.mb * 1_000_000, seed=21)
    res = {"eds_bytes": len(eds), "sites": sites, "count": a.count, "length": a.length}

    ctx.eds_genpatterns(eds, a.count, a.length, 0)                           # warm-up
    samp, wall = [], []
    for r in range(a.runs + 1):                                               # the extra last run keeps witnesses
        witness = r == a.runs
        t0 = time.perf_counter()
        out = ctx.eds_genpatterns(eds, a.count, a.length, 1 + r, witness=witness)
        info = ctx.query_last_info()
        if not witness:
            wall.append((time.perf_counter() - t0) * 1e3)
            samp.append(info["kernel_ms"])
    text, pos, off, deg = out
    res["n_symbols"], res["n_strings"] = int(info["n_symbols"]), int(info["n_strings"])
    res["tokenise_ms"], res["tables_ms"] = info["tokenise_ms"], info["tables_ms"]
    res["sample_kernel_ms_median"] = statistics.median(samp)
    res["sample_kernel_ms_all"] = samp
    res["sample_call_ms_median"] = statistics.median(wall)
    res["witness_sample_kernel_ms"] = info["kernel_ms"]
    res["patterns_per_s_kernel"] = a.count / (res["sample_kernel_ms_median"] / 1e3)
    res["output_GB_per_s_kernel"] = a.count * (a.length + 1) / (res["sample_kernel_ms_median"] / 1e3) / 1e9

    keep = np.nonzero(pos != np.uint64(2**64 - 1))[0]
    arr = np.frombuffer(text, dtype=np.uint8).reshape(-1, a.length + 1)[keep, :a.length].tobytes()
    coff = np.append(off[keep], off[-1]).astype(np.uint64)
    poff = np.arange(len(keep) + 1, dtype=np.uint64) * np.uint64(a.length)
    p = pos[keep]
    st = ctx.eds_check_positions(eds, p, coff, deg, poff, arr)                 # warm-up
    chk = []
    for _ in range(a.runs):
        st = ctx.eds_check_positions(eds, p, coff, deg, poff, arr)
        chk.append(ctx.query_last_info()["kernel_ms"])
    res["checked"] = int(len(keep))
    res["check_all_true"] = bool((st == 1).all())
    res["check_kernel_ms_median"] = statistics.median(chk)
    res["checks_per_s_kernel"] = len(keep) / (res["check_kernel_ms_median"] / 1e3)

    # the container (host twin of the sampler) on the same EDS
    exe = os.path.join(BUILD, "test_query")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_query.cpp"),
                    os.path.join(BUILD, "libedsparser_lib.a"), "-L", os.path.join(ROOT, "edsparser_amd"), "-ledsx",
                    "-Wl,-rpath," + os.path.join(ROOT, "edsparser_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
        ef, cf, of = os.path.join(tmp, "m.eds"), os.path.join(tmp, "m.cmd"), os.path.join(tmp, "m.txt")
        with open(ef, "wb") as f:
            f.write(eds)
        with open(cf, "w") as f:
            f.write("W\t%s\t%d\t%d\t%d\t%s\n" % (ef, a.host_count, a.length, 5, of))
        t0 = time.perf_counter()
        r = subprocess.run([exe, cf], capture_output=True, text=True)
        res["host_load_and_sample_s"] = time.perf_counter() - t0
        assert r.stdout.strip() == "ok", r.stdout + r.stderr
        res["host_sample_s"] = float(r.stderr.split("sample_s ")[1].split()[0])     # EDS::generate_patterns alone
        res["host_patterns"] = a.host_count
        res["host_patterns_per_s"] = a.host_count / res["host_sample_s"]
        with open(of, "rb") as f:
            res["host_equals_device"] = ctx.eds_genpatterns(eds, a.host_count, a.length, 5) == f.read()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
