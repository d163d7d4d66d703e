"""Measurement (not a test): path spelling on BASELINE configs[1]'s EDS (64 paths x 10 Mb) and on a 100 Mbp genrandomeds
EDS.  Per shape: the device times of edsx_paths_last_timing over several repetitions after a warm-up (median and
spread), the copy kernel's rate bytes_written / copy_ms, beside it - in the same run - the rate of a hipMemsetAsync of
bytes_written bytes as the write ceiling of the box, and the time EDS::path_sequence takes for the same paths on the CPU.
Usage: python tests/measure_paths.py [reps] [genrandomeds bp]   (one JSON line per shape on stdout)"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _hip_runtime():
    """The HIP runtime this process has already mapped (torch's), not a second copy."""
    import ctypes
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime mapped")


def memset_rate(torch, nbytes, reps):
    """GB/s of hipMemsetAsync over nbytes on the stream the events are recorded on, median and spread over reps."""
    import ctypes
    hip = _hip_runtime()
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    rates = []
    for it in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = hip.hipMemsetAsync(buf.data_ptr(), 0, nbytes, stream)
        assert rc == 0, rc
        b.record()
        torch.cuda.synchronize()
        if it:                                                   # the first one warms up
            rates.append(nbytes / (a.elapsed_time(b) * 1e6))
    del buf
    return statistics.median(rates), min(rates), max(rates)


def cpu_path_sequence_ms(eds, seds):
    """Milliseconds EDS::path_sequence takes for all paths (the container is loaded first, outside the clock)."""
    exe = os.path.join(ROOT, "edsparser_amd", "host", "build", "measure_path_sequence")
    src = os.path.join(tempfile.gettempdir(), "measure_path_sequence.cpp")
    open(src, "w").write(
        '#include "edsparser/formats/eds.hpp"\n#include <chrono>\n#include <cstdio>\n'
        "int main(int, char** argv) { auto e = edsparser::EDS::load(argv[1], argv[2]);\n"
        "  auto t0 = std::chrono::steady_clock::now(); size_t total = 0;\n"
        "  for (int p = 1; p <= e.max_path_id(); p++) total += e.path_sequence(p).size();\n"
        '  std::printf("%.3f %zu\\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), total);\n'
        "  return 0; }\n")
    lib = os.path.join(ROOT, "edsparser_amd")
    subprocess.run(["make", "-s", "-C", os.path.join(lib, "host")], check=True)
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, os.path.join(lib, "host", "build", "libedsparser_lib.a"),
                    "-L", lib, "-ledsx", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "x.eds"), "wb").write(eds)
        open(os.path.join(d, "x.seds"), "wb").write(seds)
        out = subprocess.run([exe, os.path.join(d, "x.eds"), os.path.join(d, "x.seds")], capture_output=True, text=True, check=True).stdout
    return float(out.split()[0])


def measure(ctx, torch, name, eds, seds, reps, with_cpu=True):
    t0 = time.perf_counter()
    s = ctx.paths_open(eds, seds)
    open_ms = (time.perf_counter() - t0) * 1e3
    info = s.info
    rows = []
    for it in range(reps + 1):
        fa, miss = s.spell(None, 60, as_numpy=True)
        if it:
            rows.append(s.timing)
        nbytes = len(fa)
        del fa
    s.close()
    med = {k: statistics.median(r[k] for r in rows) for k in rows[0]}
    copy = [r["copy_ms"] for r in rows]
    rate = [nbytes / (c * 1e6) for c in copy]
    ms_med, ms_lo, ms_hi = memset_rate(torch, nbytes, reps)
    out = {"shape": name, "paths": info["num_paths"], "n_symbols": info["n_symbols"], "n_choice_symbols": info["n_choice_symbols"],
           "n_chars": info["n_chars"], "fasta_bytes": nbytes, "open_wall_ms": round(open_ms, 2), "reps": reps,
           "choose_ms": round(med["choose_ms"], 3), "scan_ms": round(med["scan_ms"], 3), "copy_ms": round(med["copy_ms"], 3),
           "copy_ms_min_max": [round(min(copy), 3), round(max(copy), 3)], "download_ms": round(med["download_ms"], 2),
           "copy_gbps": round(statistics.median(rate), 1), "copy_gbps_min_max": [round(min(rate), 1), round(max(rate), 1)],
           "memset_gbps": round(ms_med, 1), "memset_gbps_min_max": [round(ms_lo, 1), round(ms_hi, 1)],
           "copy_over_memset": round(statistics.median(rate) / ms_med, 3)}
    if with_cpu:
        out["cpu_path_sequence_ms"] = round(cpu_path_sequence_ms(eds, seds), 1)
    print(json.dumps(out), flush=True)


def main():
    import torch
    import edsparser_amd
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
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
    measure(ctx, torch, "configs[1] msa2eds output, 64 x 10 Mb", eds, seds, reps)
    eds, seds, _ = ctx.genrandomeds(gen_bp, seed=5)
    measure(ctx, torch, "genrandomeds %d bp" % gen_bp, eds, seds, reps)


if __name__ == "__main__":
    main()
