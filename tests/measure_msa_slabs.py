"""Measurement (not a test): the host side of the column-slab stitch of msa2eds, in the style of the other measure_*.py.
A 64 x 16,000,000 alignment is generated on the device and downloaded once; then, through the public Python API only (so
that EDSX_LIB chooses the library under measurement),
    batched   Context.msa_transform_batched(host, l, 4)                  four column batches on one GPU
    ranks     MultiGpu([0] * 4, use_rccl=False).msa_transform(host, l)    four ranks sharing the GPU, in-process exchange
for l in (0, 8): two warm-up calls, then the median of seven with a host clock around the synchronous call.  The input
must be cut (batches used == 4, last_partition()[0]).
Usage: python tests/measure_msa_slabs.py [call ...]           one JSON line per call (batched_l0 batched_l8 ranks_l0 ranks_l8; default all):
                                                              median, min, max of the seven, SHA-256 of both outputs
       python tests/measure_msa_slabs.py compare A.jsonl B.jsonl
                                                              A: lines of the library to compare with, B: of the one under
                                                              test.  Per call: the outputs must be equal, and B's median must
                                                              not exceed A's by more than A's own spread (max - min of its
                                                              seven, what the host contributes to an unchanged program);
                                                              prints a table, exit status 1 if not"""
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CALLS = ("batched_l0", "batched_l8", "ranks_l0", "ranks_l8")
S, L, PARTS, WARMUP, REPS = 64, 16_000_000, 4, 2, 7


def measure(names):
    import torch
    import edsparser_amd
    ctx = edsparser_amd.Context(0)
    n = edsparser_amd.synth_size(S, L)
    buf = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    ctx.msa_synth_device(buf.data_ptr(), n, S, L)
    torch.cuda.synchronize()
    host = bytes(buf.cpu().numpy())
    del buf
    multi = None
    for name in names:
        kind, l = name.split("_l")
        l = int(l)
        if kind == "ranks" and multi is None:
            multi = edsparser_amd.MultiGpu([0] * PARTS, use_rccl=False)
        ms, digest = [], None
        for it in range(WARMUP + REPS):
            t0 = time.perf_counter()
            if kind == "batched":
                e, s, used = ctx.msa_transform_batched(host, l, PARTS)
            else:
                e, s = multi.msa_transform(host, l)
            t1 = time.perf_counter()
            assert (used == PARTS) if kind == "batched" else multi.last_partition()[0], name
            if it >= WARMUP:
                ms.append((t1 - t0) * 1e3)
            if digest is None:
                digest = [hashlib.sha256(e).hexdigest(), hashlib.sha256(s).hexdigest(), len(e), len(s)]
            del e, s
        print(json.dumps({"call": name, "lib": os.environ.get("EDSX_LIB", "libedsx.so"), "rows": S, "cols": L, "parts": PARTS,
                          "median_ms": round(statistics.median(ms), 2), "min_ms": round(min(ms), 2), "max_ms": round(max(ms), 2),
                          "eds_sha256": digest[0], "seds_sha256": digest[1], "eds_bytes": digest[2], "seds_bytes": digest[3]}),
              flush=True)


def compare(file_a, file_b):
    def read(path):
        return {r["call"]: r for r in (json.loads(ln) for ln in open(path) if ln.startswith("{"))}
    a, b = read(file_a), read(file_b)
    good = True
    print("%-11s %30s %30s %9s %7s" % ("call", "A median [min, max] ms", "B median [min, max] ms", "A spread", "verdict"))
    for name in CALLS:
        ra, rb = a[name], b[name]
        same = (ra["eds_sha256"], ra["seds_sha256"]) == (rb["eds_sha256"], rb["seds_sha256"])
        spread = ra["max_ms"] - ra["min_ms"]
        ok = same and rb["median_ms"] <= ra["median_ms"] + spread
        good = good and ok
        print("%-11s %30s %30s %9.2f %7s" % (name, "%.2f [%.2f, %.2f]" % (ra["median_ms"], ra["min_ms"], ra["max_ms"]),
                                            "%.2f [%.2f, %.2f]" % (rb["median_ms"], rb["min_ms"], rb["max_ms"]), spread,
                                            "ok" if ok else ("slower" if same else "OUTPUT DIFFERS")))
    return 0 if good else 1


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    measure(sys.argv[1:] or CALLS)
