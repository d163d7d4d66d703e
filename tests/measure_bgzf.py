"""Measure compressed input on the GPU (not a test): BASELINE configs[3] (edsx_genvcf: 1 Gb reference, 10^7 records, 8
samples; --scale 0.1 for a tenth), both files written once as level-6 BGZF by tests/bgzf_spec.py.

Per repetition, after one warm-up:
  k_bgzf_inflate / k_bgzf_crc   device events around the kernels (edsx_gz_last_info), GB/s of text produced
  H2D                           host clock around a synchronous torch copy of the compressed bytes from pageable memory (the
                                same sizes; two synchronisations included - not the library's own hipMemcpyAsync, which
                                is inside the transform_z figure)
  edsx_vcf_transform_z          host clock around the whole call, both inputs BGZF
  (a) edsx_vcf_transform        on the plain texts alone
  (b) zlib + (a)                single-thread zlib inflate of both files, block by block, then (a)

Median [min, max] of --runs repetitions; one JSON line.  The files are compressed by Python's zlib block by block before
the first measurement: about a quarter of a minute at --scale 0.1, two to three minutes at full size (1.7 GB at level 6).

    python tests/measure_bgzf.py [--scale 1.0] [--runs 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def mmm(xs):
    return [round(statistics.median(xs), 3), round(min(xs), 3), round(max(xs), 3)]


def zlib_inflate_blocks(data):
    out, off = [], 0
    while off < len(data):
        xlen = struct.unpack_from("<H", data, off + 10)[0]
        size = struct.unpack_from("<H", data, off + 16)[0] + 1
        out.append(zlib.decompress(data[off + 12 + xlen:off + size - 8], -15))
        off += size
    return b"".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bgzf_spec as bz
    import edsparser_amd
    ctx = edsparser_amd.Context(0)
    V, F = ctx.genvcf(int(1_000_000_000 * a.scale), int(10_000_000 * a.scale), 8, 42)
    t0 = time.perf_counter()
    zv, tv = bz.write(V, a.level)
    zf, tf = bz.write(F, a.level)
    res = {"scale": a.scale, "level": a.level, "runs": a.runs, "vcf_bytes": len(V), "fasta_bytes": len(F), "vcf_bgzf_bytes": len(zv),
           "fasta_bgzf_bytes": len(zf), "blocks": len(tv) + len(tf), "compress_s": round(time.perf_counter() - t0, 1)}
    text = len(V) + len(F)
    rows = {k: [] for k in ("inflate_ms", "crc_ms", "index_ms", "h2d_ms", "transform_z_ms", "plain_ms", "zlib_ms")}
    dev = torch.empty(max(len(zv), len(zf)) + 64, dtype=torch.uint8, device="cuda:0")
    hv, hf = torch.frombuffer(bytearray(zv), dtype=torch.uint8), torch.frombuffer(bytearray(zf), dtype=torch.uint8)
    for r in range(a.runs + 1):
        t0 = time.perf_counter()
        got = ctx.vcf_transform(zv, zf, compressed=True)
        t_z = time.perf_counter() - t0
        i0, i1 = ctx.gz_last_info(0), ctx.gz_last_info(1)
        assert i0["inflated_on_device"] == 1 and i1["inflated_on_device"] == 1
        t0 = time.perf_counter()
        plain = ctx.vcf_transform(V, F)
        t_p = time.perf_counter() - t0
        assert got == plain
        t0 = time.perf_counter()
        assert len(zlib_inflate_blocks(zv)) == len(V) and len(zlib_inflate_blocks(zf)) == len(F)
        t_zlib = time.perf_counter() - t0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev[:len(zv)].copy_(hv); torch.cuda.synchronize()
        dev[:len(zf)].copy_(hf); torch.cuda.synchronize()
        t_h2d = time.perf_counter() - t0
        if r == 0:
            continue
        rows["inflate_ms"].append(i0["inflate_ms"] + i1["inflate_ms"])
        rows["crc_ms"].append(i0["crc_ms"] + i1["crc_ms"])
        rows["index_ms"].append(i0["index_ms"] + i1["index_ms"])
        rows["h2d_ms"].append(t_h2d * 1e3)
        rows["transform_z_ms"].append(t_z * 1e3)
        rows["plain_ms"].append(t_p * 1e3)
        rows["zlib_ms"].append(t_zlib * 1e3)
    for k, v in rows.items():
        res[k] = mmm(v)
    res["zlib_plus_plain_ms"] = mmm([x + y for x, y in zip(rows["zlib_ms"], rows["plain_ms"])])
    res["inflate_GB_per_s_of_text"] = round(text / (statistics.median(rows["inflate_ms"]) * 1e6), 2)
    res["crc_GB_per_s_of_text"] = round(text / (statistics.median(rows["crc_ms"]) * 1e6), 2)
    res["text_d2h_bytes"] = [i0["text_d2h_bytes"], i1["text_d2h_bytes"]]
    res["z_over_plain"] = round(res["transform_z_ms"][0] / res["plain_ms"][0], 2)
    res["z_over_zlib_plus_plain"] = round(res["transform_z_ms"][0] / res["zlib_plus_plain_ms"][0], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
