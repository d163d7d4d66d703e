"""Measure contig selection on the GPU (not a test): BASELINE configs[3] cut in eight contigs (eight edsx_genvcf outputs of
a 125 Mb reference and 1.25 M records each, renamed chr1..chr8: one VCF of ~665 MB, one FASTA of ~1 GB).

  (a) the two new passes, device events (EDSX_TRACE=1 lines of the library): FASTA record index, contig classification
      and regrouping, next to the yardstick of the same run: the record-line starts (k_vt_line_count + scan +
      k_vt_line_fill) on the same VCF, and the tokeniser's count pass (k_vt_count) per contig;
  (b) session open + eight transforms, host clock around the synchronous calls;
  (c) what a user has without sessions: eight edsx_vcf_transform calls on inputs split beforehand (split time not counted).

Median of --runs timed runs after one warm-up.  (b) and (c) run with tracing off; (a) comes from a child process of its
own with EDSX_TRACE=1 (every traced pass ends in an event synchronisation, which end-to-end figures should not carry).

    python tests/measure_vcf_contigs.py [--scale 1.0] [--runs 5] [--out FILE]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def config3_in_eight(ctx, scale=1.0, keep_parts=False):
    """(V, F, parts): parts[k] = the generator's (vcf, fasta) of contig chr<k+1> as it came (CHROM chr1), or None"""
    ref_len, nrec = int(125_000_000 * scale), int(1_250_000 * scale)
    parts, bodies, fastas, head = [], [], [], None
    for k in range(1, 9):
        v, f = ctx.genvcf(ref_len, nrec, 8, seed=k)
        at = v.index(b"\nchr1\t") + 1
        head = head or v[:at]
        body = v[at:]
        assert body.count(b"\n") == nrec and f.startswith(b">chr1 ")
        bodies.append(body if k == 1 else body.replace(b"\nchr1\t", b"\nchr%d\t" % k).replace(b"chr1\t", b"chr%d\t" % k, 1))
        fastas.append(b">chr%d" % k + f[5:])
        parts.append((v, f) if keep_parts else None)
    return head + b"".join(bodies), b"".join(fastas), parts


class _capture_stderr:
    """the library's EDSX_TRACE lines (written by C code to fd 2)"""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def _passes(text):
    out = {}
    for m in re.finditer(r"\[edsx pass\] (.+?)\s+([0-9.]+) ms", text):
        out.setdefault(m.group(1).strip(), []).append(float(m.group(2)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--passes-only", action="store_true", help="(the traced child) print the passes' device times as JSON")
    a = ap.parse_args()
    if a.passes_only:
        os.environ["EDSX_TRACE"] = "1"                               # read once by the library
    else:
        os.environ.pop("EDSX_TRACE", None)
    import edsparser_amd
    ctx = edsparser_amd.Context(0)
    V, F, parts = config3_in_eight(ctx, a.scale, keep_parts=True)
    names = [b"chr%d" % k for k in range(1, 9)]
    res = {"vcf_bytes": len(V), "fasta_bytes": len(F), "runs": a.runs}

    sess, base, passes = [], [], {}
    for r in range(a.runs + 1):
        with _capture_stderr() as cap:
            t0 = time.perf_counter()
            with ctx.vcf_session(V, F) as ses:
                t_open = time.perf_counter() - t0
                out_bytes = 0
                for nm in names:
                    e, s, _ = ses.transform(nm)
                    out_bytes += len(e) + len(s)
                    assert ctx.vcf_tokenised_on_device()
                info = ses.info()
            t_all = time.perf_counter() - t0
        assert info["classified_on_device"] == 1 and info["vcf_h2d_bytes"] == len(V) and info["fasta_h2d_bytes"] == len(F)
        t_base = 0.0
        if not a.passes_only:
            t0 = time.perf_counter()
            for v, f in parts:
                ctx.vcf_transform(v, f, 0)
            t_base = time.perf_counter() - t0
        if r == 0:
            continue                                                 # warm-up
        sess.append((t_open * 1e3, t_all * 1e3))
        base.append(t_base * 1e3)
        for k, v in _passes(cap.text).items():
            passes.setdefault(k, []).append(sum(v))                  # (the count pass runs once per contig: their sum)
    if a.passes_only:
        print(json.dumps({k: statistics.median(v) for k, v in passes.items()}))
        return
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--passes-only", "--scale", str(a.scale), "--runs", str(a.runs)],
                           capture_output=True, text=True, check=True)
    res["output_bytes"] = out_bytes
    res["session_open_ms_median"] = statistics.median(x[0] for x in sess)
    res["session_open_plus_8_transforms_ms_median"] = statistics.median(x[1] for x in sess)
    res["baseline_8_presplit_transforms_ms_median"] = statistics.median(base)
    res["session_runs_ms"] = [round(x[1], 1) for x in sess]            # the spread: (b) and (c) alternate run by run
    res["baseline_runs_ms"] = [round(x, 1) for x in base]
    res["session_over_baseline"] = res["session_open_plus_8_transforms_ms_median"] / res["baseline_8_presplit_transforms_ms_median"]
    res["passes_ms_median"] = json.loads(child.stdout.strip().splitlines()[-1])
    gb = {"fasta record index": 2 * len(F), "vcf line starts": 2 * len(V), "contig classification": len(V)}
    # bytes read: both index passes read their text twice (count, then fill); the classification is a gather, its figure
    # is the text's size over its time
    res["passes_GB_per_s"] = {k: gb[k] / (res["passes_ms_median"][k] * 1e6) for k in gb if k in res["passes_ms_median"]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
