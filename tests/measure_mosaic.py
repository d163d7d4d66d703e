"""Measurement (not a test): the mosaics of msa2eds results of synthetic alignments, one session per shape.  Shapes: 64 rows
x 10 Mb and 1000 rows x 1 Mb (rows x columns of the alignment; l = 0), as tests/measure_dist.py.  Per shape four cases:
  all        every path by all the others (both lists empty)
  one        one target (path 1) by all the others: one workgroup marches alone
  planted    a row pieced together from three rows of the alignment, appended to it before msa2eds, by the other rows (the
             first shape only unless asked for: the alignment is built a second time)
  today      what users do now: PathSession.align and a numpy greedy cover per target over the rows of the first
             `base_rows` paths, against mosaic() of the same paths, as a measured ratio of wall clocks; the host works on
             columns and the device on symbols, so the numbers of pieces are reported side by side, not compared
Per case: targets, donors, class columns, segments, the device-event time of every kernel (edsx_set_timing) and of the steps
(edsx_paths_last_timing) and the wall clock of the call, median [min, max] of the repetitions after a warm-up; k_mosaic (COUNT
and FILL together) as donor words per second - targets x donors x words per row x 2 passes.  A case that does not fit the
budget is reported with the library's text instead.
Usage: python tests/measure_mosaic.py [reps] [base_rows] [shape ...]   with shape = ROWSxCOLUMNS (JSON lines)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from measure_dist import mmm  # noqa: E402

KERNELS = ("k_mosaic", "k_mosaic_donors", "scan_segments", "k_dist_rows", "k_path_choose")


def synthetic_msa(ctx, rows, cols):
    import torch
    import edsparser_amd
    n = edsparser_amd.synth_size(rows, cols)
    buf = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    ctx.msa_synth_device(buf.data_ptr(), n, rows, cols)
    torch.cuda.synchronize()
    msa = buf.cpu().numpy()
    del buf
    return msa


def measure(ctx, s, shape, case, targets, donors, reps):
    import edsparser_amd
    walls, kernels, steps = [], [], []
    for it in range(reps + 1):
        ctx.set_timing(True)                                     # (clears the accumulators)
        t0 = time.perf_counter()
        try:
            segs, off, info = s.mosaic(targets, donors)
        except edsparser_amd.EdsxError as ex:
            ctx.set_timing(False)
            print(json.dumps({"shape": shape, "case": case, "does_not_fit": ex.message, **getattr(ex, "info", {})}), flush=True)
            return None
        wall = (time.perf_counter() - t0) * 1e3
        k = {n: ms for n, ms, _ in ctx.get_timing() if n in KERNELS}
        ctx.set_timing(False)
        if it:                                                   # the first one warms up and makes the class list
            walls.append(wall)
            kernels.append(k)
            steps.append(s.timing)
    words = (info["class_columns"] + 63) // 64
    donor_words = info["targets"] * info["donors"] * words * 2
    march_ms = statistics.median([k["k_mosaic"] for k in kernels])
    print(json.dumps({
        "shape": shape, "case": case, "reps": reps, **info,
        "kernel_ms": {n: mmm([k[n] for k in kernels]) for n in kernels[0]},
        "choose_ms": mmm([t["choose_ms"] for t in steps]), "scan_ms": mmm([t["scan_ms"] for t in steps]),
        "copy_ms": mmm([t["copy_ms"] for t in steps]), "download_ms": mmm([t["download_ms"] for t in steps]),
        "donor_words_both_passes": donor_words, "donor_words_per_s": float("%.4g" % (donor_words / (march_ms * 1e-3))),
        "record_bytes": int(segs.nbytes), "call_wall_ms": mmm(walls, 1)}), flush=True)
    return segs


def today(s, shape, base_rows):
    """what users do today: the alignment rows, then a greedy cover per target on the host - per donor the next column at
    which it differs from the target, the furthest of them from the segment's start, and over columns nobody shares the
    next column somebody does"""
    import numpy as np
    import edsparser_amd
    K = min(base_rows, s.info["num_paths"])
    ids = list(range(1, K + 1))
    t0 = time.perf_counter()
    text, _ = s.align(ids, 0, gap="-", as_numpy=True)
    W = s.align_info()["n_columns"]
    rows, at = [], 0
    for k in range(K):
        at = at + int(np.argmax(text[at:at + 64] == 10)) + 1
        rows.append(text[at:at + W])
        at += W + 1
    R = np.stack(rows)
    where = np.arange(W, dtype=np.int32)
    pieces = private = 0
    for t in range(K):
        differ = np.delete(R, t, axis=0) != R[t]
        nxt = np.minimum.accumulate(np.where(differ, where, np.int32(W))[:, ::-1], axis=1)[:, ::-1]      # per donor: the next differing column
        shared = np.minimum.accumulate(np.where(differ.all(axis=0), np.int32(W), where)[::-1])[::-1]       # the next column somebody shares
        c = 0
        while c < W:
            e = int(nxt[:, c].max())
            if e == c:
                e = int(shared[c])
                private += 1
            pieces += 1
            c = e
    host = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    try:
        segs, _, info = s.mosaic(ids, ids)
    except edsparser_amd.EdsxError as ex:
        print(json.dumps({"shape": shape, "case": "today", "does_not_fit": ex.message}), flush=True)
        return
    ours = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"shape": shape, "case": "today", "baseline": "PathSession.align + numpy greedy cover per target", "paths": K, "columns": W,
                      "column_pieces": pieces, "column_private_pieces": private, "segments": info["segments"],
                      "private_segments": info["private_segments"], "align_and_cover_wall_ms": round(host, 1),
                      "mosaic_wall_ms": round(ours, 1), "ratio": round(host / ours, 1)}), flush=True)


def planted(ctx, rows, cols, shape, reps):
    """row `rows`: thirds of the rows 0, 1 and 2"""
    import numpy as np
    msa = synthetic_msa(ctx, rows, cols)
    head = int(np.argmax(msa[:64] == 10)) + 1                    # ">s0\n"; the records of the rows 0, 1, 2 are equally long
    rec = head + cols + 1
    assert msa[rec] == 62 and msa[2 * rec] == 62 and msa[3 * rec] == 62
    cut = (cols // 3, 2 * cols // 3)
    row = np.concatenate([msa[head:head + cut[0]], msa[rec + head + cut[0]:rec + head + cut[1]], msa[2 * rec + head + cut[1]:2 * rec + head + cols]])
    msa = np.concatenate([msa, np.frombuffer(b">planted\n", dtype=np.uint8), row, np.frombuffer(b"\n", dtype=np.uint8)])
    eds, seds = ctx.msa_transform(msa, 0)
    del msa
    with ctx.paths_open(eds, seds) as s:
        P = s.info["num_paths"]
        segs = measure(ctx, s, shape, "planted", [P], list(range(1, P)), reps)
        if segs is not None:
            print(json.dumps({"shape": shape, "case": "planted", "cuts": list(cut),
                              "pieces": [[int(r["donor"]), int(r["column_first"]), int(r["column_end"])] for r in segs[:8]]}), flush=True)


def main():
    import edsparser_amd
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    base_rows = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    shapes = [tuple(int(x) for x in a.split("x")) for a in sys.argv[3:]] or [(64, 10_000_000), (1000, 1_000_000)]
    ctx = edsparser_amd.Context(0)
    for k, (rows, cols) in enumerate(shapes):
        shape = "%d rows x %d columns" % (rows, cols)
        eds, seds = ctx.msa_transform(synthetic_msa(ctx, rows, cols), 0)
        with ctx.paths_open(eds, seds) as s:
            i = s.info
            print(json.dumps({"shape": shape, "symbols": i["n_symbols"], "choice_symbols": i["n_choice_symbols"], "strings": i["n_strings"],
                              "paths": i["num_paths"], "eds_bytes": len(eds), "tokenise_ms": round(s.timing["tokenise_ms"], 1)}), flush=True)
            del eds, seds
            measure(ctx, s, shape, "all", None, None, reps)
            measure(ctx, s, shape, "one", [1], None, reps)
            today(s, shape, base_rows)
        if k == 0 or len(sys.argv) > 3:
            planted(ctx, rows, cols, shape, reps)


if __name__ == "__main__":
    main()
