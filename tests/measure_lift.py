"""Measurement (not a test): the coordinate lift on BASELINE configs[1]'s EDS (64 paths x 10 Mb) and on a 100 Mbp
genrandomeds EDS, in the style of tests/measure_msa_export.py.  Per shape and per query count (uniformly random
path -> path queries): the device times of edsx_paths_last_timing over several repetitions after a warm-up (median
[min, max]) for PathSession.lift (copy_ms: k_lift_find + k_lift_place), lift_sites (k_lift_find alone) and lift_place
(k_lift_place alone), the share of the tables (choose + scan), queries per second by device time and by the wall clock,
and the HBM read rate the traffic model of DESIGN 8i implies.  Beside it, in the same run, the same queries on the CPU:
numpy.searchsorted over per-path offset tables built on the host from the texts (one thread), whose answers the device's
must equal.
Usage: python tests/measure_lift.py [reps] [genrandomeds bp] [query counts, comma separated]   (one JSON line per run)"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LF_TOP, LF_ITEM = 2048, 2048                                     # k_lift_find: sampled symbols, queries per work item


def host_tables(eds, seds):
    """-> (size per symbol, first string per symbol, length per string, set bits per string: ids 0..63 and 64..127) of
    FULL or compact texts whose path ids are below 128"""
    eds, seds = bytes(eds).translate(None, b" \t\r\n"), bytes(seds).translate(None, b" \t\r\n")
    t = np.frombuffer(eds, dtype=np.uint8)
    d = np.flatnonzero((t == ord("{")) | (t == ord(",")) | (t == ord("}")))
    d = np.concatenate([[-1], d, [len(t)]])                      # virtual '}' in front, virtual '{' behind
    kind = np.concatenate([[ord("}")], t[d[1:-1]], [ord("{")]])
    gap = d[1:] - d[:-1] - 1
    opens = kind[:-1] != ord("}")                                 # '{' or ',' in front: a string, whatever its length
    bare = (kind[:-1] == ord("}")) & (gap > 0)                   # text outside braces: a symbol of one string
    is_str = opens | bare
    first = (kind[:-1] == ord("{")) | bare                       # the string opens a symbol
    str_len = gap[is_str].astype(np.uint64)
    sym_first = np.flatnonzero(first[is_str])
    size = np.diff(np.concatenate([sym_first, [len(str_len)]]))
    s = np.frombuffer(seds, dtype=np.uint8)
    digit = (s >= ord("0")) & (s <= ord("9"))
    start = np.flatnonzero(digit & ~np.concatenate([[False], digit[:-1]]))
    end = np.flatnonzero(digit & ~np.concatenate([digit[1:], [False]]))
    assert int((end - start).max()) <= 2, "path ids of up to three digits"
    val = np.zeros(len(start), dtype=np.int64)
    for k in range(3):
        val = np.where(start + k <= end, val * 10 + s[np.minimum(start + k, end)] - 48, val)
    assert int(val.max()) < 128
    group = np.cumsum(s == ord("{"))[start] - 1
    tok_first = np.flatnonzero(np.concatenate([[True], group[1:] != group[:-1]]))
    one = np.uint64(1)                                           # the ids of a set differ: the sum is the OR
    bits = (np.add.reduceat(np.where(val < 64, one << (val & 63).astype(np.uint64), np.uint64(0)), tok_first),
            np.add.reduceat(np.where(val >= 64, one << (val & 63).astype(np.uint64), np.uint64(0)), tok_first))
    assert len(bits[0]) == len(str_len), "source count does not match cardinality"
    return size, sym_first, str_len, bits


def path_table(tab, p):
    """-> (chosen string per symbol or -1, sym_pos with n + 1 entries) of path p"""
    size, sym_first, str_len, bits = tab
    has = ((bits[0] & np.uint64(1 | (1 << p if p < 64 else 0))) | (bits[1] & np.uint64(1 << (p - 64) if p >= 64 else 0))) != 0
    cand = np.where(has, np.arange(len(has), dtype=np.int64), np.int64(1) << 62)
    ch = np.minimum.reduceat(cand, sym_first)
    ch[ch == np.int64(1) << 62] = -1
    ln = np.where(ch >= 0, str_len[np.maximum(ch, 0)], np.uint64(0))
    return ch, np.concatenate([[np.uint64(0)], np.cumsum(ln, dtype=np.uint64)])


def cpu_lift(tab, tables, src, pos, dst):
    """The same queries with numpy.searchsorted -> (dst_pos, status)"""
    _, _, str_len, _ = tab
    out, st = np.full(len(src), np.uint64(2 ** 64 - 1)), np.full(len(src), 4, dtype=np.uint8)
    sym, sid, off = np.zeros(len(src), dtype=np.int64), np.zeros(len(src), dtype=np.int64), np.zeros(len(src), dtype=np.uint64)
    for a in np.unique(src):
        q = np.flatnonzero(src == a)
        ch, at = tables[int(a)]
        q = q[pos[q] < at[-1]]
        i = np.searchsorted(at, pos[q], side="right") - 1
        sym[q], sid[q], off[q], st[q] = i, ch[i], pos[q] - at[i], 0
    for b in np.unique(dst):
        q = np.flatnonzero((dst == b) & (st == 0))
        ch, at = tables[int(b)]
        c, start = ch[sym[q]], at[sym[q]]
        lc = np.where(c >= 0, str_len[np.maximum(c, 0)], np.uint64(0))
        gap = off[q] >= lc
        out[q] = start + np.where(gap, lc, off[q])
        st[q] = np.where(c < 0, 3, np.where(gap, 2, np.where(c == sid[q], 0, 1)))
    return out, st


def _med(rows, key):
    v = [r[key] for r in rows]
    return [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]


def measure(ctx, name, eds, seds, reps, counts):
    s = ctx.paths_open(eds, seds)
    info = s.info
    P, n, nc = info["num_paths"], info["n_symbols"], info["n_choice_symbols"]
    t0 = time.time()
    tab = host_tables(eds, seds)
    tables = {p: path_table(tab, p) for p in range(1, P + 1)}
    host_build_s = time.time() - t0
    lengths = np.array([int(tables[p][1][-1]) for p in range(1, P + 1)])
    assert [int(x) for x in s.lengths()[0]] == list(lengths)
    rng = np.random.default_rng(1)
    for nq in counts:
        src = rng.integers(1, P + 1, nq).astype(np.uint64)
        dst = rng.integers(1, P + 1, nq).astype(np.uint64)
        pos = (rng.random(nq) * lengths[src.astype(np.int64) - 1]).astype(np.uint64)
        lift, find, place, wall = [], [], [], []
        for it in range(reps + 1):                               # the first round warms up
            t0 = time.time()
            got = s.lift(src, pos, dst)
            w = time.time() - t0
            tl = s.timing
            sites, _ = s.lift_sites(src, pos)
            tf = s.timing
            s.lift_place(sites["symbol"], sites["string"], sites["offset"], dst)
            tp = s.timing
            if it:
                lift.append(tl), find.append(tf), place.append(tp), wall.append({"s": w})
        t0 = time.time()
        want = cpu_lift(tab, tables, src, pos, dst)
        cpu_s = time.time() - t0
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "device and numpy differ"
        copy = statistics.median(r["copy_ms"] for r in lift)
        tabs = statistics.median(r["choose_ms"] + r["scan_ms"] for r in lift)
        # per query the path, position, slot, 40-byte site, status and result (about 100 B streamed), the
        # dependent search steps behind the LDS table (24 B each: cf, rank, S) and 15 scattered 8-byte reads of site and
        # place; per work item of LF_ITEM queries LF_TOP sampled offsets of 24 B
        steps = max(1, int(np.ceil(np.log2(max(2, -(-n // LF_TOP))))))
        model = nq * (100 + 24 * steps + 15 * 8) + (nq // LF_ITEM + P) * LF_TOP * 24
        print(json.dumps({"shape": name, "paths": P, "n_symbols": n, "n_choice_symbols": nc, "queries": nq, "reps": reps,
                          "lift_copy_ms": _med(lift, "copy_ms"), "find_ms": _med(find, "copy_ms"), "place_ms": _med(place, "copy_ms"),
                          "choose_ms": _med(lift, "choose_ms"), "scan_ms": _med(lift, "scan_ms"),
                          "tables_share": round(tabs / (tabs + copy), 3), "wall_s": _med(wall, "s"),
                          "mqueries_per_s_kernels": round(nq / copy / 1e3, 1),
                          "mqueries_per_s_wall": round(nq / statistics.median(r["s"] for r in wall) / 1e6, 2),
                          "search_steps_behind_lds": steps, "model_bytes": model, "model_gbps": round(model / copy / 1e6, 1),
                          "cpu_searchsorted_s": round(cpu_s, 3), "cpu_mqueries_per_s": round(nq / cpu_s / 1e6, 2),
                          "host_table_build_s": round(host_build_s, 1)}), flush=True)
    s.close()


def main():
    import torch
    import edsparser_amd
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    gen_bp = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    counts = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1_000_000, 10_000_000]
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
    measure(ctx, "configs[1] msa2eds output, 64 x 10 Mb", eds, seds, reps, counts)
    eds, seds, _ = ctx.genrandomeds(gen_bp, seed=5)
    measure(ctx, "genrandomeds %d bp" % gen_bp, eds, seds, reps, counts)


if __name__ == "__main__":
    main()
