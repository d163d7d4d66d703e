"""CPU: the per-thread device code of the VCF transform (csrc/vcf_walk.hpp) as host code under the address and
undefined-behaviour sanitizers (tests/cpp/test_vcf_walk.cpp, a stand-alone program), on buffers of exactly the sizes the
library allocates, filled with NUL, line feeds, 0xFF or tabs.  Every load and store of that source is checked there, the
masked ones the guard build cannot see included; the texts must equal the oracle's under every fill.  The same program
includes the host code of the path as the library compiles it (csrc/vcf_host.hpp) and runs it in three more modes: the host
tokeniser's way through the transform (files that are not plain, files with equal positions), one position range of a
partitioned run against the oracle's range transform, and the planner of a partitioned run against multigpu.py."""
import json
import os
import random
import struct
import sys
import time

import numpy as np
import pytest

import oracle_lib as o
import vcf_cases as vc
import vcf_walk_cases as w

sys.path.insert(0, w.ROOT)
from edsparser_amd import multigpu as mg  # noqa: E402


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    d = tmp_path_factory.mktemp("vcf_walk")
    return w.build_test_vcf_walk(w.ROOT, str(d / "test_vcf_walk")), str(d)


def _oracle(vcf, fasta):
    try:
        e, s, _ = o.vcf(vcf, fasta, 0)
        return e, s
    except o.OracleError:
        return None


def _compare(twin, named, tag, fills=w.FILLS):
    """named: (name, vcf, fasta) with pairwise distinct positions.  The whole transform under every fill: where the count
    pass accepts the file the texts must be the oracle's, otherwise only the verdict and the clean exit are asserted.
    Returns the number of cases compared in full."""
    exe, workdir = twin
    for name, vcf, _ in named:
        assert w.distinct_positions(vcf), name
    res = w.run_twin(exe, workdir, [(w.FULL, fills, name, vcf, fasta) for name, vcf, fasta in named], tag)
    full = 0
    for name, vcf, fasta in named:
        runs = res[name]
        assert [r[0] for r in runs] == list(fills), name
        verdicts = {r[1] for r in runs}
        assert len(verdicts) == 1, (name, runs)                # the verdict does not depend on the fill
        verdict = verdicts.pop()
        assert verdict in (w.ACCEPTED, w.NOT_PLAIN, w.REFUSED), (name, verdict, runs[0][2])
        if verdict == w.ACCEPTED:
            want = _oracle(vcf, fasta)
            assert want is not None, name
            for fill, _, _, eds, seds in runs:
                assert (eds, seds) == want, (name, fill)
            full += 1
    return full


def test_reference_fixtures(twin):
    """Every input of gen_vcf.json and of the round-2 set.  Files with equal positions (the round-2 set is built around
    them) go through the count pass only - what the device runs on them before the order is the host sort's."""
    exe, workdir = twin
    cases = w.fixture_cases()
    distinct = [c for c in cases if w.distinct_positions(c[1])]
    equal = [c for c in cases if not w.distinct_positions(c[1])]
    assert len(cases) > 40 and len(distinct) > 20
    full = _compare(twin, distinct, "fixtures")
    res = w.run_twin(exe, workdir, [(w.COUNT, w.FILLS, n, v, f) for n, v, f in equal], "fixtures_count")
    for name, _, _ in equal:
        assert len({r[1] for r in res[name]}) == 1 and res[name][0][1] in (w.ACCEPTED, w.NOT_PLAIN), name
    print("fixtures: %d compared in full, %d with distinct positions, %d count pass only" % (full, len(distinct), len(equal)))
    assert full > 10


def test_existing_edge_files(twin):
    """vcf_cases.text_length_files in full; vcf_cases.single_damage_files (one oddity per file) through the count pass,
    which reads every such file on the device before the host tokeniser gets it."""
    exe, workdir = twin
    fasta, mod8, sized = vc.text_length_files(random.Random(88))
    named = [("mod8/%d" % i, vcf, fasta) for i, (_, _, _, vcf) in enumerate(mod8)] + [("sized256/%d" % t, vcf, fasta) for t, vcf in sized]
    assert _compare(twin, named, "edge_lengths") == len(named)
    damaged = [("damage/%d/%s" % (i, kind), v, f) for i, (kind, ch, ns, tail, line, v, f) in enumerate(vc.single_damage_files(random.Random(808)))]
    assert len(damaged) > 150
    res = w.run_twin(exe, workdir, [(w.COUNT, w.FILLS, n, v, f) for n, v, f in damaged], "edge_damage")
    taken = {w.ACCEPTED: 0, w.NOT_PLAIN: 0}
    for name, _, _ in damaged:
        verdicts = {r[1] for r in res[name]}
        assert len(verdicts) == 1 and verdicts <= set(taken), (name, res[name])
        taken[verdicts.pop()] += 1
    assert taken[w.ACCEPTED] > 20 and taken[w.NOT_PLAIN] > 60, taken


def test_text_lengths_and_open_last_lines(twin):
    rng = random.Random(5151)
    sized, opened = w.sized_texts(rng), w.open_ended_texts(rng)
    assert _compare(twin, sized, "sized") == len(sized)
    full = _compare(twin, opened, "open")
    # a last line that ends in a tab has an empty field: not plain; the other three endings are
    assert full == len(opened) - 16, full


def test_random_families(twin):
    named = w.random_families()
    t0 = time.time()
    full = _compare(twin, named, "random")
    print("random families: %d cases, %d compared in full, %.1f s" % (len(named), full, time.time() - t0))
    assert len(named) == len(w.SAMPLES) * len(w.WIDTHS) * 6
    assert full * 100 >= 95 * len(named), (full, len(named))
    for feat in w.FEATURES:                                   # (the names list the features a file really shows)
        shown = sum(feat in n.rsplit("/", 1)[1].split("+") for n, _, _ in named)
        print(feat, shown)
        assert shown >= 20, feat


def test_fa_cpos_windows(twin):
    """fa_cpos alone over every file offset of a window, against a byte-by-byte count: windows starting at every residue
    modulo 256 with lengths of every residue modulo 8, and windows that end at or one byte before the end of the file."""
    exe, workdir = twin
    cases = w.cpos_windows(random.Random(77))
    res = w.run_twin(exe, workdir, [(mode, w.FILLS, name, b"", fasta, up0, up1) for mode, name, fasta, up0, up1 in cases], "cpos")
    assert len(cases) >= 256 * 10
    for _, name, _, _, _ in cases:
        for fill, verdict, detail, _, _ in res[name]:
            assert verdict == w.ACCEPTED, (name, fill, verdict, detail)


def test_the_call_on_record(twin):
    """The input of test_larger_sharded_equals_unpartitioned (seed 11, 10 Mb reference, 10^5 records, 8 samples), the call
    in which the device tokeniser faulted in rounds 2 and 3: one case, under every fill."""
    vcf, fasta = w.call_on_record()
    t0 = time.time()
    assert _compare(twin, [("call_on_record", vcf, fasta)], "record") == 1
    print("the call on record under the sanitizers: %.1f s" % (time.time() - t0))


# ---- the host code of the path (csrc/vcf_host.hpp) through the same program --------------------------------------------
def _compare_as_library(twin, named, tag, fills=w.FILLS):
    """named: (name, vcf, fasta), any file.  The whole transform as the library runs it (host tokeniser where the count pass
    says "not plain", the host's sort for equal positions) under every fill: the oracle's texts, or "refused" where the
    oracle raises.  Returns (compared in full, refused)."""
    exe, workdir = twin
    res = w.run_twin(exe, workdir, [(w.HOST, fills, name, vcf, fasta) for name, vcf, fasta in named], tag)
    full = refused = 0
    for name, vcf, fasta in named:
        want = _oracle(vcf, fasta)
        for fill, verdict, detail, eds, seds in res[name]:
            if want is None:
                assert verdict == w.REFUSED, (name, fill, verdict, detail)
            else:
                assert verdict == w.ACCEPTED, (name, fill, verdict, detail)
                assert (eds, seds) == want, (name, fill)
        full += want is not None
        refused += want is None
    return full, refused


def _not_plain(twin, named, tag):
    exe, workdir = twin
    res = w.run_twin(exe, workdir, [(w.COUNT, (0x0A,), name, vcf, fasta) for name, vcf, fasta in named], tag)
    return [c for c in named if res[c[0]][0][1] == w.NOT_PLAIN]


def test_host_tokeniser_and_equal_positions(twin):
    """Every fixture and every single_damage_files case, each compared in full: the ones the count pass refuses go through
    tokenise -> records -> SoA -> (wrapped positions: the host sweep) -> the same group, size and emit stages on heap blocks
    of upload()'s sizes; files with equal positions take vcf_sort_order on either path."""
    t0 = time.time()
    fixtures = w.fixture_cases()
    damaged = [("damage/%d/%s" % (i, kind), v, f) for i, (kind, ch, ns, tail, line, v, f) in enumerate(vc.single_damage_files(random.Random(808)))]
    equal = [c for c in fixtures if not w.distinct_positions(c[1])]
    np_fix, np_dam = _not_plain(twin, fixtures, "host_np_fix"), _not_plain(twin, damaged, "host_np_dam")
    vcf0, fasta0 = fixtures[0][1:]
    bad_fasta = [("refused/no_header", vcf0, fasta0[1:]), ("refused/header_only", vcf0, fasta0.split(b"\n")[0]), ("refused/empty", vcf0, b"")]
    full, refused = _compare_as_library(twin, fixtures + damaged + bad_fasta, "host_all")
    print("as the library: %d files compared in full, %d refused as by the oracle; not plain: %d fixtures, %d damaged files; "
          "%d fixtures with equal positions; %.1f s" % (full, refused, len(np_fix), len(np_dam), len(equal), time.time() - t0))
    assert full == len(fixtures) + len(damaged) and refused == len(bad_fasta)      # (the oracle refuses none of them at l = 0)
    assert len(np_fix) >= 100 and len(np_dam) > 60 and len(equal) >= 60


def _order_of(pos):
    """the order of the records as every rank derives it (VcfSharder.run)"""
    if len(pos) < 2 or bool(np.all(pos[1:] > pos[:-1])):
        return np.arange(len(pos), dtype=np.int64)
    order = np.argsort(pos, kind="stable").astype(np.int64)
    sp = pos[order]
    if bool(np.any(sp[1:] == sp[:-1])):
        order = o.vcf_sort_order(pos).astype(np.int64)
    return order


def _fasta_meta(fasta):
    """(seq_size, regular) by definition: the first record's bytes that are not line feeds; regular = one record, no
    carriage return, every line but the last as wide as the first, the last one not empty and not wider"""
    seq_start = fasta.index(b"\n") + 1
    first_end = fasta.find(b"\n", seq_start)
    rest = len(fasta) if first_end < 0 else first_end + 1
    nxt = fasta.find(b"\n>", rest - 1)
    rec_end = len(fasta) if nxt < 0 else nxt + 1
    body = fasta[seq_start:rec_end]
    lines = body.split(b"\n")
    if body.endswith(b"\n"):
        lines.pop()
    lw = len(lines[0])
    regular = (rec_end == len(fasta) and b"\r" not in body and lw > 0 and all(len(x) == lw for x in lines[:-1])
               and 0 < len(lines[-1]) <= lw)
    return len(body) - body.count(b"\n"), regular


def _irregular(fasta):
    """the same sequence with lines of uneven width"""
    head, seq = fasta.split(b"\n", 1)
    seq = seq.replace(b"\n", b"")
    out, at, k = [head], 0, 0
    while at < len(seq):
        n = (13, 60, 1, 29)[k % 4]
        out.append(seq[at:at + n]); at += n; k += 1
    return b"\n".join(out) + b"\n"


def _range_cases():
    """the inputs of test_vcf_shard_cpu.py::test_random_sorted_and_shuffled at worlds 2, 3, 8 and line widths 7, 60, 5000, and
    each with an irregular FASTA once: (name, lines, fasta, cur0, next_start, seq_size, regular) per non-empty range"""
    out = []
    for seed in range(6):
        rng = random.Random(1000 + seed)
        ref = "".join(rng.choice("ACGT") for _ in range(rng.randint(300, 3000)))
        recs = vc.random_records(rng, ref, rng.randint(20, 250), rng.choice([1, 3, 8]))
        for shuffle in (None, rng):
            for lw in (60, 7, 5000, 0):
                vcf, fasta = vc.records_vcf(ref, recs, len(recs[0][3]), lw=lw or 60, shuffle=shuffle)
                if lw == 0:
                    fasta = _irregular(fasta)
                seq_size, regular = _fasta_meta(fasta)
                assert seq_size == len(ref) and regular == (lw != 0)
                pos, reflen, off, length, _ = o.vcf_index(vcf)
                order = _order_of(pos)
                for world in (2, 3, 8):
                    cuts, start, wraps = mg.plan_vcf_cuts(pos, reflen, order, world)
                    assert not wraps
                    nonempty = [r for r in range(world) if cuts[r] < cuts[r + 1]]
                    for r in nonempty:
                        g = order[cuts[r]:cuts[r + 1]]
                        lines = b"\n".join(vcf[int(off[x]):int(off[x] + length[x])] for x in g)
                        later = [q for q in nonempty if q > r]
                        cur0 = 0 if r == nonempty[0] else int(start[cuts[r]])
                        nxt = int(start[cuts[later[0]]]) if later else None
                        name = "range/%d/%s/w%d/%d/%d" % (seed, "shuffled" if shuffle else "sorted", lw, world, r)
                        out.append((name, lines, fasta, cur0, nxt, seq_size, regular))
    return out


def test_position_ranges(twin):
    """One position range as run() takes it in a partitioned run - presorted lines, cur0, next_start, the FASTA's metadata -
    through the library's own window function, with the window's out-of-range report live: every piece is the oracle's
    range transform of the same range, on regular FASTAs (a window of the file) and on irregular ones (the whole file)."""
    exe, workdir = twin
    t0 = time.time()
    cases = _range_cases()
    res = w.run_twin(exe, workdir, [(w.RANGE, w.FILLS, name, lines, fasta, cur0, 0xFFFFFFFFFFFFFFFF if nxt is None else nxt, size, int(reg))
                                    for name, lines, fasta, cur0, nxt, size, reg in cases], "ranges")
    windows = 0
    for name, lines, fasta, cur0, nxt, size, reg in cases:
        want = o.vcf_range(lines, fasta, cur0, nxt)[:2]
        for fill, verdict, detail, eds, seds in res[name]:
            assert verdict == w.ACCEPTED, (name, fill, verdict, detail)
            assert (eds, seds) == want, (name, fill)
        windows += reg
    print("position ranges: %d pieces (%d through a window), %.1f s" % (len(cases), windows, time.time() - t0))
    assert len(cases) > 500 and windows > 300 and len(cases) - windows > 100


def _plan_inputs():
    """the inputs of tests/test_vcf_shard_cpu.py: (name, vcf, fasta, world)"""
    out = []
    with open(os.path.join(w.GOLDEN, "gen_vcf.json")) as f:
        cases = [c for c in json.load(f)["cases"] if c["l"] == 0]
    for i, c in enumerate(cases):
        out.append(("plan/gen/%d" % i, c["vcf"].encode(), c["fasta"].encode(), 2 + i % 4))
    for seed in range(6):
        rng = random.Random(1000 + seed)
        ref = "".join(rng.choice("ACGT") for _ in range(rng.randint(300, 3000)))
        recs = vc.random_records(rng, ref, rng.randint(20, 250), rng.choice([1, 3, 8]))
        for shuffle in (None, rng):
            vcf, fasta = vc.records_vcf(ref, recs, len(recs[0][3]), lw=rng.choice([60, 7, 5000]), shuffle=shuffle)
            for world in (2, 3, 8):
                out.append(("plan/random/%d/%d/%d" % (seed, shuffle is not None, world), vcf, fasta, world))
    rng = random.Random(77)
    ref = "".join(rng.choice("ACGT") for _ in range(400))
    vcf, fasta = vc.records_vcf(ref, vc.random_records(rng, ref, 150, 2, dup_frac=0.5), 2)
    out += [("plan/equal/%d" % world, vcf, fasta, world) for world in (2, 4, 7)]
    ref = "ACGTACGTACGTACGTACGTACGTACGTAC"
    vcf, fasta = vc.records_vcf(ref, [(0, "A", "G", ["0|1"]), (5, "A", "C", ["1|1"]), (9, "A", "T", ["0|1"]), (20, "A", "G", ["1|0"])], 1)
    out.append(("plan/pos0", vcf, fasta, 3))
    fasta = (">c\n" + ref + "\n").encode()
    hdr = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS0\n"
    one = hdr + b"c\t7\t.\tG\tT\t.\t.\t.\tGT\t0|1\n"
    beyond = hdr + b"c\t3\t.\tG\tT\t.\t.\t.\tGT\t0|1\nc\t45\t.\tA\tG\t.\t.\t.\tGT\t1|1\n"
    for i, vcf in enumerate((b"", hdr, one, beyond, hdr + b"badline\n")):
        out += [("plan/degenerate/%d/%d" % (i, world), vcf, fasta, world) for world in (2, 5)]
    for i, fa in enumerate((_irregular(fasta), fasta[:-1], fasta + b"\n", fasta + b">d\nACGT\n", fasta.replace(b"\n", b"\r\n"),
                            (">c\n" + "\n".join(ref[k:k + 7] for k in range(0, 28, 7)) + "\n").encode())):
        out += [("plan/fasta/%d/%d" % (i, world), one, fa, world) for world in (2, 5)]
    return out


def _plan_words(vcf, fasta, world):
    """what the program's planner mode writes, from multigpu.py and the oracle's index"""
    words, text = [], []
    try:
        o.vcf(b"", fasta, 0)
        has_meta = True
    except o.OracleError:
        has_meta = False
    words += [1, *map(int, _fasta_meta(fasta))] if has_meta else [0, 0, 0]
    ranges = [mg.vcf_byte_range(vcf, r, world) for r in range(world)]
    index = [o.vcf_index(vcf[lo:hi]) for lo, hi in ranges]
    for lo, hi in ranges:
        words += [lo, hi]
    base = np.concatenate(([0], np.cumsum([len(x[0]) for x in index]))).astype(np.int64)
    pos = np.concatenate([x[0] for x in index]).astype(np.uint64)
    reflen = np.concatenate([x[1] for x in index]).astype(np.uint64)
    order = _order_of(pos)
    cuts, start, wraps = mg.plan_vcf_cuts(pos, reflen, order, world)
    words += [len(pos), int(wraps)] + [int(c) for c in cuts] + order.tolist() + [int(x) for x in start]
    if not wraps:
        for r in range(world):
            for d in range(world):
                g = order[cuts[d]:cuts[d + 1]]
                sel = np.flatnonzero((g >= base[r]) & (g < base[r + 1]))
                rk, rn, blob = mg._line_runs(g[sel], cuts[d] + sel.astype(np.int64), base[r], index[r][2], index[r][3], vcf, ranges[r][0])
                words += [len(rk)] + rk.tolist() + rn.tolist()
                text.append(blob)
    return struct.pack("<%dQ" % len(words), *words), b"".join(text)


def test_planner_of_a_partitioned_run(twin):
    """The C++ planner of vcf2eds over several GPUs (vcf_cut, the FastaMeta rule over the slices, order / starts / cuts /
    wraps, the line runs of every rank for every destination) against multigpu.py (vcf_byte_range, plan_vcf_cuts,
    _line_runs), the oracle's index and the FASTA's metadata by definition."""
    exe, workdir = twin
    t0 = time.time()
    cases = _plan_inputs()
    res = w.run_twin(exe, workdir, [(w.PLAN, (0,), name, vcf, fasta, world) for name, vcf, fasta, world in cases], "plan")
    for name, vcf, fasta, world in cases:
        _, verdict, detail, words, text = res[name][0]
        assert verdict == w.ACCEPTED, (name, verdict, detail)
        want_words, want_text = _plan_words(vcf, fasta, world)
        assert words == want_words, (name, struct.unpack("<%dQ" % (len(words) // 8), words), struct.unpack("<%dQ" % (len(want_words) // 8), want_words))
        assert text == want_text, name
    print("planner: %d inputs, %.1f s" % (len(cases), time.time() - t0))
    assert len(cases) > 200
