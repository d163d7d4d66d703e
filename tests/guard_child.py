"""Child programs of tests/test_guard_gpu.py: `python guard_child.py <name>` with EDSX_LIB=libedsx_guard.so.

The guard library (csrc/dev_alloc.hip with -DEDSX_GUARD) lays every DevBuf out as [64 KiB zone | payload | 64 KiB zone],
all filled with one byte value.  A case here is one library call on a FRESH context (buffers only grow: a reused context
would put the zones behind an earlier, larger case), run once per fill byte: the result must equal the oracle's under every
fill (it does not depend on bytes nobody wrote), and no zone may be dirty after the call nor after the context is closed (no
store outside a buffer).  Oracle results are computed once per case.  Every child prints and asserts its case count and the
guard's counters."""
import ctypes
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edsparser_amd  # noqa: E402
import oracle_lib as o  # noqa: E402

COMMON_FILLS = (0x00, 0xFF, 0x0A)
MSA_FILLS = COMMON_FILLS + (ord(">"),)
EDS_FILLS = COMMON_FILLS + (ord("{"), ord(","))
VCF_FILLS = COMMON_FILLS + (ord("\t"), ord("#"))


class Guard:
    def __init__(self):
        lib = edsparser_amd.load_library()
        assert os.path.basename(edsparser_amd._capi.lib_path()) == "libedsx_guard.so", edsparser_amd._capi.lib_path()
        lib.edsx_guard_check.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
        lib.edsx_guard_check.restype = ctypes.c_uint64
        lib.edsx_guard_set_fill.argtypes = [ctypes.c_int]
        lib.edsx_guard_set_fill.restype = None
        lib.edsx_guard_counters.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
        lib.edsx_guard_counters.restype = None
        lib.edsx_guard_selftest.argtypes = [ctypes.c_uint64, ctypes.POINTER(ctypes.c_longlong), ctypes.c_int, ctypes.c_int]
        lib.edsx_guard_selftest.restype = ctypes.c_longlong
        self.lib = lib
        self.cases = 0
        self.runs = 0
        self.t0 = time.time()

    def set_fill(self, b):
        self.lib.edsx_guard_set_fill(b)

    def check(self):
        text = ctypes.create_string_buffer(8192)
        n = self.lib.edsx_guard_check(text, 8192)
        return int(n), text.value.decode()

    def counters(self):
        out = (ctypes.c_uint64 * 5)()
        self.lib.edsx_guard_counters(out)
        return dict(zip(("allocations", "bytes", "checks", "live", "unreadable"), map(int, out)))

    def selftest(self, n, offsets, keep):
        arr = (ctypes.c_longlong * max(1, len(offsets)))(*offsets)
        return int(self.lib.edsx_guard_selftest(n, arr, len(offsets), int(keep)))

    def case(self, name, call, want, fills, make=lambda: edsparser_amd.Context(0)):
        """call(ctx) -> result, on a fresh context per fill; want: the oracle's result, computed once by the caller"""
        for fill in fills:
            self.set_fill(fill)
            ctx = make()
            got = call(ctx)
            assert got == want, "%s: result differs from the oracle under fill 0x%02x" % (name, fill)
            n, text = self.check()
            assert n == 0, "%s, fill 0x%02x, after the call:\n%s" % (name, fill, text)
            ctx.close()
            n, text = self.check()
            assert n == 0, "%s, fill 0x%02x, after close:\n%s" % (name, fill, text)
            self.runs += 1
        self.cases += 1

    def finish(self, name, min_cases):
        c = self.counters()
        print("guard %s: cases %d runs %d allocations %d guarded_bytes %d checks %d live %d unreadable %d seconds %.1f"
              % (name, self.cases, self.runs, c["allocations"], c["bytes"], c["checks"], c["live"], c["unreadable"], time.time() - self.t0))
        assert c["allocations"] > 0, "the library loaded does not guard its allocations"
        assert c["unreadable"] == 0, c
        assert self.cases >= min_cases, (self.cases, min_cases)


def _err(fn, *a):
    """library call -> result or ("ERR", text)"""
    try:
        return fn(*a)
    except edsparser_amd.EdsxError as ex:
        return ("ERR", ex.message)


def _oracle(fn, *a):
    try:
        return fn(*a)
    except o.OracleError as ex:
        return ("ERR", str(ex))


# ---- the checker itself ----------------------------------------------------------------------------------------------------

def selftest():
    """One byte stored at payload offset N-1, one at N and one at -1 (all inside the allocation): exactly two zones, at
    offsets +0 (back) and -1 (front); the store at N-1 alone: nothing.  Found live and on the way out, under several fills."""
    g = Guard()
    assert g.check()[0] == 0
    for fill in (0x0A, 0x00, 0xFF):
        g.set_fill(fill)
        for N in (1, 255, 256, 1000, 4096, 100001):
            for keep in (1, 0):
                assert g.selftest(N, [N - 1], keep) == 0          # (0: the payload held the fill)
                n, text = g.check()
                assert n == 0, text
                assert g.selftest(N, [N - 1, N, -1], keep) == 0
                n, text = g.check()
                print(text, end="")
                lines = text.splitlines()
                assert n == 2 and len(lines) == 2, (n, text)
                front = [x for x in lines if " front zone, offsets -1..-1, fill %02x, found a7" % fill in x]
                back = [x for x in lines if " back zone, offsets +0..+0, fill %02x, found a4" % fill in x]
                assert len(front) == 1 and len(back) == 1, text
                assert all(("%d bytes," % N) in x and x.endswith(", at free") == (not keep) for x in lines), text
                assert lines[0].split()[0] == lines[1].split()[0] and lines[0].startswith("#"), text    # one serial number
                assert g.check()[0] == 0                          # reported once
                g.selftest(0, [], 0)                              # releases a kept buffer: its zones were repaired
                assert g.check()[0] == 0
                g.cases += 1
                g.runs += 1
        # a range: first and last dirty offset, far from the edge as well
        assert g.selftest(500, [500 + 7, 500 + 65535, -65536, -3], 1) == 0
        n, text = g.check()
        assert n == 2 and "front zone, offsets -65536..-3," in text and "back zone, offsets +7..+65535," in text, text
        g.selftest(0, [], 0)
        assert g.check()[0] == 0
    # a fill byte equal to a stored byte hides that store: 0xA4 is what the self-test stores at offset N (documented limit)
    g.finish("selftest", 36)
    assert g.counters()["live"] == 0


# ---- MSA -> EDS ----------------------------------------------------------------------------------------------------------

def msa():
    from msa_cases import campaign_msa, random_msa, wide_msa
    import torch
    g = Guard()

    def transform(m, l):
        return lambda ctx: _err(ctx.msa_transform, m, l)

    rng = random.Random(1000)
    for i in range(40):
        m = random_msa(rng, trailing_newline=(i % 3 != 0))
        for l in (0, 3):
            g.case("random_msa %d l=%d" % (i, l), transform(m, l), _oracle(o.msa, m, l), MSA_FILLS)
    for S in (2, 64, 65, 1024, 1025, 4097, 8193):                 # the layout switches of test_row_count_boundaries
        rng = random.Random(1000 + S)
        for lw in (None, 61):
            m = random_msa(rng, S=S, L=2500, lw=lw, p_var=0.06)
            for l in (0, 3):
                g.case("rows S=%d lw=%s l=%d" % (S, lw, l), transform(m, l), _oracle(o.msa, m, l), (0x00, 0xFF))
    rng = random.Random(1)
    for it in range(60):
        m, desc = campaign_msa(rng)
        for l in (0, rng.choice([1, 2, 5, 9, 33])):
            g.case("campaign %d %r l=%d" % (it, desc, l), transform(m, l), _oracle(o.msa, m, l), MSA_FILLS)
    rng = random.Random(20)
    for it in range(40):
        m = wide_msa(rng, nul=bool(it % 2))
        l = (0, rng.choice([1, 4, 12]))[it % 4 >= 2]
        g.case("wide %d l=%d" % (it, l), transform(m, l), _oracle(o.msa, m, l), MSA_FILLS)

    # device-resident API, variant-column store overflows and the host replans ("the slots past the capacity exist only as
    # numbers"); the input and output tensors are torch's, only the library's own buffers are guarded
    S, L, vf = 50, 20000, 0.3
    n = edsparser_amd.synth_size(S, L)
    buf = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    c0 = edsparser_amd.Context(0)
    c0.msa_synth_device(buf.data_ptr(), n, S, L, variant_fraction=vf, seed=7)
    torch.cuda.synchronize()
    c0.close()
    want = o.msa(bytes(buf.cpu().numpy()), 0)

    def resident(ctx):
        E, Q = ctx.msa_plan_device(buf.data_ptr(), n, 0)
        d_eds = torch.empty(E, dtype=torch.uint8, device="cuda:0")
        d_seds = torch.empty(Q, dtype=torch.uint8, device="cuda:0")
        ctx.msa_emit_device(d_eds.data_ptr(), d_seds.data_ptr())
        torch.cuda.synchronize()
        return bytes(d_eds[:E].cpu().numpy()), bytes(d_seds[:Q].cpu().numpy())
    g.case("dense variant columns, device-resident", resident, want, MSA_FILLS)
    assert g.check()[0] == 0                                      # (c0's buffers, freed above)

    K = 3
    rng = random.Random(900 + K)
    for i in range(10):
        lw = rng.choice([None, None, 7, 60])
        l = rng.choice([0, 0, 1, 3, 8])
        m = random_msa(rng, S=rng.randint(2, 9), L=rng.randint(40 * K, 1200), lw=lw, trailing_newline=rng.random() < 0.7,
                       p_var=rng.choice([0.01, 0.05, 0.2]))
        g.case("batched %d" % i, lambda ctx: ctx.msa_transform_batched(m, l, K)[:2], o.msa(m, l), MSA_FILLS)

    rng = random.Random(4242)
    m = random_msa(rng, S=4, L=300_000, lw=None, p_var=0.03)      # 1.2 MB: uploaded as an aligned row image
    assert len(m) >= 1 << 20
    g.case("1.2 MB row image", transform(m, 0), o.msa(m, 0), MSA_FILLS)
    g.finish("msa", 80 + 28 + 120 + 40 + 1 + 10 + 1)


# ---- VCF -> EDS ----------------------------------------------------------------------------------------------------------

def _vcall(vcf, fasta, l, **kw):
    def call(ctx):
        try:
            e, s, st = ctx.vcf_transform(vcf, fasta, l, **kw)
            return {"eds": e, "seds": s, "stats": st}
        except edsparser_amd.EdsxError as ex:
            return {"error": ex.message}
    return call


def _vwant(vcf, fasta, l):
    try:
        e, s, st = o.vcf(vcf, fasta, l)
        return {"eds": e, "seds": s, "stats": st}
    except o.OracleError as ex:
        return {"error": str(ex)}


def vcf():
    import bgzf_spec as bz
    import contig_spec as cs
    from conftest import GOLDEN
    from vcf_cases import (large_key_vcf, random_records, random_vcf, records_vcf, shuffled, single_damage_files,
                           text_length_files)
    g = Guard()

    def case(name, v, f, l=0, fills=VCF_FILLS):
        g.case(name, _vcall(v, f, l), _vwant(v, f, l), fills)

    # the text ends anywhere inside its last 8-byte word (ByteWindow), and just below / at / above multiples of 256
    fasta, mod8, sized = text_length_files(random.Random(88))
    long_alt = [x for x in mod8 if x[0] == mod8[0][0]]
    assert len({(len(v) % 8, nl) for _, _, nl, v in long_alt}) == 16 == len(long_alt)
    for tail, pad, nl, v in long_alt:
        case("text length %d" % len(v), v, fasta)
    assert [t for t, _ in sized] == [255, 256, 257, 511, 512, 513, 4095, 4096, 4097]
    for target, v in sized:
        case("text length %d" % target, v, fasta)

    # as they are; shuffled: the device radix sort; half the lines twice and shuffled: the host sort.  l = 6: the merge
    for L, nvar, ns, lw in ((5000, 300, 8, 60), (3000, 200, 70, 3000), (30, 10, 0, 7)):
        rng = random.Random(L + nvar)
        v0, f = random_vcf(rng, L, nvar, ns, lw)
        for how, v in (("sorted", v0), ("shuffled", shuffled(rng, v0)), ("duplicates", shuffled(rng, v0, dup=True))):
            for l in ((0, 6) if L == 30 else (0,)):
                case("random_vcf %r %s l=%d" % ((L, nvar, ns, lw), how, l), v, f, l)
    # (without samples the l = 6 run above ends in the merge's error text; one with samples merges)
    v, f = random_vcf(random.Random(4150), 4000, 150, 4, 60)
    case("random_vcf (4000, 150, 4, 60) l=6", v, f, 6)

    # RS_TILE = SCAN_TILE = 2048 records: one tile less one, exactly one, two, three
    for n in (2047, 2048, 2049, 4097):
        rng = random.Random(n)
        v0, f = random_vcf(rng, 4 * n, n, 2, 60)
        case("shuffled %d records" % n, shuffled(rng, v0), f)
    for n in (4097, 70000):                                       # keys with every byte in use (tests/test_vcf_gpu.py)
        v, f = large_key_vcf(random.Random(n), n)
        case("large keys %d" % n, v, f)

    # one oddity per file: the host tokeniser and its upload of the record arrays
    files = list(single_damage_files(random.Random(808)))
    picked = [files[k * len(files) // 20] for k in range(18)] + [[x for x in files if x[0] == k][0] for k in ("cr", "tabs")]
    assert len(picked) == 20 and {k for k, *_ in picked} == {"gt", "alt", "pos", "line", "cr", "tabs"}
    for kind, ch, ns, tail, line, v, f in picked:
        case("damage %s %r" % (kind, ch), v, f)

    # compressed input: DEFLATE decoded on the device (BGZF) / on the host (gzip)
    texts = bz.texts()
    for name in ("vcf", "fasta", "zeros", "random"):
        for kind, data in (("bgzf", bz.write(texts[name])[0]), ("gzip", bz.gzip_member(texts[name]))):
            g.case("inflate %s %s" % (name, kind), lambda ctx: ctx.gz_inflate(data), texts[name], VCF_FILLS)
    v, f = random_vcf(random.Random(6), 20000, 1500, 3, 70)
    g.case("compressed transform", _vcall(bz.write(v, payload=4000)[0], bz.write(f, payload=3000)[0], 0, compressed=True),
           _vwant(v, f, 0), VCF_FILLS)

    # several contigs in one input, through a session (its buffers are released inside the call: found on their way out)
    fixtures = cs.load_fixtures(GOLDEN)
    for k, (V, F, parts, left) in enumerate(cs.compose(fixtures, 1)):
        if k == 3:
            break

        def session(ctx, V=V, F=F, parts=parts):
            out = []
            with ctx.vcf_session(V, F) as ses:
                for nm, c in parts:
                    try:
                        e, s, st = ses.transform(nm, c["l"])
                        out.append({"eds": e.decode(), "seds": s.decode(), "stats": st})
                    except edsparser_amd.EdsxError as ex:
                        out.append({"error": ex.message})
            return out
        g.case("contig composition %d" % k, session, [c["expect"] for _, c in parts], VCF_FILLS)

    # the unpartitioned call of test_larger_sharded_equals_unpartitioned (10 Mb reference, 10^5 records, 8 samples): the call
    # whose array sizes scale, once
    rng = random.Random(11)
    L, n = 10_000_000, 100_000
    ref = "".join(rng.choices("ACGT", k=L))
    v, f = records_vcf(ref, random_records(rng, ref, n, 8), 8)
    case("10 Mb unpartitioned", v, f, 0, (0x0A,))
    g.finish("vcf", 16 + 9 + 12 + 1 + 4 + 2 + 20 + 8 + 1 + 3 + 1)


# ---- EDS -> l-EDS --------------------------------------------------------------------------------------------------------

def merge():
    from merge_cases import big_eds, boundary_shifted, boundary_texts, campaign_eds, long_leaf_eds
    g = Guard()

    def case(name, eds, seds, l, compact):
        g.case(name, lambda ctx: _err(ctx.leds_merge, eds, seds, l, compact), _oracle(o.merge, eds, seds, l, compact), EDS_FILLS)

    rng = random.Random(96)
    ran = 0
    while ran < 120:                                              # LINEAR and CARTESIAN, error texts included
        eds, seds, l, compact, desc = campaign_eds(rng)
        if desc[-1] > 100000:
            continue                                              # (the reference and the oracle exhaust memory on these)
        case("campaign %d %r" % (ran, desc), eds, seds, l, compact)
        ran += 1
    body, sbody, _ = boundary_texts()                            # 16-byte threads, 4 KB blocks of the device tokenisers
    for p in list(range(0, 17)) + list(range(4085, 4108, 2)):
        eds, seds = boundary_shifted(body, sbody, p) if p else (body.encode(), sbody.encode())
        case("boundary shift %d" % p, eds, seds, 4, True)
    lens, nsym = (3, 4095, 4096, 4113, 9000), 120                # leaves copied by the whole workgroup, several 4 KB trips
    eds, seds = long_leaf_eds(random.Random(len(lens) * 1000 + nsym), nsym, 5, lens)
    for l in (1, 6, 5000):
        case("long leaves l=%d" % l, eds, seds, l, True)
    case("long leaves CARTESIAN", eds, None, 1, False)
    for compact_in in (False, True):                              # 1 MB and more: the chunk-parallel host tokenisers
        eds, seds = big_eds(random.Random(7 + compact_in), 140000, 6, compact_in, 60)
        assert len(eds) >= 1 << 20 and len(seds) >= 1 << 20
        case("1 MB input compact_in=%d" % compact_in, eds, seds, 24, True)
    g.finish("merge", 120 + 29 + 4 + 2)


# ---- what reads an EDS: statistics, pattern sampling, position checks, locate, path spelling, subset ------------------------

def eds_consumers():
    import numpy as np
    import locate_oracle as lo
    import path_spec as ps
    import query_oracle as qo
    import subset_spec as ss
    g = Guard()
    kind = {True: 1, False: 0, "out_of_range": -1, "invalid_argument": -2}
    rng = random.Random(2026)
    for i in range(20):
        sources, wide = i % 2 == 0, i % 4 == 0                    # half with sources, a quarter with two words per path set
        eds, seds = lo.random_eds(rng, rng.randint(30, 90), sources, paths=130 if wide else 5)
        e = qo.Eds(eds, seds)
        if wide:
            assert max(max(x) for x in e.sources) >= 64
        eb, sb = eds.encode(), (seds.encode() if sources else None)
        tag = "eds %d" % i

        g.case(tag + " stats", lambda ctx: ctx.eds_stats(eb, sb, 2), o.eds_stats(eb, sb, 2), EDS_FILLS)

        try:
            text, wit = qo.generate(qo.Eds(eds), 50, 3, 11 + i)
            want = (text, [2 ** 64 - 1 if wp is None else wp for wp, _ in wit], [c for _, wc in wit for c in wc])
        except RuntimeError:
            text, wit, want = b"", [], "ERR"

        def sample(ctx):
            try:
                t, pos, off, deg = ctx.eds_genpatterns(eb, 50, 3, 11 + i, witness=True)
            except edsparser_amd.EdsxError:
                return "ERR"
            assert [int(x) for x in np.diff(off.astype(np.int64))] == [len(wc) for _, wc in wit]
            return t, [int(x) for x in pos], [int(x) for x in deg]
        g.case(tag + " genpatterns", sample, want, EDS_FILLS)

        pats = [x.decode() for x in text.split(b"\n")[:-1]]
        queries = []
        for k, (wp, wc) in enumerate(wit):
            if wp is None:
                continue
            flip = pats[k][:-1] + ("C" if pats[k][-1] != "C" else "A")
            queries += [(wp, wc, pats[k]), (wp, wc, flip), (wp + 1, wc, pats[k]), (wp, wc[:-1], pats[k]), (wp, wc + [10 ** 6], pats[k])]
        queries += [(0, [], "A"), (10 ** 9, [], "A"), (0, [-1], "AC")]
        coff = np.zeros(len(queries) + 1, dtype=np.uint64)
        coff[1:] = np.cumsum([len(q[1]) for q in queries])
        poff = np.zeros(len(queries) + 1, dtype=np.uint64)
        poff[1:] = np.cumsum([len(q[2]) for q in queries])
        ch = np.array([c for q in queries for c in q[1]], dtype=np.int32)
        ptext = "".join(q[2] for q in queries).encode()
        g.case(tag + " check_positions",
               lambda ctx: [int(x) for x in ctx.eds_check_positions(eb, [q[0] for q in queries], coff, ch, poff, ptext, seds=sb)],
               [kind[qo.check(e, *q)] for q in queries], EDS_FILLS)

        lpats = sorted(set(pats))[:20] + ["A", "C", "AC", "CA", "ACCA", "ACCAACCAC", "G"]
        r = lo.locate(e, lpats)
        want = [r["hit_off"], [tuple(h) for h in r["hits"]], r["choice_off"], r["choices"], r["totals"], r["flags"]]
        g.case(tag + " locate", lambda ctx: [[tuple(int(v) for v in x) if x.dtype.names else int(x) for x in a]
                                             for a in ctx.eds_locate(eb, [x.encode() for x in lpats], seds=sb)], want, EDS_FILLS)
        if not sources:
            continue
        P = ps.parse(eb, sb)[2]
        for lw in (0, 7):
            wf, wm = ps.fasta(eb, sb, None, lw)

            def spell(ctx, lw=lw):
                with ctx.paths_open(eb, sb) as ses:
                    f, m = ses.spell(None, lw)
                return f, [int(x) for x in m]
            g.case(tag + " spell lw=%d" % lw, spell, (wf, wm), EDS_FILLS)
        K = sorted(rng.sample(range(1, P + 1), rng.randint(1, P - 1)))
        for ids in (K, ss.complement(K, P)):
            g.case(tag + " subset of %d paths" % len(ids), lambda ctx: tuple(ctx.eds_subset(eb, sb, ids)), tuple(ss.subset(eb, sb, ids)), EDS_FILLS)
    g.finish("eds_consumers", 10 * 4 + 10 * 8)


# ---- rank threads inside the library, three ranks on one device through the in-process exchange ---------------------------

def multi_rank_one_device():
    from merge_cases import genrandomeds_shaped
    from msa_cases import random_msa
    from vcf_cases import random_records, records_vcf
    g = Guard()

    def three():
        return edsparser_amd.MultiGpu([0, 0, 0], use_rccl=False)

    rng = random.Random(303)
    m = random_msa(rng, S=6, L=600, lw=60, p_var=0.1)

    def msa_multi(mg):
        got = mg.msa_transform(m, 0)
        assert mg.last_partition()[0], "the alignment was not cut into slabs"
        return got
    g.case("msa_transform_multi", msa_multi, o.msa(m, 0), MSA_FILLS, make=three)

    ref = "".join(rng.choice("ACGT") for _ in range(5000))
    v, f = records_vcf(ref, random_records(rng, ref, 400, 3), 3)

    def vcf_multi(mg):
        got = mg.vcf_transform(v, f)
        assert mg.last_vcf()["partitioned"], mg.last_vcf()
        return got
    g.case("vcf_transform_multi", vcf_multi, o.vcf(v, f, 0), VCF_FILLS, make=three)

    eds, seds = genrandomeds_shaped(0.03, 0.05, 3)

    def merge_multi(mg):
        got = mg.leds_merge(eds, seds, 6, True)
        assert mg.last_merge()["partitioned"], mg.last_merge()
        return got
    g.case("leds_merge_multi", merge_multi, o.merge(eds, seds, 6, True), EDS_FILLS, make=three)
    g.finish("multi_rank_one_device", 3)


# ---- contig selection: the inputs whose subject is where a byte falls (tests/contig_walk_cases.py) ----------------------------

def contig_edges():
    import contig_walk_cases as cw
    import contig_walk_expect as cx
    g = Guard()
    fam = cw.families()
    shifts = fam["shift"][::len(fam["shift"]) // 12][:12]                 # a dozen values of p, spread over the sweep
    cases = shifts + fam["ends"] + fam["walks"] + [c for c in fam["counts"] if c["name"] == "counts/K256"]
    assert len(shifts) == 12 and len(cases) == 12 + len(fam["ends"]) + len(fam["walks"]) + 1

    def session(case):
        def call(ctx):
            with ctx.vcf_session(case["V"], case["F"]) as ses:
                info = ses.info()
                recs = [tuple(r[f] for f in cw.REC_FIELDS) for r in ses.contigs()]
                texts = []
                for nm in case["pick"]:
                    try:
                        e, s, st = ses.transform(nm, 0)
                        texts.append({"eds": e, "seds": s, "stats": st})
                    except edsparser_amd.EdsxError as ex:
                        texts.append({"error": ex.message})
                return (recs, info["classified_on_device"], info["records_total"], info["records_without_token"], info["records_unknown_contig"],
                        ses.unknown_contigs(), texts)
        return call

    for case in cases:
        e = cx.expected(case)
        recs = [tuple(int(v) for v in e["recs"][i]) + (int(e["counts"][i]), int(e["duplicate"][i])) for i in range(e["K"])]
        want = (recs, 0 if e["host"] else 1, e["nr"], e["without_token"], e["unknown"], e["unknown_names"],
                [cx.expected_texts(case, nm) for nm in case["pick"]])
        g.case(case["name"], session(case), want, VCF_FILLS + (ord(">"),))
    g.finish("contig_edges", len(cases))


if __name__ == "__main__":
    {"selftest": selftest, "msa": msa, "vcf": vcf, "merge": merge, "eds_consumers": eds_consumers,
     "multi_rank_one_device": multi_rank_one_device, "contig_edges": contig_edges}[sys.argv[1]]()
