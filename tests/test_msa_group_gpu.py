"""The wave64 grouping code of the MSA transform, called directly: fast_group<true, HEAVY> (csrc/msa_fast_kernels.hpp),
fused_group_run<ROWS64> (csrc/msa_scan_kernels.hpp) and the helpers of csrc/msa_wave.hpp, through the plain C launchers of
tests/hip/msa_group_harness.hip (edsparser_amd/libedsx_msagroup.so, built by edsparser_amd.build for the tests only;
DESIGN.md section 2.4).

Expected values: tests/msa_group_spec.py (plain Python: the distinct gap-stripped strings in the order of their first rows,
and the routing table of fast_group as the RETURN CODE it promises - a branch that wrongly gives up still produces the right
text through its fallback, so the code is asserted exactly) and numpy for the helpers.  Every buffer a launcher writes
lies between two margins of a known byte and is poisoned before the call; the padding rows S .. Spad-1 of every vc column
are filled in turn with 0x00, 'A' and 0xA5 and every fill must give the expected result."""
import ctypes
import os

import numpy as np
import pytest
import torch

import msa_group_spec as spec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("EDSX_MSAGROUP_LIB") or os.path.join(ROOT, "edsparser_amd", "libedsx_msagroup.so")   # (another build of the harness)
DEV = "cuda:0"
MARGIN = 4096                    # bytes on either side of every written buffer
FENCE = 0x3C                     # what the margins hold
POISON = 0xA5                    # what a written buffer holds before the call
FILLS = (0x00, ord("A"), 0xA5)   # the padding rows of the columns
U32, U64 = np.uint32, np.uint64
P = ctypes.c_void_p


class MsaView(ctypes.Structure):                               # csrc/msa_device.hpp
    _fields_ = [("file", P), ("row_start", P), ("V", P), ("Vraw", P), ("word_slot", P), ("vc", P), ("hdr", P),
                ("L", ctypes.c_uint64), ("lw", ctypes.c_uint64), ("S", ctypes.c_uint32), ("Spad", ctypes.c_uint32), ("tileW", ctypes.c_uint32)]


class K1Params(ctypes.Structure):                              # csrc/msa_scan_launch.hpp
    _fields_ = [("file", P), ("row_start", P), ("hdr", P), ("Vraw", P), ("word_slot", P), ("vc", P), ("vc_cap_cols", ctypes.c_uint64),
                ("Draw", ctypes.c_uint64), ("lw", ctypes.c_uint64), ("S", ctypes.c_uint32), ("Spad", ctypes.c_uint32),
                ("cpr_log2", ctypes.c_uint32), ("cap_cols", ctypes.c_uint32), ("ntiles", ctypes.c_uint64), ("fuse", ctypes.c_uint32),
                ("Fraw", P), ("rec_info", P), ("recf", P), ("recf_stride", ctypes.c_uint32), ("recf_gid", ctypes.c_uint32)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        assert os.path.exists(LIB), "python -m edsparser_amd.build builds it"
        L = ctypes.CDLL(LIB)
        u32, u64, I = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
        L.mg_sizeof.argtypes, L.mg_sizeof.restype = [I], u64
        L.mg_group.argtypes = [I, P, P, P, P, u64, P]
        L.mg_fused.argtypes = [I, P, P, P, P, u32, u32, u64, P]
        L.mg_wave.argtypes = [P, P, u64, P, P, P]
        L.mg_bytes.argtypes = [P, P, P, u64, P]
        for f in ("mg_group", "mg_fused", "mg_wave", "mg_bytes"):
            getattr(L, f).restype = I
        assert L.mg_sizeof(0) == ctypes.sizeof(MsaView) and L.mg_sizeof(1) == ctypes.sizeof(K1Params)
        assert (L.mg_sizeof(2), L.mg_sizeof(3), L.mg_sizeof(4), L.mg_sizeof(5)) == (GROUP_WORDS, WAVE_WORDS, BYTES_WORDS, 64)
        _lib = L
    return _lib


GROUP_WORDS, WAVE_WORDS, BYTES_WORDS = 516, 12, 56


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def sync():
    torch.cuda.current_stream().synchronize()


def dev(a):
    """a numpy array on the device, as bytes"""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(DEV)
    if t.numel() == 0:
        t = torch.zeros(16, dtype=torch.uint8, device=DEV)
    assert t.data_ptr() % 16 == 0
    return t


def dev_struct(s):
    return dev(np.frombuffer(bytes(s), dtype=np.uint8))


class Guarded:
    """nbytes of device memory filled with `poison`, between two margins of FENCE bytes"""

    def __init__(self, nbytes, poison=POISON):
        self.n = int(nbytes)
        self.t = torch.empty(2 * MARGIN + self.n, dtype=torch.uint8, device=DEV)
        assert self.t.data_ptr() % 16 == 0
        self.t[:MARGIN] = FENCE
        self.t[MARGIN + self.n:] = FENCE
        self.t[MARGIN:MARGIN + self.n] = poison
        self.ptr = self.t.data_ptr() + MARGIN

    def bytes(self):
        return self.t[MARGIN:MARGIN + self.n].cpu().numpy()

    def check(self, what=""):
        front, back = self.t[:MARGIN].cpu().numpy(), self.t[MARGIN + self.n:].cpu().numpy()
        bad_f, bad_b = np.flatnonzero(front != FENCE), np.flatnonzero(back != FENCE)
        assert bad_f.size == 0, "%s: front margin written at byte offsets %s" % (what, (bad_f[:8] - MARGIN).tolist())
        assert bad_b.size == 0, "%s: back margin written at byte offsets +%s" % (what, bad_b[:8].tolist())


# ================================================================================================================
# fast_group
# ================================================================================================================
def run_group(S, segs, heavy, fill, lw):
    """one launch over all the segments -> u32[n][GROUP_WORDS]"""
    w = spec.World(S, segs, fill, lw)
    keep = [dev(w.file), dev(np.array([w.row0], dtype=U64)), dev(w.V), dev(w.Vraw), dev(w.word_slot), dev(w.vc)]
    mv = MsaView(*[t.data_ptr() for t in keep], 0, w.L, lw, S, w.Spad, spec.TILE_W)
    d_mv, d_cm, d_sa = dev_struct(mv), dev(w.cmeta), dev(w.seg_a_list)
    out = Guarded(4 * GROUP_WORDS * len(segs))
    rc = lib().mg_group(int(heavy), d_mv.data_ptr(), d_cm.data_ptr(), d_sa.data_ptr(), out.ptr, len(segs), stream())
    assert rc == 0, rc
    sync()
    out.check("mg_group S %d heavy %d fill %#x" % (S, heavy, fill))
    assert np.array_equal(keep[5].cpu().numpy(), w.vc.reshape(-1)), "vc changed"
    return out.bytes().view(U32).reshape(len(segs), GROUP_WORDS)


def check_group(seg, o, heavy, what):
    """one segment's output against the reference; the figures are in the message"""
    S, g = seg.S, seg.groups
    lanes = o[:512].reshape(64, 8)
    rc, want_rc = int(o[514]), seg.route(heavy)
    assert rc == want_rc, "%s: return code %d, the routing table says %d (k %d, raw classes %d)" % (what, rc, want_rc, g.k, seg.raw_classes())
    if rc != 1:
        return
    assert (int(o[512]), int(o[513])) == (g.k, g.sumlen), "%s: k, sumlen = %d, %d, want %d, %d" % (what, o[512], o[513], g.k, g.sumlen)
    gid = np.ascontiguousarray(lanes[:, :4]).view(np.uint8).reshape(-1)[:S]
    bad = np.flatnonzero(gid != g.gid)
    assert bad.size == 0, "%s: gid wrong at rows %s: got %s want %s" % (what, bad[:8].tolist(), gid[bad[:8]].tolist(), g.gid[bad[:8]].tolist())
    rep = lanes[:g.k, 7]
    assert np.array_equal(rep, np.array(g.rep, dtype=U32)), "%s: rep %s, want %s" % (what, rep.tolist(), g.rep)
    if g.k <= 4:
        assert np.array_equal(lanes[:, 4:5], spec.pack_ids(g.gid, 2)), what + ": 2-bit ids"
    elif g.k <= 16:
        assert np.array_equal(lanes[:, 5:7], spec.pack_ids(g.gid, 4)), what + ": 4-bit ids"
    assert int(o[515]) == seg.saw_nl(), "%s: saw_nl %d" % (what, o[515])


@pytest.mark.parametrize("heavy", [False, True], ids=["light", "heavy"])
@pytest.mark.parametrize("S", spec.SIZES)
def test_fast_group(S, heavy):
    segs = spec.cases(S)
    for lw, part in spec.split_launches(segs):
        for fill in FILLS:
            out = run_group(S, part, heavy, fill, lw)
            for seg, o in zip(part, out):
                check_group(seg, o, heavy, "S %d %s %s fill %#x" % (S, "heavy" if heavy else "light", seg.name, fill))


# ================================================================================================================
# fused_group_run
# ================================================================================================================
def recf_geometry(S):
    """as MsaPipeline::plan computes them (csrc/msa_device.hip)"""
    gid = (8 * ((S + 15) // 16) + 15) & ~15
    return gid, (gid + 4 + spec.REC_TEXT_MAX + 63) & ~63


def run_fused(S, runs, rows64, fill):
    Spad = spec.vc_pitch(S)
    recf_gid, stride = recf_geometry(S)
    cap = min(65536 // Spad, 2047)
    chunks, cur, used = [], [], 0
    for r in runs:                                             # images of at most 64 KiB, a poison column behind every run
        if used + r.ncol + 1 > cap:
            chunks.append(cur)
            cur, used = [], 0
        cur.append(r)
        used += r.ncol + 1
    chunks.append(cur)
    for chunk in chunks:
        ncols = sum(r.ncol + 1 for r in chunk)
        img = np.full((ncols, Spad), spec.POISON_COL, dtype=np.uint8)
        desc, slot_base, slots, at, SB = [], [], [], 0, 2
        for i, r in enumerate(chunk):
            img[at:at + r.ncol, :S] = r.M.T
            img[at:at + r.ncol, S:] = fill
            desc.append(at | (r.ncol << 11))
            slot_base.append(SB + 3 * i)
            slots.append(SB + 3 * i + at)
            at += r.ncol + 1
        nslot = slots[-1] + chunk[-1].ncol + 2
        vc, recf, info = Guarded(nslot * Spad), Guarded(nslot * stride), Guarded(4 * nslot)
        p = K1Params(0, 0, 0, 0, 0, vc.ptr, nslot, 0, 0, S, Spad, 0, 0, 0, 1, 0, info.ptr, recf.ptr, stride, recf_gid)
        d_p, d_img, d_desc, d_sb = dev_struct(p), dev(img), dev(np.array(desc, dtype=U32)), dev(np.array(slot_base, dtype=U64))
        rc = lib().mg_fused(int(rows64), d_p.data_ptr(), d_img.data_ptr(), d_desc.data_ptr(), d_sb.data_ptr(), ncols, Spad, len(chunk), stream())
        assert rc == 0, rc
        sync()
        what = "S %d rows64 %d fill %#x" % (S, rows64, fill)
        for b, name in ((vc, "vc"), (recf, "recf"), (info, "rec_info")):
            b.check(what + " " + name)
        # the expected images of the three buffers: poison but for what the runs write
        e_vc = np.full((nslot, Spad), POISON, dtype=np.uint8)
        e_recf = np.full((nslot, stride), POISON, dtype=np.uint8)
        e_info = np.full(nslot, POISON * 0x01010101, dtype=U32)
        nl = (S + 15) // 16
        for r, d, slot in zip(chunk, desc, slots):
            g = r.groups
            if not r.fused_ok():
                e_info[slot] = 0
                e_vc[slot:slot + r.ncol] = img[d & 0x7FF:(d & 0x7FF) + r.ncol]
                continue
            text = g.text()
            ids = spec.pack_ids(g.gid, 2 if g.k <= 4 else 4)[:nl]
            e_recf[slot, :ids.size * 4] = ids.reshape(-1).view(np.uint8)
            e_recf[slot, recf_gid:recf_gid + 4] = np.array([g.k | (len(text) << 8)], dtype=U32).view(np.uint8)
            e_recf[slot, recf_gid + 4:recf_gid + 4 + len(text)] = np.frombuffer(text, dtype=np.uint8)
            e_info[slot] = g.k | (len(text) << 8) | ((1 << 30) if g.k > 4 else 0) | (1 << 31)
        g_vc, g_recf, g_info = vc.bytes().reshape(nslot, Spad), recf.bytes().reshape(nslot, stride), info.bytes().view(U32)
        for r, slot in zip(chunk, slots):
            w = "%s %s (k %d, text %d)" % (what, r.name, r.groups.k, len(r.groups.text()))
            assert g_info[slot] == e_info[slot], "%s: rec_info %#x, want %#x" % (w, g_info[slot], e_info[slot])
            assert np.array_equal(g_recf[slot], e_recf[slot]), "%s: record differs at bytes %s: %r" % (
                w, np.flatnonzero(g_recf[slot] != e_recf[slot])[:8].tolist(), g_recf[slot, recf_gid:recf_gid + 72].tobytes())
            assert np.array_equal(g_vc[slot:slot + r.ncol], e_vc[slot:slot + r.ncol]), w + ": vc columns"
        assert np.array_equal(g_info, e_info) and np.array_equal(g_recf, e_recf) and np.array_equal(g_vc, e_vc), what + ": a write outside the runs' own slots"


@pytest.mark.parametrize("S,rows64", [(S, False) for S in spec.SIZES] + [(S, True) for S in spec.SIZES if S <= 64])
def test_fused_group_run(S, rows64):
    runs = spec.fused_runs(S, rows64)
    for fill in FILLS:
        run_fused(S, runs, rows64, fill)


# ================================================================================================================
# helpers
# ================================================================================================================
def wave_vectors():
    rng = np.random.default_rng(7)
    lane = np.arange(64, dtype=U32)
    v = [np.zeros((64, 4), dtype=U32), np.ones((64, 4), dtype=U32), np.stack([lane, lane * 3 + 1, 63 - lane, lane ^ 21], axis=1)]
    v += [rng.integers(0, 1 << 32, (64, 4), dtype=np.uint64).astype(U32) for _ in range(8)]
    for p in range(64):                                        # a single non-zero lane at each position
        a = np.zeros((64, 4), dtype=U32)
        a[p] = (0x80000001 + p, p + 1, 0xFFFFFFFF, 1 << (p % 32))
        v.append(a)
    v = np.stack(v)
    v[3:11, 0, 2] = np.arange(8) * 9                           # (readlane64's source lane is lane 0's c)
    return v


def test_wave_helpers():
    v = wave_vectors()
    n = len(v)
    rng = np.random.default_rng(8)
    lead = rng.integers(0, 256, (64, 16), dtype=np.uint8)
    out, out_l = Guarded(4 * WAVE_WORDS * 64 * n), Guarded(4 * 64 * 16 * 64)
    d_in, d_lead = dev(v), dev(lead)
    assert lib().mg_wave(d_in.data_ptr(), out.ptr, n, d_lead.data_ptr(), out_l.ptr, stream()) == 0
    sync()
    out.check("mg_wave")
    out_l.check("mg_wave leader")
    o = out.bytes().view(U32).reshape(n, 64, WAVE_WORDS)
    a, b, c = v[:, :, 0], v[:, :, 1], v[:, :, 2]
    cs = np.cumsum(v.astype(np.uint64), axis=1).astype(U32)    # (sums wrap mod 2^32)
    assert np.array_equal(o[:, :, 0], cs[:, :, 0]), "wave_scan_incl"
    assert np.array_equal(o[:, :, 1:5], cs), "wave_scan_incl4"
    assert np.array_equal(o[:, :, 5], np.repeat(np.bitwise_xor.reduce(a, axis=1)[:, None], 64, axis=1)), "wave_xor_all"
    assert np.array_equal(o[:, :, 6], np.repeat(np.bitwise_or.reduce(a, axis=1)[:, None], 64, axis=1)), "wave_or_all"
    assert np.array_equal(o[:, :, 7], np.repeat(a[:, :8].min(axis=1)[:, None], 64, axis=1)), "min_lanes8"
    src = (c[:, 0] & 63).astype(np.int64)
    idx = np.arange(n)
    assert np.array_equal(o[:, :, 8], np.repeat(a[idx, src][:, None], 64, axis=1)) and \
        np.array_equal(o[:, :, 9], np.repeat(b[idx, src][:, None], 64, axis=1)), "readlane64"
    assert np.array_equal(o[:, :, 10], np.repeat(a[:, :1], 64, axis=1)) and np.array_equal(o[:, :, 11], np.repeat(b[:, :1], 64, axis=1)), "uniform64"
    ol = out_l.bytes().view(U32).reshape(64, 16, 64)
    assert np.array_equal(ol, np.repeat(lead.astype(U32)[:, :, None], 64, axis=2)), "leader_byte"


def bytes_items():
    """a, b, c (16 bytes each), x, lane, S: every byte value at every position, against equal and different bytes"""
    rng = np.random.default_rng(9)
    A, B, C, X, LANE, SS = [], [], [], [], [], []
    specials = np.array(list(b"ACGTN-\n\0acgtnRY") + [0x80, 0xFF, 0x7F, 0x2C, 0x2E, 0x0B, 0x09, 0x01], dtype=np.uint8)
    for v in range(256):
        for p in range(16):
            a = specials[rng.integers(0, len(specials), 16)] if (v + p) % 3 else rng.integers(0, 256, 16, dtype=np.uint8)
            a[p] = v
            b = a.copy()
            flip = rng.integers(0, 16, 3)
            b[flip] ^= np.array([1, 0x80, 1 << (v % 8)], dtype=np.uint8)
            c = np.where(rng.integers(0, 4, 16) > 0, 0xFF, 0).astype(np.uint8) if p % 2 else spec_mask(int(rng.integers(0, 17)))
            A.append(a), B.append(b), C.append(c), X.append((v if p % 4 else int(a[(p + 5) % 16])) * 0x01010101), LANE.append(0), SS.append(0)
    for size in (8, 16, 32, 64):                               # lutN: every index below the table's size
        for i in range(size):
            a = np.zeros(16, dtype=np.uint8)
            a[:4] = (i, (i + 1) % size, size - 1 - i, (i * 5) % size)
            A.append(a), B.append(a.copy()), C.append(spec_mask(16)), X.append(0), LANE.append(0), SS.append(0)
    for p in range(17):                                        # masks of 0x00 / 0xFF bytes: the first set byte is byte p
        a = np.zeros(16, dtype=np.uint8)
        a[p:] = np.where(rng.integers(0, 2, 16 - p) > 0, 0xFF, 0)
        if p < 16:
            a[p] = 0xFF
        A.append(a), B.append(a.copy()), C.append(spec_mask(16)), X.append(0), LANE.append(0), SS.append(0)
    for S in range(0, 1041):                                   # fast_valid_mask at every S
        for lane in range(64):
            A.append(np.zeros(16, dtype=np.uint8)), B.append(np.zeros(16, dtype=np.uint8)), C.append(np.zeros(16, dtype=np.uint8))
            X.append(0), LANE.append(lane), SS.append(S)
    return np.stack(A), np.stack(B), np.stack(C), np.array(X, dtype=U32), np.array(LANE, dtype=U32), np.array(SS, dtype=U32)


def spec_mask(n):
    m = np.zeros(16, dtype=np.uint8)
    m[:n] = 0xFF
    return m


def test_byte_helpers():
    A, B, C, X, LANE, SS = bytes_items()
    n = len(A)
    item = np.zeros((n, 64), dtype=np.uint8)
    item[:, 0:16], item[:, 16:32], item[:, 32:48] = A, B, C
    item[:, 48:60] = np.stack([X, LANE, SS], axis=1).view(np.uint8)
    rng = np.random.default_rng(10)
    table = rng.integers(0, 256, 64, dtype=np.uint8)
    out = Guarded(4 * BYTES_WORDS * n)
    d_item, d_table = dev(item), dev(table)
    assert lib().mg_bytes(d_item.data_ptr(), d_table.data_ptr(), out.ptr, n, stream()) == 0
    sync()
    out.check("mg_bytes")
    o = out.bytes().view(U32).reshape(n, BYTES_WORDS)
    b4 = lambda words: np.ascontiguousarray(words).view(np.uint8).reshape(n, -1)      # u32 words -> their bytes
    xb = (X & 0xFF).astype(np.uint8)[:, None]
    bits16 = lambda m: (m.astype(U32) << np.arange(16, dtype=U32)).sum(axis=1).astype(U32)
    ff = lambda m: np.where(m, 0xFF, 0).astype(np.uint8)
    assert np.array_equal(b4(o[:, 0:1]), ff(A[:, :4] != B[:, :4])), "bytes_ne_mask"
    assert np.array_equal(b4(o[:, 1:5]), ff(A == xb)), "bytes_eq_mask"
    nz = A != 0
    assert np.array_equal(o[:, 5], np.where(nz.any(axis=1), nz.argmax(axis=1), 16).astype(U32)), "first_byte_index"
    assert np.array_equal(o[:, 6], bits16(A != B)), "chunk_ne16"
    assert np.array_equal(o[:, 7], bits16(A == xb)), "chunk_eq16"
    assert np.array_equal(b4(o[:, 8:12]), C | (A ^ B)), "acc_or_xor"
    gap, nl = A == 0x2D, A == 0x0A
    assert np.array_equal(b4(o[:, 12:16]), np.where(gap | nl, 0, A)), "normalise_col<true>"
    assert np.array_equal(o[:, 16], (nl & (C == 0xFF)).any(axis=1).astype(U32)), "normalise_col<true>: saw_nl"
    assert np.array_equal(b4(o[:, 17:21]), np.where(gap, 0, A)) and not o[:, 54].any(), "normalise_col<false>"
    full = (C == 0xFF) | (C == 0)                              # any_nul, dna_bad: masks of whole bytes
    assert full.all()
    assert np.array_equal(o[:, 21], ((A == 0) & (C == 0xFF)).any(axis=1).astype(U32)), "any_nul"
    assert np.array_equal(o[:, 22:38], A.astype(U32)), "byte_at"
    rows = 16 * LANE[:, None].astype(np.int64) + np.arange(16)
    assert np.array_equal(b4(o[:, 38:42]), ff(rows < SS[:, None])), "fast_valid_mask"
    cls = np.full(256, 0xFF, dtype=np.uint8)                   # class codes as msa_wave.hpp documents them
    for ch, code in zip(b"ACGN-T", (0, 1, 2, 4, 5, 7)):
        cls[ch] = code
    ind = spec._D_SET[A]
    assert np.array_equal(b4(o[:, 42:46])[ind], cls[A][ind]), "dna_classes"
    assert np.array_equal(o[:, 46] != 0, (~ind & (C == 0xFF)).any(axis=1)), "dna_bad"
    ids = np.where(C == 0xFF, A, 0)
    p2 = ((ids & 3).astype(U32) << (2 * np.arange(16, dtype=U32))).sum(axis=1).astype(U32)
    p4 = ((ids & 15).astype(np.uint64) << (4 * np.arange(16, dtype=np.uint64))).sum(axis=1)
    assert np.array_equal(o[:, 47], p2), "pack_gid2"
    assert np.array_equal(o[:, 48].astype(np.uint64) | (o[:, 49].astype(np.uint64) << 32), p4), "pack_gid4"
    for j, size in enumerate((8, 16, 32, 64)):                 # lutN at every index below its size
        idxs = A[:, :4]
        ok = (idxs < size).all(axis=1)
        assert ok.sum() > 200 and set(np.unique(idxs[ok])) == set(range(size)), size
        assert np.array_equal(b4(o[:, 50 + j:51 + j])[ok], table[idxs & 63][ok]), "lutN<%d>" % size
