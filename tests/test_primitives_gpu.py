"""The shared device primitives of csrc/dev_util.hpp and csrc/byte_ops.hpp, called directly: the device-wide scans
(exclusive sum, inclusive max, N sums in one pass), write_set_ids, last_le, the 16-byte, byte and wave helpers and
PinnedDownload::copy, through the plain C launchers of tests/hip/primitives_harness.hip (edsparser_amd/libedsx_primitives.so,
built by edsparser_amd.build for the tests only).

Every expected value is computed by numpy or plain Python on the host.  Every device buffer a primitive writes lies between
two margins of 512 u64 of a known byte, its payload is filled with a poison byte (0x00, then 0xA5) before the call, and the
margins are compared after the call.  The scans get exactly the scratch that dev_util.hpp documents: ceil(n / 2048) u64
for one scan, N * (ceil(n / 2048) + 1) for N in one pass; the back margin begins right behind it."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("EDSX_PRIM_LIB") or os.path.join(ROOT, "edsparser_amd", "libedsx_primitives.so")   # (another build of the harness)
DEV = "cuda:0"
MARGIN = 512 * 8                 # bytes on either side of every written buffer
FENCE = 0x3C                     # what the margins hold
POISONS = (0x00, 0xA5)
TILE = 2048                      # SCAN_TILE
NONE = (1 << 64) - 1
U64 = np.uint64

_lib = None


def lib():
    global _lib
    if _lib is None:
        assert os.path.exists(LIB), "python -m edsparser_amd.build builds it"
        L = ctypes.CDLL(LIB)
        P, u32, u64, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
        L.prim_scan.argtypes = [I, P, P, P, P, P, P]
        L.prim_mscan.argtypes = [I, P, P, P, P, P, P]
        L.prim_last_le.argtypes = [P, P, P, P, P, u64, P]
        L.prim_bytes16.argtypes = [P, P, P, P, P, P, u64, P]
        L.prim_wave.argtypes = [P, P, P, P, P]
        L.prim_byte_ops.argtypes = [P, P, P, P, P, P, u64, P]
        L.prim_set_ids.argtypes = [P, u32, u32, P, u32, P, u64, P, P]
        L.prim_download.argtypes = [P, P, ctypes.c_size_t, P]
        for f in ("prim_scan", "prim_mscan", "prim_last_le", "prim_bytes16", "prim_wave", "prim_byte_ops", "prim_set_ids", "prim_download"):
            getattr(L, f).restype = I
        _lib = L
    return _lib


def stream():
    """the torch stream that is current: the launchers enqueue where the test's own fills and copies are enqueued"""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def sync():
    torch.cuda.current_stream().synchronize()


def dev(a):
    """a numpy array on the device (uint64 / uint32 travel as int64 / int32)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(DEV)


class Guarded:
    """nbytes of device memory filled with `poison`, between two margins of FENCE bytes"""

    def __init__(self, nbytes, poison):
        self.n = int(nbytes)
        self.t = torch.empty(2 * MARGIN + self.n, dtype=torch.uint8, device=DEV)
        assert self.t.data_ptr() % 16 == 0
        self.t[:MARGIN] = FENCE
        self.t[MARGIN + self.n:] = FENCE
        self.payload = self.t[MARGIN:MARGIN + self.n]
        self.payload.fill_(poison)
        self.ptr = self.t.data_ptr() + MARGIN

    def put(self, a, at=0):
        """host or device data into the payload, from byte `at`"""
        src = a if isinstance(a, torch.Tensor) else dev(a)
        if src.numel():
            src = src.contiguous().view(-1).view(torch.uint8)
            self.payload[at:at + src.numel()] = src
        return self

    def bytes(self):
        return self.payload.cpu().numpy()

    def u64(self):
        return self.bytes().view(U64)

    def check(self, what=""):
        front, back = self.t[:MARGIN].cpu().numpy(), self.t[MARGIN + self.n:].cpu().numpy()
        bad_f, bad_b = np.flatnonzero(front != FENCE), np.flatnonzero(back != FENCE)
        assert bad_f.size == 0, "%s: front margin written at byte offsets %s" % (what, (bad_f[:8] - MARGIN).tolist())
        assert bad_b.size == 0, "%s: back margin written at byte offsets +%s" % (what, bad_b[:8].tolist())


# ================================================================================================================
# scans
# ================================================================================================================
SCAN_N = [0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4096, 131071, 131072, 131073, 2097151, 2097152, 2097153,
          4194307]
MSCAN_N5 = [n for n in SCAN_N if n <= 2097153]
MSCAN_N14 = [0, 1, 2049, 131073, 2097153]


def ntiles_of(n):
    return (n + TILE - 1) // TILE


def edge_positions(n):
    """first, last, and the last / first elements of the tiles at the tile, 64-tile and 1024-tile edges and of the last tile"""
    last_tile = (n - 1) // TILE * TILE if n else 0
    pos = {0, n - 1, TILE - 1, TILE, 64 * TILE - 1, 64 * TILE, 1024 * TILE - 1, 1024 * TILE, last_tile - 1, last_tile}
    return sorted(p for p in pos if 0 <= p < n)


def scan_values(kind, n, salt=0):
    rng = np.random.default_rng(1000 * salt + n % 997 + 17)
    if kind == "ones":
        return np.full(n, 1 + salt, dtype=U64)                 # (array k of a multi-scan: all k + 1)
    if kind == "random":
        return rng.integers(0, 1 << 40, n, dtype=U64)          # the sum of 4 194 307 of them stays below 2^62
    if kind == "sparse":
        a = np.zeros(n, dtype=U64)
        for j, p in enumerate(edge_positions(n)):
            a[p] = (1 << 56) + ((salt * 131 + j * 7919 + 5) << 20) % (1 << 40)      # ten of them stay below 2^60
        return a
    i = np.arange(n, dtype=U64)
    if kind == "decreasing":
        return (U64(n) - i) << U64(33)
    if kind == "increasing":
        return (i + U64(1)) << U64(33)
    if kind == "max_first":
        a = rng.integers(0, 1 << 40, n, dtype=U64)
        if n:
            a[0] = 1 << 41
        return a
    raise ValueError(kind)


def scan_expect(op, a):
    """(out, total) of the scan of a, by numpy on uint64"""
    if len(a) == 0:
        return a.copy(), U64(0)
    if op == 0:
        cs = np.cumsum(a, dtype=U64)
        return np.concatenate([np.zeros(1, dtype=U64), cs[:-1]]), cs[-1]
    m = np.maximum.accumulate(a)
    return m, m[-1]


def run_scan(op, a, poison, inplace, what, want=None, d_a=None):
    """one call on fresh buffers; want = scan_expect(op, a) and d_a = dev(a) where the caller has them already"""
    n = len(a)
    d_a = dev(a) if d_a is None else d_a
    src = Guarded(8 * n, poison).put(d_a)
    out = src if inplace else Guarded(8 * n, poison)
    tmp, tot = Guarded(8 * ntiles_of(n), poison), Guarded(8, poison)
    d_n = dev(np.array([n], dtype=U64))
    rc = lib().prim_scan(op, src.ptr, out.ptr, d_n.data_ptr(), tot.ptr, tmp.ptr, stream())
    assert rc == 0, (what, rc)
    sync()
    want, want_total = want or scan_expect(op, a)
    got, got_total = out.u64(), tot.u64()[0]
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s: %d of %d wrong, first at %d (tile %d, item %d): got %#x want %#x"
                             % (what, bad.size, n, bad[0], bad[0] // TILE, bad[0] % TILE, got[bad[0]], want[bad[0]]))
    assert got_total == want_total, "%s: total %#x, want %#x" % (what, got_total, want_total)
    if not inplace:
        assert np.array_equal(src.u64(), a), what + ": the input changed"
    for g, name in ((src, "in"), (out, "out"), (tmp, "tmp"), (tot, "total")):
        g.check(what + " " + name)


def scan_kinds(op, n):
    kinds = ["ones", "random", "sparse"] + (["decreasing", "increasing", "max_first"] if op == 1 else [])
    return kinds if n else kinds[:1]


@pytest.mark.parametrize("n", SCAN_N)
@pytest.mark.parametrize("op", [0, 1], ids=["sum", "max"])
def test_scan(op, n):
    for kind in scan_kinds(op, n):
        a = scan_values(kind, n)
        want, d_a = scan_expect(op, a), dev(a)
        for poison in POISONS:
            for inplace in (False, True):
                run_scan(op, a, poison, inplace, "op %d n %d %s poison %#x %s" % (op, n, kind, poison, "in place" if inplace else "out of place"),
                         want, d_a)


def run_mscan(N, arrays, poison, inplace, what, wants=None):
    n = len(arrays[0])
    nt = ntiles_of(n)
    srcs = [Guarded(8 * n, poison).put(a) for a in arrays]
    outs = srcs if inplace else [Guarded(8 * n, poison) for _ in range(N)]
    tots = [Guarded(8, poison) for _ in range(N)]
    tmp = Guarded(8 * N * (nt + 1), poison)
    d_n = dev(np.array([n], dtype=U64))
    PA = ctypes.c_void_p * N
    rc = lib().prim_mscan(N, PA(*[s.ptr for s in srcs]), PA(*[o.ptr for o in outs]), PA(*[t.ptr for t in tots]), d_n.data_ptr(), tmp.ptr,
                          stream())
    assert rc == 0, (what, rc)
    sync()
    for k in range(N):
        want, want_total = wants[k] if wants else scan_expect(0, arrays[k])
        got, got_total = outs[k].u64(), tots[k].u64()[0]
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError("%s array %d: %d of %d wrong, first at %d (tile %d, item %d): got %#x want %#x"
                                 % (what, k, bad.size, n, bad[0], bad[0] // TILE, bad[0] % TILE, got[bad[0]], want[bad[0]]))
        assert got_total == want_total, "%s array %d: total %#x, want %#x" % (what, k, got_total, want_total)
        if not inplace:
            assert np.array_equal(srcs[k].u64(), arrays[k]), "%s array %d: the input changed" % (what, k)
    for g, name in [(tmp, "tmp")] + [(x, "in/out/total %d" % (i % N)) for i, x in enumerate(srcs + outs + tots)]:
        g.check(what + " " + name)


def mscan_arrays(kind, N, n):
    """every array its own contents: array k is class `kind` with its own salt"""
    return [scan_values(kind, n, salt=k) for k in range(N)]


@pytest.mark.parametrize("N,n", [(5, n) for n in MSCAN_N5] + [(N, n) for N in (1, 2, 3, 4) for n in MSCAN_N14])
def test_mscan(N, n):
    for kind in ("ones", "random", "sparse") if n else ("ones",):
        arrays = mscan_arrays(kind, N, n)
        wants = [scan_expect(0, a) for a in arrays]
        for poison in POISONS:
            for inplace in (False, True):
                run_mscan(N, arrays, poison, inplace, "N %d n %d %s poison %#x %s" % (N, n, kind, poison, "in place" if inplace else "out of place"),
                          wants)


def test_mscan_mixed_classes():
    """the five arrays of one call of five different kinds, so that a sum that lands in a neighbour's slot cannot cancel"""
    n = 131073
    kinds = ["random", "ones", "sparse", "random", "ones"]
    arrays = [scan_values(k, n, salt=i) for i, k in enumerate(kinds)]
    for poison in POISONS:
        run_mscan(5, arrays, poison, False, "mixed n %d poison %#x" % (n, poison))


@pytest.mark.parametrize("op", [0, 1], ids=["sum", "max"])
def test_scan_n_from_device_memory(op):
    """n = 4 194 307, then n = 9 on the same buffers with tmp as the first call left it: the second call reads its n from
    device memory, writes nine results and one tile sum, and nothing behind either"""
    big, small = 4194307, 9
    a = scan_values("random", big)
    for poison in POISONS:
        src, out = Guarded(8 * big, poison).put(a), Guarded(8 * big, poison)
        tmp, tot = Guarded(8 * ntiles_of(big), poison), Guarded(8, poison)
        d_n = dev(np.array([big], dtype=U64))
        assert lib().prim_scan(op, src.ptr, out.ptr, d_n.data_ptr(), tot.ptr, tmp.ptr, stream()) == 0
        sync()
        want, want_total = scan_expect(op, a)
        first, tmp_first = out.u64(), tmp.u64()
        assert np.array_equal(first, want) and tot.u64()[0] == want_total
        b = scan_values("max_first" if op else "random", small, salt=3)
        src.put(b)
        d_n.copy_(dev(np.array([small], dtype=U64)))
        assert lib().prim_scan(op, src.ptr, out.ptr, d_n.data_ptr(), tot.ptr, tmp.ptr, stream()) == 0
        sync()
        want_b, want_b_total = scan_expect(op, b)
        second, tmp_second = out.u64(), tmp.u64()
        assert np.array_equal(second[:small], want_b) and tot.u64()[0] == want_b_total
        assert np.array_equal(second[small:], first[small:]), "results behind n were written"
        assert np.array_equal(tmp_second[1:], tmp_first[1:]), "tile sums behind the one tile were written"
        for g in (src, out, tmp, tot):
            g.check("op %d poison %#x" % (op, poison))


def test_mscan_n_from_device_memory():
    """the same for five sums in one pass (whose scratch layout depends on n: array k's tile sums begin at k * (ntiles + 1))"""
    N, big, small = 5, 2097153, 9
    arrays = mscan_arrays("random", N, big)
    for poison in POISONS:
        srcs = [Guarded(8 * big, poison).put(a) for a in arrays]
        outs = [Guarded(8 * big, poison) for _ in range(N)]
        tots = [Guarded(8, poison) for _ in range(N)]
        tmp = Guarded(8 * N * (ntiles_of(big) + 1), poison)
        d_n = dev(np.array([big], dtype=U64))
        PA = ctypes.c_void_p * N
        args = (N, PA(*[s.ptr for s in srcs]), PA(*[o.ptr for o in outs]), PA(*[t.ptr for t in tots]), d_n.data_ptr(), tmp.ptr)
        assert lib().prim_mscan(*args, stream()) == 0
        sync()
        first = [o.u64() for o in outs]
        for k in range(N):
            want, want_total = scan_expect(0, arrays[k])
            assert np.array_equal(first[k], want) and tots[k].u64()[0] == want_total, k
        tmp_first = tmp.u64()
        small_arrays = mscan_arrays("random", N, small)
        for s, b in zip(srcs, small_arrays):
            s.put(b)
        d_n.copy_(dev(np.array([small], dtype=U64)))
        assert lib().prim_mscan(*args, stream()) == 0
        sync()
        tmp_second = tmp.u64()
        for k in range(N):
            want, want_total = scan_expect(0, small_arrays[k])
            second = outs[k].u64()
            assert np.array_equal(second[:small], want) and tots[k].u64()[0] == want_total, k
            assert np.array_equal(second[small:], first[k][small:]), "array %d: results behind n were written" % k
        # one tile: array k's one tile sum is tmp[2 k]; every other slot is as the first call left it
        keep = np.ones(tmp_first.size, dtype=bool)
        keep[[2 * k for k in range(N)]] = False
        assert np.array_equal(tmp_second[keep], tmp_first[keep]), "scratch outside the N tile sums was written"
        for g in srcs + outs + tots + [tmp]:
            g.check("mscan poison %#x" % poison)


# ================================================================================================================
# last_le
# ================================================================================================================
def run_last_le(length, seed, poison):
    rng = np.random.default_rng(seed)
    # runs of equal values, neighbours at least 4 apart, so that x can fall between two runs
    a = np.sort(rng.integers(1, max(2, length // 3 + 1) + 1, length)).astype(U64) * U64(4)
    run_first = np.flatnonzero(np.concatenate([[True], a[1:] != a[:-1]]))
    run_last = np.flatnonzero(np.concatenate([a[1:] != a[:-1], [True]]))
    windows = [(0, length - 1), (0, 0), (length - 1, length - 1)]
    for _ in range(200 if length > 3 else 8):
        lo = int(rng.integers(0, length))
        windows.append((lo, int(rng.integers(lo, length))))
        windows.append((lo, lo))                                                     # lo == hi
        if length >= 3:
            lo = int(rng.integers(1, length - 1))
            windows.append((lo, int(rng.integers(lo, length - 1))))                  # strictly inside the array
    los, his, xs = [], [], []
    for lo, hi in windows:
        cand = {int(a[lo]), int(a[hi]), int(a[hi]) + 1, int(a[hi]) + 1000, NONE, int(a[(lo + hi) // 2]), int(a[(lo + hi) // 2]) + 1,
                int(a[(lo + hi) // 2]) + 3}
        inside_f = run_first[(run_first >= lo) & (run_first <= hi)]
        inside_l = run_last[(run_last >= lo) & (run_last <= hi)]
        for k in list(inside_f[:3]) + list(inside_f[-3:]) + list(inside_l[:3]) + list(inside_l[-3:]):
            cand.update((int(a[k]), int(a[k]) + 2))                                  # first / last element of a run, and just above it
        for x in cand:
            if x >= int(a[lo]):                                                      # the contract: a[lo] <= x
                los.append(lo), his.append(hi), xs.append(x)
    q = len(xs)
    los, his, xs = np.array(los, dtype=U64), np.array(his, dtype=U64), np.array(xs, dtype=U64)
    want = np.array([lo + np.searchsorted(a[lo:hi + 1], x, side="right") - 1 for lo, hi, x in zip(los.astype(np.int64), his.astype(np.int64), xs)],
                    dtype=U64)
    assert np.all(want >= los) and np.all(want <= his)
    d_a, d_lo, d_hi, d_x = dev(a), dev(los), dev(his), dev(xs)
    out = Guarded(8 * q, poison)
    assert lib().prim_last_le(d_a.data_ptr(), d_lo.data_ptr(), d_hi.data_ptr(), d_x.data_ptr(), out.ptr, q, stream()) == 0
    sync()
    got = out.u64()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "length %d: query lo %d hi %d x %d: got %d want %d" % (length, los[bad[0]], his[bad[0]], xs[bad[0]], got[bad[0]], want[bad[0]])
    out.check("last_le")
    return q


@pytest.mark.parametrize("length", [1, 2, 3, 1000, 100001])
def test_last_le(length):
    for poison in POISONS:
        assert run_last_le(length, 7 + length, poison) >= 3


# ================================================================================================================
# load16u / store16u / load_partial / byte_of
# ================================================================================================================
SLOT = 48       # bytes of dst per thread: its 16 at offset 16 + alignment, poison around them


def run_bytes16(L, poison):
    """a source of L >= 64 bytes whose payload ends at the front of a margin: full 16-byte moves for every source x destination
    alignment, and partial loads of n = 0..15 bytes that end exactly where the payload ends"""
    rng = np.random.default_rng(L)
    data = rng.integers(1, 256, L, dtype=np.uint8)                                   # no zero byte: zero padding cannot come from it
    src = Guarded(L, 0).put(data)
    assert src.ptr % 16 == 0
    so, do, nb = [], [], []
    for sa in range(16):
        for da in range(16):
            so.append(sa + 16 * (da % 2)), do.append(SLOT * len(do) + 16 + da), nb.append(16)
    so.append(L - 16), do.append(SLOT * len(do) + 16), nb.append(16)                 # the last 16 bytes of the payload
    for n in range(16):
        so.append(L - n), do.append(SLOT * len(do) + 16 + (n * 7) % 16), nb.append(n)
    q = len(so)
    dst, outb = Guarded(SLOT * q + 16, poison), Guarded(16 * q, poison)
    d_so, d_do, d_nb = dev(np.array(so, dtype=U64)), dev(np.array(do, dtype=U64)), dev(np.array(nb, dtype=np.uint32))
    assert lib().prim_bytes16(src.ptr, d_so.data_ptr(), dst.ptr, d_do.data_ptr(), d_nb.data_ptr(), outb.ptr, q, stream()) == 0
    sync()
    want_dst = np.full(SLOT * q + 16, poison, dtype=np.uint8)
    want_b = np.zeros(16 * q, dtype=np.uint8)
    for i in range(q):
        v = np.zeros(16, dtype=np.uint8)
        v[:nb[i]] = data[so[i]:so[i] + nb[i]]
        want_dst[do[i]:do[i] + 16] = v
        want_b[16 * i:16 * i + 16] = v
    got_dst, got_b = dst.bytes(), outb.bytes()
    bad = np.flatnonzero(got_dst != want_dst)
    assert bad.size == 0, "L %d: dst byte %d (thread %d, src alignment %d, n %d): got %#x want %#x" % (
        L, bad[0], bad[0] // SLOT, so[min(bad[0] // SLOT, q - 1)] % 16, nb[min(bad[0] // SLOT, q - 1)], got_dst[bad[0]], want_dst[bad[0]])
    bad = np.flatnonzero(got_b != want_b)
    assert bad.size == 0, "L %d: byte_of(v, %d) of thread %d: got %#x want %#x" % (L, bad[0] % 16, bad[0] // 16, got_b[bad[0]], want_b[bad[0]])
    assert np.array_equal(src.bytes(), data)
    for g in (src, dst, outb):
        g.check("bytes16")
    return {(s % 16, n) for s, n in zip(so, nb) if n < 16}


def test_bytes16():
    """L = 64..79: the partial loads, which end at the payload's end, begin at every alignment for every n"""
    seen = set()
    for L in range(64, 80):
        for poison in POISONS:
            seen |= run_bytes16(L, poison)
    assert seen == {(sa, n) for sa in range(16) for n in range(16)}


# ================================================================================================================
# lane_id / mbcnt / ballot64 / wave_sum
# ================================================================================================================
def wave_masks():
    rng = np.random.default_rng(5)
    rnd = [int(x) for x in rng.integers(0, 1 << 63, 2, dtype=np.int64)]
    masks = [0, NONE, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA, 1, 1 << 63, (1 << 31) | (1 << 32), rnd[0] | 1, rnd[1] << 1]
    return masks + [rnd[0] ^ rnd[1]] * (-len(masks) % 4)


def run_wave(masks4, poison, seed):
    rng = np.random.default_rng(seed)
    bits = np.array([(m >> i) & 1 for m in masks4 for i in range(64)], dtype=U64)
    vals = ((rng.integers((1 << 40) - 4096, (1 << 40) + 4096, 256, dtype=U64)) & ~U64(1)) | bits
    outs = [Guarded(8 * 256, poison) for _ in range(3)]
    d_in = dev(vals)
    assert lib().prim_wave(d_in.data_ptr(), outs[0].ptr, outs[1].ptr, outs[2].ptr, stream()) == 0
    sync()
    want_cnt = np.concatenate([np.concatenate([np.zeros(1, dtype=U64), np.cumsum(bits[64 * w:64 * w + 64], dtype=U64)[:-1]]) for w in range(4)])
    want_sum = np.repeat([vals[64 * w:64 * w + 64].sum(dtype=U64) for w in range(4)], 64).astype(U64)
    assert np.array_equal(outs[0].u64(), want_cnt), ("mbcnt", [hex(m) for m in masks4])
    assert np.array_equal(outs[1].u64(), want_sum), ("wave_sum", [hex(m) for m in masks4])
    assert np.array_equal(outs[2].u64(), np.arange(256, dtype=U64) % U64(64)), "lane_id"
    for g in outs:
        g.check("wave")


def test_wave():
    masks = wave_masks()
    for i in range(0, len(masks), 4):
        for poison in POISONS:
            run_wave(masks[i:i + 4], poison, i)


# ================================================================================================================
# ne_bytes4 / eq_byte4 / ndigits: the device compilation of byte_ops.hpp (the host one: tests/test_primitives_cpu.py)
# ================================================================================================================
def byte_op_cases(nrandom):
    a, b = [], []
    edge = [(0x00, 0x80), (0x7f, 0xff), (0x80, 0x80), (0x00, 0x00), (0xff, 0xff), (0x00, 0xff), (0x7f, 0x80), (0x01, 0x00), (0x80, 0x00)]
    for x, y in edge:
        for k in range(4):
            rest = 0x55555555 & ~(0xff << (8 * k))
            a += [x << (8 * k), y << (8 * k), (x << (8 * k)) | rest]
            b += [y << (8 * k), x << (8 * k), (y << (8 * k)) | rest]
        a.append(x * 0x01010101), b.append(y * 0x01010101)
    a += [0x12345678, 0x12345678, 0x00000000, 0x7f7f7f7f, 0x80808080]
    b += [0x12345678, 0x87654321, 0x80808080, 0xffffffff, 0x80808080]
    rng = np.random.default_rng(11)
    a = np.concatenate([np.array(a, dtype=np.uint32), rng.integers(0, 1 << 32, nrandom, dtype=np.uint32)])
    b = np.concatenate([np.array(b, dtype=np.uint32), rng.integers(0, 1 << 32, nrandom, dtype=np.uint32)])
    # every byte position with equal bytes next to different ones, at random
    same = rng.integers(0, 16, a.size, dtype=np.uint32)
    keep = sum(((same >> k) & 1) * np.uint32(0xff << (8 * k)) for k in range(4)).astype(np.uint32)
    half = a.size // 2
    b[half:] = (b[half:] & ~keep[half:]) | (a[half:] & keep[half:])
    v = [1, 2, 9, 4294967295, 4294967294, 2147483648]
    for p in range(1, 10):
        v += [10 ** p - 1, 10 ** p, 10 ** p + 1]
    v = np.concatenate([np.array(v, dtype=np.uint32), np.maximum(1, rng.integers(0, 1 << 32, a.size - len(v), dtype=np.uint32) >> rng.integers(0, 32, a.size - len(v), dtype=np.uint32))])
    return a, b, v.astype(np.uint32)


def run_byte_ops(nrandom, poison):
    a, b, v = byte_op_cases(nrandom)
    q = a.size
    want_ne = np.zeros(q, dtype=np.uint32)
    for k in range(4):
        want_ne |= (((a >> np.uint32(8 * k)) & np.uint32(0xff)) != ((b >> np.uint32(8 * k)) & np.uint32(0xff))).astype(np.uint32) << np.uint32(k)
    want_nd = (np.searchsorted(np.array([10 ** p for p in range(1, 10)], dtype=np.uint64), v.astype(np.uint64), side="right") + 1).astype(np.uint32)
    assert want_nd[3] == 10 and [len(str(int(x))) for x in v[:40]] == want_nd[:40].tolist()
    d_a, d_b, d_v = dev(a), dev(b), dev(v)
    outs = [Guarded(4 * q, poison) for _ in range(3)]
    assert lib().prim_byte_ops(d_a.data_ptr(), d_b.data_ptr(), outs[0].ptr, outs[1].ptr, d_v.data_ptr(), outs[2].ptr, q, stream()) == 0
    sync()
    ne, eq, nd = (o.bytes().view(np.uint32) for o in outs)
    bad = np.flatnonzero(ne != want_ne)
    assert bad.size == 0, "ne_bytes4(%#x, %#x) = %#x, want %#x" % (a[bad[0]], b[bad[0]], ne[bad[0]], want_ne[bad[0]])
    bad = np.flatnonzero(eq != (want_ne ^ np.uint32(0xF)))
    assert bad.size == 0, "eq_byte4(%#x, %#x) = %#x, want %#x" % (a[bad[0]], b[bad[0]], eq[bad[0]], want_ne[bad[0]] ^ 0xF)
    bad = np.flatnonzero(nd != want_nd)
    assert bad.size == 0, "ndigits(%d) = %d, want %d" % (v[bad[0]], nd[bad[0]], want_nd[bad[0]])
    for g in outs:
        g.check("byte_ops")


def test_byte_ops_device():
    for poison in POISONS:
        run_byte_ops(1000000, poison)


# ================================================================================================================
# write_set_ids
# ================================================================================================================
SET_G = [1, 2, 4, 8, 16, 32, 64]


def set_widths(G):
    ws = {1, max(1, G - 1), G, G + 1, 3 * G + 1}
    if G in (1, 64):
        ws |= {157, 1563}                        # ids across 9|10, 99|100, 999|1000, 9 999|10 000 (157 words) and 99 999|100 000 (1563)
    return sorted(ws)


def set_rows(W, G, rng):
    """the sets as rows of W words, and which of them are written"""
    per_block = 256 // G
    big = W > 100
    nsets = 41 if big else max(2 * per_block + 1, 41)                                # (wide sets: few, the reference text is host work)
    while nsets % per_block == 0:
        nsets += 1                                                                   # the last block is partly filled
    rows = np.zeros((nsets, W), dtype=U64)
    full = np.full(W, NONE, dtype=U64)

    def bit(p):
        r = np.zeros(W, dtype=U64)
        r[p // 64] = U64(1) << U64(p % 64)
        return r

    def rand(density):
        return np.packbits(rng.random((W, 64)) < density, axis=1, bitorder="little").view(U64).reshape(W)

    shapes = [np.zeros(W, dtype=U64), full, bit(0), bit(63), bit(min(64, 64 * W - 1)), bit(64 * W - 1), rand(0.5), rand(0.03), bit(1),
              bit(0) | bit(64 * W - 1), rand(0.9), np.zeros(W, dtype=U64)]
    for s in range(nsets):
        if s < len(shapes):
            rows[s] = shapes[s]
        elif big:
            rows[s] = rand(float(rng.choice([0.0, 0.002, 0.02, 0.2])))
        else:
            rows[s] = rand(float(rng.choice([0.0, 0.05, 0.5, 1.0])))
    # unwritten sets between written ones inside one wave and inside one aligned pair of groups: every other set of the
    # first eight, pairs in the next eight, twelve written ones, then at random
    written = rng.random(nsets) < 0.7
    for s in range(16):
        written[s] = s % 2 == 0 if s < 8 else (s // 2) % 2 == 1
    written[16:28] = True
    # the special shapes at written places drawn at random, so that over the cases they meet every group of lanes
    order = np.arange(nsets)
    at = rng.permutation(np.flatnonzero(written))[:len(shapes)]
    for s, p in enumerate(at):
        q = int(np.flatnonzero(order == s)[0])
        order[q], order[p] = order[p], order[q]
    return rows[order], written


def set_text(row, mask, id_base):
    x = row & mask
    if not x.any():
        return b""                                                                   # write_set_ids writes nothing for an empty set
    bits = np.unpackbits(x.view(np.uint8), bitorder="little")
    ids = np.flatnonzero(bits) + id_base
    return (",".join(map(str, ids.tolist())) + "}").encode()


def run_set_ids(G, W, rows, written, mask, id_base, poison, what):
    nsets = rows.shape[0]
    texts = [set_text(rows[s], mask, id_base) if written[s] else b"" for s in range(nsets)]
    off = np.full(2 * nsets, NONE, dtype=U64)
    pos = 5
    for s in range(nsets):
        if written[s]:
            off[2 * s], off[2 * s + 1] = pos, pos + len(texts[s])
            pos += len(texts[s]) + s % 4                                             # 0..3 bytes that stay poison
    total = pos + 3
    want = np.full(total, poison, dtype=np.uint8)
    for s in range(nsets):
        if texts[s]:
            want[int(off[2 * s]):int(off[2 * s + 1])] = np.frombuffer(texts[s], dtype=np.uint8)
    sout = Guarded(total, poison)
    d_rows, d_mask, d_off = dev(rows.reshape(-1)), dev(mask), dev(off)
    assert lib().prim_set_ids(d_rows.data_ptr(), W, G, d_mask.data_ptr(), id_base, d_off.data_ptr(), nsets, sout.ptr, stream()) == 0
    sync()
    got = sout.bytes()
    if not np.array_equal(got, want):
        p = int(np.flatnonzero(got != want)[0])
        s = max(i for i in range(nsets) if written[i] and int(off[2 * i]) <= p) if p >= 5 else -1
        raise AssertionError("%s: byte %d (set %d, its bytes [%d, %d)): got %r want %r" % (
            what, p, s, int(off[2 * s]), int(off[2 * s + 1]), bytes(got[max(0, p - 12):p + 12]), bytes(want[max(0, p - 12):p + 12])))
    sout.check(what)


@pytest.mark.parametrize("G", SET_G)
def test_set_ids(G):
    for W in set_widths(G):
        rng = np.random.default_rng(100 * G + W)
        rows, written = set_rows(W, G, rng)
        ones = np.full(W, NONE, dtype=U64)
        own = ones.copy()
        own[0] &= ~U64(1)                                                            # id 0 is never written (OwnIds of the slice)
        rmask = rng.integers(0, 1 << 63, W, dtype=np.int64).view(U64) << U64(1) | rng.integers(0, 2, W, dtype=np.int64).view(U64)
        configs = [(0, own), (1, ones), (0, rmask & own), (1, rmask)]
        if W > 100:
            configs = configs[:3]
        for id_base, mask in configs:
            for poison in POISONS:
                run_set_ids(G, W, rows, written, mask, id_base, poison, "G %d W %d id_base %d poison %#x" % (G, W, id_base, poison))


# ================================================================================================================
# PinnedDownload::copy
# ================================================================================================================
MiB = 1 << 20
DOWNLOAD_N = [0, 1, 16 * MiB - 1, 16 * MiB, 32 * MiB, 32 * MiB + 1, 64 * MiB + 65, 96 * MiB - 63]
_source = None


def download_source():
    """96 MiB of device bytes from a position hash, made once"""
    global _source
    if _source is None:
        i = torch.arange(96 * MiB, dtype=torch.int64, device=DEV)
        _source = ((((i * 0x9E3779B1 + 0x7F4A7C15) >> 11) ^ (i >> 3) ^ i) & 0xFF).to(torch.uint8)
        del i
    return _source


@pytest.mark.parametrize("n", DOWNLOAD_N)
def test_pinned_download(n):
    src = download_source()[:n] if n else download_source()[:1]
    want = src[:n].cpu().numpy()
    if n > 4096:
        assert len(np.unique(want[:4096])) > 100                                     # the source is not a constant
    tail = 4096
    for shift in (0, 1, 63):
        for poison in POISONS:
            raw = np.full(n + 64 + 64 + tail, poison, dtype=np.uint8)
            base = (-raw.ctypes.data) % 64 + shift                                   # 0, 1 and 63 bytes behind a 64-byte boundary
            assert lib().prim_download(raw.ctypes.data + base, src.data_ptr(), n, stream()) == 0
            assert np.array_equal(raw[base:base + n], want), "n %d shift %d: first difference at byte %d" % (
                n, shift, int(np.flatnonzero(raw[base:base + n] != want)[0]))
            assert np.all(raw[:base] == poison) and np.all(raw[base + n:] == poison), "n %d shift %d: bytes around the destination written" % (n, shift)
    if n:
        assert not np.all(want == POISONS[0]) and not np.all(want == POISONS[1])


# ================================================================================================================
# every entry point once on a stream of the test's own, its inputs produced on that stream
# ================================================================================================================
def test_non_default_stream():
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    with torch.cuda.stream(s):
        assert stream().value == s.cuda_stream
        n = 131073
        run_scan(0, scan_values("random", n), 0xA5, False, "stream sum")
        run_scan(1, scan_values("max_first", n), 0xA5, True, "stream max")
        run_mscan(3, mscan_arrays("random", 3, n), 0xA5, False, "stream mscan")
        run_last_le(1000, 3, 0xA5)
        run_bytes16(64 + 5, 0xA5)
        run_wave(wave_masks()[4:8], 0xA5, 1)
        run_byte_ops(4096, 0xA5)
        rng = np.random.default_rng(9)
        rows, written = set_rows(9, 8, rng)
        run_set_ids(8, 9, rows, written, np.full(9, NONE, dtype=U64), 1, 0xA5, "stream set ids")
        m = 32 * MiB + 1
        src = download_source()[7:7 + m] + 0                                         # a copy made on this stream
        raw = np.full(m + 64, 0xA5, dtype=np.uint8)
        assert lib().prim_download(raw.ctypes.data, src.data_ptr(), m, stream()) == 0
        assert np.array_equal(raw[:m], src.cpu().numpy()) and np.all(raw[m:] == 0xA5)
    s.synchronize()
