// primitives_harness.hip — plain C launchers around the shared device primitives of csrc/dev_util.hpp and csrc/byte_ops.hpp,
// for tests/test_primitives_gpu.py only (edsparser_amd/libedsx_primitives.so).  Never loaded by the product.
// Every launcher takes device pointers and a stream, enqueues and returns the hipGetLastError() code; it allocates nothing
// and keeps no state: the test owns memory, poison, canaries and synchronisation.
#include "dev_util.hpp"

using namespace edsx;

namespace {

constexpr u64 NONE = ~0ull;
constexpr int MAX_N = 5;

template <int N>
int mscan(const u64* const* in, u64* const* out, u64* const* total, const u64* d_n, u64* tmp, hipStream_t st)
{
    ScanSet<N> a;
    for (int k = 0; k < N; k++) { a.in[k] = in[k]; a.out[k] = out[k]; a.total[k] = total[k]; }
    exclusive_scan_multi<N>(a, d_n, tmp, st);
    return (int)hipGetLastError();
}

__global__ void k_prim_last_le(const u64* __restrict__ a, const u64* __restrict__ lo, const u64* __restrict__ hi, const u64* __restrict__ x,
                               u64* __restrict__ out, u64 q)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < q) out[i] = last_le(a, lo[i], hi[i], x[i]);
}

// thread i: 16 bytes (nbytes[i] == 16) or the first nbytes[i] bytes, zero padded, of src + src_off[i] to dst + dst_off[i];
// the same 16 bytes once more through byte_of to out_bytes[16 i ..]
__global__ void k_prim_bytes16(const uint8_t* __restrict__ src, const u64* __restrict__ src_off, uint8_t* __restrict__ dst,
                               const u64* __restrict__ dst_off, const u32* __restrict__ nbytes, uint8_t* __restrict__ out_bytes, u64 q)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= q) return;
    const uint8_t* p = src + src_off[i];
    const uint4 v = nbytes[i] == 16 ? load16u(p) : load_partial(p, (int)nbytes[i]);
    store16u(dst + dst_off[i], v);
    for (int k = 0; k < 16; k++) out_bytes[16 * i + k] = (uint8_t)byte_of(v, k);
}

__global__ void k_prim_wave(const u64* __restrict__ in, u64* __restrict__ out_mbcnt, u64* __restrict__ out_sum, u64* __restrict__ out_lane)
{
    const u32 i = threadIdx.x;
    const u64 v = in[i];
    out_mbcnt[i] = mbcnt(ballot64(v & 1));
    out_sum[i] = wave_sum(v);
    out_lane[i] = lane_id();
}

__global__ void k_prim_byte_ops(const u32* __restrict__ a, const u32* __restrict__ b, u32* __restrict__ out_ne, u32* __restrict__ out_eq,
                                const u32* __restrict__ v, u32* __restrict__ out_nd, u64 q)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= q) return;
    out_ne[i] = ne_bytes4(a[i], b[i]);
    out_eq[i] = eq_byte4(a[i], b[i]);
    out_nd[i] = ndigits(v[i]);
}

// the harness's own statement of a write_set_ids policy: the ids are id_base + the bit's position, the bytes a plain loop
struct PlainIds {
    const u64* mask_;
    u32 id_base;
    __device__ __forceinline__ u64 mask(u32 w) const { return mask_[w]; }
    __device__ __forceinline__ u32 id(u32 w, u32 b) const { return id_base + 64u * w + b; }
    __device__ __forceinline__ u64 bytes(u32 w, u64 x) const
    {
        u64 n = 0;
        for (u32 b = 0; b < 64; b++)
            if ((x >> b) & 1) n += ndigits(id(w, b)) + 1;
        return n;
    }
};

// G lanes per set, 256 / G sets per block per round, the loop block-uniform (as k_sub_seds).  Set s: "a,b,c}" to
// sout[off[2 s] .. off[2 s + 1]); off[2 s] == ~0: not written, its lanes still shuffle.
__global__ void __launch_bounds__(256) k_prim_set_ids(const u64* __restrict__ rows, u32 W, u32 G, PlainIds pol, const u64* __restrict__ off, u64 nsets,
                                                      uint8_t* __restrict__ sout)
{
    const u32 g = threadIdx.x & (G - 1), per_block = 256 / G;
    for (u64 base = (u64)blockIdx.x * per_block; base < nsets; base += (u64)gridDim.x * per_block) {
        const u64 s = base + threadIdx.x / G;
        const u64 p0 = s < nsets ? off[2 * s] : NONE;
        const bool act = p0 != NONE;
        const u64 end = act ? off[2 * s + 1] : 0;
        write_set_ids(pol, rows + s * W, act, W, G, g, p0, end, sout);
    }
}

} // namespace

extern "C" {

// op 0: exclusive_scan_u64, op 1: inclusive_max_scan_u64
int prim_scan(int op, const u64* in, u64* out, const u64* d_n, u64* d_total, u64* tmp, hipStream_t st)
{
    if (op == 0) exclusive_scan_u64(in, out, d_n, d_total, tmp, st);
    else if (op == 1) inclusive_max_scan_u64(in, out, d_n, d_total, tmp, st);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

// exclusive_scan_multi<N>; in / out / total: host arrays of N device pointers
int prim_mscan(int N, const u64* const* in, u64* const* out, u64* const* total, const u64* d_n, u64* tmp, hipStream_t st)
{
    static_assert(MAX_N == 5, "one case per N below");
    switch (N) {
    case 1: return mscan<1>(in, out, total, d_n, tmp, st);
    case 2: return mscan<2>(in, out, total, d_n, tmp, st);
    case 3: return mscan<3>(in, out, total, d_n, tmp, st);
    case 4: return mscan<4>(in, out, total, d_n, tmp, st);
    case 5: return mscan<5>(in, out, total, d_n, tmp, st);
    }
    return (int)hipErrorInvalidValue;
}

int prim_last_le(const u64* a, const u64* lo, const u64* hi, const u64* x, u64* out, u64 q, hipStream_t st)
{
    if (q) hipLaunchKernelGGL(k_prim_last_le, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, st, a, lo, hi, x, out, q);
    return (int)hipGetLastError();
}

int prim_bytes16(const uint8_t* src, const u64* src_off, uint8_t* dst, const u64* dst_off, const u32* nbytes, uint8_t* out_bytes, u64 q,
                 hipStream_t st)
{
    if (q) hipLaunchKernelGGL(k_prim_bytes16, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, st, src, src_off, dst, dst_off, nbytes, out_bytes, q);
    return (int)hipGetLastError();
}

// one block of 256 threads: four waves
int prim_wave(const u64* in, u64* out_mbcnt, u64* out_sum, u64* out_lane, hipStream_t st)
{
    hipLaunchKernelGGL(k_prim_wave, dim3(1), dim3(256), 0, st, in, out_mbcnt, out_sum, out_lane);
    return (int)hipGetLastError();
}

int prim_byte_ops(const u32* a, const u32* b, u32* out_ne, u32* out_eq, const u32* v, u32* out_nd, u64 q, hipStream_t st)
{
    if (q) hipLaunchKernelGGL(k_prim_byte_ops, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, st, a, b, out_ne, out_eq, v, out_nd, q);
    return (int)hipGetLastError();
}

// rows: nsets rows of W words; mask: W words; off: 2 * nsets (begin, end) byte offsets into sout, begin == ~0 for no set
int prim_set_ids(const u64* rows, u32 W, u32 G, const u64* mask, u32 id_base, const u64* off, u64 nsets, uint8_t* sout, hipStream_t st)
{
    if (G == 0 || G > 64 || (G & (G - 1)) || W == 0) return (int)hipErrorInvalidValue;
    if (nsets) hipLaunchKernelGGL(k_prim_set_ids, dim3(grid_for(nsets * G, 16384)), dim3(256), 0, st, rows, W, G, PlainIds{mask, id_base}, off, nsets, sout);
    return (int)hipGetLastError();
}

// PinnedDownload::copy; synchronous.  -1: it threw
int prim_download(void* dst_host, const void* dev_src, size_t n, hipStream_t st)
{
    try {
        PinnedDownload::copy(dst_host, dev_src, n, st);
    } catch (const std::exception&) {
        return -1;
    }
    return (int)hipGetLastError();
}

} // extern "C"
