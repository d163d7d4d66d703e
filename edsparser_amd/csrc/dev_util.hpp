// dev_util.hpp — small device/host helpers shared by the gfx950 kernels (wave64 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "draw.hpp"
#include "byte_ops.hpp"
#include "errors.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>

namespace edsx {

// DeviceError: errors.hpp
struct OutOfDeviceMemory : DeviceError { using DeviceError::DeviceError; };     // hipMalloc said so: the caller may retry with less

#define EDSX_HIP(call)                                                                        \
    do {                                                                                      \
        hipError_t e__ = (call);                                                              \
        if (e__ != hipSuccess)                                                                \
            throw ::edsx::DeviceError(std::string(#call) + ": " + hipGetErrorString(e__));    \
    } while (0)

typedef unsigned long long u64;
typedef unsigned int u32;

// ---- large device-to-host copies ----------------------------------------------------------------------
// hipMemcpy into pageable memory is copied out of the runtime's staging buffer by ONE host thread (≈18 GB/s into
// huge-page-backed memory on this stack), well under what the link gives a pinned destination.  Outputs of this
// engine are GB-sized text, so large downloads go through two pinned staging chunks: the DMA of chunk i+1 overlaps
// the copy of chunk i into the caller's buffer by several host threads.  Synchronous: returns when dst is complete.
class PinnedDownload {
public:
    static void copy(void* dst, const void* dev_src, size_t n, hipStream_t st)
    {
        if (n < MIN_BYTES) {
            if (n) EDSX_HIP(hipMemcpyAsync(dst, dev_src, n, hipMemcpyDeviceToHost, st));
            EDSX_HIP(hipStreamSynchronize(st));
            return;
        }
        // one set of staging buffers and events per device (events belong to the device that is current when they
        // are created; contexts on different GPUs of one process download side by side)
        int dev = 0;
        EDSX_HIP(hipGetDevice(&dev));
        static Stage stages[MAX_DEVICES];
        if (dev < 0 || dev >= MAX_DEVICES) {
            EDSX_HIP(hipMemcpyAsync(dst, dev_src, n, hipMemcpyDeviceToHost, st));
            EDSX_HIP(hipStreamSynchronize(st));
            return;
        }
        Stage& sg = stages[dev];
        std::lock_guard<std::mutex> lock(sg.mu);
        sg.ensure();
        uint8_t* out = static_cast<uint8_t*>(dst);
        const uint8_t* src = static_cast<const uint8_t*>(dev_src);
        const size_t nchunks = (n + CHUNK - 1) / CHUNK;
        auto issue = [&](size_t i) {
            const size_t off = i * CHUNK, len = std::min(CHUNK, n - off);
            EDSX_HIP(hipMemcpyAsync(sg.pin[i & 1], src + off, len, hipMemcpyDeviceToHost, st));
            EDSX_HIP(hipEventRecord(sg.ev[i & 1], st));
        };
        issue(0);
        for (size_t i = 0; i < nchunks; i++) {
            if (i + 1 < nchunks) issue(i + 1);
            EDSX_HIP(hipEventSynchronize(sg.ev[i & 1]));
            const size_t off = i * CHUNK, len = std::min(CHUNK, n - off);
            const uint8_t* from = sg.pin[i & 1];
            std::thread th[THREADS - 1];
            const size_t part = ((len + THREADS - 1) / THREADS + 63) & ~(size_t)63;     // THREADS * part >= len
            for (unsigned t = 1; t < THREADS; t++) {
                const size_t lo = std::min(len, part * t), hi = std::min(len, part * (t + 1));
                th[t - 1] = std::thread([=] { if (hi > lo) std::memcpy(out + off + lo, from + lo, hi - lo); });
            }
            std::memcpy(out + off, from, std::min(len, part));
            for (auto& x : th) x.join();
        }
    }

private:
    static constexpr size_t MIN_BYTES = (size_t)16 << 20, CHUNK = (size_t)32 << 20;
    static constexpr unsigned THREADS = 8;
    static constexpr int MAX_DEVICES = 16;
    struct Stage {
        std::mutex mu;
        uint8_t* pin[2] = {nullptr, nullptr};
        hipEvent_t ev[2];
        bool ready = false;
        void ensure()
        {
            if (ready) return;
            for (int k = 0; k < 2; k++) {
                EDSX_HIP(hipHostMalloc(reinterpret_cast<void**>(&pin[k]), CHUNK, hipHostMallocPortable));
                EDSX_HIP(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
            }
            ready = true;
        }
    };
};

// The device tokenisers keep a few u64 per input byte (flags and their scans): fine for the GB-sized texts they are
// meant for, but a text whose scratch would not fit comfortably is left to the host tokenisers instead of failing.
inline bool device_scratch_fits(size_t bytes)
{
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
    return bytes <= free_b / 2;
}

// ---- host-side launch helpers ----------------------------------------------------------------------------
inline double since_ms(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// two device events around a stretch of a stream; ms() after the stream has been synchronised
struct EventPair {
    hipEvent_t a, b;
    EventPair() { EDSX_HIP(hipEventCreate(&a)); EDSX_HIP(hipEventCreate(&b)); }
    ~EventPair() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); }
    float ms() const { float v = 0; EDSX_HIP(hipEventElapsedTime(&v, a, b)); return v; }
};

// blocks of 256 threads for a grid-stride kernel over `work` items, at most `cap`
inline unsigned grid_for(u64 work, u64 cap) { return (unsigned)std::max<u64>(1, std::min<u64>((work + 255) / 256, cap)); }

// ---- wave64 primitives -------------------------------------------------------------------
__device__ __forceinline__ u32 lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
// number of set bits of `mask` strictly below this lane
__device__ __forceinline__ u32 mbcnt(u64 mask)
{
    return __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
}
__device__ __forceinline__ u64 ballot64(bool p) { return __ballot(p); }
// the sum of v over the 64 lanes, in every lane
__device__ __forceinline__ u64 wave_sum(u64 v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the last k in [lo, hi] with a[k] <= x, given a[lo] <= x
__device__ __forceinline__ u64 last_le(const u64* __restrict__ a, u64 lo, u64 hi, u64 x)
{
    while (lo < hi) { const u64 mid = lo + ((hi - lo + 1) >> 1); if (a[mid] <= x) lo = mid; else hi = mid - 1; }
    return lo;
}

// The ids of one source set as decimal text, "a,b,c}", by the G lanes (a power of two, lane g of them) that share the set:
// lane g takes the words g, g + G, ... of `row` (!act: no set, but the lane still takes part in the shuffles).  Per round
// every lane counts the bytes of its word, a shuffle scan inside the group places them behind `cur`, and the lane writes
// its ids, each followed by a comma or, where the set ends (`end`: one past the closing brace), the brace.  pol:
//   mask(w)      the bits of word w that count          bytes(w, x)  the text bytes of the ids of x, separators included
//   id(w, b)     the number written for bit b of word w
template <class Policy>
__device__ __forceinline__ void write_set_ids(const Policy& pol, const u64* __restrict__ row, bool act, u32 W, u32 G, u32 g, u64 cur, u64 end,
                                              uint8_t* __restrict__ sout)
{
    for (u32 wb = 0; wb < W; wb += G) {
        const u32 w = wb + g;
        u64 x = (act && w < W) ? row[w] & pol.mask(w) : 0;
        const u64 nb = pol.bytes(w < W ? w : 0, x);
        u64 incl = nb;
        for (u32 o = 1; o < G; o <<= 1) { const u64 t = __shfl_up(incl, o, 64); if (g >= o) incl += t; }
        const u64 total = __shfl(incl, (int)((threadIdx.x & 63u) | (G - 1)), 64);
        u64 p = cur + incl - nb;
        while (x) {
            const u32 b = (u32)__builtin_ctzll(x);
            x &= x - 1;
            u32 v = pol.id(w, b);
            const u32 dg = ndigits(v);
            for (u32 k = dg; k-- > 0;) { sout[p + k] = (uint8_t)('0' + v % 10u); v /= 10u; }
            p += dg;
            sout[p] = p + 1 == end ? '}' : ',';
            p++;
        }
        cur += total;
    }
}

// mix64 / hash3 (splitmix64): draw.hpp, shared with the host library

// 16 bytes from an arbitrarily aligned address (gfx950 global loads tolerate misalignment;
// hipcc emits one global_load_dwordx4 for this)
struct __attribute__((packed, aligned(1))) U128u { uint32_t x, y, z, w; };
__device__ __forceinline__ uint4 load16u(const uint8_t* p)
{
    U128u v;
    __builtin_memcpy(&v, p, 16);
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void store16u(uint8_t* p, const uint4& v)   // 16 bytes to an arbitrarily aligned address
{
    U128u t{v.x, v.y, v.z, v.w};
    __builtin_memcpy(p, &t, 16);
}
// partial load of n (<16) bytes, zero padded
__device__ __forceinline__ uint4 load_partial(const uint8_t* p, int n)
{
    u64 lo = 0, hi = 0;
    for (int i = 0; i < n; i++) {
        u64 b = p[i];
        if (i < 8) lo |= b << (8 * i);
        else hi |= b << (8 * (i - 8));
    }
    return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}

// ne_bytes4 / eq_byte4 (per-byte compare masks of a dword) and ndigits: byte_ops.hpp, shared with host-compiled code

__device__ __forceinline__ u32 byte_of(const uint4& v, int i)
{
    uint32_t w = (i < 8) ? ((i < 4) ? v.x : v.y) : ((i < 12) ? v.z : v.w);
    return (w >> ((i & 3) * 8)) & 0xffu;
}

// ---- device-wide scans on u64 arrays, element count read from device memory -----------------
// OP 0: exclusive sum (out[i] = sum(in[0..i)), *total = sum of all)
// OP 1: inclusive max (out[i] = max(in[0..i]),  *total = max of all)
// in/out may alias (they are not __restrict__: callers scan in place).  Three grid-stride kernels.  tmp: exactly
// ceil(n / SCAN_TILE) u64, one sum per tile; nothing behind them is read or written, and n = 0 touches none
// (tests/test_primitives_gpu.py gives the scans this much and no more).
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;   // 2048

template <int OP> __device__ __forceinline__ u64 scan_op(u64 a, u64 b) { return OP == 0 ? a + b : (a > b ? a : b); }

template <int OP>
__device__ __forceinline__ u64 block_reduce(u64 v, u64* sh /*[SCAN_THREADS/64]*/)
{
    for (int o = 32; o > 0; o >>= 1) v = scan_op<OP>(v, __shfl_down(v, o, 64));
    int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    u64 t = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); i++) t = scan_op<OP>(t, sh[i]);
    __syncthreads();
    return t;
}

template <int OP>
static __global__ void k_scan_tile_sums(const u64* in, const u64* __restrict__ n_ptr,
                                        u64* __restrict__ bsum)
{
    __shared__ u64 sh[SCAN_THREADS / 64];
    const u64 n = *n_ptr;
    const u64 ntiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        u64 base = t * SCAN_TILE;
        u64 s = 0;
        for (int i = 0; i < SCAN_ITEMS; i++) {
            u64 idx = base + (u64)i * SCAN_THREADS + threadIdx.x;
            if (idx < n) s = scan_op<OP>(s, in[idx]);
        }
        s = block_reduce<OP>(s, sh);
        if (threadIdx.x == 0) bsum[t] = s;
    }
}

// single workgroup: exclusive scan of bsum[0..ntiles) in place, total -> *total
template <int OP>
static __global__ void k_scan_spine(u64* __restrict__ bsum, const u64* __restrict__ n_ptr,
                                    u64* __restrict__ total)
{
    __shared__ u64 sh[1024];
    __shared__ u64 carry_sh;
    const u64 n = *n_ptr;
    const u64 ntiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    if (threadIdx.x == 0) carry_sh = 0;
    __syncthreads();
    for (u64 base = 0; base < ntiles; base += blockDim.x) {
        u64 idx = base + threadIdx.x;
        u64 v = idx < ntiles ? bsum[idx] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < (int)blockDim.x; o <<= 1) {       // Hillis-Steele inclusive
            u64 a = threadIdx.x >= (u32)o ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] = scan_op<OP>(sh[threadIdx.x], a);
            __syncthreads();
        }
        u64 incl = sh[threadIdx.x];
        u64 excl = threadIdx.x ? sh[threadIdx.x - 1] : 0;
        u64 carry = carry_sh;
        if (idx < ntiles) bsum[idx] = scan_op<OP>(carry, excl);
        __syncthreads();
        if (threadIdx.x == blockDim.x - 1) carry_sh = scan_op<OP>(carry, incl);
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry_sh;
}

template <int OP>
static __global__ void k_scan_apply(const u64* in, u64* out,
                                    const u64* __restrict__ n_ptr, const u64* __restrict__ bsum)
{
    __shared__ u64 wsum[SCAN_THREADS / 64];
    const u64 n = *n_ptr;
    const u64 ntiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        // blocked arrangement: thread owns SCAN_ITEMS consecutive items
        u64 base = t * SCAN_TILE + (u64)threadIdx.x * SCAN_ITEMS;
        u64 v[SCAN_ITEMS];
        u64 s = 0;
        for (int i = 0; i < SCAN_ITEMS; i++) {
            v[i] = (base + i < n) ? in[base + i] : 0;
            s = scan_op<OP>(s, v[i]);
        }
        u64 incl = s;                                           // wave inclusive scan of s
        for (int o = 1; o < 64; o <<= 1) {
            u64 a = __shfl_up(incl, o, 64);
            if (lane >= o) incl = scan_op<OP>(incl, a);
        }
        u64 excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 0;
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        u64 woff = 0;
        for (int i = 0; i < w; i++) woff = scan_op<OP>(woff, wsum[i]);
        u64 run = scan_op<OP>(scan_op<OP>(bsum[t], woff), excl);   // everything before this thread's items
        for (int i = 0; i < SCAN_ITEMS; i++) {
            if (OP == 0) { if (base + i < n) out[base + i] = run; run += v[i]; }
            else { run = scan_op<OP>(run, v[i]); if (base + i < n) out[base + i] = run; }
        }
        __syncthreads();
    }
}

template <int OP>
inline void device_scan_u64(const u64* in, u64* out, const u64* d_n, u64* d_total, u64* tmp, hipStream_t st)
{
    hipLaunchKernelGGL((k_scan_tile_sums<OP>), dim3(1024), dim3(SCAN_THREADS), 0, st, in, d_n, tmp);
    hipLaunchKernelGGL((k_scan_spine<OP>), dim3(1), dim3(1024), 0, st, tmp, d_n, d_total);
    hipLaunchKernelGGL((k_scan_apply<OP>), dim3(1024), dim3(SCAN_THREADS), 0, st, in, out, d_n, tmp);
}
inline void exclusive_scan_u64(const u64* in, u64* out, const u64* d_n, u64* d_total, u64* tmp, hipStream_t st)
{
    device_scan_u64<0>(in, out, d_n, d_total, tmp, st);
}

// ---- N exclusive sums over arrays of the same length in ONE pass of the three kernels (the MSA planner scans two or
// three size / flag arrays per step: a third of the launches and of the tail latencies).  in[k] / out[k] may alias.
// tmp: exactly N * (ceil(n / SCAN_TILE) + 1) u64: the tile sums of array k begin at k * (ceil(n / SCAN_TILE) + 1), and the last
// slot of each stretch is never touched (N * (n / SCAN_TILE + 2), the callers' form, is at least this much).
template <int N> struct ScanSet { const u64* in[N]; u64* out[N]; u64* total[N]; };

template <int N>
static __global__ void k_mscan_tile_sums(ScanSet<N> a, const u64* __restrict__ n_ptr, u64* __restrict__ bsum)
{
    __shared__ u64 sh[SCAN_THREADS / 64];
    const u64 n = *n_ptr;
    const u64 ntiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const u64 base = t * SCAN_TILE;
        u64 s[N];
#pragma unroll
        for (int k = 0; k < N; k++) s[k] = 0;
        for (int i = 0; i < SCAN_ITEMS; i++) {
            const u64 idx = base + (u64)i * SCAN_THREADS + threadIdx.x;
            if (idx < n) {
#pragma unroll
                for (int k = 0; k < N; k++) s[k] += a.in[k][idx];
            }
        }
#pragma unroll
        for (int k = 0; k < N; k++) {
            const u64 r = block_reduce<0>(s[k], sh);
            if (threadIdx.x == 0) bsum[(u64)k * (ntiles + 1) + t] = r;
        }
    }
}
template <int N>
static __global__ void k_mscan_spine(ScanSet<N> a, u64* __restrict__ bsum, const u64* __restrict__ n_ptr)
{
    // N waves, one per array: a wave walks its tile sums 64 at a time (DPP-free shuffle scan)
    const u64 n = *n_ptr;
    const u64 ntiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (k >= N) return;
    u64* b = bsum + (u64)k * (ntiles + 1);
    u64 carry = 0;
    for (u64 base = 0; base < ntiles; base += 64) {
        const u64 idx = base + lane;
        const u64 v = idx < ntiles ? b[idx] : 0;
        u64 incl = v;
        for (int o = 1; o < 64; o <<= 1) { const u64 x = __shfl_up(incl, o, 64); if (lane >= o) incl += x; }
        if (idx < ntiles) b[idx] = carry + incl - v;
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) *a.total[k] = carry;
}
template <int N>
static __global__ void k_mscan_apply(ScanSet<N> a, const u64* __restrict__ n_ptr, const u64* __restrict__ bsum)
{
    __shared__ u64 wsum[N][SCAN_THREADS / 64];
    const u64 n = *n_ptr;
    const u64 ntiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const u64 base = t * SCAN_TILE + (u64)threadIdx.x * SCAN_ITEMS;
        u64 v[N][SCAN_ITEMS], excl[N];
#pragma unroll
        for (int k = 0; k < N; k++) {
            u64 s = 0;
            for (int i = 0; i < SCAN_ITEMS; i++) { v[k][i] = (base + i < n) ? a.in[k][base + i] : 0; s += v[k][i]; }
            u64 incl = s;
            for (int o = 1; o < 64; o <<= 1) { const u64 x = __shfl_up(incl, o, 64); if (lane >= o) incl += x; }
            excl[k] = incl - s;
            if (lane == 63) wsum[k][w] = incl;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < N; k++) {
            u64 woff = 0;
            for (int i = 0; i < w; i++) woff += wsum[k][i];
            u64 run = bsum[(u64)k * (ntiles + 1) + t] + woff + excl[k];
            for (int i = 0; i < SCAN_ITEMS; i++) { if (base + i < n) a.out[k][base + i] = run; run += v[k][i]; }
        }
        __syncthreads();
    }
}
template <int N>
inline void exclusive_scan_multi(const ScanSet<N>& a, const u64* d_n, u64* tmp, hipStream_t st)
{
    hipLaunchKernelGGL((k_mscan_tile_sums<N>), dim3(1024), dim3(SCAN_THREADS), 0, st, a, d_n, tmp);
    hipLaunchKernelGGL((k_mscan_spine<N>), dim3(1), dim3(64 * N), 0, st, a, tmp, d_n);
    hipLaunchKernelGGL((k_mscan_apply<N>), dim3(1024), dim3(SCAN_THREADS), 0, st, a, d_n, tmp);
}
inline void inclusive_max_scan_u64(const u64* in, u64* out, const u64* d_n, u64* d_total, u64* tmp, hipStream_t st)
{
    device_scan_u64<1>(in, out, d_n, d_total, tmp, st);
}

} // namespace edsx
