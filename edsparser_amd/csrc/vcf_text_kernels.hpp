// vcf_text_kernels.hpp — device pieces that every pass over VCF text shares: the byte window, the record-line starts
// and the stable LSD radix sort.  Used by the tokeniser (vcf_device.hip) and by the contig session (vcf_contig.hip);
// the kernels are static, every translation unit that includes this gets its own copy.
#pragma once

#include "msa_device.hpp"
#include "vcf_walk.hpp"

namespace edsx {

struct WalkGrid {                                            // the grid of a thread-per-item kernel, as its body asks for it
    u32 bi, bd, ti, gd;                                      // (read in the kernel itself; the products are taken where the body uses them)
    __device__ __forceinline__ u64 first() const { return bi * (u64)bd + ti; }
    __device__ __forceinline__ u64 stride() const { return (u64)gd * bd; }
    __device__ __forceinline__ bool lead() const { return bi == 0 && ti == 0; }
};
#define WALK_THREAD WalkGrid{blockIdx.x, blockDim.x, threadIdx.x, gridDim.x}      /* last argument of every body */

// VtCtl, ByteWindow (the text through 8-byte aligned loads), VT_BLOCK and vt_line_start_mask: vcf_walk.hpp, which the
// host twin compiles too.  A wave owns VT_BLOCK bytes of the text (16 per lane); pass 1 counts the line starts of every
// such block, a scan over the block counts numbers them, pass 2 finds them again and writes their positions.
static __global__ void __launch_bounds__(256) k_vt_line_count(const uint8_t* __restrict__ raw, u64 n, u64* __restrict__ cnt, VtCtl* ctl)
{
    const u64 nblk = (n + VT_BLOCK - 1) / VT_BLOCK;
    const u32 lane = threadIdx.x & 63;
    bool cr = false;
    for (u64 b = (blockIdx.x * (u64)blockDim.x + threadIdx.x) >> 6; b < nblk; b += ((u64)gridDim.x * blockDim.x) >> 6) {
        u32 c = (u32)__builtin_popcount(vt_line_start_mask(raw, n, b * VT_BLOCK + lane * 16u, cr));
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) cnt[b] = c;
    }
    if (cr) ctl->bad = 1;
}
static __global__ void __launch_bounds__(256) k_vt_line_fill(const uint8_t* __restrict__ raw, u64 n, const u64* __restrict__ base, u64* __restrict__ lstart)
{
    const u64 nblk = (n + VT_BLOCK - 1) / VT_BLOCK;
    const u32 lane = threadIdx.x & 63;
    bool cr = false;
    for (u64 b = (blockIdx.x * (u64)blockDim.x + threadIdx.x) >> 6; b < nblk; b += ((u64)gridDim.x * blockDim.x) >> 6) {
        const u64 i0 = b * VT_BLOCK + lane * 16u;
        u32 m = vt_line_start_mask(raw, n, i0, cr);
        const u32 c = (u32)__builtin_popcount(m);
        u32 incl = c;
        for (int o = 1; o < 64; o <<= 1) { const u32 x = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += x; }
        u64 at = base[b] + (incl - c);
        while (m) { lstart[at++] = i0 + (u32)__builtin_ctz(m); m &= m - 1; }
    }
}

// The line starts of a text in HBM (raw: n bytes, 256-byte aligned, vcf_size::text(n) allocated), in two steps so that a
// caller can put a trace span around the device work alone.  vt_line_starts_reset sizes idx (the scanned block counts)
// and tmp (the scan's scratch) and resets ctl (n = the number of blocks); vt_line_starts then runs count pass, block
// scan and fill pass, sizes lstart and returns the number of record lines, or VT_NOT_PLAIN ('\r' somewhere, or 2^32
// lines and more).
constexpr u64 VT_NOT_PLAIN = ~0ull;
static void vt_line_starts_reset(u64 n, VtCtl* ctl, DevBuf& idx, DevBuf& tmp, hipStream_t st)
{
    idx.ensure(vcf_size::line_counts(vcf_size::line_blocks(n)));           // line starts per 1 KB block of the text
    tmp.ensure(8 * ((n + 2) / SCAN_TILE + 4));
    VtCtl h{};
    h.n = vcf_size::line_blocks(n);                                         // element count of the block scan
    EDSX_HIP(hipMemcpyAsync(ctl, &h, sizeof(h), hipMemcpyHostToDevice, st));
}
static u64 vt_line_starts(const uint8_t* raw, u64 n, VtCtl* ctl, DevBuf& idx, DevBuf& lstart, DevBuf& tmp, hipStream_t st)
{
    hipLaunchKernelGGL(k_vt_line_count, dim3(2048), dim3(256), 0, st, raw, n, idx.as<u64>(), ctl);
    exclusive_scan_u64(idx.as<u64>(), idx.as<u64>(), &ctl->n, &ctl->nrec, tmp.as<u64>(), st);
    VtCtl h{};
    EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    if (h.bad || h.nrec >= 0xffffffffull) return VT_NOT_PLAIN;
    if (h.nrec) {
        lstart.ensure(vcf_size::line_starts(h.nrec));
        hipLaunchKernelGGL(k_vt_line_fill, dim3(2048), dim3(256), 0, st, raw, n, idx.as<u64>(), lstart.as<u64>());
    }
    return h.nrec;
}

// ---- LSD radix sort of (u64 key, u32 value) pairs: eight stable passes of eight bits (unsorted VCFs with distinct
// positions only; the usual VCF ascends and skips it).  A wave owns a tile of RS_TILE consecutive elements: pass 1 counts
// its digits into a bin-major table (bin * ntiles + tile), one exclusive scan over the table gives every (bin, tile) its
// first output position, pass 2 walks the tile 64 elements at a time - lanes with the same digit find each other with
// one ballot per digit bit, their rank among them keeps the order stable - and moves the running positions in LDS.
constexpr u32 RS_TILE = 2048;
static __global__ void __launch_bounds__(64) k_rs_hist(const u64* __restrict__ keys, u64 n, u32 shift, u64 ntiles, u64* __restrict__ table)
{
    __shared__ u32 hist[256];
    const u32 lane = threadIdx.x;
    for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (u32 b = lane; b < 256; b += 64) hist[b] = 0;
        __syncthreads();
        const u64 base = tile * RS_TILE;
        for (u32 o = lane; o < RS_TILE; o += 64)
            if (base + o < n) atomicAdd(&hist[(u32)(keys[base + o] >> shift) & 0xffu], 1u);
        __syncthreads();
        for (u32 b = lane; b < 256; b += 64) table[(u64)b * ntiles + tile] = hist[b];
        __syncthreads();
    }
}
static __global__ void __launch_bounds__(64) k_rs_scatter(const u64* __restrict__ keys, const u32* __restrict__ vals, u64 n, u32 shift,
                                                   u64 ntiles, const u64* __restrict__ table, u64* __restrict__ keys_out,
                                                   u32* __restrict__ vals_out)
{
    __shared__ u64 at[256];                                    // next output position of every digit of this tile
    const u32 lane = threadIdx.x;
    for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (u32 b = lane; b < 256; b += 64) at[b] = table[(u64)b * ntiles + tile];
        __syncthreads();
        const u64 base = tile * RS_TILE;
        for (u32 o = 0; o < RS_TILE && base + o < n; o += 64) {
            const u64 i = base + o + lane;
            const bool valid = i < n;
            const u64 key = valid ? keys[i] : 0;
            const u32 val = valid ? (vals ? vals[i] : (u32)i) : 0u;         // vals == nullptr: the element's index (first pass)
            const u32 d = (u32)(key >> shift) & 0xffu;
            u64 same = ballot64(valid);                                      // lanes with this lane's digit
#pragma unroll
            for (int b = 0; b < 8; b++) {
                const u64 m = ballot64(valid && ((d >> b) & 1u));
                same &= ((d >> b) & 1u) ? m : ~m;
            }
            const u32 rank = mbcnt(same);
            if (valid) {
                const u64 pos = at[d] + rank;
                keys_out[pos] = key;
                vals_out[pos] = val;
            }
            __syncthreads();                                                 // (one wave: every lane has read at[] before it moves)
            if (valid && rank == 0) at[d] += (u64)__builtin_popcountll(same);
            __syncthreads();
        }
        __syncthreads();
    }
}

} // namespace edsx
