// gfa_device.hip — an EDS as a GFA 1.0 graph on gfx950 (edsx_eds_gfa_graph): header, S lines, L lines.
//
// Semantics: include/edsx.h.  Every non-empty string is a segment whose id is its 1-based rank among the non-empty
// strings; the segments of symbol i are linked to those of the symbols i + 1 .. R(i), where R(i) is the first symbol
// behind i without an empty string (or the last symbol).  The kernels read the context's DeviceEds through its view and
// write nothing to it.
//
// Count -> scan -> fill.  Ids are ranks, so every length is a closed form of scanned counts (gfa_text.hpp):
//   strings j   k_gfa_flags     non-empty flag; its scan is seg_rank (m + 1 entries).  The S line of string j starts
//                               4 * rank + dsum(rank) + str_off[j] bytes into the S lines: no second scan
//   symbols i   k_gfa_closed    closed flag (no empty string: size equals the segments, a difference of seg_rank); scan -> C
//               k_gfa_compact   the closed symbols in order: R(i) = closed[C[i + 1]], or n - 1 behind the last one
//               k_gfa_reach     vend[i] = 1 + the segments up to the end of R(i); links and link bytes of the symbol from
//                               the closed form, no loop over its strings; one scan of both -> loff and the link total
//   one download of the totals: the link limit is checked and the text is sized exactly
// Fill: both emitters tile the OUTPUT in aligned 16-byte chunks, one chunk per lane and step.  A workgroup finds the first
// and last string (symbol) of its 16 KiB by bisection; a lane finds the line its chunk starts in by bisection between
// them (for a link, then u and v inside the symbol's block by bisection in the closed form, so one symbol with 10^5
// links spreads over as many lanes as its text has chunks), assembles the 16 bytes in two registers and stores them with
// one aligned 16-byte store; only the chunks at the two ends of a section are stored by bytes.
//   k_gfa_segments  a chunk that lies inside one string's sequence is one 16-byte load from the pool and the store
//   k_gfa_links     at most two lines per chunk (a line has 15 bytes or more)
#include "gfa_device.hpp"

#include <string>

namespace edsx {

namespace {

constexpr int GT = 256;                        // threads per block
constexpr u32 GFA_TILE = 16384;                // output bytes per block step of the emitters: 4 chunks of 16 bytes per lane
enum { CT_M1, CT_N1, CT_SEGS, CT_CLOSED, CT_LINKS, CT_LBYTES, CT_COUNT };

__global__ void __launch_bounds__(GT) k_gfa_flags(const u32* __restrict__ elen, u64 m, u64* __restrict__ flag)
{
    for (u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x; j <= m; j += (u64)gridDim.x * blockDim.x)
        flag[j] = j < m && elen[j] ? 1 : 0;
}

__global__ void __launch_bounds__(GT) k_gfa_closed(const u64* __restrict__ size, const u64* __restrict__ ent_off, u64 n,
                                                   const u64* __restrict__ seg_rank, u64* __restrict__ cflag)
{
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i <= n; i += (u64)gridDim.x * blockDim.x) {
        u64 c = 0;
        if (i < n) { const u64 e0 = ent_off[i], e1 = e0 + size[i]; c = seg_rank[e1] - seg_rank[e0] == size[i] ? 1 : 0; }
        cflag[i] = c;
    }
}

__global__ void __launch_bounds__(GT) k_gfa_compact(const u64* __restrict__ C, u64 n, u64* __restrict__ closed)
{
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 r = C[i];
        if (C[i + 1] != r) closed[r] = i;
    }
}

__global__ void __launch_bounds__(GT) k_gfa_reach(const u64* __restrict__ size, const u64* __restrict__ ent_off, u64 n,
                                                  const u64* __restrict__ seg_rank, const u64* __restrict__ C,
                                                  const u64* __restrict__ closed, u64* __restrict__ vend, u64* __restrict__ lcount,
                                                  u64* __restrict__ lbytes)
{
    const u64 nC = C[n];
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i <= n; i += (u64)gridDim.x * blockDim.x) {
        if (i == n) { vend[n] = 0; lcount[n] = 0; lbytes[n] = 0; continue; }
        const u64 k = C[i + 1], R = k < nC ? closed[k] : n - 1;      // the first closed symbol behind i
        const u64 e0 = ent_off[i], e1 = e0 + size[i];
        const u64 a = seg_rank[e0] + 1, b = seg_rank[e1] + 1, d = seg_rank[ent_off[R] + size[R]] + 1;
        vend[i] = d;
        lcount[i] = (b - a) * (d - b);
        lbytes[i] = gfa::link_block_bytes(a, b, b, d);
    }
}

__device__ __forceinline__ void store_chunk(uint8_t* out, u64 c0, u64 lo, u32 nb, const gfa::B16& x)
{
    if (nb == 16) {                                                  // (lo == c0: the buffer is aligned, so is the chunk)
        *reinterpret_cast<uint4*>(out + c0) = make_uint4((u32)x.lo, (u32)(x.lo >> 32), (u32)x.hi, (u32)(x.hi >> 32));
    } else {
        for (u32 b = 0; b < nb; b++) out[lo + b] = (uint8_t)((b < 8 ? x.lo >> (8u * b) : x.hi >> (8u * (b - 8u))) & 0xffu);
    }
}

// sec0: where the S lines start in out; bytes: their length (> 0)
__global__ void __launch_bounds__(GT) k_gfa_segments(gfa::SegTab t, u64 sec0, u64 bytes, uint8_t* __restrict__ out)
{
    __shared__ u64 sj[2];
    const u64 sec1 = sec0 + bytes, tile0 = sec0 / GFA_TILE, tile1 = (sec1 - 1) / GFA_TILE;
    for (u64 tile = tile0 + blockIdx.x; tile <= tile1; tile += gridDim.x) {
        const u64 A0 = max(sec0, tile * GFA_TILE), A1 = min(sec1, (tile + 1) * GFA_TILE);
        if (threadIdx.x == 0) sj[0] = gfa::seg_find(t, 0, t.m - 1, A0 - sec0);
        if (threadIdx.x == 64) sj[1] = gfa::seg_find(t, 0, t.m - 1, A1 - 1 - sec0);
        __syncthreads();
        const u64 jA = sj[0], jB = sj[1];
        for (u64 c0 = tile * GFA_TILE + (u64)threadIdx.x * 16; c0 < A1; c0 += (u64)GT * 16) {
            const u64 lo = max(c0, A0), hi = min(c0 + 16, A1);
            if (lo >= hi) continue;
            const u32 nb = (u32)(hi - lo);
            gfa::B16 x;
            u64 pool = 0;
            if (gfa::seg_chunk(t, jA, jB, lo - sec0, nb, x, pool)) {
                const uint4 v = load16u(t.chars + pool);
                x.lo = ((u64)v.y << 32) | v.x; x.hi = ((u64)v.w << 32) | v.z;
            }
            store_chunk(out, c0, lo, nb, x);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(GT) k_gfa_links(gfa::LinkTab t, u64 sec0, u64 bytes, uint8_t* __restrict__ out)
{
    __shared__ u64 si[2];
    const u64 sec1 = sec0 + bytes, tile0 = sec0 / GFA_TILE, tile1 = (sec1 - 1) / GFA_TILE;
    for (u64 tile = tile0 + blockIdx.x; tile <= tile1; tile += gridDim.x) {
        const u64 A0 = max(sec0, tile * GFA_TILE), A1 = min(sec1, (tile + 1) * GFA_TILE);
        if (threadIdx.x == 0 || threadIdx.x == 64) {                 // the last i with loff[i] <= the tile's first / last byte
            const u64 o = threadIdx.x == 0 ? A0 - sec0 : A1 - 1 - sec0;
            si[threadIdx.x >> 6] = last_le(t.loff, 0, t.n - 1, o);
        }
        __syncthreads();
        const u64 iA = si[0], iB = si[1];
        for (u64 c0 = tile * GFA_TILE + (u64)threadIdx.x * 16; c0 < A1; c0 += (u64)GT * 16) {
            const u64 lo = max(c0, A0), hi = min(c0 + 16, A1);
            if (lo >= hi) continue;
            const u32 nb = (u32)(hi - lo);
            store_chunk(out, c0, lo, nb, gfa::link_chunk(t, iA, iB, lo - sec0, nb));
        }
        __syncthreads();
    }
}

unsigned tile_grid(u64 sec0, u64 bytes)
{
    const u64 tiles = (sec0 + bytes - 1) / GFA_TILE - sec0 / GFA_TILE + 1;
    return (unsigned)std::min<u64>(tiles, 1u << 16);
}

} // namespace

void segment_ranks(const EdsView& v, u64* seg_rank, const u64* d_m1, u64* d_total, u64* tmp, hipStream_t st)
{
    if (v.m >= GFA_MAX_STRINGS)
        throw LimitError("An EDS of " + std::to_string(v.m) + " strings is beyond the 4294967295 this build numbers as GFA segments");
    hipLaunchKernelGGL(k_gfa_flags, dim3(grid_for(v.m + 1, 8192)), dim3(GT), 0, st, v.elen, v.m, seg_rank);
    exclusive_scan_u64(seg_rank, seg_rank, d_m1, d_total, tmp, st);
}

void GfaPipeline::run(DeviceEds& de, const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, u64 max_links,
                      HostBytes& out, GfaInfo& info, hipStream_t st)
{
    info = GfaInfo{};
    TimedRuns timed(st, &times_);

    de.load(eds, eds_n, seds, seds_n, seds != nullptr, st);
    const u64 n = de.n(), m = de.m(), N = de.n_chars();
    static const char header[] = "H\tVN:Z:1.0\n";
    static_assert(sizeof(header) - 1 == gfa::HEADER_BYTES, "header");
    info.n_symbols = n; info.n_strings = m; info.header_bytes = gfa::HEADER_BYTES;

    u64 hctl[CT_COUNT] = {};
    EdsView v{};
    if (m) {
        v = de.view();
        seg_rank_.ensure(8 * (m + 1));
        for (DevBuf* b : {&cscan_, &closed_, &vend_, &lcount_, &loff_}) b->ensure(8 * (n + 1));
        ctl_.ensure(8 * CT_COUNT);
        scan_tmp_.ensure(8 * 2 * ((m + 1) / SCAN_TILE + (n + 1) / SCAN_TILE + 8));
        hctl[CT_M1] = m + 1; hctl[CT_N1] = n + 1;
        u64 *ctl = ctl_.as<u64>(), *tmp = scan_tmp_.as<u64>(), *seg_rank = seg_rank_.as<u64>(), *C = cscan_.as<u64>(),
            *closed = closed_.as<u64>(), *vend = vend_.as<u64>(), *lcount = lcount_.as<u64>(), *loff = loff_.as<u64>();
        EDSX_HIP(hipMemcpyAsync(ctl, hctl, sizeof(hctl), hipMemcpyHostToDevice, st));
        timed.run("scan_segments", [&] { segment_ranks(v, seg_rank, ctl + CT_M1, ctl + CT_SEGS, tmp, st); });
        timed.run("k_gfa_closed", [&] {
            hipLaunchKernelGGL(k_gfa_closed, dim3(grid_for(n + 1, 8192)), dim3(GT), 0, st, v.sym.size, v.sym.ent_off, n, seg_rank, C);
        });
        timed.run("scan_closed", [&] { exclusive_scan_u64(C, C, ctl + CT_N1, ctl + CT_CLOSED, tmp, st); });
        timed.run("k_gfa_reach", [&] {
            hipLaunchKernelGGL(k_gfa_compact, dim3(grid_for(n, 8192)), dim3(GT), 0, st, C, n, closed);
            hipLaunchKernelGGL(k_gfa_reach, dim3(grid_for(n + 1, 8192)), dim3(GT), 0, st, v.sym.size, v.sym.ent_off, n, seg_rank, C, closed,
                               vend, lcount, loff);
        });
        timed.run("scan_links", [&] {
            ScanSet<2> ss{{lcount, loff}, {lcount, loff}, {ctl + CT_LINKS, ctl + CT_LBYTES}};
            exclusive_scan_multi<2>(ss, ctl + CT_N1, tmp, st);
        });
        EDSX_HIP(hipMemcpyAsync(hctl, ctl, sizeof(hctl), hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        EDSX_HIP(hipGetLastError());
    }
    const u64 M = hctl[CT_SEGS], links = hctl[CT_LINKS], lbytes = hctl[CT_LBYTES];
    const u64 sbytes = 4 * M + gfa::dsum(M) + (M ? N : 0);
    info.n_segments = M; info.n_empty_strings = m - M; info.n_open_symbols = m ? n - hctl[CT_CLOSED] : 0;
    info.n_links = links; info.segment_bytes = sbytes; info.link_bytes = lbytes;
    const u64 cap = max_links ? max_links : 1ull << 32;
    if (links > cap) {
        timed.harvest();
        throw ParamError("Graph has " + std::to_string(links) + " links, above the limit of " + std::to_string(cap));
    }

    // ---- fill: the text is sized exactly (+ 16 bytes of slack as every output buffer here)
    const u64 total = gfa::HEADER_BYTES + sbytes + lbytes;
    out_.ensure(total + 16);
    uint8_t* o = out_.as<uint8_t>();
    EDSX_HIP(hipMemcpyAsync(o, header, gfa::HEADER_BYTES, hipMemcpyHostToDevice, st));
    if (sbytes)
        timed.run("k_gfa_segments", [&] {
            const gfa::SegTab t{seg_rank_.as<u64>(), v.str_off, v.elen, v.chars, m};
            hipLaunchKernelGGL(k_gfa_segments, dim3(tile_grid(gfa::HEADER_BYTES, sbytes)), dim3(GT), 0, st, t, (u64)gfa::HEADER_BYTES, sbytes, o);
        });
    if (lbytes)
        timed.run("k_gfa_links", [&] {
            const gfa::LinkTab t{v.sym.size, v.sym.ent_off, seg_rank_.as<u64>(), vend_.as<u64>(), loff_.as<u64>(), n};
            hipLaunchKernelGGL(k_gfa_links, dim3(tile_grid(gfa::HEADER_BYTES + sbytes, lbytes)), dim3(GT), 0, st, t,
                               gfa::HEADER_BYTES + sbytes, lbytes, o);
        });
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    timed.harvest();
    out.take(total);
    PinnedDownload::copy(out.data, o, total, st);
}

} // namespace edsx
