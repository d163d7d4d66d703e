// slice_device.hip — cut regions out of an EDS with sources on gfx950 (edsx_paths_slice, edsparser-slice).
//
// Semantics: include/edsx.h; the per-region arithmetic: slice_core.hpp.  A region is a symbol range i0 .. i1 with two cut
// offsets; its texts are the symbols' own with every string of the two edge symbols cut.  Regions overlap and repeat, so
// nothing is kept per string of the EDS: everything a region needs is worked out from the session's scanned tables.
//
//   session, once   k_slice_setbytes  G lanes per string (as k_sub_filter): the .seds bytes of "{ids}", scanned -> sb
//                   k_slice_symof     the symbol of every string, by bisection in ent_off
//   resolve         the ends of the path regions go through the lift's site search (k_lift_find) and stay on the device
//                   k_slice_ends      one lane per region: its two sites, or two bisections in col for a column region
//   count           k_slice_count     one wave per region: A and B, the sums of min(len, cut) over the strings of the two
//                                     edge symbols (lanes stride over the strings, shuffle reduction); the inner symbols
//                                     are differences of str_off, ent_off and sb.  Bytes of both texts, edge strings,
//                                     string tiles and copy tiles per region; one scan of the five over R + 1 entries gives
//                                     every offset table and the totals that size the outputs
//   fill            work items are (region, tile): item t belongs to the last region whose scanned tile count is <= t; an
//                   item is a wave's, so that small regions fill a workgroup four at a time
//                   k_slice_place     a tile is 64 strings of a region, one per lane: characters removed in
//                                     front of the wave's first string (strided over the edge symbol's strings in front of
//                                     it), a shuffle scan inside the wave -> where the string goes; braces, commas, the line
//                                     feed; the destinations of edge strings go to a table of the region's own (edst)
//                   k_slice_seds      the same tiles, G lanes per string as k_sub_seds: decimal ids from the bitsets
//                   k_slice_copy      a tile is 1024 characters of the pool stretch that holds the region's kept
//                                     characters: a lane owns 16 aligned source bytes, finds their string between the
//                                     tile's first and last, and when all 16 are kept characters of one string moves them
//                                     with one aligned 16-byte load and one 16-byte store; the rest goes byte by byte
#include "path_device.hpp"
#include "slice_core.hpp"
#include "subset_device.hpp"

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

namespace edsx {

namespace {

constexpr u64 NONE = ~0ull;
constexpr int ST = 256;                    // threads per block
constexpr u32 WAVES = ST / 64;             // a work item of the fill kernels is a wave's: small regions fill a workgroup four at a time
constexpr u32 PL_TILE = 64;                // strings per place / seds tile
constexpr u32 CP_TILE = 64 * 16;           // source characters per copy tile
// scanned per region (R + 1 entries each, one behind the other in slice_.scan): bytes of both texts, edge strings, tiles
enum { SC_EDS, SC_SEDS, SC_EDGE, SC_PTILE, SC_CTILE, SC_COUNT };

__device__ __forceinline__ slice::Ends ends_of(const SliceRegion& r)
{
    return slice::Ends{r.symbol_first, r.symbol_last, r.cut_first, r.cut_end, r.column_first, r.column_end};
}

__global__ void __launch_bounds__(ST) k_slice_setbytes(const u64* __restrict__ bits, u32 W, u32 G, u64 m, u64* __restrict__ sb)
{
    const u32 g = threadIdx.x & (G - 1), per_block = ST / G;
    for (u64 base = (u64)blockIdx.x * per_block; base <= m; base += (u64)gridDim.x * per_block) {   // block-uniform: the shuffles
        const u64 j = base + threadIdx.x / G;                                                      // below run with every lane
        u64 bytes = 0;
        bool univ = false;
        if (j < m) {
            const u64* row = bits + j * W;
            for (u32 w = g; w < W; w += G) {
                const u64 b = row[w];
                if (w == 0) univ = b & 1;
                bytes += slice::word_bytes(w, w == 0 ? b & ~1ull : b);
            }
        }
        for (u32 o = G >> 1; o > 0; o >>= 1) bytes += __shfl_xor(bytes, o, 64);
        if (j <= m && g == 0) sb[j] = j < m ? slice::set_bytes(univ, bytes) : 0;   // (word 0 is this lane's: it knows `univ`)
    }
}

__global__ void __launch_bounds__(ST) k_slice_symof(const u64* __restrict__ ent_off, u64 n, u64 m, u64* __restrict__ symof)
{
    for (u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x; j < m; j += (u64)gridDim.x * blockDim.x)
        symof[j] = last_le(ent_off, 0, n - 1, j);
}

struct EndsArgs {
    slice::SliceTab t;
    const u64* path; const u64* start; const u64* end; const u64* qidx;      // qidx: the region's first site, NONE for columns
    const lift::Site* site; const uint8_t* sst;
    u64 R;
    SliceRegion* reg; uint8_t* status;
};

__global__ void __launch_bounds__(ST) k_slice_ends(EndsArgs a)
{
    for (u64 r = blockIdx.x * (u64)blockDim.x + threadIdx.x; r < a.R; r += (u64)gridDim.x * blockDim.x) {
        slice::Ends e;
        bool ok;
        if (a.path[r] == 0) ok = slice::column_ends(a.t, a.start[r], a.end[r], e);
        else {
            const u64 q = a.qidx[r];
            ok = a.start[r] < a.end[r] && a.sst[q] == 0 && a.sst[q + 1] == 0;
            if (ok) slice::path_ends(a.site[q].symbol, a.site[q].offset, a.site[q].column, a.site[q + 1].symbol, a.site[q + 1].offset,
                                     a.site[q + 1].column, e);
        }
        SliceRegion g;
        g.symbol_first = g.symbol_last = g.cut_first = g.cut_end = g.column_first = g.column_end = g.strings = g.chars = g.eds_off = g.seds_off = NONE;
        g.eds_len = g.seds_len = 0;
        if (ok) { g.symbol_first = e.i0; g.symbol_last = e.i1; g.cut_first = e.o0; g.cut_end = e.o1e; g.column_first = e.c0; g.column_end = e.c1e; }
        a.reg[r] = g;
        a.status[r] = ok ? slice::OK : slice::RANGE;
    }
}

// sum over the strings [ja, jb) of symbol i of what the cuts remove (which == 0), or of min(len, cut) (which == 1): the
// lanes of a wave stride over the strings
__device__ __forceinline__ u64 wave_strings(const slice::SliceTab& t, const slice::Ends& e, u64 i, u64 ja, u64 jb, u64 cutoff, int which)
{
    u64 s = 0;
    for (u64 j = ja + (threadIdx.x & 63); j < jb; j += 64) {
        const u64 len = t.str_off[j + 1] - t.str_off[j];
        s += which ? slice::min64(len, cutoff) : slice::removed(e, i, len);
    }
    return wave_sum(s);
}

__global__ void __launch_bounds__(ST) k_slice_count(slice::SliceTab t, u64 R, SliceRegion* __restrict__ reg, u64* __restrict__ asum,
                                                    u64* __restrict__ sc)
{
    const u32 lane = threadIdx.x & 63;
    for (u64 r = blockIdx.x * (u64)(ST / 64) + (threadIdx.x >> 6); r <= R; r += (u64)gridDim.x * (ST / 64)) {   // wave-uniform
        u64 v[SC_COUNT] = {0, 0, 0, 0, 0};
        if (r < R && reg[r].symbol_first != NONE) {
            const slice::Ends e = ends_of(reg[r]);
            const u64 A = wave_strings(t, e, e.i0, t.ent_off[e.i0], slice::ent_end(t, e.i0), e.o0, 1);
            const u64 B = wave_strings(t, e, e.i1, t.ent_off[e.i1], slice::ent_end(t, e.i1), e.o1e, 1);
            slice::Counts c;
            slice::counts(t, e, A, B, c);
            u64 lo, hi;
            slice::copy_span(t, e, lo, hi);
            v[SC_EDS] = c.eds_len; v[SC_SEDS] = c.seds_len; v[SC_EDGE] = c.edge_strings;
            v[SC_PTILE] = (c.strings + PL_TILE - 1) / PL_TILE;
            v[SC_CTILE] = hi > lo ? (hi - (lo & ~15ull) + CP_TILE - 1) / CP_TILE : 0;
            if (lane == 0) {
                asum[r] = A;
                reg[r].strings = c.strings; reg[r].chars = c.chars; reg[r].eds_len = c.eds_len; reg[r].seds_len = c.seds_len;
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < SC_COUNT; k++) sc[(u64)k * (R + 1) + r] = v[k];
        }
    }
}

__global__ void __launch_bounds__(ST) k_slice_offsets(u64 R, const u64* __restrict__ sc, SliceRegion* __restrict__ reg)
{
    for (u64 r = blockIdx.x * (u64)blockDim.x + threadIdx.x; r < R; r += (u64)gridDim.x * blockDim.x)
        if (reg[r].symbol_first != NONE) { reg[r].eds_off = sc[SC_EDS * (R + 1) + r]; reg[r].seds_off = sc[SC_SEDS * (R + 1) + r]; }
}

struct FillArgs {
    slice::SliceTab t;
    const u64* symof; const uint8_t* chars; const u64* bits;
    const SliceRegion* reg; const u64* asum; const u64* sc;
    u64 R, tiles;
    u32 W, G;
    u64* edst; uint8_t* out; uint8_t* sout;
};

__global__ void __launch_bounds__(ST) k_slice_place(FillArgs a)
{
    const u32 lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u64* poff = a.sc + SC_PTILE * (a.R + 1);
    for (u64 tile = (u64)blockIdx.x * WAVES + wave; tile < a.tiles; tile += (u64)gridDim.x * WAVES) {   // wave-uniform; no barrier
        const u64 r = last_le(poff, 0, a.R, tile);                             // the same for every lane: scalar loads
        const slice::Ends e = ends_of(a.reg[r]);
        const u64 e0 = a.t.ent_off[e.i0], e1 = slice::ent_end(a.t, e.i1);
        const u64 ja = e0 + (tile - poff[r]) * PL_TILE;
        // characters removed in front of string ja
        u64 base;
        if (e.i0 == e.i1) base = wave_strings(a.t, e, e.i0, e0, ja, 0, 0);
        else {
            const u64 end0 = slice::ent_end(a.t, e.i0), first1 = a.t.ent_off[e.i1];
            base = ja >= end0 ? a.asum[r] : wave_strings(a.t, e, e.i0, e0, ja, 0, 0);
            if (ja > first1) base += wave_strings(a.t, e, e.i1, first1, ja, 0, 0);
        }
        const u64 j = ja + lane;
        const bool act = j < e1;
        u64 i = 0, begin = 0, kept = 0, rem = 0;
        if (act) {
            i = a.symof[j];
            const u64 len = a.t.str_off[j + 1] - a.t.str_off[j];
            slice::cut(e, i, len, begin, kept);
            rem = len - kept;
        }
        u64 incl = rem;
        for (u32 o = 1; o < 64; o <<= 1) { const u64 x = __shfl_up(incl, o, 64); if (lane >= o) incl += x; }
        if (!act) continue;
        const u64 eoff = a.sc[SC_EDS * (a.R + 1) + r];
        const u64 d = eoff + slice::string_dst(a.t, e, i, j, base + incl - rem);
        const u64 k = j - a.t.ent_off[i];
        a.out[d - 1] = k ? ',' : '{';
        if (k + 1 == a.t.size[i]) a.out[d + kept] = '}';
        if (j + 1 == e1) a.out[d + kept + 1] = '\n';
        const u64 slot = slice::edge_slot(a.t, e, i, j);
        if (slot != NONE) a.edst[a.sc[SC_EDGE * (a.R + 1) + r] + slot] = d;
    }
}

// write_set_ids over the set as it is, without its bit 0
struct OwnIds {
    __device__ __forceinline__ u64 mask(u32 w) const { return w == 0 ? ~1ull : ~0ull; }
    __device__ __forceinline__ u64 bytes(u32 w, u64 x) const { return slice::word_bytes(w, x); }
    __device__ __forceinline__ u32 id(u32 w, u32 b) const { return 64u * w + b; }
};

__global__ void __launch_bounds__(ST) k_slice_seds(FillArgs a)
{
    const u32 G = a.G, W = a.W, lane = threadIdx.x & 63, g = lane & (G - 1), per_pass = 64 / G;
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u64* poff = a.sc + SC_PTILE * (a.R + 1);
    for (u64 tile = (u64)blockIdx.x * WAVES + wave; tile < a.tiles; tile += (u64)gridDim.x * WAVES) {   // wave-uniform throughout:
        const u64 r = last_le(poff, 0, a.R, tile);                             // the shuffles below run with every lane
        const slice::Ends e = ends_of(a.reg[r]);
        const u64 e1 = slice::ent_end(a.t, e.i1), soff = a.sc[SC_SEDS * (a.R + 1) + r];
        const u64 ja = a.t.ent_off[e.i0] + (tile - poff[r]) * PL_TILE;
        for (u32 s0 = 0; s0 < PL_TILE; s0 += per_pass) {
            const u64 j = ja + s0 + lane / G;
            const bool act = j < e1;
            const u64 p0 = act ? soff + slice::set_dst(a.t, e, j) : 0;
            const u64 end = act ? p0 + (a.t.sb[j + 1] - a.t.sb[j]) : 0;        // one past the closing brace
            const bool univ = act && (a.bits[j * W] & 1);
            if (act && g == 0) {
                a.sout[p0] = '{';
                a.sout[end - 1] = '}';                                         // (of "{}" and "{0}" too)
                if (univ) a.sout[p0 + 1] = '0';
                if (j + 1 == e1) a.sout[end] = '\n';
            }
            write_set_ids(OwnIds{}, a.bits + j * W, act && !univ, W, G, g, p0 + 1, end, a.sout);
        }
    }
}

// where string j of symbol i of region r begins in the .eds buffer
__device__ __forceinline__ u64 dst_of(const FillArgs& a, const slice::Ends& e, u64 r, u64 i, u64 j)
{
    const u64 slot = slice::edge_slot(a.t, e, i, j);
    if (slot != NONE) return a.edst[a.sc[SC_EDGE * (a.R + 1) + r] + slot];
    return a.sc[SC_EDS * (a.R + 1) + r] + slice::string_dst(a.t, e, i, j, a.asum[r]);
}

__global__ void __launch_bounds__(ST) k_slice_copy(FillArgs a)
{
    const u32 lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u64* coff = a.sc + SC_CTILE * (a.R + 1);
    for (u64 tile = (u64)blockIdx.x * WAVES + wave; tile < a.tiles; tile += (u64)gridDim.x * WAVES) {   // wave-uniform; no barrier
        const u64 r = last_le(coff, 0, a.R, tile);
        const slice::Ends e = ends_of(a.reg[r]);
        const u64 e0 = a.t.ent_off[e.i0], e1 = slice::ent_end(a.t, e.i1);
        u64 lo, hi;
        slice::copy_span(a.t, e, lo, hi);
        const u64 t0 = (lo & ~15ull) + (tile - coff[r]) * CP_TILE, t1 = min(hi, t0 + (u64)CP_TILE);   // max(t0, lo) < t1
        u64 edge = 0;                                                          // lanes 0 and 1: the tile's first and last string
        if (lane < 2) edge = last_le(a.t.str_off, e0, e1 - 1, lane ? t1 - 1 : max(t0, lo));
        const u64 j0 = __shfl(edge, 0, 64), j1 = __shfl(edge, 1, 64);
        const u64 c0 = t0 + (u64)lane * 16, cb = max(c0, lo), c1 = min(t1, c0 + 16);
        if (cb < c1) {
            u64 j = last_le(a.t.str_off, j0, j1, cb);
            u64 s0 = a.t.str_off[j], s1 = a.t.str_off[j + 1], begin, kept;
            slice::cut(e, a.symof[j], s1 - s0, begin, kept);
            if (cb == c0 && c1 == c0 + 16 && c0 >= s0 + begin && c0 + 16 <= s0 + begin + kept) {   // 16 kept characters of string j
                const u64 d = dst_of(a, e, r, a.symof[j], j);
                store16u(a.out + d + (c0 - s0 - begin), *reinterpret_cast<const uint4*>(a.chars + c0));
            } else {
                u64 d = NONE;                                                  // worked out when string j has a kept character here
                for (u64 c = cb; c < c1; c++) {
                    while (c >= s1) {                                          // (c < hi: j stays below e1)
                        j++; s0 = s1; s1 = a.t.str_off[j + 1]; d = NONE;
                        slice::cut(e, a.symof[j], s1 - s0, begin, kept);
                    }
                    if (c < s0 + begin || c >= s0 + begin + kept) continue;
                    if (d == NONE) d = dst_of(a, e, r, a.symof[j], j);
                    a.out[d + (c - s0 - begin)] = a.chars[c];
                }
            }
        }
    }
}

} // namespace

void PathPipeline::slice_open(hipStream_t st)
{
    lift_open(st);                                               // col
    if (slice_.ready || n_ == 0) return;
    const EdsView v = eds_.view();
    slice_.sb.ensure(8 * (v.m + 1));
    slice_.symof.ensure(8 * v.m);
    ctl_.ensure(8 * 8);
    scan_tmp_.ensure(8 * (v.m / SCAN_TILE + 4));
    const u64 cnt = v.m + 1;
    u64* ctl = ctl_.as<u64>();
    EDSX_HIP(hipMemcpyAsync(ctl, &cnt, 8, hipMemcpyHostToDevice, st));
    const u32 G = SubsetPipeline::group_for(v.W);
    hipLaunchKernelGGL(k_slice_setbytes, dim3(grid_for((v.m + 1) * G, 16384)), dim3(ST), 0, st, v.bits, v.W, G, v.m, slice_.sb.as<u64>());
    exclusive_scan_u64(slice_.sb.as<u64>(), slice_.sb.as<u64>(), ctl, ctl + 1, scan_tmp_.as<u64>(), st);
    hipLaunchKernelGGL(k_slice_symof, dim3(grid_for(v.m, 8192)), dim3(ST), 0, st, v.sym.ent_off, n_, v.m, slice_.symof.as<u64>());
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    slice_.ready = true;
}

void PathPipeline::slice(size_t n, const u64* path, const u64* start, const u64* end, u64 max_bytes, HostBytes& eds_out,
                         HostBytes& seds_out, SliceRegion* region, uint8_t* status, KernelTimes* times, hipStream_t st)
{
    // the ends of the path regions as lift queries, two per region
    std::vector<u64> qpath, qpos, qidx(n, NONE);
    for (size_t r = 0; r < n; r++) {
        if (path[r] == 0) continue;
        qidx[r] = qpath.size();
        qpath.push_back(path[r]); qpath.push_back(path[r]);
        qpos.push_back(start[r]); qpos.push_back(end[r] - 1);
    }
    check_ids(qpath.data(), qpath.size());
    begin_call();
    eds_out.take(0); seds_out.take(0);
    if (n == 0) return;
    if (n_ == 0) {                                               // an empty EDS has no paths and no columns
        for (size_t r = 0; r < n; r++) {
            status[r] = slice::RANGE;
            if (region) { region[r] = SliceRegion{NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, 0, NONE, 0}; }
        }
        return;
    }
    slice_open(st);
    const u64 R = n, Q = qpath.size();
    slice_.site.ensure(sizeof(LiftSite) * std::max<u64>(Q, 1)); slice_.sst.ensure(std::max<u64>(Q, 1));
    if (Q) {
        lift_run(Q, qpath.data(), qpos.data(), nullptr, nullptr, nullptr, nullptr, nullptr, slice_.site.as<LiftSite>(), slice_.sst.as<uint8_t>(), st);
        timing_.scan_ms += timing_.copy_ms;                      // the site search is part of the resolve step
        timing_.copy_ms = 0;
    }
    TimedRuns timed(st, times);                                  // every run with a bucket: PathTiming is filled whether timing is on or not

    const EdsView v = eds_.view();
    const slice::SliceTab tab{v.sym.size, v.sym.ent_off, v.str_off, slice_.sb.as<u64>(), align_.col.as<u64>(), n_, v.m};
    slice_.in.ensure(8 * 4 * R); slice_.reg.ensure(sizeof(SliceRegion) * R); slice_.st.ensure(R); slice_.sum.ensure(8 * R);
    slice_.scan.ensure(8 * SC_COUNT * (R + 1));
    ctl_.ensure(8 * 8);
    scan_tmp_.ensure(8 * SC_COUNT * ((R + 1) / SCAN_TILE + 4));
    u64 *in = slice_.in.as<u64>(), *sc = slice_.scan.as<u64>(), *ctl = ctl_.as<u64>();
    const u64* cols[4] = {path, start, end, qidx.data()};
    for (int k = 0; k < 4; k++) EDSX_HIP(hipMemcpyAsync(in + k * R, cols[k], 8 * R, hipMemcpyHostToDevice, st));
    u64 hctl[1 + SC_COUNT] = {R + 1, 0, 0, 0, 0, 0};
    EDSX_HIP(hipMemcpyAsync(ctl, hctl, sizeof(hctl), hipMemcpyHostToDevice, st));
    SliceRegion* reg = slice_.reg.as<SliceRegion>();
    const EndsArgs ea{tab, in, in + R, in + 2 * R, in + 3 * R, slice_.site.as<LiftSite>(), slice_.sst.as<uint8_t>(), R, reg, slice_.st.as<uint8_t>()};
    timed.run("k_slice_ends", [&] { hipLaunchKernelGGL(k_slice_ends, dim3(grid_for(R, 8192)), dim3(ST), 0, st, ea); }, &timing_.scan_ms);
    timed.run("k_slice_count", [&] {
        hipLaunchKernelGGL(k_slice_count, dim3(grid_for((R + 1) * 64, 65536)), dim3(ST), 0, st, tab, R, reg, slice_.sum.as<u64>(), sc);
    }, &timing_.scan_ms);
    timed.run("scan_regions", [&] {
        ScanSet<SC_COUNT> ss;
        for (int k = 0; k < SC_COUNT; k++) { ss.in[k] = ss.out[k] = sc + (u64)k * (R + 1); ss.total[k] = ctl + 1 + k; }
        exclusive_scan_multi<SC_COUNT>(ss, ctl, scan_tmp_.as<u64>(), st);
    }, &timing_.scan_ms);
    timed.run("k_slice_offsets", [&] { hipLaunchKernelGGL(k_slice_offsets, dim3(grid_for(R, 8192)), dim3(ST), 0, st, R, sc, reg); }, &timing_.scan_ms);
    EDSX_HIP(hipMemcpyAsync(hctl, ctl, sizeof(hctl), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    timed.harvest();
    const u64 E = hctl[1 + SC_EDS], S = hctl[1 + SC_SEDS], X = hctl[1 + SC_EDGE], PT = hctl[1 + SC_PTILE], CT = hctl[1 + SC_CTILE];
    if (max_bytes && E + S > max_bytes)
        throw ParamError("Slices have " + std::to_string(E + S) + " bytes, above the limit of " + std::to_string(max_bytes));

    // ---- fill: both buffers are sized exactly (+ 16 bytes of slack as every output buffer here)
    slice_.eds.ensure(E + 16); slice_.seds.ensure(S + 16); slice_.edst.ensure(8 * std::max<u64>(X, 1));
    FillArgs fa{tab, slice_.symof.as<u64>(), v.chars, v.bits, reg, slice_.sum.as<u64>(), sc, R, PT, v.W, SubsetPipeline::group_for(v.W),
                slice_.edst.as<u64>(), slice_.eds.as<uint8_t>(), slice_.seds.as<uint8_t>()};
    if (PT) {
        const unsigned grid = (unsigned)std::min<u64>((PT + WAVES - 1) / WAVES, 1u << 18);
        timed.run("k_slice_place", [&] { hipLaunchKernelGGL(k_slice_place, dim3(grid), dim3(ST), 0, st, fa); }, &timing_.copy_ms);
        timed.run("k_slice_seds", [&] { hipLaunchKernelGGL(k_slice_seds, dim3(grid), dim3(ST), 0, st, fa); }, &timing_.copy_ms);
    }
    if (CT) {
        fa.tiles = CT;
        timed.run("k_slice_copy", [&] {
            hipLaunchKernelGGL(k_slice_copy, dim3((unsigned)std::min<u64>((CT + WAVES - 1) / WAVES, 1u << 18)), dim3(ST), 0, st, fa);
        }, &timing_.copy_ms);
    }
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    timed.harvest();
    const auto t0 = std::chrono::steady_clock::now();
    eds_out.take(E); seds_out.take(S);
    PinnedDownload::copy(eds_out.data, slice_.eds.ptr, E, st);
    PinnedDownload::copy(seds_out.data, slice_.seds.ptr, S, st);
    if (region) EDSX_HIP(hipMemcpyAsync(region, reg, sizeof(SliceRegion) * R, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipMemcpyAsync(status, slice_.st.ptr, R, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    timing_.download_ms += since_ms(t0);
    timing_.bytes_written = E + S;
}

} // namespace edsx
