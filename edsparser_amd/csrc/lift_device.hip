// lift_device.hip — positions between the paths of an EDS with sources on gfx950 (edsx_paths_lift, edsparser-lift;
// DESIGN 8i): the part of the path session (path_device.hpp) that answers point queries over its choice tables.
//
// Semantics: include/edsx.h; the per-query code: lift_core.hpp.  The tables of a path are one row of the session's choice
// tables (PathPipeline::tables, path_device.hip), so the queries of a call are grouped by path first:
//   first call k_lift_common  the common characters of every symbol, scanned once (cum_common) next to col, kept with the session
//   per chunk  k_lift_group   queries to table rows: a count, a scan and a second pass that hands every query a slot
//              k_lift_find    src: the site of a position, a workgroup per (row, 2048 queries) with sampled offsets in LDS
//              k_lift_pack    or the sites as given, packed from their three columns
//              k_lift_place   dst: the place of every site on its destination path, one lane per query
#include "path_device.hpp"

#include <chrono>

namespace edsx {

namespace {

constexpr u64 NONE = ~0ull;
constexpr int CP_THREADS = 256;      // threads of k_lift_find, as the copy kernels of path_device.hip

constexpr u32 LF_TOP = 2048;         // sym_pos of evenly spaced symbols kept in LDS per work item (16 KiB)
constexpr u32 LF_ITEM = 2048;        // queries of one table row per work item
constexpr u32 LF_MIN = 256;          // a work item with fewer queries does not fill the LDS table: global search only

constexpr u32 LG_ROWS = 4096;        // rows whose counters a workgroup keeps in LDS (16 KiB)
constexpr u32 LG_PER = 16;           // queries per lane and tile

// queries to table rows, in two passes over cur (one entry per distinct path of the call, D of them): perm == null counts
// the queries of every row; after the scan, with cur[d] the first slot of row d, perm != null hands every query a slot of
// its row.  A workgroup takes tiles of 4096 queries: it counts the rows of a tile in LDS, asks for the slots of each row
// with one global atomic, and the queries take theirs by the rank the LDS atomic gave them - a few rows with millions of
// queries would otherwise queue up on a few addresses.  More than LG_ROWS rows: one global atomic per query, spread over
// as many addresses.  The order inside a row is whatever the atomics give: every query keeps its own index, so no result
// depends on it.  Slots are below 2^28 (the chunk size of lift()).
__global__ void __launch_bounds__(256) k_lift_group(const u64* __restrict__ path, u64 nq, const u32* __restrict__ rowmap, u64 D,
                                                    u64* __restrict__ cur, u32* __restrict__ perm)
{
    __shared__ u32 cnt[LG_ROWS];
    const u64 tile = 256ull * LG_PER;
    const bool local = D <= LG_ROWS;                                      // the same for every workgroup
    for (u64 t0 = blockIdx.x * tile; t0 < nq; t0 += (u64)gridDim.x * tile) {
        if (!local) {
            for (u32 j = 0; j < LG_PER; j++) {
                const u64 q = t0 + (u64)j * 256 + threadIdx.x;
                if (q >= nq) break;
                const u64 slot = atomicAdd((unsigned long long*)&cur[rowmap[path[q]]], 1ull);
                if (perm) perm[slot] = (u32)q;
            }
            continue;
        }
        for (u32 r = threadIdx.x; r < (u32)D; r += 256) cnt[r] = 0;
        __syncthreads();
        u32 row[LG_PER], idx[LG_PER];
#pragma unroll
        for (u32 j = 0; j < LG_PER; j++) {
            const u64 q = t0 + (u64)j * 256 + threadIdx.x;
            row[j] = q < nq ? rowmap[path[q]] : ~0u;
        }
#pragma unroll
        for (u32 j = 0; j < LG_PER; j++) idx[j] = row[j] != ~0u ? atomicAdd(&cnt[row[j]], 1u) : 0u;
        __syncthreads();
        for (u32 r = threadIdx.x; r < (u32)D; r += 256) {                 // the tile's count of row r becomes its first slot
            const u32 c = cnt[r];
            if (c) cnt[r] = (u32)atomicAdd((unsigned long long*)&cur[r], (unsigned long long)c);
        }
        __syncthreads();
        if (perm) {
#pragma unroll
            for (u32 j = 0; j < LG_PER; j++)
                if (row[j] != ~0u) perm[cnt[row[j]] + idx[j]] = (u32)(t0 + (u64)j * 256 + threadIdx.x);
        }
        __syncthreads();                                                  // the next tile clears cnt
    }
}

struct LiftItem { u64 row, q0, q1; };        // slots [q0, q1) of perm hold queries of this row of the current tables

// One workgroup per item.  It keeps sym_pos of every stride-th symbol of its row in LDS; a lane finds the stretch of
// its query there and finishes with at most log2(stride) dependent steps in global memory.
__global__ void __launch_bounds__(CP_THREADS) k_lift_find(lift::LiftTab t, const LiftItem* __restrict__ items, u64 nitems,
                                                          const u32* __restrict__ perm, const u64* __restrict__ qpos,
                                                          lift::Site* __restrict__ site, uint8_t* __restrict__ status)
{
    __shared__ u64 top[LF_TOP];
    const u64 stride = (t.n + LF_TOP - 1) / LF_TOP;
    for (u64 it = blockIdx.x; it < nitems; it += gridDim.x) {
        const LiftItem item = items[it];
        const u64 kb = item.row * t.nc;
        const bool sampled = item.q1 - item.q0 >= LF_MIN && t.n > LF_TOP;      // the same for the whole workgroup
        __syncthreads();                                                       // the last item's readers of top are through
        if (sampled) {
            for (u32 j = threadIdx.x; j < LF_TOP; j += CP_THREADS) {
                const u64 i = (u64)j * stride;
                top[j] = i < t.n ? lift::sym_pos(t, kb, i) : NONE;
            }
            __syncthreads();
        }
        const u64 len = lift::sym_pos(t, kb, t.n);
        for (u64 k = item.q0 + threadIdx.x; k < item.q1; k += CP_THREADS) {
            const u64 q = perm[k], x = qpos[q];
            lift::Site s;
            uint8_t stt = lift::RANGE;
            if (x >= len) lift::no_site(s);
            else {
                u64 lo = 0, hi = t.n;
                if (sampled) {
                    u32 a = 0, b = LF_TOP;                                     // top[0] = 0 <= x
                    while (b - a > 1) { const u32 mid = (a + b) >> 1; if (top[mid] <= x) a = mid; else b = mid; }
                    lo = (u64)a * stride;
                    hi = min(lo + stride, t.n);
                }
                lift::site_at(t, kb, lift::search(t, kb, lo, hi, x), x, s);
                stt = 0;
            }
            site[q] = s;
            status[q] = stt;
        }
    }
}

// one lane per query of slots [k0, k1): the tables hold the rows of the distinct paths d0 ..; no search
__global__ void __launch_bounds__(256) k_lift_place(lift::LiftTab t, const u32* __restrict__ perm, u64 k0, u64 k1,
                                                    const u64* __restrict__ dpath, const u32* __restrict__ rowmap, u64 d0,
                                                    const lift::Site* __restrict__ site, const uint8_t* __restrict__ st_in,
                                                    u64* __restrict__ pos, uint8_t* __restrict__ st_out)
{
    for (u64 k = k0 + blockIdx.x * (u64)blockDim.x + threadIdx.x; k < k1; k += (u64)gridDim.x * blockDim.x) {
        const u64 q = perm[k], kb = ((u64)rowmap[dpath[q]] - d0) * t.nc;
        u64 p = NONE;
        uint8_t stt = lift::RANGE;
        if (st_in[q] != lift::RANGE) stt = lift::place(t, kb, site[q].symbol, site[q].string, site[q].offset, p);
        pos[q] = p;
        st_out[q] = stt;
    }
}

// the (symbol, string, offset) columns of a lift_place call as sites (the other two fields are not read)
__global__ void k_lift_pack(const u64* __restrict__ symbol, const u64* __restrict__ string, const u64* __restrict__ offset, u64 nq,
                            lift::Site* __restrict__ site)
{
    for (u64 q = blockIdx.x * (u64)blockDim.x + threadIdx.x; q < nq; q += (u64)gridDim.x * blockDim.x)
        site[q] = lift::Site{symbol[q], string[q], offset[q], 0, 0};
}

// common characters of symbol i into cc[i] (scanned in place afterwards; cc[n] = 0 becomes the total)
__global__ void k_lift_common(const u64* __restrict__ size, const u64* __restrict__ len1, u64 n, u64* __restrict__ cc)
{
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i <= n; i += (u64)gridDim.x * blockDim.x)
        cc[i] = i < n && size[i] == 1 ? len1[i] : 0;
}

} // namespace

void PathPipeline::lift_open(hipStream_t st)
{
    align_open(st);                                              // col
    if (lift_.ready || n_ == 0) return;
    const EdsView v = eds_.view();
    lift_.cum_common.ensure(8 * (n_ + 1));
    ctl_.ensure(8 * 8);
    scan_tmp_.ensure(8 * (n_ / SCAN_TILE + 4));
    const u64 cnt = n_ + 1;
    u64* ctl = ctl_.as<u64>();
    EDSX_HIP(hipMemcpyAsync(ctl, &cnt, 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_lift_common, dim3(grid_for(n_ + 1, 8192)), dim3(256), 0, st, v.sym.size, v.sym.len1, n_, lift_.cum_common.as<u64>());
    exclusive_scan_u64(lift_.cum_common.as<u64>(), lift_.cum_common.as<u64>(), ctl, ctl + 1, scan_tmp_.as<u64>(), st);
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    lift_.ready = true;
}

// queries [0, m) of lift_.q_path to the rows of the D distinct paths: lift_.perm holds them row by row, start (D + 1) where each row begins
void PathPipeline::lift_group(u64 m, u64 D, std::vector<u64>& start, hipStream_t st)
{
    u64 *cnt = lift_.cnt.as<u64>(), *cur = lift_.cur.as<u64>();
    EDSX_HIP(hipMemsetAsync(cnt, 0, 8 * (D + 1), st));
    EDSX_HIP(hipMemcpyAsync(ctl_.ptr, &D, 8, hipMemcpyHostToDevice, st));
    const unsigned grid = (unsigned)std::min<u64>((m + 256 * LG_PER - 1) / (256 * LG_PER), 4096);
    hipLaunchKernelGGL(k_lift_group, dim3(grid), dim3(256), 0, st, lift_.q_path.as<u64>(), m, lift_.map.as<u32>(), D, cnt, (u32*)nullptr);
    exclusive_scan_u64(cnt, cnt, ctl_.as<u64>(), cnt + D, scan_tmp_.as<u64>(), st);
    EDSX_HIP(hipMemcpyAsync(cur, cnt, 8 * D, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_lift_group, dim3(grid), dim3(256), 0, st, lift_.q_path.as<u64>(), m, lift_.map.as<u32>(), D, cur, lift_.perm.as<u32>());
    start.assign(D + 1, 0);
    EDSX_HIP(hipMemcpyAsync(start.data(), cnt, 8 * (D + 1), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
}

void PathPipeline::lift(size_t n, const u64* src_path, const u64* src_pos, const LiftColumns* site_in, const u64* dst_path,
                        LiftSite* site_out, u64* dst_pos, uint8_t* status, hipStream_t st)
{
    lift_run(n, src_path, src_pos, site_in, dst_path, site_out, dst_pos, status, nullptr, nullptr, st);
}

// dev_site / dev_status (device memory, n entries each; only with src_path and without dst_path): the sites and their
// statuses stay on the device for the caller's kernels, and nothing is downloaded
void PathPipeline::lift_run(size_t n, const u64* src_path, const u64* src_pos, const LiftColumns* site_in, const u64* dst_path,
                            LiftSite* site_out, u64* dst_pos, uint8_t* status, LiftSite* dev_site, uint8_t* dev_status, hipStream_t st)
{
    const bool find = src_path != nullptr, put = dst_path != nullptr;
    if (find) check_ids(src_path, n);
    if (put) check_ids(dst_path, n);
    begin_call();
    if (n == 0) return;
    lift_open(st);
    // the distinct paths of the call, ascending: one table row each
    const u64 P = info_.num_paths;
    std::vector<u32> rowmap(P + 1, 0);
    for (size_t q = 0; q < n; q++) {
        if (find) rowmap[src_path[q]] = 1;
        if (put) rowmap[dst_path[q]] = 1;
    }
    std::vector<u64> ids;
    for (u64 p = 1; p <= P; p++) if (rowmap[p]) { rowmap[p] = (u32)ids.size(); ids.push_back(p); }
    const u64 D = ids.size();
    lift_.map.ensure(4 * (P + 1));
    EDSX_HIP(hipMemcpyAsync(lift_.map.ptr, rowmap.data(), 4 * (P + 1), hipMemcpyHostToDevice, st));
    const u64 KT = table_batch(D);
    const bool single = KT >= D;
    std::vector<u64> bl, bm, start;
    if (single) tables(ids.data(), D, bl, bm, st);               // one table batch: made once for every chunk and both steps
    // queries per chunk: 88 bytes each within a quarter of the free HBM, never fewer than 65 536
    const u64 QC = std::min<u64>(std::max<u64>(budget(4) / 88, 1u << 16), 1u << 28);
    lift_.cnt.ensure(8 * (D + 1)); lift_.cur.ensure(8 * (D + 1));
    ctl_.ensure(8 * 8);
    scan_tmp_.ensure(8 * (D / SCAN_TILE + 4));
    const EdsView v = eds_.view();
    auto tab = [&] {
        return lift::LiftTab{v.sym.size, v.sym.ent_off, v.str_off, cum_fixed_.as<u64>(), rank_.as<u64>(), nc_ ? csid_.as<u64>() : nullptr,
                             nc_ ? clen_.as<u64>() : nullptr, align_.col.as<u64>(), lift_.cum_common.as<u64>(), n_, nc_};
    };
    std::vector<LiftItem> items;
    TimedRuns timed(st, nullptr);
    for (size_t c0 = 0; c0 < n; c0 += QC) {
        const u64 m = std::min<u64>(QC, n - c0);
        lift_.q_path.ensure(8 * m); lift_.q_pos.ensure(8 * m); lift_.perm.ensure(4 * m); lift_.site.ensure(sizeof(LiftSite) * m);
        lift_.st.ensure(m); lift_.st2.ensure(m);
        if (find) {
            EDSX_HIP(hipMemcpyAsync(lift_.q_path.ptr, src_path + c0, 8 * m, hipMemcpyHostToDevice, st));
            EDSX_HIP(hipMemcpyAsync(lift_.q_pos.ptr, src_pos + c0, 8 * m, hipMemcpyHostToDevice, st));
            lift_group(m, D, start, st);
            for (u64 d0 = 0; d0 < D; d0 += KT) {
                const u64 d1 = std::min<u64>(D, d0 + KT);
                if (start[d1] == start[d0]) continue;
                if (!single) tables(ids.data() + d0, d1 - d0, bl, bm, st);
                items.clear();
                for (u64 d = d0; d < d1; d++)
                    for (u64 q0 = start[d]; q0 < start[d + 1]; q0 += LF_ITEM)
                        items.push_back(LiftItem{d - d0, q0, std::min<u64>(start[d + 1], q0 + LF_ITEM)});
                lift_.items.ensure(sizeof(LiftItem) * items.size());
                EDSX_HIP(hipMemcpyAsync(lift_.items.ptr, items.data(), sizeof(LiftItem) * items.size(), hipMemcpyHostToDevice, st));
                timed.run("k_lift_find", [&] {
                    hipLaunchKernelGGL(k_lift_find, dim3((unsigned)std::min<u64>(items.size(), 1u << 20)), dim3(CP_THREADS), 0, st, tab(),
                                       lift_.items.as<LiftItem>(), (u64)items.size(), lift_.perm.as<u32>(), lift_.q_pos.as<u64>(),
                                       lift_.site.as<LiftSite>(), lift_.st.as<uint8_t>());
                }, &timing_.copy_ms);
                EDSX_HIP(hipStreamSynchronize(st));
                EDSX_HIP(hipGetLastError());
                timed.harvest();
            }
        } else {
            lift_.q_aux.ensure(8 * m);                               // the three columns as they are; packed on the device
            EDSX_HIP(hipMemcpyAsync(lift_.q_path.ptr, site_in->symbol + c0, 8 * m, hipMemcpyHostToDevice, st));
            EDSX_HIP(hipMemcpyAsync(lift_.q_pos.ptr, site_in->string + c0, 8 * m, hipMemcpyHostToDevice, st));
            EDSX_HIP(hipMemcpyAsync(lift_.q_aux.ptr, site_in->offset + c0, 8 * m, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_lift_pack, dim3(grid_for(m, 8192)), dim3(256), 0, st, lift_.q_path.as<u64>(), lift_.q_pos.as<u64>(),
                               lift_.q_aux.as<u64>(), m, lift_.site.as<LiftSite>());
            EDSX_HIP(hipMemsetAsync(lift_.st.ptr, 0, m, st));
        }
        if (put) {                                               // the sites stay where k_lift_find wrote them
            EDSX_HIP(hipMemcpyAsync(lift_.q_path.ptr, dst_path + c0, 8 * m, hipMemcpyHostToDevice, st));
            lift_group(m, D, start, st);
            for (u64 d0 = 0; d0 < D; d0 += KT) {
                const u64 d1 = std::min<u64>(D, d0 + KT);
                if (start[d1] == start[d0]) continue;
                if (!single) tables(ids.data() + d0, d1 - d0, bl, bm, st);
                timed.run("k_lift_place", [&] {
                    hipLaunchKernelGGL(k_lift_place, dim3(grid_for(start[d1] - start[d0], 8192)), dim3(256), 0, st, tab(), lift_.perm.as<u32>(),
                                       start[d0], start[d1], lift_.q_path.as<u64>(), lift_.map.as<u32>(), d0, lift_.site.as<LiftSite>(),
                                       lift_.st.as<uint8_t>(), lift_.q_pos.as<u64>(), lift_.st2.as<uint8_t>());
                }, &timing_.copy_ms);
                EDSX_HIP(hipStreamSynchronize(st));
                EDSX_HIP(hipGetLastError());
                timed.harvest();
            }
        }
        if (dev_site) {
            EDSX_HIP(hipMemcpyAsync(dev_site + c0, lift_.site.ptr, sizeof(LiftSite) * m, hipMemcpyDeviceToDevice, st));
            EDSX_HIP(hipMemcpyAsync(dev_status + c0, lift_.st.ptr, m, hipMemcpyDeviceToDevice, st));
            EDSX_HIP(hipStreamSynchronize(st));
            continue;
        }
        const auto t0 = std::chrono::steady_clock::now();
        if (site_out) EDSX_HIP(hipMemcpyAsync(site_out + c0, lift_.site.ptr, sizeof(LiftSite) * m, hipMemcpyDeviceToHost, st));
        if (dst_pos) EDSX_HIP(hipMemcpyAsync(dst_pos + c0, lift_.q_pos.ptr, 8 * m, hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipMemcpyAsync(status + c0, put ? lift_.st2.ptr : lift_.st.ptr, m, hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        timing_.download_ms += since_ms(t0);
        timing_.bytes_written += m * ((site_out ? sizeof(LiftSite) : 0) + (dst_pos ? 8 : 0) + 1);
    }
}

} // namespace edsx
