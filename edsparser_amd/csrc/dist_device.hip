// dist_device.hip — pairwise distances between the paths of an EDS with sources on gfx950 (edsparser-dist).
//
// Two paths differ only at choice symbols, and there every string's source set is a bitset over paths that is already in
// HBM.  dist_core.hpp gives every compared unit - a choice symbol (STRINGS) or an alignment column of one (COLUMNS) - a set
// of class columns such that a path has exactly one class per unit; with R[k] the bit row of path k over the C class
// columns of the V listed units,  D[a][b] = V - popcount(R[a] & R[b]).
//
//   first call      k_dist_symbols  per choice symbol: may it leave a path without a string (the OR of its sets lacks an id
//                                   of 1..P and none is universal), and its width, scanned once (ccol)
//   first call per metric: the class list, session state - it does not depend on the request
//                   k_dist_count    one lane per unit: its classes (COLUMNS: a 256-bit mask of the bytes present, in
//                                   registers); a unit with one class is not listed
//                   one exclusive scan, then k_dist_fill: one 8-byte descriptor per class column
//   per table batch k_path_choose (tables()), then
//                   k_dist_rows     one lane per (path, 64 class columns): reads the descriptors, tests csid and the
//                                   string's byte at the offset, stores one u64; no atomics, padding bits are zero
//   per call        k_dist_pairs    one workgroup of 256 lanes per (64 x 64 tile of path pairs with tile row <= tile
//                                   column, chunk of class words): both 64-row operand slices go through LDS 32 words at a
//                                   time, rows 33 words apart so that the 16 rows a wave reads lie in different banks; a
//                                   lane holds 4 x 4 pairs, and + 2 x v_bcnt_u32_b32 per 64-bit pair-word, 32-bit sums
//                                   within a chunk, one 64-bit atomic add per pair and chunk.  Rows past K and words past
//                                   the row read as zero.  (MFMA does not fit: i8 operands would be the bit rows blown up
//                                   eight times for no gain in rate.)
//                   k_dist_finish   D = V - S into both triangles, zeros on the diagonal
#include "path_device.hpp"

#include <chrono>
#include <cstring>

namespace edsx {

namespace {

constexpr int DT = 256;
constexpr u32 LDS_STRIDE = dist::STAGE_WORDS + 1;
typedef unsigned __int128 u128;

// r <= nc: ccol[r] = the width of choice symbol r (0 at nc: scanned in place afterwards), mm[r] = it may leave a path out
__global__ void __launch_bounds__(DT) k_dist_symbols(const u64* __restrict__ size, const u64* __restrict__ ent_off,
                                                     const u64* __restrict__ bits, u32 W, u64 P, const u64* __restrict__ cidx,
                                                     const u64* __restrict__ col, u64 nc, u64* __restrict__ ccol, uint8_t* __restrict__ mm)
{
    for (u64 r = blockIdx.x * (u64)blockDim.x + threadIdx.x; r <= nc; r += (u64)gridDim.x * blockDim.x) {
        if (r == nc) { ccol[r] = 0; continue; }
        const u64 i = cidx[r];
        ccol[r] = col[i + 1] - col[i];
        mm[r] = dist::may_miss(bits, W, ent_off[i], size[i], P) ? 1 : 0;
    }
}

// cnt[u] = the class columns of unit u (u <= U; 0 at U: scanned in place afterwards); ctl[2] += the units listed, ctl[3] =
// the size of the largest symbol that has no room in a descriptor
template <int METRIC>
__global__ void __launch_bounds__(DT) k_dist_count(dist::DistTab t, u64 U, u64* __restrict__ cnt, u64* __restrict__ ctl)
{
    for (u64 base = blockIdx.x * (u64)blockDim.x; base <= U; base += (u64)gridDim.x * blockDim.x) {       // block-uniform
        const u64 u = base + threadIdx.x;
        u64 c = 0;
        if (u < U) {
            if (METRIC == dist::STRINGS) {
                c = dist::string_count(t, u);
                const u64 sz = t.size[t.cidx[u]];
                if (sz >= dist::NOSTRING) atomicMax((unsigned long long*)&ctl[3], sz);
            } else {
                const u64 r = dist::unit_symbol(t, u);
                dist::Present m;
                bool nochar;
                dist::column_classes(t, r, u - t.ccol[r], m, nochar);
                c = dist::column_count(m, nochar);
            }
        }
        if (u <= U) cnt[u] = c;
        const u64 listed = wave_sum(c ? 1 : 0);
        if ((threadIdx.x & 63) == 0 && listed) atomicAdd((unsigned long long*)&ctl[2], listed);
    }
}

// cnt: scanned (U + 1 entries)
template <int METRIC>
__global__ void __launch_bounds__(DT) k_dist_fill(dist::DistTab t, u64 U, const u64* __restrict__ cnt, u64* __restrict__ desc)
{
    for (u64 u = blockIdx.x * (u64)blockDim.x + threadIdx.x; u < U; u += (u64)gridDim.x * blockDim.x) {
        const u64 at = cnt[u];
        if (cnt[u + 1] == at) continue;
        if (METRIC == dist::STRINGS) dist::string_fill(t, u, desc + at);
        else {
            const u64 r = dist::unit_symbol(t, u);
            dist::Present m;
            bool nochar;
            dist::column_classes(t, r, u - t.ccol[r], m, nochar);
            dist::column_fill(m, nochar, u, desc + at);
        }
    }
}

struct RowArgs {
    dist::DistTab t; dist::Metric metric;
    const u64* desc; u64 C, row_words;
    const u64* csid; u64 K;                    // the table batch: K rows of nc chosen strings
    u64* rows;                                 // the bit row of the batch's first path
};

__global__ void __launch_bounds__(DT) k_dist_rows(RowArgs a)
{
    const u64 total = a.K * a.row_words;
    for (u64 x = blockIdx.x * (u64)blockDim.x + threadIdx.x; x < total; x += (u64)gridDim.x * blockDim.x) {
        const u64 k = x / a.row_words, wd = x - k * a.row_words;
        a.rows[x] = dist::row_word(a.t, a.metric, a.desc, a.C, a.csid + k * a.t.nc, wd);
    }
}

struct PairArgs { const u64* rows; u64 K, row_words, chunk_words, tiles; u64* sums; };

// blockIdx.x: the tile pair, blockIdx.y: the chunk.  Lane (ty, tx) of 16 x 16 holds the pairs (ty + 16 i, tx + 16 j)
__global__ void __launch_bounds__(DT) k_dist_pairs(PairArgs a)
{
    __shared__ u64 sa[dist::TILE * LDS_STRIDE];
    __shared__ u64 sb[dist::TILE * LDS_STRIDE];
    u64 tr, tc;
    dist::tile_of(a.tiles, blockIdx.x, tr, tc);
    const u64 w0 = (u64)blockIdx.y * a.chunk_words, w1 = min(a.row_words, w0 + a.chunk_words);
    const u32 tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    u32 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = 0;
    for (u64 ws = w0; ws < w1; ws += dist::STAGE_WORDS) {
        __syncthreads();                                                   // the last stage's readers are through
        for (u32 e = threadIdx.x; e < dist::TILE * dist::STAGE_WORDS; e += DT) {
            const u32 row = e / dist::STAGE_WORDS, w = e % dist::STAGE_WORDS;
            const u64 ra = tr * dist::TILE + row, rb = tc * dist::TILE + row, gw = ws + w;
            sa[row * LDS_STRIDE + w] = gw < w1 && ra < a.K ? a.rows[ra * a.row_words + gw] : 0;
            sb[row * LDS_STRIDE + w] = gw < w1 && rb < a.K ? a.rows[rb * a.row_words + gw] : 0;
        }
        __syncthreads();
#pragma unroll 2
        for (u32 w = 0; w < dist::STAGE_WORDS; w++) {
            u64 x[4], y[4];
#pragma unroll
            for (int i = 0; i < 4; i++) { x[i] = sa[(ty + 16 * i) * LDS_STRIDE + w]; y[i] = sb[(tx + 16 * i) * LDS_STRIDE + w]; }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] += (u32)__builtin_popcountll(x[i] & y[j]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u64 ra = tr * dist::TILE + ty + 16 * i, rb = tc * dist::TILE + tx + 16 * j;
            if (ra < a.K && rb < a.K && acc[i][j]) atomicAdd((unsigned long long*)&a.sums[ra * a.K + rb], (unsigned long long)acc[i][j]);
        }
}

// in place: the lane of a pair a < b reads the sum of the upper triangle and writes both entries; nobody reads the lower
__global__ void __launch_bounds__(DT) k_dist_finish(u64* __restrict__ sums, u64 K, u64 V)
{
    const u64 total = K * K;
    for (u64 x = blockIdx.x * (u64)blockDim.x + threadIdx.x; x < total; x += (u64)gridDim.x * blockDim.x) {
        const u64 p = x / K, q = x - p * K;
        if (p == q) sums[x] = 0;
        else if (p < q) { const u64 d = V - sums[x]; sums[x] = d; sums[q * K + p] = d; }
    }
}

} // namespace

void PathPipeline::dist_open(hipStream_t st)
{
    if (dist_.ready || nc_ == 0) return;
    align_open(st);                                              // col
    const EdsView v = eds_.view();
    dist_.may_miss.ensure(nc_);
    dist_.ccol.ensure(8 * (nc_ + 1));
    ctl_.ensure(8 * 8);
    scan_tmp_.ensure(8 * ((nc_ + 1) / SCAN_TILE + 4));
    u64 h[2] = {nc_ + 1, 0};
    u64 *ctl = ctl_.as<u64>(), *ccol = dist_.ccol.as<u64>();
    EDSX_HIP(hipMemcpyAsync(ctl, h, sizeof(h), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_dist_symbols, dim3(grid_for(nc_ + 1, 8192)), dim3(DT), 0, st, v.sym.size, v.sym.ent_off, v.bits, v.W,
                       info_.num_paths, cidx_.as<u64>(), align_.col.as<u64>(), nc_, ccol, dist_.may_miss.as<uint8_t>());
    exclusive_scan_u64(ccol, ccol, ctl, ctl + 1, scan_tmp_.as<u64>(), st);
    EDSX_HIP(hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    dist_.CW = h[1];
    dist_.ready = true;
}

void PathPipeline::dist_classes(dist::Metric metric, TimedRuns& timed, hipStream_t st)
{
    DistClasses& c = dist_.cls[metric];
    if (c.ready) return;
    const EdsView v = eds_.view();
    const dist::DistTab t{v.sym.size, v.sym.ent_off, v.str_off, v.chars, cidx_.as<u64>(), dist_.ccol.as<u64>(), dist_.may_miss.as<uint8_t>(), nc_};
    const u64 U = metric == dist::STRINGS ? nc_ : dist_.CW;
    dist_.cnt.ensure(8 * (U + 1));
    ctl_.ensure(8 * 8);
    scan_tmp_.ensure(8 * ((U + 1) / SCAN_TILE + 4));
    u64 h[4] = {U + 1, 0, 0, 0};                                 // count; C; V; a symbol with too many strings
    u64 *ctl = ctl_.as<u64>(), *cnt = dist_.cnt.as<u64>();
    EDSX_HIP(hipMemcpyAsync(ctl, h, sizeof(h), hipMemcpyHostToDevice, st));
    const dim3 grid(grid_for(U + 1, 16384));
    timed.run("k_dist_count", [&] {
        if (metric == dist::STRINGS) hipLaunchKernelGGL((k_dist_count<dist::STRINGS>), grid, dim3(DT), 0, st, t, U, cnt, ctl);
        else hipLaunchKernelGGL((k_dist_count<dist::COLUMNS>), grid, dim3(DT), 0, st, t, U, cnt, ctl);
    }, &timing_.scan_ms);
    timed.run("scan_classes", [&] { exclusive_scan_u64(cnt, cnt, ctl, ctl + 1, scan_tmp_.as<u64>(), st); }, &timing_.scan_ms);
    EDSX_HIP(hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    timed.harvest();
    if (h[3]) throw LimitError("A symbol has " + std::to_string(h[3]) + " strings, above the " + std::to_string(dist::NOSTRING - 1) +
                               " a distance descriptor can name");
    c.C = h[1]; c.V = h[2];
    c.desc.ensure(8 * std::max<u64>(c.C, 1));
    if (c.C) {
        timed.run("k_dist_fill", [&] {
            if (metric == dist::STRINGS) hipLaunchKernelGGL((k_dist_fill<dist::STRINGS>), grid, dim3(DT), 0, st, t, U, cnt, c.desc.as<u64>());
            else hipLaunchKernelGGL((k_dist_fill<dist::COLUMNS>), grid, dim3(DT), 0, st, t, U, cnt, c.desc.as<u64>());
        }, &timing_.scan_ms);
        EDSX_HIP(hipStreamSynchronize(st));
        EDSX_HIP(hipGetLastError());
        timed.harvest();
    }
    dist_.cnt.release();                                         // 8 bytes per unit, needed once per metric
    c.ready = true;
}

// The class list of `metric` and the bit rows of ids[0..n) in dist_.rows, K x plan.row_words words: dist_open, dist_classes,
// then fits(classes, plan) - the caller's info and its budget check, which throws -, then the batched tables() + k_dist_rows
// loop.  missing (nullable): n entries.  Needs nc_ > 0.  distances() and ibs() (ibs_device.hip) both build their rows here.
dist::Plan PathPipeline::dist_rows(const u64* ids, size_t n, dist::Metric m, u64* missing, TimedRuns& timed,
                                   const std::function<void(const DistClasses&, const dist::Plan&)>& fits, hipStream_t st)
{
    dist_open(st);
    dist_classes(m, timed, st);
    const DistClasses& c = dist_.cls[m];
    const dist::Plan pl = dist::plan(n, c.C);
    fits(c, pl);
    dist_.rows.ensure(std::max<u64>(8 * (u64)n * pl.row_words, 8));

    const EdsView v = eds_.view();
    const dist::DistTab t{v.sym.size, v.sym.ent_off, v.str_off, v.chars, cidx_.as<u64>(), dist_.ccol.as<u64>(), dist_.may_miss.as<uint8_t>(), nc_};
    const u64 KT = table_batch(n);
    std::vector<u64> len, miss;
    for (size_t i0 = 0; i0 < n; i0 += KT) {
        const u64 Kb = std::min<u64>(KT, n - i0);
        tables(ids + i0, Kb, len, miss, st);
        if (missing) std::memcpy(missing + i0, miss.data(), 8 * Kb);
        if (!c.C) continue;
        const RowArgs ra{t, m, c.desc.as<u64>(), c.C, pl.row_words, csid_.as<u64>(), Kb, dist_.rows.as<u64>() + i0 * pl.row_words};
        timed.run("k_dist_rows", [&] {
            hipLaunchKernelGGL(k_dist_rows, dim3(grid_for(Kb * pl.row_words, 16384)), dim3(DT), 0, st, ra);
        }, &timing_.copy_ms);
    }
    return pl;
}

void PathPipeline::distances(const u64* ids, size_t n, int metric, u64 max_bytes, u64* matrix, u64* missing, DistInfo& info,
                             KernelTimes* times, hipStream_t st)
{
    info = DistInfo{};
    if (metric != dist::COLUMNS && metric != dist::STRINGS)
        throw ParamError("Distance metric " + std::to_string(metric) + " is not known (0: columns, 1: strings)");
    check_ids(ids, n);
    const u128 mat128 = (u128)8 * n * n;
    if ((max_bytes && mat128 > max_bytes) || mat128 > ~0ull) {
        const std::string have = mat128 > ~0ull ? "more than " + std::to_string(~0ull) : std::to_string((u64)mat128);
        throw ParamError("Distance matrix has " + have + " bytes, above the limit of " + std::to_string(max_bytes ? max_bytes : ~0ull));
    }
    if (n && !matrix) throw ParamError("null argument");
    begin_call();
    const dist::Metric m = (dist::Metric)metric;
    if (m == dist::COLUMNS) { align_open(st); info.units = align_.info.n_columns; }
    else info.units = n_;
    info.chunk_columns = 64ull * dist::MIN_CHUNK_WORDS;
    if (n == 0) return;
    const u64 K = n, mat = (u64)mat128;
    std::memset(matrix, 0, mat);
    if (missing) std::memset(missing, 0, 8 * K);
    timing_.bytes_written = mat;
    if (nc_ == 0) return;                                        // no choice symbol: all paths are the same sequence

    TimedRuns timed(st, times);                                  // every run with a bucket, as slice()
    const u64 cap = budget(2);
    const dist::Plan pl = dist_rows(ids, n, m, missing, timed, [&](const DistClasses& c, const dist::Plan& pl) {
        info.variable_units = c.V; info.class_columns = c.C; info.chunk_columns = 64 * pl.chunk_words; info.chunks = pl.chunks;
        const u128 rows128 = (u128)8 * K * pl.row_words;
        if (rows128 + mat128 > cap)
            throw LimitError("The distance rows (" + std::to_string((u64)std::min<u128>(rows128, ~0ull)) + " bytes) and the matrix (" +
                             std::to_string(mat) + " bytes) do not fit the budget of " + std::to_string(cap) +
                             " bytes; request fewer paths at a time");
    }, st);
    const DistClasses& c = dist_.cls[m];
    dist_.sums.ensure(mat);
    EDSX_HIP(hipMemsetAsync(dist_.sums.ptr, 0, mat, st));
    if (c.C) {
        const PairArgs pa{dist_.rows.as<u64>(), K, pl.row_words, pl.chunk_words, pl.tiles, dist_.sums.as<u64>()};
        timed.run("k_dist_pairs", [&] {
            hipLaunchKernelGGL(k_dist_pairs, dim3((unsigned)pl.tile_pairs, (unsigned)pl.chunks), dim3(DT), 0, st, pa);
        }, &timing_.copy_ms);
        timed.run("k_dist_finish", [&] {
            hipLaunchKernelGGL(k_dist_finish, dim3(grid_for(K * K, 16384)), dim3(DT), 0, st, dist_.sums.as<u64>(), K, c.V);
        }, &timing_.copy_ms);
    }
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    timed.harvest();
    if (c.C) {
        const auto t0 = std::chrono::steady_clock::now();
        PinnedDownload::copy(matrix, dist_.sums.ptr, mat, st);
        timing_.download_ms += since_ms(t0);
    }
}

} // namespace edsx
