// ibs_device.hip — the segments two paths of an EDS with sources share, on gfx950 (edsparser-ibs).
//
// Under the STRINGS class list of dist_device.hip every path has exactly one bit per listed choice symbol, so with R[k]
// the bit row of path k, R[a] ^ R[b] is zero exactly where the two paths agree; its set bits, read through the
// descriptors (desc[c] >> 24 is the choice rank), are the symbols where they differ, and the shared segments are the gaps
// between consecutive differing symbols (ibs_core.hpp).  Per pair: one xor per 64 class columns plus work per difference.
//
//   rows            dist_rows (dist_device.hip): the class list of the session and the bit rows of the request
//   k_ibs_scan      one workgroup of 256 lanes per (64 x 64 tile of path pairs with tile row <= tile column, chunk of
//                   class words): both 64-row slices go through LDS 32 words at a time, rows 33 words apart as in
//                   k_dist_pairs; lane (ty, tx) holds the 4 x 4 pairs (ty + 16 i, tx + 16 j) and keeps the last differing
//                   rank of each in registers.  A zero xor word costs an xor and a compare; a non-zero word is walked
//                   bit by bit through the descriptors.  Only x < y is produced: a diagonal tile skips its lower half and
//                   its diagonal.  COUNT stores per (pair, chunk) the reported interior segments and the chunk's first
//                   and last differing rank; FILL writes the records behind the scanned offset.
//   k_ibs_stitch    one lane per pair walks its chunk edges in order and adds the segments no chunk sees: the head, the
//                   seam between the last difference of a chunk and the first of the next chunk that has one (equal
//                   ranks: none), the tail, or the whole EDS.  A seam segment belongs to the chunk where it ends and the
//                   tail to a slot of its own, so one exclusive scan over [pair][chunk + 1] gives every offset, pair_off
//                   and the total, and the records come out in (x, y, symbol_first) order without a sort.
#include "path_device.hpp"

#include <chrono>
#include <cstring>

namespace edsx {

namespace {

constexpr int IT = 256;
constexpr u32 LDS_STRIDE = dist::STAGE_WORDS + 1;
typedef unsigned __int128 u128;

enum { C_N = 0, C_TOTAL, C_CAND, C_WORDS };
enum { IBS_COUNT = 0, IBS_FILL = 1 };

struct ScanArgs {
    const u64* rows; const u64* desc;
    ibs::IbsTab t; ibs::Rule rule;
    u64 K, row_words, chunk_words, chunks, tiles;
    u64* icnt; u64* first; u64* last;          // COUNT: written; FILL: icnt is read
    const u64* off;                            // FILL: tot, scanned
    u64* ctl; IbsSegment* out;
};

// blockIdx.x: the tile pair, blockIdx.y: the chunk.  Lane (ty, tx) of 16 x 16 holds the pairs (ty + 16 i, tx + 16 j)
template <int MODE>
__global__ void __launch_bounds__(IT) k_ibs_scan(ScanArgs a)
{
    __shared__ u64 sa[dist::TILE * LDS_STRIDE];
    __shared__ u64 sb[dist::TILE * LDS_STRIDE];
    u64 tr, tc;
    dist::tile_of(a.tiles, blockIdx.x, tr, tc);
    const u64 w0 = (u64)blockIdx.y * a.chunk_words, w1 = min(a.row_words, w0 + a.chunk_words);
    const u32 tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const u64 ra0 = tr * dist::TILE + ty, rb0 = tc * dist::TILE + tx;
    u64 last[4][4], aux[4][4];                 // aux: COUNT - the reported segments so far; FILL - where the next one goes
    u32 valid = 0, cand = 0;
    int any = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u64 ra = ra0 + 16 * i, rb = rb0 + 16 * j;
            last[i][j] = ibs::NONE;
            aux[i][j] = 0;
            if (!(ra < rb && rb < a.K)) continue;
            valid |= 1u << (4 * i + j);
            if (MODE == IBS_FILL) {
                const u64 p = ibs::pair_index(a.K, ra, rb), ic = a.icnt[p * a.chunks + blockIdx.y];
                aux[i][j] = a.off[p * (a.chunks + 1) + blockIdx.y + 1] - ic;
                any |= ic != 0;
            }
        }
    if (MODE == IBS_FILL && !__syncthreads_or(any)) return;     // a tile without a reported interior segment is not walked again
    for (u64 ws = w0; ws < w1; ws += dist::STAGE_WORDS) {
        __syncthreads();                                                   // the last stage's readers are through
        for (u32 e = threadIdx.x; e < dist::TILE * dist::STAGE_WORDS; e += IT) {
            const u32 row = e / dist::STAGE_WORDS, w = e % dist::STAGE_WORDS;
            const u64 ra = tr * dist::TILE + row, rb = tc * dist::TILE + row, gw = ws + w;
            sa[row * LDS_STRIDE + w] = gw < w1 && ra < a.K ? a.rows[ra * a.row_words + gw] : 0;
            sb[row * LDS_STRIDE + w] = gw < w1 && rb < a.K ? a.rows[rb * a.row_words + gw] : 0;
        }
        __syncthreads();
        for (u32 w = 0; w < dist::STAGE_WORDS; w++) {
            u64 x[4], y[4];
#pragma unroll
            for (int i = 0; i < 4; i++) { x[i] = sa[(ty + 16 * i) * LDS_STRIDE + w]; y[i] = sb[(tx + 16 * i) * LDS_STRIDE + w]; }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const u64 d = x[i] ^ y[j];
                    if (d == 0 || !((valid >> (4 * i + j)) & 1)) continue;
                    const u64 ra = ra0 + 16 * i, rb = rb0 + 16 * j;
                    ibs::walk_word(a.desc, ws + w, d, last[i][j],
                        [&](u64 r) { if (MODE == IBS_COUNT) a.first[ibs::pair_index(a.K, ra, rb) * a.chunks + blockIdx.y] = r; },
                        [&](u64 r_prev, u64 r_next) {
                            IbsSegment s;
                            if (!ibs::gap(a.t, r_prev, r_next, s)) return;
                            if (MODE == IBS_COUNT) cand++;
                            if (!ibs::reported(a.rule, s)) return;
                            if (MODE == IBS_FILL) { s.x = ra; s.y = rb; a.out[aux[i][j]] = s; }
                            aux[i][j]++;
                        });
                }
        }
    }
    if (MODE == IBS_FILL) return;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (!((valid >> (4 * i + j)) & 1)) continue;
            const u64 slot = ibs::pair_index(a.K, ra0 + 16 * i, rb0 + 16 * j) * a.chunks + blockIdx.y;
            a.icnt[slot] = aux[i][j];
            a.last[slot] = last[i][j];
            if (last[i][j] == ibs::NONE) a.first[slot] = ibs::NONE;
        }
    const u64 c = wave_sum(cand);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd((unsigned long long*)&a.ctl[C_CAND], (unsigned long long)c);
}

struct StitchArgs {
    ibs::IbsTab t; ibs::Rule rule;
    u64 K, chunks, pairs;
    const u64* icnt; const u64* first; const u64* last;
    u64* tot;                                  // COUNT: written; FILL: scanned
    u64* pair_off; u64* ctl; IbsSegment* out;
};

// one lane per (x, y) of K x K; the lanes with x < y work
template <int MODE>
__global__ void __launch_bounds__(IT) k_ibs_stitch(StitchArgs a)
{
    const u64 total = a.K * a.K;
    for (u64 base = blockIdx.x * (u64)blockDim.x; base < total; base += (u64)gridDim.x * blockDim.x) {    // block-uniform
        const u64 e = base + threadIdx.x, x = e / a.K, y = e - x * a.K;
        u32 cand = 0;
        if (e < total && x < y) {
            const u64 p = ibs::pair_index(a.K, x, y);
            u64* tot = a.tot + p * (a.chunks + 1);
            if (MODE == IBS_COUNT) {
                for (u64 c = 0; c < a.chunks; c++) tot[c] = a.icnt[p * a.chunks + c];
                tot[a.chunks] = 0;
            } else {
                a.pair_off[p] = tot[0];
                if (p + 1 == a.pairs) a.pair_off[a.pairs] = tot[a.chunks + 1];
            }
            ibs::stitch(a.first + p * a.chunks, a.last + p * a.chunks, a.chunks, [&](u64 c, u64 r_prev, u64 r_next) {
                IbsSegment s;
                if (!ibs::gap(a.t, r_prev, r_next, s)) return;
                if (MODE == IBS_COUNT) cand++;
                if (!ibs::reported(a.rule, s)) return;
                if (MODE == IBS_COUNT) tot[c]++;
                else { s.x = x; s.y = y; a.out[tot[c]] = s; }
            });
        }
        if (MODE == IBS_COUNT) {
            const u64 c = wave_sum(cand);
            if ((threadIdx.x & 63) == 0 && c) atomicAdd((unsigned long long*)&a.ctl[C_CAND], (unsigned long long)c);
        }
    }
}

std::string bytes_text(u128 v) { return std::to_string((u64)std::min<u128>(v, ~0ull)); }

} // namespace

void PathPipeline::ibs(const u64* ids, size_t n, u64 min_sites, u64 min_columns, u64 max_segments, HostBytes& segments,
                       HostBytes& pair_off, IbsInfo& info, KernelTimes* times, hipStream_t st)
{
    info = IbsInfo{};
    check_ids(ids, n);
    begin_call();
    segments.take(0);
    pair_off.take(8);
    std::memset(pair_off.data, 0, 8);
    std::vector<u64> all;
    if (n == 0) {
        for (u64 p = 1; p <= info_.num_paths; p++) all.push_back(p);
        ids = all.data(); n = all.size();
    }
    const u64 K = n;
    const u128 pairs128 = K ? (u128)K * (K - 1) / 2 : 0;
    info.paths = K; info.choice_symbols = nc_; info.chunk_columns = 64ull * dist::MIN_CHUNK_WORDS;
    info.pairs = (u64)std::min<u128>(pairs128, ~0ull);
    if (pairs128 == 0) return;

    if (!ibs_.ready) { align_open(st); ibs_.ready = true; }      // col
    TimedRuns timed(st, times);
    const u64 cap = budget(2);
    u64 C = 0;
    u128 rows128 = 0, scratch128 = 0;
    auto fits = [&](u64 columns, const dist::Plan& pl) {
        C = columns;
        info.class_columns = C; info.chunk_columns = 64 * pl.chunk_words; info.chunks = pl.chunks;
        rows128 = (u128)8 * K * pl.row_words;
        scratch128 = pairs128 * (24 * pl.chunks + 8 * (pl.chunks + 1)) + 8 + 8 * (pairs128 + 1);
        if (rows128 + scratch128 > cap)
            throw LimitError("The IBS rows (" + bytes_text(rows128) + " bytes) and the pair scratch (" + bytes_text(scratch128) +
                             " bytes) do not fit the budget of " + std::to_string(cap) + " bytes; request fewer paths at a time");
    };
    dist::Plan pl = dist::plan(K, 0);
    if (nc_) pl = dist_rows(ids, n, dist::STRINGS, nullptr, timed, [&](const DistClasses& c, const dist::Plan& p) { fits(c.C, p); }, st);
    else fits(0, pl);                                            // no choice symbol: every pair shares the whole EDS

    const u64 pairs = (u64)pairs128, chunks = pl.chunks, slots = pairs * chunks, N = pairs * (chunks + 1) + 1;
    ibs_.icnt.ensure(8 * std::max<u64>(slots, 1));
    ibs_.first.ensure(8 * std::max<u64>(slots, 1));
    ibs_.last.ensure(8 * std::max<u64>(slots, 1));
    ibs_.tot.ensure(8 * N);
    ibs_.pair_off.ensure(8 * (pairs + 1));
    ctl_.ensure(8 * 8);
    scan_tmp_.ensure(8 * (N / SCAN_TILE + 4));
    u64 h[C_WORDS] = {N, 0, 0};
    u64 *ctl = ctl_.as<u64>(), *tot = ibs_.tot.as<u64>();
    EDSX_HIP(hipMemcpyAsync(ctl, h, sizeof(h), hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemsetAsync(tot + (N - 1), 0, 8, st));
    const ibs::IbsTab t{cidx_.as<u64>(), align_.col.as<u64>(), n_, nc_};
    const ibs::Rule rule{min_sites, min_columns};
    ScanArgs sa{dist_.rows.as<u64>(), chunks ? dist_.cls[dist::STRINGS].desc.as<u64>() : nullptr, t, rule, K, pl.row_words, pl.chunk_words,
                chunks, pl.tiles, ibs_.icnt.as<u64>(), ibs_.first.as<u64>(), ibs_.last.as<u64>(), tot, ctl, nullptr};
    StitchArgs sg{t, rule, K, chunks, pairs, ibs_.icnt.as<u64>(), ibs_.first.as<u64>(), ibs_.last.as<u64>(), tot, ibs_.pair_off.as<u64>(), ctl,
                  nullptr};
    const dim3 scan_grid((unsigned)pl.tile_pairs, (unsigned)std::max<u64>(chunks, 1)), stitch_grid(grid_for(K * K, 16384));
    if (chunks)
        timed.run("k_ibs_scan", [&] { hipLaunchKernelGGL((k_ibs_scan<IBS_COUNT>), scan_grid, dim3(IT), 0, st, sa); }, &timing_.copy_ms);
    timed.run("k_ibs_stitch", [&] { hipLaunchKernelGGL((k_ibs_stitch<IBS_COUNT>), stitch_grid, dim3(IT), 0, st, sg); }, &timing_.scan_ms);
    timed.run("scan_segments", [&] { exclusive_scan_u64(tot, tot, ctl + C_N, ctl + C_TOTAL, scan_tmp_.as<u64>(), st); }, &timing_.scan_ms);
    EDSX_HIP(hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    timed.harvest();
    const u64 total = h[C_TOTAL];
    info.candidate_segments = h[C_CAND]; info.segments = total;
    if (max_segments && total > max_segments)
        throw ParamError("IBS has " + std::to_string(total) + " segments, above the limit of " + std::to_string(max_segments));
    const u128 out128 = (u128)sizeof(IbsSegment) * total;
    if (rows128 + scratch128 + out128 > cap)
        throw LimitError("The IBS rows (" + bytes_text(rows128) + " bytes), the pair scratch (" + bytes_text(scratch128) + " bytes) and the segments (" +
                         bytes_text(out128) + " bytes) do not fit the budget of " + std::to_string(cap) +
                         " bytes; request fewer paths at a time");
    pair_off.take(8 * (pairs + 1));
    std::memset(pair_off.data, 0, pair_off.size);
    segments.take((size_t)out128);
    timing_.bytes_written = (u64)out128 + 8 * (pairs + 1);
    if (total == 0) return;
    ibs_.seg.ensure((u64)out128);
    sa.off = tot; sa.out = sg.out = ibs_.seg.as<IbsSegment>();
    if (chunks)
        timed.run("k_ibs_scan", [&] { hipLaunchKernelGGL((k_ibs_scan<IBS_FILL>), scan_grid, dim3(IT), 0, st, sa); }, &timing_.copy_ms);
    timed.run("k_ibs_stitch", [&] { hipLaunchKernelGGL((k_ibs_stitch<IBS_FILL>), stitch_grid, dim3(IT), 0, st, sg); }, &timing_.scan_ms);
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    timed.harvest();
    const auto t0 = std::chrono::steady_clock::now();
    PinnedDownload::copy(segments.data, ibs_.seg.ptr, (size_t)out128, st);
    PinnedDownload::copy(pair_off.data, ibs_.pair_off.ptr, 8 * (pairs + 1), st);
    timing_.download_ms += since_ms(t0);
}

} // namespace edsx
