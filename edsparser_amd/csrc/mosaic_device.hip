// mosaic_device.hip — a path of an EDS with sources as a minimal mosaic of other paths, on gfx950 (edsparser-mosaic,
// DESIGN 8o).
//
// Under the STRINGS class list of dist_device.hip every path has exactly one bit per listed choice symbol, so with R[k] the
// bit row of path k, R[t] & ~R[d] has one set bit per symbol where donor d differs from target t, at the column of the
// target's own bit (mosaic_core.hpp).  The mosaic is a greedy march along the class words: a set of alive donors - those
// that agree with the target since the segment's start - shrinks until its last members die inside one word; the donor that
// dies last (then the smallest request position) gives the segment, and the march restarts at that symbol with the donors
// that agree there, or with a private run when nobody does.
//
//   rows             dist_rows (dist_device.hip): the class list of the session and the bit rows of the distinct paths of
//                    both lists
//   k_mosaic_donors  the donor rows word-major in request order, RT[w][y] = R[donors[y]][w], through 32 x 32 LDS tiles, so
//                    that the march reads one word of 256 donors as 2 KiB in a row, whatever the donor list names
//   k_mosaic         one workgroup of 256 lanes per target, donors across lanes (lane l: donors l, l + 256, ..), the alive
//                    bits of a lane's donors in words of its own.  Per class word a lane forms R[t] & ~R[d] for its alive
//                    donors; while a donor of the workgroup survives the word that is all (one __syncthreads_or).  When
//                    none does, the lanes reduce (furthest bit, smallest position) with a 64-bit LDS max, lane 0 closes
//                    the segment, and one bit test per eligible donor in the same word gives the next alive set.  COUNT
//                    stores the segments per target, one exclusive scan gives target_off, FILL repeats the march and
//                    writes the records, so they are sized exactly and come back in (target, symbol_first) order.
// An EDS without class columns has no word to march over: the code behind the loop writes the one segment per target.
// A single target is one workgroup marching alone: the parallelism is targets x donors (Measured).
#include "path_device.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>

namespace edsx {

namespace {

constexpr int MT = 256;
constexpr u32 TR = 32;                         // the transpose tile
typedef unsigned __int128 u128;

enum { C_N = 0, C_TOTAL, C_PRIV_SEGS, C_PRIV_SYMS, C_WORDS };
enum { MOSAIC_COUNT = 0, MOSAIC_FILL = 1 };

struct DonorArgs { const u64* rows; const u64* drow; u64 D, RW; u64* rt; };

// blockIdx.x: 32 donors, blockIdx.y: 32 words (grid-stride over both); 256 lanes move a 32 x 32 tile in four steps
__global__ void __launch_bounds__(MT) k_mosaic_donors(DonorArgs a)
{
    __shared__ u64 tile[TR * (TR + 1)];
    const u32 lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const u64 ty_n = (a.D + TR - 1) / TR, tw_n = (a.RW + TR - 1) / TR;
    for (u64 q = blockIdx.x; q < ty_n * tw_n; q += gridDim.x) {            // block-uniform
        const u64 y0 = q % ty_n * TR, w0 = q / ty_n * TR;
        __syncthreads();
        for (u32 k = ly; k < TR; k += 8) {                                 // donor y0 + k, word w0 + lx
            const u64 y = y0 + k, w = w0 + lx;
            tile[k * (TR + 1) + lx] = y < a.D && w < a.RW ? a.rows[a.drow[y] * a.RW + w] : 0;
        }
        __syncthreads();
        for (u32 k = ly; k < TR; k += 8) {                                 // word w0 + k, donor y0 + lx
            const u64 y = y0 + lx, w = w0 + k;
            if (y < a.D && w < a.RW) a.rt[w * a.D + y] = tile[lx * (TR + 1) + k];
        }
    }
}

struct MosaicArgs {
    const u64* rows; const u64* rt; const u64* desc;
    mosaic::Tab t;
    const u64* trow; const u64* drow;          // the row of every target and of every donor
    u64 T, D, RW, KW;
    u64* alive;                                // T x KW x 256
    u64* cnt;                                  // COUNT: written; FILL: scanned
    u64* ctl; MosaicSegment* out;
};

// what goes over the donors of one workgroup (mosaic_core.hpp, march)
struct Lanes {
    const MosaicArgs& a;
    u64 tr;                                    // the target's row: a donor of that row is the target itself
    u64* al;                                   // this lane's alive words, 256 apart
    u64* sh;                                   // one LDS word

    __device__ u64 donor(u64 kk, u32 b) const { return mosaic::donor_of(kk, b, threadIdx.x, MT); }
    __device__ bool eligible(u64 y) const { return y < a.D && a.drow[y] != tr; }
    __device__ void reset() const
    {
        for (u64 kk = 0; kk < a.KW; kk++) {
            u64 m = 0;
            for (u32 b = 0; b < 64; b++) m |= (u64)eligible(donor(kk, b)) << b;
            al[kk * MT] = m;
        }
    }
    // the alive donors of word kk that have no difference in class word w
    __device__ u64 clean(u64 kk, u64 am, u64 w, u64 tw, u64 mask) const
    {
        u64 nm = 0;
        for (u64 x = am; x; x &= x - 1) {
            const u32 b = (u32)__builtin_ctzll(x);
            if (!mosaic::differ_word(tw, a.rt[w * a.D + donor(kk, b)], mask)) nm |= 1ull << b;
        }
        return nm;
    }
    __device__ bool survive(u64 w, u64 tw, u64 mask) const
    {
        int some = 0, changed = 0;
        for (u64 kk = 0; kk < a.KW; kk++) {
            const u64 am = al[kk * MT], nm = clean(kk, am, w, tw, mask);
            some |= nm != 0;
            changed |= nm != am;
        }
        if (!__syncthreads_or(some)) return false;
        if (changed)
            for (u64 kk = 0; kk < a.KW; kk++) {
                const u64 am = al[kk * MT], nm = clean(kk, am, w, tw, mask);
                if (nm != am) al[kk * MT] = nm;
            }
        return true;
    }
    __device__ u64 death(u64 w, u64 tw, u64 mask) const
    {
        if (threadIdx.x == 0) *sh = 0;
        __syncthreads();
        u64 best = 0;
        for (u64 kk = 0; kk < a.KW; kk++)
            for (u64 x = al[kk * MT]; x; x &= x - 1) {
                const u64 y = donor(kk, (u32)__builtin_ctzll(x));
                const u64 d = mosaic::differ_word(tw, a.rt[w * a.D + y], mask);      // not zero: nobody survived
                best = max(best, mosaic::death_key((u32)__builtin_ctzll(d), y));
            }
        if (best) atomicMax((unsigned long long*)sh, (unsigned long long)best);
        __syncthreads();
        const u64 key = *sh;
        __syncthreads();
        return key;
    }
    __device__ bool agree(u64 w, u64 c) const
    {
        int some = 0;
        for (u64 kk = 0; kk < a.KW; kk++) {
            u64 m = 0;
            for (u32 b = 0; b < 64; b++) {
                const u64 y = donor(kk, b);
                if (eligible(y) && mosaic::agrees_at(a.rt[w * a.D + y], c)) m |= 1ull << b;
            }
            al[kk * MT] = m;
            some |= m != 0;
        }
        return __syncthreads_or(some);
    }
    __device__ u64 first() const
    {
        if (threadIdx.x == 0) *sh = mosaic::NONE;
        __syncthreads();
        for (u64 kk = 0; kk < a.KW; kk++) {
            const u64 am = al[kk * MT];
            if (am) { atomicMin((unsigned long long*)sh, (unsigned long long)donor(kk, (u32)__builtin_ctzll(am))); break; }
        }
        __syncthreads();
        const u64 y = *sh;
        __syncthreads();
        return y;
    }
};

// blockIdx.x: the target (request position)
template <int MODE>
__global__ void __launch_bounds__(MT) k_mosaic(MosaicArgs a)
{
    __shared__ u64 sh;
    const u64 x = blockIdx.x;
    if (a.t.n == 0) {
        if (MODE == MOSAIC_COUNT && threadIdx.x == 0) a.cnt[x] = 0;
        return;
    }
    const Lanes lanes{a, a.trow[x], a.alive + x * a.KW * MT + threadIdx.x, &sh};
    const u64 base = MODE == MOSAIC_FILL ? a.cnt[x] : 0;
    auto emit = [&](u64 k, u64 donor, u64 first, u64 end) {
        if (MODE == MOSAIC_FILL && threadIdx.x == 0) a.out[base + k] = mosaic::segment(a.t, x, donor, first, end);
    };
    int some = 0;
    for (u64 y = threadIdx.x; y < a.D; y += MT) some |= lanes.eligible(y);
    mosaic::March m;
    if (__syncthreads_or(some)) m = mosaic::march(a.t, a.desc, a.rows + lanes.tr * a.RW, a.RW, lanes, emit);
    else mosaic::close(m, mosaic::NONE, a.t.n, emit);                      // nobody to copy from
    if (MODE == MOSAIC_FILL || threadIdx.x) return;
    a.cnt[x] = m.segments;
    if (m.private_segments) {
        atomicAdd((unsigned long long*)&a.ctl[C_PRIV_SEGS], (unsigned long long)m.private_segments);
        atomicAdd((unsigned long long*)&a.ctl[C_PRIV_SYMS], (unsigned long long)m.private_symbols);
    }
}

std::string bytes_text(u128 v) { return std::to_string((u64)std::min<u128>(v, ~0ull)); }

} // namespace

void PathPipeline::mosaic(const u64* targets, size_t nt, const u64* donors, size_t nd, u64 max_segments, HostBytes& segments,
                          HostBytes& target_off, MosaicInfo& info, KernelTimes* times, hipStream_t st)
{
    info = MosaicInfo{};
    check_ids(targets, nt);
    check_ids(donors, nd);
    begin_call();
    segments.take(0);
    std::vector<u64> all;
    if (nt == 0 || nd == 0)
        for (u64 p = 1; p <= info_.num_paths; p++) all.push_back(p);
    if (nt == 0) { targets = all.data(); nt = all.size(); }
    if (nd == 0) { donors = all.data(); nd = all.size(); }
    const u64 T = nt, D = nd;
    target_off.take(8 * (T + 1));
    std::memset(target_off.data, 0, target_off.size);
    info.targets = T; info.donors = D; info.choice_symbols = nc_;
    if (T == 0 || n_ == 0) return;                               // no path, or no symbol: no record

    // the distinct paths of both lists, ascending: one bit row each
    std::vector<u64> ids(targets, targets + T);
    ids.insert(ids.end(), donors, donors + D);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const u64 K = ids.size();
    std::vector<u64> rowof(T + D);
    for (u64 k = 0; k < T + D; k++) rowof[k] = (u64)(std::lower_bound(ids.begin(), ids.end(), k < T ? targets[k] : donors[k - T]) - ids.begin());

    if (!mosaic_.ready) { align_open(st); mosaic_.ready = true; }      // col
    TimedRuns timed(st, times);
    const u64 cap = budget(2), KW = mosaic::alive_words(D, MT);
    u64 RW = 0;
    u128 rows128 = 0, scratch128 = 0;
    auto fits = [&](u64 columns, const dist::Plan& pl) {
        RW = pl.row_words;
        info.class_columns = columns;
        rows128 = (u128)8 * K * RW;
        scratch128 = (u128)8 * D * RW + (u128)8 * T * KW * MT + 8 * ((u128)T + 1) + 8 * ((u128)T + D);
        if (rows128 + scratch128 > cap)
            throw LimitError("The mosaic rows (" + bytes_text(rows128) + " bytes) and the donor scratch (" + bytes_text(scratch128) +
                             " bytes) do not fit the budget of " + std::to_string(cap) + " bytes; request fewer paths at a time");
    };
    if (nc_) dist_rows(ids.data(), K, dist::STRINGS, nullptr, timed, [&](const DistClasses& c, const dist::Plan& p) { fits(c.C, p); }, st);
    else fits(0, dist::plan(K, 0));                              // no choice symbol: one segment per target

    mosaic_.rowof.ensure(8 * (T + D));
    mosaic_.rt.ensure(std::max<u64>(8 * D * RW, 8));
    mosaic_.alive.ensure(8 * T * KW * MT);
    mosaic_.cnt.ensure(8 * (T + 1));
    ctl_.ensure(8 * 8);
    scan_tmp_.ensure(8 * ((T + 1) / SCAN_TILE + 4));
    u64 h[C_WORDS] = {T + 1, 0, 0, 0};
    u64 *ctl = ctl_.as<u64>(), *cnt = mosaic_.cnt.as<u64>();
    EDSX_HIP(hipMemcpyAsync(ctl, h, sizeof(h), hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemcpyAsync(mosaic_.rowof.ptr, rowof.data(), 8 * (T + D), hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemsetAsync(cnt + T, 0, 8, st));
    const u64 *trow = mosaic_.rowof.as<u64>(), *drow = trow + T;
    const u64* rows = RW ? dist_.rows.as<u64>() : nullptr;
    if (RW) {
        const DonorArgs da{rows, drow, D, RW, mosaic_.rt.as<u64>()};
        const u64 tiles = ((D + TR - 1) / TR) * ((RW + TR - 1) / TR);
        timed.run("k_mosaic_donors", [&] {
            hipLaunchKernelGGL(k_mosaic_donors, dim3((unsigned)std::min<u64>(tiles, 65536)), dim3(MT), 0, st, da);
        }, &timing_.copy_ms);
    }
    MosaicArgs ma{rows, mosaic_.rt.as<u64>(), RW ? dist_.cls[dist::STRINGS].desc.as<u64>() : nullptr,
                  mosaic::Tab{cidx_.as<u64>(), align_.col.as<u64>(), n_, nc_}, trow, drow, T, D, RW, KW, mosaic_.alive.as<u64>(), cnt, ctl,
                  nullptr};
    // (the pointer arithmetic of an absent row table: a.rows + row * 0)
    timed.run("k_mosaic", [&] { hipLaunchKernelGGL((k_mosaic<MOSAIC_COUNT>), dim3((unsigned)T), dim3(MT), 0, st, ma); }, &timing_.copy_ms);
    timed.run("scan_segments", [&] { exclusive_scan_u64(cnt, cnt, ctl + C_N, ctl + C_TOTAL, scan_tmp_.as<u64>(), st); }, &timing_.scan_ms);
    EDSX_HIP(hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    timed.harvest();
    const u64 total = h[C_TOTAL];
    info.segments = total; info.private_segments = h[C_PRIV_SEGS]; info.private_symbols = h[C_PRIV_SYMS]; info.switches = total - T;
    if (max_segments && total > max_segments)
        throw ParamError("Mosaic has " + std::to_string(total) + " segments, above the limit of " + std::to_string(max_segments));
    const u128 out128 = (u128)sizeof(MosaicSegment) * total;
    if (rows128 + scratch128 + out128 > cap)
        throw LimitError("The mosaic rows (" + bytes_text(rows128) + " bytes), the donor scratch (" + bytes_text(scratch128) +
                         " bytes) and the segments (" + bytes_text(out128) + " bytes) do not fit the budget of " + std::to_string(cap) +
                         " bytes; request fewer paths at a time");
    segments.take((size_t)out128);
    timing_.bytes_written = (u64)out128 + 8 * (T + 1);
    mosaic_.seg.ensure((u64)out128);
    ma.out = mosaic_.seg.as<MosaicSegment>();
    timed.run("k_mosaic", [&] { hipLaunchKernelGGL((k_mosaic<MOSAIC_FILL>), dim3((unsigned)T), dim3(MT), 0, st, ma); }, &timing_.copy_ms);
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    timed.harvest();
    const auto t0 = std::chrono::steady_clock::now();
    PinnedDownload::copy(segments.data, mosaic_.seg.ptr, (size_t)out128, st);
    PinnedDownload::copy(target_off.data, mosaic_.cnt.ptr, 8 * (T + 1), st);
    timing_.download_ms += since_ms(t0);
}

} // namespace edsx
