// div_device.hip — windowed diversity between groups of paths of an EDS with sources on gfx950 (edsparser-diversity).
//
// The source set of every string is a bitset over paths in HBM, allele-major; every statistic is a sum over choice symbols
// of small products of c_g(r, j) = popcount(T(r, j) & mask_g) (div_core.hpp).
//
//   per call  k_div_sites    LG = min(pow2ceil(WP), 32) lanes share a choice symbol, 64 / LG symbols a wave; a lane keeps the
//                            `seen` words of its RW row words in registers (RW = 1: WP <= 32; RW = 4: WP <= 128; RW = 0:
//                            a row of `seen` per lane group in HBM).  Per string the counts of GT groups (DIAG: the pairs
//                            inside one tile of GT groups) or 2 GT groups (the pairs between two tiles) by popcounts and a
//                            shuffle reduction inside the lane group; n_g, the strings with a carrier and sum_j c_g c_h stay
//                            in registers; lane 0 of the group writes seg, present, diff and comp of the symbol, array-major.
//                            G <= 4 is one launch, G = 16 ten.  DIAG launches walk a symbol at which a group is complete a
//                            second time for the SFS bins: an LDS histogram per workgroup when all bins fit, else HBM atomics
//             scans          the NA arrays, four at a time (exclusive_scan_multi)
//             k_div_windows  a lane per (window, group or pair): the difference of two prefixes; in COLUMNS the ranks of the
//                            window by bisection over the columns of the choice symbols
#include "path_device.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>

namespace edsx {

namespace {

namespace dv = diversity;

constexpr int LT = 256;
constexpr u32 SFS_LDS_BINS = 2048;
constexpr u32 MAX_LG = 32;
typedef unsigned __int128 u128;

struct SiteArgs {
    const u64* size; const u64* ent_off; const u64* bits; u32 W;
    const u64* cidx; u64 nc;
    const u64* masks; u64 P, WP;                  // G x WP
    u32 G, ga, gb, LG;                            // the tiles begin at the groups ga and gb (DIAG: ga == gb)
    u64 K[dv::MAX_GROUPS], sfs_off[dv::MAX_GROUPS + 1];
    u64* arr; u64 stride;
    u64* sfs; int sfs_lds;                        // sfs == nullptr: no spectrum
    u64* seen;                                    // RW == 0: WP words per lane group of the grid
};

// the counts c[0..NG) of string j of the symbol for the lane group, in every lane of the group; seen takes the carriers.
// RW != 0: the lane's words of the mask rows are in registers (mreg), and so is seen; RW == 0: both in HBM
template <int NG, int RW>
__device__ __forceinline__ void count_string(const SiteArgs& a, const u64* __restrict__ b, const u64* (&mrow)[NG], const u64 (&mreg)[NG][RW ? RW : 1],
                                             u32 g, u64* seen_row, u64 (&seen)[RW ? RW : 1], u32 (&c)[NG])
{
#pragma unroll
    for (int x = 0; x < NG; x++) c[x] = 0;
    if constexpr (RW != 0) {
#pragma unroll
        for (int k = 0; k < RW; k++) {
            const u64 w = g + (u64)k * a.LG;
            if (w < a.WP) {
                const u64 t = ld::walk_step(b, a.W, w, dv::valid_word(a.P, a.WP, w), seen[k]);
#pragma unroll
                for (int x = 0; x < NG; x++) c[x] += dv::group_count(t, mreg[x][k]);
            }
        }
    } else {
        for (u64 w = g; w < a.WP; w += a.LG) {
            u64 s = seen_row[w];
            const u64 t = ld::walk_step(b, a.W, w, dv::valid_word(a.P, a.WP, w), s);
            seen_row[w] = s;
#pragma unroll
            for (int x = 0; x < NG; x++) if (mrow[x]) c[x] += dv::group_count(t, mrow[x][w]);
        }
    }
    for (u32 o = a.LG >> 1; o > 0; o >>= 1) {
#pragma unroll
        for (int x = 0; x < NG; x++) c[x] += __shfl_xor(c[x], (int)o, 64);
    }
}

// entry nc of every array: 0, so that the scans leave the totals there
__global__ void __launch_bounds__(LT) k_div_tails(u64* __restrict__ arr, u64 stride, u64 nc, u64 NA)
{
    for (u64 x = blockIdx.x * (u64)blockDim.x + threadIdx.x; x < NA; x += (u64)gridDim.x * blockDim.x) arr[x * stride + nc] = 0;
}

template <int GT, int RW, bool DIAG>
__global__ void __launch_bounds__(LT) k_div_sites(SiteArgs a)
{
    constexpr int NG = DIAG ? GT : 2 * GT;
    constexpr int NACC = DIAG ? GT * (GT + 1) / 2 : GT * GT;
    constexpr int RR = RW ? RW : 1;
    __shared__ u64 hist[DIAG ? SFS_LDS_BINS : 1];
    const bool lds = DIAG && a.sfs && a.sfs_lds;
    if (lds) {
        for (u32 k = threadIdx.x; k < SFS_LDS_BINS; k += LT) hist[k] = 0;
        __syncthreads();
    }
    const u32 g = threadIdx.x & (a.LG - 1);
    const u64 slot = (blockIdx.x * (u64)blockDim.x + threadIdx.x) / a.LG, nslots = ((u64)gridDim.x * blockDim.x) / a.LG;
    const u64* mrow[NG];                                          // the mask rows of the groups of this launch; null: no such group
    u64 mreg[NG][RR];
#pragma unroll
    for (int x = 0; x < NG; x++) {
        const u32 grp = (x < GT ? a.ga : a.gb - GT) + x;
        mrow[x] = grp < a.G ? a.masks + (u64)grp * a.WP : nullptr;
#pragma unroll
        for (int k = 0; k < RR; k++) {
            const u64 w = g + (u64)k * a.LG;
            mreg[x][k] = RW && mrow[x] && w < a.WP ? mrow[x][w] : 0;
        }
    }
    u64* seen_row = RW ? nullptr : a.seen + slot * a.WP;
    for (u64 r = slot; r < a.nc; r += nslots) {                   // the lanes of a group share r, and so every branch below
        const u64 i = a.cidx[r], e0 = a.ent_off[i], sz = a.size[i];
        u64 seen[RR];
#pragma unroll
        for (int k = 0; k < RR; k++) seen[k] = 0;
        if (!RW) for (u64 w = g; w < a.WP; w += a.LG) seen_row[w] = 0;
        u32 c[NG];
        dv::GroupSums gs[NG];
        u64 acc[NACC];
#pragma unroll
        for (int x = 0; x < NG; x++) gs[x] = dv::GroupSums{0, 0};
#pragma unroll
        for (int q = 0; q < NACC; q++) acc[q] = 0;
        for (u64 j = 0; j < sz; j++) {
            count_string<NG, RW>(a, a.bits + (e0 + j) * a.W, mrow, mreg, g, seen_row, seen, c);
#pragma unroll
            for (int x = 0; x < NG; x++) dv::add_string(gs[x], c[x]);
            int q = 0;
#pragma unroll
            for (int x = 0; x < GT; x++)
#pragma unroll
                for (int y = DIAG ? x : 0; y < GT; y++) acc[q++] += (u64)c[x] * c[DIAG ? y : GT + y];
        }
        if (g == 0) {
            int q = 0;
#pragma unroll
            for (int x = 0; x < GT; x++) {
                const u32 gx = a.ga + x;
                if (DIAG && gx < a.G) {
                    a.arr[dv::arr_seg(a.G, gx) * a.stride + r] = dv::segregating(gs[x]);
                    a.arr[dv::arr_present(a.G, gx) * a.stride + r] = gs[x].n;
                }
#pragma unroll
                for (int y = DIAG ? x : 0; y < GT; y++, q++) {
                    const u32 gy = a.gb + y;
                    if (gx >= a.G || gy >= a.G) continue;
                    const u64 p = dv::pair_index(a.G, gx, gy);
                    const u64 nx = gs[x].n, ny = gs[DIAG ? y : GT + y].n;
                    const bool same = DIAG && x == y;
                    a.arr[dv::arr_diff(a.G, p) * a.stride + r] = same ? dv::diff_within(nx, acc[q]) : dv::diff_between(nx, ny, acc[q]);
                    a.arr[dv::arr_comp(a.G, p) * a.stride + r] = same ? dv::comp_within(nx) : dv::comp_between(nx, ny);
                }
            }
        }
        if (DIAG && a.sfs) {                                      // the spectrum: complete groups only, so the symbol is walked again
            u32 complete = 0;
#pragma unroll
            for (int x = 0; x < GT; x++) if (a.ga + x < a.G && gs[x].n == a.K[a.ga + x]) complete |= 1u << x;
            if (complete) {
#pragma unroll
                for (int k = 0; k < RR; k++) seen[k] = 0;
                if (!RW) for (u64 w = g; w < a.WP; w += a.LG) seen_row[w] = 0;
                for (u64 j = 0; j < sz; j++) {
                    count_string<NG, RW>(a, a.bits + (e0 + j) * a.W, mrow, mreg, g, seen_row, seen, c);
                    if (g != 0) continue;
#pragma unroll
                    for (int x = 0; x < GT; x++) {
                        if (a.ga + x >= a.G || !dv::sfs_counts(j, gs[x].n, a.K[a.ga + x])) continue;
                        const u64 bin = a.sfs_off[a.ga + x] + c[x];
                        if (lds) atomicAdd((unsigned long long*)&hist[bin], 1ull);
                        else atomicAdd((unsigned long long*)&a.sfs[bin], 1ull);
                    }
                }
            }
        }
    }
    if (lds) {
        __syncthreads();
        const u64 bins = a.sfs_off[a.G];
        for (u32 k = threadIdx.x; k < bins; k += LT) if (hist[k]) atomicAdd((unsigned long long*)&a.sfs[k], (unsigned long long)hist[k]);
    }
}

struct WinArgs {
    const u64* arr; u64 stride, nc, NW, E, size, step; int unit;
    const u64* cidx; const u64* col;
    u64 G, NP;
    DivWindow* win; DivGroup* grp; DivPair* pr;
};

// one lane per (window, group or pair); the lane of group 0 writes the window record
__global__ void __launch_bounds__(LT) k_div_windows(WinArgs a)
{
    const u64 items = a.G + a.NP, total = a.NW * items;
    for (u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x; t < total; t += (u64)gridDim.x * blockDim.x) {
        const u64 k = t / items, x = t % items;
        u64 start, end;
        dv::window_bounds(k, a.E, a.size, a.step, start, end);
        const u64 r0 = dv::rank_at(a.unit, a.nc, a.cidx, a.col, a.E, start), r1 = dv::rank_at(a.unit, a.nc, a.cidx, a.col, a.E, end);
        if (x == 0) a.win[k] = DivWindow{start, end, r0, r1};
        if (x < a.G) {
            const u64 *s = a.arr + dv::arr_seg(a.G, x) * a.stride, *p = a.arr + dv::arr_present(a.G, x) * a.stride;
            a.grp[k * a.G + x] = DivGroup{s[r1] - s[r0], p[r1] - p[r0]};
        } else {
            const u64 q = x - a.G;
            const u64 *d = a.arr + dv::arr_diff(a.G, q) * a.stride, *c = a.arr + dv::arr_comp(a.G, q) * a.stride;
            a.pr[k * a.NP + q] = DivPair{d[r1] - d[r0], c[r1] - c[r0]};
        }
    }
}

template <int GT, int RW>
void launch_sites(const SiteArgs& a, unsigned grid, hipStream_t st)
{
    if (a.ga == a.gb) hipLaunchKernelGGL((k_div_sites<GT, RW, true>), dim3(grid), dim3(LT), 0, st, a);
    else if constexpr (GT > 1) hipLaunchKernelGGL((k_div_sites<GT, RW, false>), dim3(grid), dim3(LT), 0, st, a);
}

std::string bytes_text(u128 v) { return std::to_string((u64)std::min<u128>(v, ~0ull)); }

} // namespace

void PathPipeline::diversity(const u64* group_off, const u64* group_ids, size_t n_groups, const DivOpts& o, HostBytes& windows, HostBytes& groups,
                             HostBytes& pairs, HostBytes* sfs, DivInfo& info, KernelTimes* times, hipStream_t st)
{
    info = DivInfo{};
    const u64 G = n_groups ? n_groups : 1, P = info_.num_paths, WP = (P + 63) / 64;
    if (G > dv::MAX_GROUPS)
        throw ParamError("Diversity has " + std::to_string(G) + " groups, above the limit of " + std::to_string(dv::MAX_GROUPS));
    if (o.unit != dv::SYMBOLS && o.unit != dv::COLUMNS) throw ParamError("The diversity unit is neither symbols nor columns");
    const u64 n_ids = n_groups ? group_off[n_groups] : 0;
    if (n_groups) {
        for (size_t g = 0; g < n_groups; g++)
            if (group_off[g] > group_off[g + 1]) throw ParamError("The group offsets decrease at group " + std::to_string(g));
        check_ids(group_ids + group_off[0], n_ids - group_off[0]);
        for (size_t g = 0; g < n_groups; g++)
            if (group_off[g] == group_off[g + 1]) throw ParamError("Group " + std::to_string(g) + " is empty");
    }
    begin_call();
    windows.take(0); groups.take(0); pairs.take(0);
    if (sfs) sfs->take(0);

    std::vector<u64> mask(G * std::max<u64>(WP, 1), 0);          // group-major rows: path p at bit p - 1
    if (n_groups == 0) for (u64 p = 1; p <= P; p++) mask[(p - 1) >> 6] |= 1ull << ((p - 1) & 63);
    else {
        std::vector<std::pair<u64, u64>> owner;                  // (path, group), duplicates inside a group once
        for (size_t g = 0; g < n_groups; g++)
            for (u64 k = group_off[g]; k < group_off[g + 1]; k++) owner.emplace_back(group_ids[k], (u64)g);
        std::sort(owner.begin(), owner.end());
        owner.erase(std::unique(owner.begin(), owner.end()), owner.end());
        for (size_t k = 1; k < owner.size(); k++)
            if (owner[k].first == owner[k - 1].first)
                throw ParamError("Path id " + std::to_string(owner[k].first) + " is in groups " + std::to_string(owner[k - 1].second) + " and " +
                                 std::to_string(owner[k].second));
        for (const auto& pg : owner) mask[pg.second * WP + ((pg.first - 1) >> 6)] |= 1ull << ((pg.first - 1) & 63);
    }
    SiteArgs sa{};
    u64 kmax = 0, ktotal = 0, bins = 0;
    for (u64 g = 0; g < G; g++) {
        u64 K = 0;
        for (u64 w = 0; w < WP; w++) K += (u64)__builtin_popcountll(mask[g * WP + w]);
        sa.K[g] = K; sa.sfs_off[g] = bins;
        bins += K + 1; ktotal += K; kmax = std::max(kmax, K);
    }
    sa.sfs_off[G] = bins;
    const u64 NP = dv::num_pairs(G), NA = dv::num_arrays(G);
    info.groups = G; info.paths = ktotal; info.choice_symbols = nc_; info.pairs = NP; info.row_words = WP;
    u64 E = nc_;
    if (o.unit == dv::COLUMNS) { align_open(st); E = std::max<u64>(align_.info.n_columns, 1); }
    info.extent = E;
    if (nc_ == 0) return;                                        // (P >= 1 here: a choice symbol names a path)

    const u64 NW = dv::window_count(E, o.size, o.step);
    info.windows = NW;
    if (o.max_windows && NW > o.max_windows)
        throw ParamError("Diversity has " + std::to_string(NW) + " windows, above the limit of " + std::to_string(o.max_windows));
    if (!dv::sums_fit(nc_, kmax))
        throw LimitError("Diversity sums of " + std::to_string(nc_) + " choice symbols over groups of up to " + std::to_string(kmax) +
                         " paths do not fit 64 bits");

    // geometry: lanes per symbol, the register path, the grid
    u32 LG = 1;
    while (LG < WP && LG < MAX_LG) LG <<= 1;
    const int RW = WP <= LG ? 1 : WP <= 4 * (u64)LG ? 4 : 0;
    const u64 want_blocks = (nc_ * LG + LT - 1) / LT;
    unsigned grid = (unsigned)std::max<u64>(1, std::min<u64>(want_blocks, RW ? 4096 : 512));
    const u64 cap = budget(2);
    const u128 arr128 = (u128)8 * NA * (nc_ + 1);
    const u128 out128 = (u128)NW * (sizeof(DivWindow) + G * sizeof(DivGroup) + NP * sizeof(DivPair)) + (u128)8 * bins;
    u128 seen128 = 0;
    if (!RW) {                                                   // the seen rows: as many lane groups as the budget leaves room for
        const u128 row = (u128)8 * WP, left = arr128 + out128 < cap ? cap - arr128 - out128 : 0;
        const u64 fit = (u64)std::min<u128>(left / row / (LT / LG), grid);
        grid = (unsigned)std::max<u64>(1, fit);
        seen128 = row * grid * (LT / LG);
    }
    if (arr128 + out128 + seen128 > cap)
        throw LimitError("The diversity sums per choice symbol (" + bytes_text(arr128) + " bytes), the records (" + bytes_text(out128) +
                         " bytes) and the walk rows (" + bytes_text(seen128) + " bytes) do not fit the budget of " + std::to_string(cap) +
                         " bytes; request fewer groups or slice the EDS");

    TimedRuns timed(st, times);
    const EdsView v = eds_.view();
    div_.masks.ensure(std::max<u64>(8 * G * WP, 8));
    div_.arr.ensure((u64)arr128);
    div_.win.ensure(sizeof(DivWindow) * NW);
    div_.grp.ensure(sizeof(DivGroup) * NW * G);
    div_.pr.ensure(sizeof(DivPair) * NW * NP);
    if (sfs) div_.sfs.ensure(8 * bins);
    if (!RW) div_.seen.ensure((u64)seen128);
    ctl_.ensure(8 * 8);
    scan_tmp_.ensure(8 * 4 * ((nc_ + 1) / SCAN_TILE + 4));
    u64* ctl = ctl_.as<u64>();
    const u64 stride = nc_ + 1;
    EDSX_HIP(hipMemcpyAsync(ctl, &stride, 8, hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemcpyAsync(div_.masks.ptr, mask.data(), 8 * G * WP, hipMemcpyHostToDevice, st));
    if (sfs) EDSX_HIP(hipMemsetAsync(div_.sfs.ptr, 0, 8 * bins, st));

    sa.size = v.sym.size; sa.ent_off = v.sym.ent_off; sa.bits = v.bits; sa.W = v.W;
    sa.cidx = cidx_.as<u64>(); sa.nc = nc_;
    sa.masks = div_.masks.as<u64>(); sa.P = P; sa.WP = WP;
    sa.G = (u32)G; sa.LG = LG;
    sa.arr = div_.arr.as<u64>(); sa.stride = stride;
    sa.sfs = sfs ? div_.sfs.as<u64>() : nullptr; sa.sfs_lds = bins <= SFS_LDS_BINS ? 1 : 0;
    sa.seen = RW ? nullptr : div_.seen.as<u64>();
    const u32 GT = G == 1 ? 1 : 4;
    timed.run("k_div_tails", [&] { hipLaunchKernelGGL(k_div_tails, dim3(grid_for(NA, 8)), dim3(LT), 0, st, sa.arr, stride, nc_, NA); }, &timing_.scan_ms);
    for (u32 ga = 0; ga < G; ga += GT)
        for (u32 gb = ga; gb < G; gb += GT) {
            sa.ga = ga; sa.gb = gb;
            timed.run("k_div_sites", [&] {
                if (GT == 1) { if (RW == 1) launch_sites<1, 1>(sa, grid, st); else if (RW == 4) launch_sites<1, 4>(sa, grid, st); else launch_sites<1, 0>(sa, grid, st); }
                else { if (RW == 1) launch_sites<4, 1>(sa, grid, st); else if (RW == 4) launch_sites<4, 4>(sa, grid, st); else launch_sites<4, 0>(sa, grid, st); }
            }, &timing_.copy_ms);
        }
    u64* arr = div_.arr.as<u64>();
    for (u64 a0 = 0; a0 < NA; a0 += 4)                           // NA is even
        timed.run("scan_div", [&] {
            if (NA - a0 >= 4) {
                ScanSet<4> ss;
                for (int k = 0; k < 4; k++) { ss.in[k] = ss.out[k] = arr + (a0 + k) * stride; ss.total[k] = ctl + 1 + k; }
                exclusive_scan_multi<4>(ss, ctl, scan_tmp_.as<u64>(), st);
            } else {
                ScanSet<2> ss;
                for (int k = 0; k < 2; k++) { ss.in[k] = ss.out[k] = arr + (a0 + k) * stride; ss.total[k] = ctl + 1 + k; }
                exclusive_scan_multi<2>(ss, ctl, scan_tmp_.as<u64>(), st);
            }
        }, &timing_.scan_ms);
    const WinArgs wa{arr, stride, nc_, NW, E, o.size, o.step, o.unit, cidx_.as<u64>(), o.unit == dv::COLUMNS ? align_.col.as<u64>() : nullptr,
                     G, NP, div_.win.as<DivWindow>(), div_.grp.as<DivGroup>(), div_.pr.as<DivPair>()};
    timed.run("k_div_windows", [&] {
        hipLaunchKernelGGL(k_div_windows, dim3(grid_for(NW * (G + NP), 8192)), dim3(LT), 0, st, wa);
    }, &timing_.scan_ms);
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    timed.harvest();

    const auto t0 = std::chrono::steady_clock::now();
    windows.take(sizeof(DivWindow) * NW);
    groups.take(sizeof(DivGroup) * NW * G);
    pairs.take(sizeof(DivPair) * NW * NP);
    PinnedDownload::copy(windows.data, div_.win.ptr, windows.size, st);
    PinnedDownload::copy(groups.data, div_.grp.ptr, groups.size, st);
    PinnedDownload::copy(pairs.data, div_.pr.ptr, pairs.size, st);
    timing_.bytes_written = windows.size + groups.size + pairs.size;
    if (sfs) {
        sfs->take(8 * bins);
        PinnedDownload::copy(sfs->data, div_.sfs.ptr, 8 * bins, st);
        timing_.bytes_written += 8 * bins;
    }
    timing_.download_ms += since_ms(t0);
}

} // namespace edsx
