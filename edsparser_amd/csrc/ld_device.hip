// ld_device.hip — linkage disequilibrium between the alleles of an EDS with sources on gfx950 (edsparser-ld).
//
// The source set of every string is a bitset over paths that is already in HBM, allele-major: the co-occurrence count of
// two alleles is popcount(T_x & T_y) over their carrier rows (ld_core.hpp), and the r² of all pairs within a window of
// choice symbols is a banded popcount product over allele rows.
//
//   first call  soff            the strings in front of every choice symbol, scanned once
//   per call    k_ld_count      a wave per choice symbol, lanes over row words: the prefix-OR walk over its strings; per
//                               string its carriers by a wave reduction, the paths present, how many alleles are listed
//                               and whether the symbol needs a presence row; one scan gives afirst, uidx, A
//               k_ld_rows       the same walk again: the T rows of the listed alleles (A x WP words, padding zero), the U
//                               rows of the symbols that leave a path of M out, the allele table
//               k_ld_tiles      per row tile of 64 alleles the column tiles its band touches, scanned (tstart); per
//                               allele its partners, summed: the candidate pairs
//               k_ld_pairs      one workgroup of 256 lanes per (row tile, column tile) for ALL row words: both 64-row
//                               slices go through LDS 32 words at a time, rows 33 words apart as in k_dist_pairs; lane
//                               (ty, tx) keeps the 4 x 4 pairs (ty + 16 i, tx + 16 j), and + 2 x v_bcnt_u32_b32 per pair
//                               word, sums complete in registers.  The epilogue tests the band, takes n, n_a, n_b from K
//                               and the counts - or, where a symbol has a U row, from three more popcounts over the rows
//                               in HBM -, computes ld::r2 and sets the bit of a reported pair in a 64-bit mask per tile
//                               row in LDS.  COUNT stores popcount(mask) per (allele, column tile), allele-major, and adds
//                               the undefined pairs; one scan; FILL runs the tiles whose counters are not all zero again
//                               and writes pair (x, y) at start[x][tile] + popcount(mask & below(y)).
//                               (MFMA does not fit, for the reason dist_device.hip gives.)
#include "path_device.hpp"

#include <chrono>
#include <cmath>
#include <cstring>

namespace edsx {

namespace {

constexpr int LT = 256;
constexpr u32 LDS_STRIDE = ld::STAGE_WORDS + 1;
typedef unsigned __int128 u128;

// ctl words
enum { C_N = 0, C_A, C_NU, C_CAND, C_UNDEF, C_TN, C_NT, C_PN, C_PAIRS, C_WORDS };

__global__ void __launch_bounds__(LT) k_ld_sizes(const u64* __restrict__ size, const u64* __restrict__ cidx, u64 nc, u64* __restrict__ soff)
{
    for (u64 r = blockIdx.x * (u64)blockDim.x + threadIdx.x; r <= nc; r += (u64)gridDim.x * blockDim.x) soff[r] = r < nc ? size[cidx[r]] : 0;
}

struct WalkArgs {
    const u64* size; const u64* ent_off; const u64* bits; u32 W;
    const u64* cidx; const u64* soff; u64 nc;
    const u64* mask; u64 WP, K;
    u64 min_count; int all_strings;
};

// cnt: S; pres: nc; lcount, hasu: nc + 1 (0 at nc: scanned in place afterwards)
__global__ void __launch_bounds__(LT) k_ld_count(WalkArgs a, u64* __restrict__ cnt, u64* __restrict__ pres, u64* __restrict__ lcount,
                                                 u64* __restrict__ hasu)
{
    const u32 lane = threadIdx.x & 63;
    const u64 nwaves = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 r = (blockIdx.x * (u64)blockDim.x + threadIdx.x) >> 6; r <= a.nc; r += nwaves) {            // wave-uniform
        if (r == a.nc) { if (lane == 0) { lcount[r] = 0; hasu[r] = 0; } continue; }
        const u64 i = a.cidx[r], e0 = a.ent_off[i], sz = a.size[i], s0 = a.soff[r];
        u64 present = 0;
        for (u64 wb = 0; wb < a.WP; wb += 64) {
            const u64 w = wb + lane;
            const bool act = w < a.WP;
            const u64 m = act ? a.mask[w] : 0;
            u64 seen = 0;
            for (u64 j = 0; j < sz; j++) {
                const u64 t = act ? ld::walk_step(a.bits + (e0 + j) * a.W, a.W, w, m, seen) : 0;
                const u64 c = wave_sum((u64)__builtin_popcountll(t));
                if (lane == 0) cnt[s0 + j] = (wb ? cnt[s0 + j] : 0) + c;
            }
            present += wave_sum((u64)__builtin_popcountll(seen));
        }
        if (lane == 0) {                                          // (the lane that wrote the counts reads them)
            u64 l = 0;
            for (u64 j = 0; j < sz; j++) l += ld::listed(j, a.all_strings != 0, cnt[s0 + j], present, a.min_count) ? 1 : 0;
            pres[r] = present;
            lcount[r] = l;
            hasu[r] = l && present < a.K ? 1 : 0;
        }
    }
}

// afirst, uidx: scanned
__global__ void __launch_bounds__(LT) k_ld_rows(WalkArgs a, const u64* __restrict__ cnt, const u64* __restrict__ pres,
                                                const u64* __restrict__ afirst, const u64* __restrict__ uidx, u64* __restrict__ trows,
                                                u64* __restrict__ urows, LdAllele* __restrict__ al, u64* __restrict__ ar)
{
    const u32 lane = threadIdx.x & 63;
    const u64 nwaves = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 r = (blockIdx.x * (u64)blockDim.x + threadIdx.x) >> 6; r < a.nc; r += nwaves) {
        const u64 a0 = afirst[r];
        if (afirst[r + 1] == a0) continue;
        const u64 i = a.cidx[r], e0 = a.ent_off[i], sz = a.size[i], s0 = a.soff[r], present = pres[r];
        const u64 ui = uidx[r + 1] != uidx[r] ? uidx[r] : ld::NONE;
        for (u64 wb = 0; wb < a.WP; wb += 64) {
            const u64 w = wb + lane;
            const bool act = w < a.WP;
            const u64 m = act ? a.mask[w] : 0;
            u64 seen = 0, x = a0;
            for (u64 j = 0; j < sz; j++) {
                const u64 t = act ? ld::walk_step(a.bits + (e0 + j) * a.W, a.W, w, m, seen) : 0;
                const u64 c = cnt[s0 + j];
                if (!ld::listed(j, a.all_strings != 0, c, present, a.min_count)) continue;
                if (act) trows[x * a.WP + w] = t;
                if (wb == 0 && lane == 0) { al[x] = LdAllele{i, j, c, present}; ar[x] = r; }
                x++;
            }
            if (ui != ld::NONE && act) urows[ui * a.WP + w] = seen;
        }
    }
}

// ntile[t] (t <= RT; 0 at RT: scanned in place afterwards); ctl[C_CAND] += the partners of every allele
__global__ void __launch_bounds__(LT) k_ld_tiles(const u64* __restrict__ afirst, const u64* __restrict__ ar, u64 nc, u64 A, u64 RT, u64 window,
                                                 u64* __restrict__ ntile, u64* __restrict__ ctl)
{
    for (u64 base = blockIdx.x * (u64)blockDim.x; base < A; base += (u64)gridDim.x * blockDim.x) {        // block-uniform; RT < A
        const u64 x = base + threadIdx.x;
        u64 partners = 0;
        if (x < A) { const u64 r = ar[x]; partners = ld::partner_hi(afirst, nc, r, window) - ld::partner_lo(afirst, r); }
        if (x <= RT) {
            u64 c0 = 0, c1 = 0;
            if (x < RT) ld::tile_columns(afirst, nc, ar[x * ld::TILE], ar[min(A, (x + 1) * ld::TILE) - 1], window, c0, c1);
            ntile[x] = c1 - c0;
        }
        partners = wave_sum(partners);
        if ((threadIdx.x & 63) == 0 && partners) atomicAdd((unsigned long long*)&ctl[C_CAND], partners);
    }
}

struct PairArgs {
    const u64* trows; const u64* urows; const u64* mask;
    const u64* ar; const LdAllele* al; const u64* pres; const u64* uidx; const u64* afirst; const u64* tstart;
    u64 A, WP, K, nc, RT, window;
    double min_r2;
    u64* cntx;                                 // COUNT: the counters, written; FILL: scanned
    u64* ctl; LdPair* out;
};

enum { LD_COUNT = 0, LD_FILL = 1 };
enum { P_NONE = 0, P_UNDEFINED, P_BELOW, P_REPORTED };

// the pair of the alleles x < A and y < A with n_ab common carriers
__device__ __forceinline__ int pair_eval(const PairArgs& a, u64 x, u64 y, u64 n_ab, LdPair& p)
{
    const u64 rx = a.ar[x], ry = a.ar[y];
    if (!ld::pair_valid(rx, ry, a.window)) return P_NONE;
    const u64 px = a.pres[rx], py = a.pres[ry];
    u64 n = a.K, n_a = a.al[x].count, n_b = a.al[y].count;
    if (px < a.K || py < a.K) {                                  // rare: three more popcounts straight from the rows
        const u64* ux = px < a.K ? a.urows + a.uidx[rx] * a.WP : a.mask;
        const u64* uy = py < a.K ? a.urows + a.uidx[ry] * a.WP : a.mask;
        const u64 *tx = a.trows + x * a.WP, *ty = a.trows + y * a.WP;
        n = n_a = n_b = 0;
        for (u64 w = 0; w < a.WP; w++) {
            n += (u64)__builtin_popcountll(ux[w] & uy[w]);
            n_a += (u64)__builtin_popcountll(tx[w] & uy[w]);
            n_b += (u64)__builtin_popcountll(ty[w] & ux[w]);
        }
    }
    p.n_ab = n_ab; p.n_a = n_a; p.n_b = n_b; p.n = n;
    if (!ld::r2(n, n_a, n_b, n_ab, p.r2)) return P_UNDEFINED;
    return p.r2 >= a.min_r2 ? P_REPORTED : P_BELOW;
}

// blockIdx.x: the tile of the list.  Lane (ty, tx) of 16 x 16 holds the pairs (ty + 16 i, tx + 16 j)
template <int MODE>
__global__ void __launch_bounds__(LT) k_ld_pairs(PairArgs a)
{
    __shared__ u64 sa[ld::TILE * LDS_STRIDE];
    __shared__ u64 sb[ld::TILE * LDS_STRIDE];
    __shared__ u64 rmask[ld::TILE];
    __shared__ u32 undef;
    const u64 tr = ld::tile_row(a.tstart, a.RT, blockIdx.x), t0 = a.tstart[tr], nt = a.tstart[tr + 1] - t0, ci = blockIdx.x - t0;
    u64 c0, c1;
    ld::tile_columns(a.afirst, a.nc, a.ar[tr * ld::TILE], a.ar[min(a.A, (tr + 1) * ld::TILE) - 1], a.window, c0, c1);
    const u64 tc = c0 + ci;
    u64 slot = 0;
    if (threadIdx.x < ld::TILE) slot = ld::counter_slot(t0, nt, threadIdx.x, ci);
    if (MODE == LD_FILL) {                                       // a tile without a reported pair is not computed again
        const int any = threadIdx.x < ld::TILE && a.cntx[slot + 1] != a.cntx[slot];
        if (!__syncthreads_or(any)) return;
    }
    if (threadIdx.x < ld::TILE) rmask[threadIdx.x] = 0;
    if (threadIdx.x == 0) undef = 0;
    const u32 tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    u32 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = 0;
    for (u64 ws = 0; ws < a.WP; ws += ld::STAGE_WORDS) {
        __syncthreads();                                                   // the last stage's readers are through
        for (u32 e = threadIdx.x; e < ld::TILE * ld::STAGE_WORDS; e += LT) {
            const u32 row = e / ld::STAGE_WORDS, w = e % ld::STAGE_WORDS;
            const u64 ra = tr * ld::TILE + row, rb = tc * ld::TILE + row, gw = ws + w;
            sa[row * LDS_STRIDE + w] = gw < a.WP && ra < a.A ? a.trows[ra * a.WP + gw] : 0;
            sb[row * LDS_STRIDE + w] = gw < a.WP && rb < a.A ? a.trows[rb * a.WP + gw] : 0;
        }
        __syncthreads();
#pragma unroll 2
        for (u32 w = 0; w < ld::STAGE_WORDS; w++) {
            u64 x[4], y[4];
#pragma unroll
            for (int i = 0; i < 4; i++) { x[i] = sa[(ty + 16 * i) * LDS_STRIDE + w]; y[i] = sb[(tx + 16 * i) * LDS_STRIDE + w]; }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] += (u32)__builtin_popcountll(x[i] & y[j]);
        }
    }
    u32 und = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u64 x = tr * ld::TILE + ty + 16 * i, y = tc * ld::TILE + tx + 16 * j;
            if (x >= a.A || y >= a.A) continue;
            LdPair p;
            const int s = pair_eval(a, x, y, acc[i][j], p);
            if (s == P_UNDEFINED) und++;
            if (s == P_REPORTED) atomicOr((unsigned long long*)&rmask[ty + 16 * i], 1ull << (tx + 16 * j));
        }
    if (MODE == LD_COUNT && und) atomicAdd(&undef, und);
    __syncthreads();
    if (MODE == LD_COUNT) {
        if (threadIdx.x < ld::TILE) a.cntx[slot] = (u64)__builtin_popcountll(rmask[threadIdx.x]);
        if (threadIdx.x == 0 && undef) atomicAdd((unsigned long long*)&a.ctl[C_UNDEF], (unsigned long long)undef);
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u32 xi = ty + 16 * i, yi = tx + 16 * j;
            const u64 m = rmask[xi];
            if (!((m >> yi) & 1)) continue;
            const u64 x = tr * ld::TILE + xi, y = tc * ld::TILE + yi;
            LdPair p;
            pair_eval(a, x, y, acc[i][j], p);
            p.symbol_a = a.al[x].symbol; p.string_a = a.al[x].string;
            p.symbol_b = a.al[y].symbol; p.string_b = a.al[y].string;
            a.out[a.cntx[ld::counter_slot(t0, nt, xi, ci)] + (u64)__builtin_popcountll(m & ((1ull << yi) - 1))] = p;
        }
}

unsigned wave_grid(u64 waves) { return (unsigned)std::max<u64>(1, std::min<u64>((waves + 3) / 4, 16384)); }

} // namespace

void PathPipeline::ld_open(hipStream_t st)
{
    if (ld_.ready || nc_ == 0) return;
    const EdsView v = eds_.view();
    ld_.soff.ensure(8 * (nc_ + 1));
    ctl_.ensure(8 * C_WORDS);
    scan_tmp_.ensure(8 * ((nc_ + 1) / SCAN_TILE + 4));
    u64 h[2] = {nc_ + 1, 0};
    u64 *ctl = ctl_.as<u64>(), *soff = ld_.soff.as<u64>();
    EDSX_HIP(hipMemcpyAsync(ctl, h, sizeof(h), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_ld_sizes, dim3(grid_for(nc_ + 1, 8192)), dim3(LT), 0, st, v.sym.size, cidx_.as<u64>(), nc_, soff);
    exclusive_scan_u64(soff, soff, ctl, ctl + 1, scan_tmp_.as<u64>(), st);
    EDSX_HIP(hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    ld_.S = h[1];
    ld_.ready = true;
}

void PathPipeline::ld(const u64* ids, size_t n, const LdOpts& o, HostBytes& pairs, HostBytes* alleles, LdInfo& info, KernelTimes* times,
                      hipStream_t st)
{
    info = LdInfo{};
    if (o.window == 0) throw ParamError("The LD window is 0; it counts choice symbols and is at least 1");
    if (!(o.min_r2 >= 0.0 && o.min_r2 <= 1.0)) throw ParamError("The LD threshold min_r2 is not a number of [0, 1]");
    check_ids(ids, n);
    begin_call();
    pairs.take(0);
    if (alleles) alleles->take(0);
    const u64 P = info_.num_paths, WP = (P + 63) / 64;
    std::vector<u64> mask(WP, 0);                                // the row of M: path p at bit p - 1
    if (n == 0) for (u64 p = 1; p <= P; p++) mask[(p - 1) >> 6] |= 1ull << ((p - 1) & 63);
    for (size_t k = 0; k < n; k++) mask[(ids[k] - 1) >> 6] |= 1ull << ((ids[k] - 1) & 63);
    u64 K = 0;
    for (u64 w : mask) K += (u64)__builtin_popcountll(w);
    info.paths = K; info.choice_symbols = nc_; info.row_words = WP;
    if (K == 0 || nc_ == 0) return;

    ld_open(st);
    TimedRuns timed(st, times);
    const EdsView v = eds_.view();
    ld_.mask.ensure(8 * WP);
    ld_.cnt.ensure(8 * ld_.S);
    ld_.pres.ensure(8 * nc_);
    ld_.afirst.ensure(8 * (nc_ + 1));
    ld_.uidx.ensure(8 * (nc_ + 1));
    ctl_.ensure(8 * C_WORDS);
    scan_tmp_.ensure(8 * 2 * ((nc_ + 1) / SCAN_TILE + 4));
    u64 h[C_WORDS] = {};
    h[C_N] = nc_ + 1;
    u64* ctl = ctl_.as<u64>();
    EDSX_HIP(hipMemcpyAsync(ctl, h, sizeof(h), hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemcpyAsync(ld_.mask.ptr, mask.data(), 8 * WP, hipMemcpyHostToDevice, st));
    const WalkArgs wa{v.sym.size, v.sym.ent_off, v.bits, v.W, cidx_.as<u64>(), ld_.soff.as<u64>(), nc_, ld_.mask.as<u64>(), WP, K,
                      o.min_count, o.all_strings};
    u64 *afirst = ld_.afirst.as<u64>(), *uidx = ld_.uidx.as<u64>();
    timed.run("k_ld_count", [&] {
        hipLaunchKernelGGL(k_ld_count, dim3(wave_grid(nc_ + 1)), dim3(LT), 0, st, wa, ld_.cnt.as<u64>(), ld_.pres.as<u64>(), afirst, uidx);
    }, &timing_.scan_ms);
    timed.run("scan_alleles", [&] {
        ScanSet<2> ss{{afirst, uidx}, {afirst, uidx}, {ctl + C_A, ctl + C_NU}};
        exclusive_scan_multi<2>(ss, ctl + C_N, scan_tmp_.as<u64>(), st);
    }, &timing_.scan_ms);
    EDSX_HIP(hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    timed.harvest();
    const u64 A = h[C_A], NU = h[C_NU];
    info.alleles = A;
    if (A == 0) return;

    const u128 rows128 = (u128)8 * WP * A, urows128 = (u128)8 * WP * NU;
    const u64 cap = budget(2);
    if (rows128 + urows128 > cap)
        throw LimitError("The allele rows (" + std::to_string((u64)std::min<u128>(rows128, ~0ull)) + " bytes) and the presence rows (" +
                         std::to_string((u64)std::min<u128>(urows128, ~0ull)) + " bytes) do not fit the budget of " + std::to_string(cap) +
                         " bytes; request a larger min_count or fewer paths");
    const u64 RT = (A + ld::TILE - 1) / ld::TILE;
    ld_.trows.ensure((u64)rows128);
    ld_.urows.ensure(std::max<u64>((u64)urows128, 8));
    ld_.al.ensure(sizeof(LdAllele) * A);
    ld_.ar.ensure(8 * A);
    ld_.tstart.ensure(8 * (RT + 1));
    scan_tmp_.ensure(8 * ((RT + 1) / SCAN_TILE + 4));
    const u64 tn = RT + 1;
    EDSX_HIP(hipMemcpyAsync(ctl + C_TN, &tn, 8, hipMemcpyHostToDevice, st));
    u64* tstart = ld_.tstart.as<u64>();
    timed.run("k_ld_rows", [&] {
        hipLaunchKernelGGL(k_ld_rows, dim3(wave_grid(nc_)), dim3(LT), 0, st, wa, ld_.cnt.as<u64>(), ld_.pres.as<u64>(), afirst, uidx,
                           ld_.trows.as<u64>(), ld_.urows.as<u64>(), ld_.al.as<LdAllele>(), ld_.ar.as<u64>());
    }, &timing_.copy_ms);
    timed.run("k_ld_tiles", [&] {
        hipLaunchKernelGGL(k_ld_tiles, dim3(grid_for(A, 8192)), dim3(LT), 0, st, afirst, ld_.ar.as<u64>(), nc_, A, RT, o.window, tstart, ctl);
    }, &timing_.scan_ms);
    timed.run("scan_tiles", [&] { exclusive_scan_u64(tstart, tstart, ctl + C_TN, ctl + C_NT, scan_tmp_.as<u64>(), st); }, &timing_.scan_ms);
    EDSX_HIP(hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    timed.harvest();
    const u64 NT = h[C_NT];
    info.candidate_pairs = h[C_CAND]; info.tiles = NT;
    if (NT > 0x7fffffffull) throw LimitError("LD has " + std::to_string(NT) + " tiles of 64 x 64 alleles, above the " + std::to_string(0x7fffffffull) +
                                             " of one launch; request a smaller window");

    PairArgs pa{ld_.trows.as<u64>(), ld_.urows.as<u64>(), ld_.mask.as<u64>(), ld_.ar.as<u64>(), ld_.al.as<LdAllele>(), ld_.pres.as<u64>(), uidx,
                afirst, tstart, A, WP, K, nc_, RT, o.window, o.min_r2, nullptr, ctl, nullptr};
    u64 npairs = 0;
    if (NT) {
        const u64 pn = ld::TILE * NT + 1;
        ld_.cntx.ensure(8 * pn);
        scan_tmp_.ensure(8 * (pn / SCAN_TILE + 4));
        u64* cntx = ld_.cntx.as<u64>();
        pa.cntx = cntx;
        EDSX_HIP(hipMemcpyAsync(ctl + C_PN, &pn, 8, hipMemcpyHostToDevice, st));
        EDSX_HIP(hipMemsetAsync(cntx + (pn - 1), 0, 8, st));
        timed.run("k_ld_pairs", [&] { hipLaunchKernelGGL((k_ld_pairs<LD_COUNT>), dim3((unsigned)NT), dim3(LT), 0, st, pa); }, &timing_.copy_ms);
        timed.run("scan_pairs", [&] { exclusive_scan_u64(cntx, cntx, ctl + C_PN, ctl + C_PAIRS, scan_tmp_.as<u64>(), st); }, &timing_.scan_ms);
        EDSX_HIP(hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        EDSX_HIP(hipGetLastError());
        timed.harvest();
        npairs = h[C_PAIRS];
        info.undefined_pairs = h[C_UNDEF];
    }
    info.pairs = npairs;
    if (o.max_pairs && npairs > o.max_pairs)
        throw ParamError("LD has " + std::to_string(npairs) + " pairs, above the limit of " + std::to_string(o.max_pairs));
    const u128 out128 = (u128)sizeof(LdPair) * npairs;
    if (out128 > cap)
        throw LimitError("The LD pairs (" + std::to_string((u64)std::min<u128>(out128, ~0ull)) + " bytes) do not fit the budget of " +
                         std::to_string(cap) + " bytes; request a larger min_r2 or set max_pairs");
    if (npairs) {
        ld_.pairs.ensure((u64)out128);
        pa.out = ld_.pairs.as<LdPair>();
        timed.run("k_ld_pairs", [&] { hipLaunchKernelGGL((k_ld_pairs<LD_FILL>), dim3((unsigned)NT), dim3(LT), 0, st, pa); }, &timing_.copy_ms);
        EDSX_HIP(hipStreamSynchronize(st));
        EDSX_HIP(hipGetLastError());
        timed.harvest();
    }
    const auto t0 = std::chrono::steady_clock::now();
    pairs.take((size_t)out128);
    if (npairs) PinnedDownload::copy(pairs.data, ld_.pairs.ptr, (size_t)out128, st);
    timing_.bytes_written = (u64)out128;
    if (alleles) {
        alleles->take(sizeof(LdAllele) * A);
        PinnedDownload::copy(alleles->data, ld_.al.ptr, sizeof(LdAllele) * A, st);
        timing_.bytes_written += sizeof(LdAllele) * A;
    }
    timing_.download_ms += since_ms(t0);
}

} // namespace edsx
