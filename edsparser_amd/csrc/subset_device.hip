// subset_device.hip — restrict an EDS with sources to a keep set K of paths on gfx950 (edsx_eds_subset).
//
// Semantics: include/edsx.h.  A string is kept when its source set holds 0 or meets K; a symbol without a kept string is
// removed; a symbol whose only kept string is universal or covers K is COMMON; runs of adjacent common symbols (removed
// ones in between do not count) become one symbol with the set {0}, and a run without a character is dropped.  The
// kernels read the context's DeviceEds through its view and write nothing to it.
//
// Count -> scan -> fill, over four index spaces, each derived from the one before by an exclusive scan:
//   strings j   k_sub_filter    G lanes per string (G: the power of two that covers the W bitset words, at most a wave; a
//                               lane reads words g, g + G, ...: consecutive lanes read consecutive 8-byte words whatever W
//                               is): S & K, its popcount, the .seds bytes of the renumbered ids; shuffle reduction in the
//                               group -> kept flag, kept length, .seds bytes, universal / covers-K flags.
//                               One scan of the three -> kscan, lscan, bscan (m + 1 entries: [m] is the total)
//   symbols i   k_sub_classify  kept strings of a symbol = kscan[e1] - kscan[e0]: no loop over a symbol's strings; the only
//                               kept string of a symbol is found by bisection in kscan.  Scan of the survivor flags
//   survivors r k_sub_compact / k_sub_heads: symbol index, class and common length per survivor; a survivor is a run head
//                               unless it and the survivor before it are both common.  Scan of heads and common lengths
//   runs q      k_sub_runs / k_sub_runinfo: first survivor of every run; the length of a common run is a difference of
//                               the scanned common lengths (the segmented sum); bytes of the run in both texts, alive
//                               flag.  Scan of the three -> eoff, soff and the totals that size the output buffers
// Fill:
//   k_sub_place   one lane per string: symbol by bisection in ent_off, then survivor, run and the byte where the string's
//                 text goes (dst) and where its set goes (sdst); writes the braces and commas of both texts and the "{0}"s
//   k_sub_copy    over tiles of the SOURCE character pool (kept strings keep their order, so the copy is monotone): a lane
//                 owns 16 aligned source bytes, finds their string between the tile's first and last string, and when all
//                 16 lie in one emitted string moves them with one aligned 16-byte load and one 16-byte store; chunks that
//                 straddle strings go byte by byte.  A 100 000-character string is 6 250 lanes' work, not one lane's
//   k_sub_seds    G lanes per string as in the filter: bytes per word, prefix in the group, decimal ids
#include "subset_device.hpp"

#include <algorithm>
#include <chrono>
#include <string>

namespace edsx {

namespace {

constexpr u64 NONE = ~0ull;
constexpr int ST = 256;                    // threads per block
constexpr u32 CP_TILE = ST * 16;           // source characters per block step of the copy kernel
enum : uint8_t { C_REMOVED = 0, C_COMMON = 1, C_EXPLICIT = 2, C_DEGENERATE = 3 };
// control block (u64): scan lengths and totals
enum { CT_M1, CT_N1, CT_R, CT_R1, CT_Q, CT_Q1, CT_E, CT_S, CT_SYMS, CT_STRINGS, CT_MERGED, CT_T0, CT_T1, CT_T2, CT_CCH, CT_COUNT };

// K on the device: W mask words (bit 0 clear), ranks below each word, and per word the digits of its ids when they all
// have the same number of digits (0: count them one by one)
struct KeepSet { const u64* mask; const u32* below; const uint8_t* dig; u32 W, nK, keep_ids; };

__device__ __forceinline__ u32 new_id(const KeepSet& ks, u32 w, u32 b)
{
    if (ks.keep_ids) return 64u * w + b;
    return ks.below[w] + (u32)__popcll(ks.mask[w] & ((1ull << b) - 1)) + 1u;
}

// bytes of the ids of x (= set & mask, word w) in the .seds text, each with the comma or brace behind it
__device__ __forceinline__ u64 word_bytes(const KeepSet& ks, u32 w, u64 x)
{
    if (!x) return 0;
    const u32 d = ks.dig[w];
    if (d) return (u64)__popcll(x) * (d + 1);
    u64 n = 0;
    while (x) {
        const u32 b = (u32)__builtin_ctzll(x);
        x &= x - 1;
        n += ndigits(new_id(ks, w, b)) + 1;
    }
    return n;
}

__global__ void __launch_bounds__(ST) k_sub_or(const u64* __restrict__ bits, u32 W, u64 m, u64* __restrict__ orbits)
{
    const u64 t0 = blockIdx.x * (u64)blockDim.x + threadIdx.x, step = (u64)gridDim.x * blockDim.x;
    for (u32 w = 0; w < W; w++) {
        u64 o = 0;
        for (u64 k = t0; k < m; k += step) o |= bits[k * W + w];
        for (int sh = 32; sh > 0; sh >>= 1) o |= __shfl_xor(o, sh, 64);
        if ((threadIdx.x & 63) == 0 && o) atomicOr((unsigned long long*)&orbits[w], (unsigned long long)o);
    }
}

__global__ void __launch_bounds__(ST) k_sub_filter(const u64* __restrict__ bits, const u32* __restrict__ elen, u64 m, KeepSet ks, u32 G,
                                                   u64* __restrict__ kept, u64* __restrict__ klen, u64* __restrict__ ksb,
                                                   uint8_t* __restrict__ sflag)
{
    const u32 g = threadIdx.x & (G - 1), per_block = ST / G;
    for (u64 base = (u64)blockIdx.x * per_block; base < m; base += (u64)gridDim.x * per_block) {   // block-uniform: the shuffles
        const u64 j = base + threadIdx.x / G;                                                     // below run with every lane
        u64 cnt = 0, bytes = 0;
        bool univ = false;
        if (j < m) {
            const u64* row = bits + j * ks.W;
            for (u32 w = g; w < ks.W; w += G) {
                const u64 b = row[w];
                if (w == 0) univ = b & 1;
                const u64 x = b & ks.mask[w];
                cnt += (u64)__popcll(x);
                bytes += word_bytes(ks, w, x);
            }
        }
        for (u32 o = G >> 1; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o, 64); bytes += __shfl_xor(bytes, o, 64); }
        if (j < m && g == 0) {                                       // (word 0 is this lane's: it knows `univ`)
            const bool k = univ || cnt;
            kept[j] = k;
            klen[j] = k ? elen[j] : 0;
            ksb[j] = !k ? 0 : univ ? 3 : bytes + 1;                  // "{0}", or '{' + ids with their separators
            sflag[j] = (uint8_t)((univ ? 1 : 0) | (cnt == ks.nK ? 2 : 0));
        }
    }
}

__global__ void __launch_bounds__(ST) k_sub_classify(const u64* __restrict__ size, const u64* __restrict__ ent_off, u64 n,
                                                     const u64* __restrict__ kscan, const uint8_t* __restrict__ sflag,
                                                     u64* __restrict__ surv, uint8_t* __restrict__ scls, u64* __restrict__ kj)
{
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 e0 = ent_off[i], e1 = e0 + size[i], k0 = kscan[e0], kc = kscan[e1] - k0;
        uint8_t cls = kc ? C_DEGENERATE : C_REMOVED;
        u64 j = NONE;
        if (kc == 1) {                                               // the kept one: first j with kscan[j + 1] > k0
            u64 lo = e0, hi = e1 - 1;
            while (lo < hi) { const u64 mid = lo + ((hi - lo) >> 1); if (kscan[mid + 1] > k0) hi = mid; else lo = mid + 1; }
            j = lo;
            cls = (sflag[j] & 3) ? C_COMMON : C_EXPLICIT;
        }
        surv[i] = kc ? 1 : 0;
        scls[i] = cls;
        kj[i] = j;
    }
}

__global__ void __launch_bounds__(ST) k_sub_compact(u64 n, const u64* __restrict__ sscan, const uint8_t* __restrict__ scls,
                                                    const u64* __restrict__ kj, const u32* __restrict__ elen, u64* __restrict__ sidx,
                                                    uint8_t* __restrict__ rcls, u64* __restrict__ clen, u64* __restrict__ ctl)
{
    const u64 t0 = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (t0 == 0) { const u64 R = sscan[n]; ctl[CT_R1] = R + 1; clen[R] = 0; }
    for (u64 i = t0; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 r = sscan[i];
        if (sscan[i + 1] == r) continue;
        const uint8_t c = scls[i];
        sidx[r] = i;
        rcls[r] = c;
        clen[r] = c == C_COMMON ? elen[kj[i]] : 0;
    }
}

__device__ __forceinline__ bool is_head(const uint8_t* rcls, u64 r) { return !(r > 0 && rcls[r] == C_COMMON && rcls[r - 1] == C_COMMON); }

__global__ void __launch_bounds__(ST) k_sub_heads(const u64* __restrict__ ctl, const uint8_t* __restrict__ rcls, u64* __restrict__ head)
{
    const u64 R = ctl[CT_R], t0 = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (t0 == 0) head[R] = 0;
    for (u64 r = t0; r < R; r += (u64)gridDim.x * blockDim.x) head[r] = is_head(rcls, r) ? 1 : 0;
}

__global__ void __launch_bounds__(ST) k_sub_runs(u64* __restrict__ ctl, const uint8_t* __restrict__ rcls, const u64* __restrict__ hscan,
                                                 u64* __restrict__ headpos)
{
    const u64 R = ctl[CT_R], t0 = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (t0 == 0) { const u64 Q = hscan[R]; headpos[Q] = R; ctl[CT_Q1] = Q + 1; }
    for (u64 r = t0; r < R; r += (u64)gridDim.x * blockDim.x)
        if (is_head(rcls, r)) headpos[hscan[r]] = r;
}

struct RunArgs {
    const u64* size; const u64* ent_off;
    const u64* kscan; const u64* lscan; const u64* bscan;
    const u64* sidx; const uint8_t* rcls; const u64* cscan; const u64* headpos;
};

__global__ void __launch_bounds__(ST) k_sub_runinfo(RunArgs a, u64* __restrict__ ctl, u64* __restrict__ eb, u64* __restrict__ sb,
                                                    u64* __restrict__ al)
{
    const u64 Q = ctl[CT_Q];
    if (blockIdx.x == 0 && threadIdx.x == 0) { eb[Q] = 0; sb[Q] = 0; al[Q] = 0; }
    u64 strings = 0, merged = 0;
    for (u64 base = blockIdx.x * (u64)ST; base < Q; base += (u64)gridDim.x * ST) {
        const u64 q = base + threadIdx.x;
        if (q >= Q) continue;
        const u64 r0 = a.headpos[q], r1 = a.headpos[q + 1];
        if (a.rcls[r0] == C_COMMON) {
            const u64 len = a.cscan[r1] - a.cscan[r0];
            eb[q] = len ? len + 2 : 0;
            sb[q] = len ? 3 : 0;
            al[q] = len ? 1 : 0;
            strings += len ? 1 : 0;
            merged += r1 - r0 >= 2 ? 1 : 0;
        } else {
            const u64 i = a.sidx[r0], e0 = a.ent_off[i], e1 = e0 + a.size[i], kc = a.kscan[e1] - a.kscan[e0];
            eb[q] = 2 + (a.lscan[e1] - a.lscan[e0]) + (kc - 1);
            sb[q] = a.bscan[e1] - a.bscan[e0];
            al[q] = 1;
            strings += kc;
        }
    }
    strings = wave_sum(strings);                                     // (every lane is back here: the loop above only skips)
    merged = wave_sum(merged);
    if ((threadIdx.x & 63) == 0) {
        if (strings) atomicAdd((unsigned long long*)&ctl[CT_STRINGS], (unsigned long long)strings);
        if (merged) atomicAdd((unsigned long long*)&ctl[CT_MERGED], (unsigned long long)merged);
    }
}

struct PlaceArgs {
    RunArgs r;
    const uint8_t* sflag; const u64* sscan; const u64* hscan; const u64* eoff; const u64* soff;
    u64 n, m, E, S;
    u64* dst; u64* sdst; uint8_t* out; uint8_t* sout;
};

__device__ __forceinline__ void put_zero_set(uint8_t* p) { p[0] = '{'; p[1] = '0'; p[2] = '}'; }

__global__ void __launch_bounds__(ST) k_sub_place(PlaceArgs a)
{
    const u64 t0 = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (t0 == 0) { a.out[a.E] = '\n'; a.sout[a.S] = '\n'; }
    for (u64 j = t0; j < a.m; j += (u64)gridDim.x * blockDim.x) {
        u64 d = NONE, sd = NONE;
        if (a.r.kscan[j + 1] != a.r.kscan[j]) {
            const u64 i = last_le(a.r.ent_off, 0, a.n - 1, j), r = a.sscan[i];   // the symbol of j
            const uint8_t cls = a.r.rcls[r];
            const u64 q = a.hscan[r] + (is_head(a.r.rcls, r) ? 1 : 0) - 1, e = a.eoff[q], e_end = a.eoff[q + 1];
            if (e_end != e) {                                        // (an empty common run has no bytes)
                if (cls == C_COMMON) {
                    const u64 r0 = a.r.headpos[q];
                    d = e + 1 + (a.r.cscan[r] - a.r.cscan[r0]);
                    if (r == r0) { a.out[e] = '{'; put_zero_set(a.sout + a.soff[q]); }
                    if (r + 1 == a.r.headpos[q + 1]) a.out[e_end - 1] = '}';
                } else {
                    const u64 e0 = a.r.ent_off[i], e1 = e0 + a.r.size[i];
                    const u64 t = a.r.kscan[j] - a.r.kscan[e0], kc = a.r.kscan[e1] - a.r.kscan[e0];
                    d = e + 1 + (a.r.lscan[j] - a.r.lscan[e0]) + t;
                    a.out[d - 1] = t ? ',' : '{';
                    if (t + 1 == kc) a.out[e_end - 1] = '}';
                    const u64 sp = a.soff[q] + (a.r.bscan[j] - a.r.bscan[e0]);
                    if (a.sflag[j] & 1) put_zero_set(a.sout + sp); else sd = sp;
                }
            }
        }
        a.dst[j] = d;
        a.sdst[j] = sd;
    }
}

__global__ void __launch_bounds__(ST) k_sub_copy(const uint8_t* __restrict__ chars, const u64* __restrict__ str_off, u64 m, u64 N,
                                                 const u64* __restrict__ dst, uint8_t* __restrict__ out)
{
    __shared__ u64 sj[2];
    for (u64 t0 = blockIdx.x * (u64)CP_TILE; t0 < N; t0 += (u64)gridDim.x * CP_TILE) {
        const u64 t1 = min(N, t0 + (u64)CP_TILE);
        if (threadIdx.x == 0) sj[0] = last_le(str_off, 0, m - 1, t0);
        if (threadIdx.x == 64) sj[1] = last_le(str_off, 0, m - 1, t1 - 1);
        __syncthreads();
        const u64 c0 = t0 + (u64)threadIdx.x * 16;
        if (c0 < t1) {
            u64 j = last_le(str_off, sj[0], sj[1], c0);
            const u64 s0 = str_off[j], s1 = str_off[j + 1];
            if (c0 + 16 <= s1) {                                     // all 16 in string j (so c0 + 16 <= N)
                const u64 d = dst[j];
                if (d != NONE) store16u(out + d + (c0 - s0), *reinterpret_cast<const uint4*>(chars + c0));
            } else {
                u64 base = s0, end = s1, d = dst[j];
                const u64 c1 = min(t1, c0 + 16);
                for (u64 c = c0; c < c1; c++) {
                    while (c >= end) { j++; base = end; end = str_off[j + 1]; d = dst[j]; }
                    if (d != NONE) out[d + (c - base)] = chars[c];
                }
            }
        }
        __syncthreads();
    }
}

// write_set_ids over S & K with the renumbered ids
struct KeptIds {
    const KeepSet& ks;
    __device__ __forceinline__ u64 mask(u32 w) const { return ks.mask[w]; }
    __device__ __forceinline__ u64 bytes(u32 w, u64 x) const { return word_bytes(ks, w, x); }
    __device__ __forceinline__ u32 id(u32 w, u32 b) const { return new_id(ks, w, b); }
};

__global__ void __launch_bounds__(ST) k_sub_seds(const u64* __restrict__ bits, u64 m, KeepSet ks, u32 G, const u64* __restrict__ sdst,
                                                 const u64* __restrict__ bscan, uint8_t* __restrict__ sout)
{
    const u32 g = threadIdx.x & (G - 1), per_block = ST / G;
    for (u64 base = (u64)blockIdx.x * per_block; base < m; base += (u64)gridDim.x * per_block) {   // block-uniform, as the filter
        const u64 j = base + threadIdx.x / G;
        const u64 p0 = j < m ? sdst[j] : NONE;
        const bool act = p0 != NONE;
        const u64 end = act ? p0 + (bscan[j + 1] - bscan[j]) : 0;     // one past the closing brace
        if (act && g == 0) sout[p0] = '{';
        write_set_ids(KeptIds{ks}, bits + j * ks.W, act, ks.W, G, g, p0 + 1, end, sout);
    }
}

u32 digits_of(u64 v) { u32 d = 1; while (v >= 10) { v /= 10; d++; } return d; }

} // namespace

void SubsetPipeline::run(DeviceEds& de, const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, const u64* ids, size_t nids,
                         bool keep_ids, HostBytes& eds_out, HostBytes& seds_out, SubsetInfo& info, hipStream_t st)
{
    if (!seds) throw ParamError("Path subsetting needs sources (.seds)");
    if (nids == 0) throw ParamError("No paths selected");
    info = SubsetInfo{};
    TimedRuns timed(st, &times_);

    de.load(eds, eds_n, seds, seds_n, true, st);
    const u64 n = de.n(), m = de.m(), N = de.n_chars();
    const u32 W = de.W();

    // ---- P: the highest bit of the OR of all sets
    u64 P = 0;
    EdsView v{};
    if (n) {
        v = de.view();
        orbits_.ensure(8 * (size_t)W);
        EDSX_HIP(hipMemsetAsync(orbits_.ptr, 0, 8 * (size_t)W, st));
        timed.run("k_sub_or", [&] { hipLaunchKernelGGL(k_sub_or, dim3(1024), dim3(ST), 0, st, v.bits, W, m, orbits_.as<u64>()); });
        std::vector<u64> orb(W, 0);
        EDSX_HIP(hipMemcpyAsync(orb.data(), orbits_.ptr, 8 * (size_t)W, hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        EDSX_HIP(hipGetLastError());
        for (u32 w = 0; w < W; w++)
            if (orb[w]) P = 64ull * w + 63 - (u64)__builtin_clzll(orb[w]);
    }

    // ---- K as a mask, the ranks below each word, the common digit count of each word's ids
    std::vector<u64> mask(std::max<u32>(W, 1), 0);
    for (size_t k = 0; k < nids; k++) {
        const u64 p = ids[k];
        if (p == 0 || p > P) throw ParamError("Path id " + std::to_string(p) + " out of range (1.." + std::to_string(P) + ")");
        if (mask[p >> 6] >> (p & 63) & 1) throw ParamError("Path id " + std::to_string(p) + " given twice");
        mask[p >> 6] |= 1ull << (p & 63);
    }
    std::vector<u32> below(W, 0);
    std::vector<uint8_t> dig(W, 1);
    u32 rank = 0;
    for (u32 w = 0; w < W; w++) {
        below[w] = rank;
        const u32 cnt = (u32)__builtin_popcountll(mask[w]);
        if (cnt) {
            const u64 first = keep_ids ? 64ull * w + (u64)__builtin_ctzll(mask[w]) : (u64)rank + 1;
            const u64 last = keep_ids ? 64ull * w + 63 - (u64)__builtin_clzll(mask[w]) : (u64)rank + cnt;
            dig[w] = digits_of(first) == digits_of(last) ? (uint8_t)digits_of(first) : 0;
        }
        rank += cnt;
    }
    info.symbols_in = n; info.strings_in = m; info.chars_in = N; info.paths_in = P; info.paths_out = nids;

    mask_.ensure(8 * (size_t)W); below_.ensure(4 * (size_t)W); dig_.ensure(W);
    EDSX_HIP(hipMemcpyAsync(mask_.ptr, mask.data(), 8 * (size_t)W, hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemcpyAsync(below_.ptr, below.data(), 4 * (size_t)W, hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemcpyAsync(dig_.ptr, dig.data(), W, hipMemcpyHostToDevice, st));
    const KeepSet ks{mask_.as<u64>(), below_.as<u32>(), dig_.as<uint8_t>(), W, (u32)nids, keep_ids ? 1u : 0u};
    const u32 G = group_for(W);

    // ---- buffers: every index space is at most as long as the one it comes from
    for (DevBuf* b : {&kscan_, &lscan_, &bscan_, &dst_, &sdst_}) b->ensure(8 * (m + 1));
    sflag_.ensure(m + 1);
    for (DevBuf* b : {&sscan_, &kj_, &sidx_, &hscan_, &cscan_, &headpos_, &eoff_, &soff_, &aoff_}) b->ensure(8 * (n + 2));
    scls_.ensure(n + 2); rcls_.ensure(n + 2);
    ctl_.ensure(8 * CT_COUNT);
    scan_tmp_.ensure(8 * 3 * ((m + 1) / SCAN_TILE + 4));
    u64 hctl[CT_COUNT] = {};
    hctl[CT_M1] = m + 1; hctl[CT_N1] = n + 1;
    u64* ctl = ctl_.as<u64>();
    EDSX_HIP(hipMemcpyAsync(ctl, hctl, sizeof(hctl), hipMemcpyHostToDevice, st));
    u64 *kscan = kscan_.as<u64>(), *lscan = lscan_.as<u64>(), *bscan = bscan_.as<u64>(), *sscan = sscan_.as<u64>(), *kj = kj_.as<u64>(),
        *sidx = sidx_.as<u64>(), *hscan = hscan_.as<u64>(), *cscan = cscan_.as<u64>(), *headpos = headpos_.as<u64>(),
        *eoff = eoff_.as<u64>(), *soff = soff_.as<u64>(), *aoff = aoff_.as<u64>(), *tmp = scan_tmp_.as<u64>();
    uint8_t *sflag = sflag_.as<uint8_t>(), *scls = scls_.as<uint8_t>(), *rcls = rcls_.as<uint8_t>();
    for (u64* p : {kscan + m, lscan + m, bscan + m, sscan + n}) EDSX_HIP(hipMemsetAsync(p, 0, 8, st));

    // ---- strings
    timed.run("k_sub_filter", [&] {
        hipLaunchKernelGGL(k_sub_filter, dim3(grid_for(m * G, 16384)), dim3(ST), 0, st, v.bits, v.elen, m, ks, G, kscan, lscan, bscan, sflag);
    });
    timed.run("scan_strings", [&] {
        ScanSet<3> ss{{kscan, lscan, bscan}, {kscan, lscan, bscan}, {ctl + CT_T0, ctl + CT_T1, ctl + CT_T2}};
        exclusive_scan_multi<3>(ss, ctl + CT_M1, tmp, st);
    });
    // ---- symbols
    timed.run("k_sub_classify", [&] {
        hipLaunchKernelGGL(k_sub_classify, dim3(grid_for(n, 8192)), dim3(ST), 0, st, v.sym.size, v.sym.ent_off, n, kscan, sflag, sscan, scls, kj);
    });
    timed.run("scan_symbols", [&] { exclusive_scan_u64(sscan, sscan, ctl + CT_N1, ctl + CT_R, tmp, st); });
    // ---- survivors
    timed.run("k_sub_compact", [&] {
        hipLaunchKernelGGL(k_sub_compact, dim3(grid_for(n, 8192)), dim3(ST), 0, st, n, sscan, scls, kj, v.elen, sidx, rcls, cscan, ctl);
        hipLaunchKernelGGL(k_sub_heads, dim3(grid_for(n, 8192)), dim3(ST), 0, st, ctl, rcls, hscan);
    });
    timed.run("scan_survivors", [&] {
        ScanSet<2> ss{{hscan, cscan}, {hscan, cscan}, {ctl + CT_Q, ctl + CT_CCH}};
        exclusive_scan_multi<2>(ss, ctl + CT_R1, tmp, st);
    });
    // ---- runs
    const RunArgs ra{v.sym.size, v.sym.ent_off, kscan, lscan, bscan, sidx, rcls, cscan, headpos};
    timed.run("k_sub_runs", [&] {
        hipLaunchKernelGGL(k_sub_runs, dim3(grid_for(n, 8192)), dim3(ST), 0, st, ctl, rcls, hscan, headpos);
        hipLaunchKernelGGL(k_sub_runinfo, dim3(grid_for(n, 8192)), dim3(ST), 0, st, ra, ctl, eoff, soff, aoff);
    });
    timed.run("scan_runs", [&] {
        ScanSet<3> ss{{eoff, soff, aoff}, {eoff, soff, aoff}, {ctl + CT_E, ctl + CT_S, ctl + CT_SYMS}};
        exclusive_scan_multi<3>(ss, ctl + CT_Q1, tmp, st);
    });
    EDSX_HIP(hipMemcpyAsync(hctl, ctl, sizeof(hctl), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    const u64 E = hctl[CT_E], S = hctl[CT_S];
    info.symbols_out = hctl[CT_SYMS]; info.strings_out = hctl[CT_STRINGS]; info.common_runs_merged = hctl[CT_MERGED];
    info.symbols_removed = n - hctl[CT_R];
    info.chars_out = E - 2 * info.symbols_out - (info.strings_out - info.symbols_out);   // braces, then commas

    // ---- fill: both texts are sized exactly (+ the line feed, + 16 bytes of slack as every output buffer here)
    out_eds_.ensure(E + 1 + 16); out_seds_.ensure(S + 1 + 16);
    uint8_t *oe = out_eds_.as<uint8_t>(), *os = out_seds_.as<uint8_t>();
    const PlaceArgs pa{ra, sflag, sscan, hscan, eoff, soff, n, m, E, S, dst_.as<u64>(), sdst_.as<u64>(), oe, os};
    timed.run("k_sub_place", [&] { hipLaunchKernelGGL(k_sub_place, dim3(grid_for(m, 8192)), dim3(ST), 0, st, pa); });
    if (N)
        timed.run("k_sub_copy", [&] {
            hipLaunchKernelGGL(k_sub_copy, dim3((unsigned)std::min<u64>((N + CP_TILE - 1) / CP_TILE, 1u << 16)), dim3(ST), 0, st, v.chars,
                               v.str_off, m, N, dst_.as<u64>(), oe);
        });
    timed.run("k_sub_seds", [&] {
        hipLaunchKernelGGL(k_sub_seds, dim3(grid_for(m * G, 16384)), dim3(ST), 0, st, v.bits, m, ks, G, sdst_.as<u64>(), bscan, os);
    });
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    timed.harvest();
    eds_out.take(E + 1);
    seds_out.take(S + 1);
    PinnedDownload::copy(eds_out.data, oe, E + 1, st);
    PinnedDownload::copy(seds_out.data, os, S + 1, st);
}

} // namespace edsx
