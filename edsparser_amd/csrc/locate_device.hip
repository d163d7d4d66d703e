// locate_device.hip — find every occurrence of every pattern in an EDS on gfx950 (edsx_eds_locate).
//
// An occurrence is (string g, offset o, choices): the walk takes g[o:], then the only string of every common symbol and
// the chosen string of every degenerate one, each cut to what the pattern still needs, until the pattern's length is
// reached; with sources the strings used must share a path (first_empty_step, the rule of k_pat_check).  Hits come back
// per pattern, ascending by (g, o), then by choices: depth-first order over the alternatives in file order.
//
// Work is (characters of the pool) x (patterns), so the test per pair is a masked compare of 8 bytes:
//   - patterns are taken in chunks of LCHUNK whose seeds (first min(L, 8) bytes as a u64, and a mask) sit in LDS; all
//     lanes read the same LDS word, which broadcasts;
//   - one lane owns one character of the pool: it loads its 8 text bytes once per chunk and compares them with every
//     seed, masked to min(L, 8, what is left of its string);
//   - only on a seed match does the lane read the pattern from HBM and walk.  The walk is a depth-first search with an
//     explicit stack of local string indices in LDS (MAX_CHOICES x LNT u32: out of registers and out of scratch); a
//     step re-walks from the start with the stack as its choices, so the stack is the whole state.
// Position -> string: two binary searches in str_off per tile (its first and last character), then every lane searches
// between the two.  String -> symbol: a table built once per call.
//
// Order without a sort: count -> scan -> fill.  k_locate<M_COUNT> writes one counter per (pattern, tile of LTILE
// positions); an exclusive scan over the [pattern][tile] array places every tile, the per-pattern sums give totals, the
// cap and hit_off.  k_locate<M_HITS> recomputes the tiles that have hits (a tile whose LCHUNK counters are all zero is
// skipped, which is nearly every tile for patterns of useful length): per (pattern, 64-position wave segment) counters
// in LDS, a prefix over the segments, then a wave prefix over the lanes place each start's hits.  It also leaves every
// hit's number of choices; a scan of those is choice_off, and k_locate<M_CHOICES>, the same kernel, writes the choices.
// No atomics on the result path; the counters use LDS atomics and the flags one atomicOr per flagged start.
#include "locate_device.hpp"
#include "kernel_times.hpp"

#include <chrono>
#include <cstring>

namespace edsx {

namespace {

constexpr int LNT = 128;                 // lanes per block
constexpr int LCHUNK = 64;               // patterns per chunk (seeds in LDS)
constexpr int LTILE = 2048;              // positions per tile
constexpr int LSEG = LTILE / 64;         // wave segments per tile
constexpr u32 MAXC = LocatePipeline::MAX_CHOICES;
enum { M_COUNT = 0, M_HITS = 1, M_CHOICES = 2 };
enum { W_LEAF, W_DEAD, W_BRANCH, W_OVER };

struct LocArgs {
    const u64* size; const u64* ent_off; const u64* str_off; const uint8_t* chars; const u64* bits; u32 W;
    const u64* cc; const u64* cd; const u64* str_sym; u64 n, m, N;
    u64 np; const u64* poff; const uint8_t* pat; const u64* seed; const u64* pmask;    // this launch's patterns
    u64 max_hits; u32 common_only; u64 ntiles;
    u64* counts;                         // M_COUNT: out, [np][ntiles]; fill: their exclusive scan, np * ntiles + 1 entries
    u32* flags;                          // per pattern (M_COUNT)
    const u64* hoff; LocateHit* hits; u64* hit_k;      // M_HITS
    const u64* coff; int32_t* choices;                 // M_CHOICES
};

__global__ void k_loc_str_sym(const u64* __restrict__ size, const u64* __restrict__ ent_off, u64 n, u64* __restrict__ str_sym)
{
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 e0 = ent_off[i], sz = size[i];
        for (u64 j = 0; j < sz; j++) str_sym[e0 + j] = i;
    }
}

// last g in [lo, hi) with str_off[g] <= p (str_off[lo] <= p): the string that holds character p, never an empty one
__device__ __forceinline__ u64 find_string(const u64* __restrict__ str_off, u64 lo, u64 hi, u64 p)
{
    while (hi - lo > 1) { const u64 mid = lo + ((hi - lo) >> 1); if (str_off[mid] <= p) lo = mid; else hi = mid; }
    return lo;
}

struct Start { bool ok; u64 g, s, o, text, lmask; };

__device__ __forceinline__ Start lane_start(const LocArgs& a, u64 p, u64 pe, u64 glo, u64 ghi)
{
    Start r{};
    if (p >= pe) return r;
    r.g = find_string(a.str_off, glo, ghi + 1, p);
    const u64 s0 = a.str_off[r.g], rem = a.str_off[r.g + 1] - p;
    r.o = p - s0;
    r.s = a.str_sym[r.g];
    r.ok = !(a.common_only && a.size[r.s] > 1);
    // the 8 bytes at p from two aligned words; the word after the pool's last one is not read
    const u64* words = reinterpret_cast<const u64*>(a.chars);
    const u64 w = p >> 3;
    const u32 sh = (u32)(p & 7) * 8;
    const u64 lo = words[w], hi = ((w + 1) << 3) < a.N ? words[w + 1] : 0;
    r.text = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
    r.lmask = ~0ull >> (64 - 8 * (u32)min(rem, (u64)8));
    return r;
}

__device__ __forceinline__ bool same_bytes(const uint8_t* __restrict__ x, const uint8_t* __restrict__ y, u64 n)
{
    for (u64 j = 0; j < n; j++) if (x[j] != y[j]) return false;
    return true;
}

// One descent: from string g of symbol s at offset o, with stk[0 .. k) (stride LNT) as the choices.  W_LEAF: the pattern
// is spelt with exactly these choices, over T symbols; W_BRANCH: a (k+1)-th choice is needed; W_OVER: choice k - 1 is past
// its symbol's last string; W_DEAD: a mismatch, or the EDS ends first.
__device__ int walk(const LocArgs& a, u64 s, u64 g, u64 o, const uint8_t* __restrict__ P, u64 L, const u32* stk, u32 k, u64& T)
{
    u64 s0 = a.str_off[g] + o;
    u64 got = min(a.str_off[g + 1] - s0, L);
    if (!same_bytes(a.chars + s0, P, got)) return W_DEAD;
    u64 sym = s + 1;
    u32 d = 0;
    for (; got < L && sym < a.n; sym++) {
        const u64 sz = a.size[sym];
        if (sz == 0) continue;                                 // (the tokenisers never make one)
        u64 sid = a.ent_off[sym];
        if (sz > 1) {
            if (d == k) return W_BRANCH;
            const u64 j = stk[(u64)d * LNT];
            if (j >= sz) return W_OVER;
            sid += j;
            d++;
        }
        s0 = a.str_off[sid];
        const u64 take = min(a.str_off[sid + 1] - s0, L - got);
        if (!same_bytes(a.chars + s0, P + got, take)) return W_DEAD;
        got += take;
    }
    T = sym - s;
    return got == L ? W_LEAF : W_DEAD;
}

// Depth-first search from one start; emit(i, k, T) for occurrence i < limit with k choices on the stack.  Returns
// min(occurrences, limit); flg: bit 0 when there was one more, bit 1 when a walk was cut at choice MAXC + 1.
template <class Emit>
__device__ u64 dfs(const LocArgs& a, const Start& st, const uint8_t* __restrict__ P, u64 L, u32* stk, u64 limit, u32& flg, Emit emit)
{
    u64 count = 0, T = 0;
    u32 k = 0;
    for (;;) {
        const int r = walk(a, st.s, st.g, st.o, P, L, stk, k, T);
        if (r == W_BRANCH) {
            if (k < MAXC) { stk[(u64)k * LNT] = 0; k++; continue; }
            flg |= 2;
        } else if (r == W_LEAF) {
            bool ok = true;
            if (a.bits)
                ok = first_empty_step(a.bits, a.W, T, [&](u64 t, u64& d) {
                         if (t == 0) return st.g;
                         const u64 sym = st.s + t;
                         u64 sid = a.ent_off[sym];
                         if (a.size[sym] > 1) { sid += stk[d * LNT]; d++; }
                         return sid;
                     }) == Q_NONE;
            if (ok) {
                if (count == limit) { flg |= 1; return count; }
                emit(count, k, T);
                count++;
            }
        } else if (r == W_OVER) {
            k--;
        }
        if (k == 0) return count;
        stk[(u64)(k - 1) * LNT]++;
    }
}

// f(q, seg, m, st) for every pattern q of the chunk and every 64-position wave segment seg of the tile, in the same
// order in every wave: m says whether the lane's character passes pattern q's seed.
template <class F>
__device__ __forceinline__ void each_pair(const LocArgs& a, u64 p0, u64 pe, u64 glo, u64 ghi, u32 nq, const u64* seed,
                                          const u64* pmask, F f)
{
    for (u32 it = 0; it < LTILE / LNT; it++) {
        const u64 base = p0 + (u64)it * LNT;
        if (base >= pe) break;
        const Start st = lane_start(a, base + threadIdx.x, pe, glo, ghi);
        const u32 seg = it * (LNT / 64) + (threadIdx.x >> 6);
        for (u32 q = 0; q < nq; q++) f(q, seg, st.ok && ((st.text ^ seed[q]) & pmask[q] & st.lmask) == 0, st);
    }
}

template <int MODE>
__global__ void __launch_bounds__(LNT) k_locate(LocArgs a)
{
    constexpr int NCNT = MODE == M_COUNT ? LCHUNK : LCHUNK * LSEG;
    __shared__ u32 stack[MAXC * LNT];
    __shared__ u64 seed[LCHUNK], pmask[LCHUNK], cnt[NCNT], grange[2];
    const u32 tid = threadIdx.x;
    const u64 q0 = (u64)blockIdx.y * LCHUNK;
    const u32 nq = (u32)min((u64)LCHUNK, a.np - q0);
    if (tid < nq) { seed[tid] = a.seed[q0 + tid]; pmask[tid] = a.pmask[q0 + tid]; }
    u32* stk = stack + tid;
    auto pattern = [&](u32 q, const uint8_t*& P, u64& L) { const u64 b = a.poff[q0 + q]; P = a.pat + b; L = a.poff[q0 + q + 1] - b; };
    for (u64 tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        if (MODE != M_COUNT) {                                 // only the tiles that have hits are recomputed
            const u64* c = a.counts + (q0 + tid) * a.ntiles + tile;
            if (!__syncthreads_or(tid < nq && c[1] != c[0])) continue;
        }
        const u64 p0 = tile * LTILE, pe = min(p0 + (u64)LTILE, a.N);
        if (tid == 0) grange[0] = find_string(a.str_off, 0, a.m, p0);
        if (tid == 64) grange[1] = find_string(a.str_off, 0, a.m, pe - 1);
        for (u32 i = tid; i < (u32)NCNT; i += LNT) cnt[i] = 0;
        __syncthreads();
        const u64 glo = grange[0], ghi = grange[1];
        // counts: per pattern (M_COUNT), or per pattern and wave segment
        each_pair(a, p0, pe, glo, ghi, nq, seed, pmask, [&](u32 q, u32 seg, bool m, const Start& st) {
            if (!m) return;
            const uint8_t* P; u64 L;
            pattern(q, P, L);
            u32 flg = 0;
            const u64 c = dfs(a, st, P, L, stk, a.max_hits, flg, [](u64, u32, u64) {});
            if (c) atomicAdd((unsigned long long*)&cnt[MODE == M_COUNT ? q : q * LSEG + seg], (unsigned long long)c);
            if (MODE == M_COUNT && flg) atomicOr(&a.flags[q0 + q], flg);
        });
        __syncthreads();
        if (MODE == M_COUNT) {
            if (tid < nq) a.counts[(q0 + tid) * a.ntiles + tile] = cnt[tid];
            __syncthreads();
            continue;
        }
        if (tid < nq) {                                        // exclusive prefix over the segments of pattern tid
            u64 run = 0;
            for (int g = 0; g < LSEG; g++) { const u64 v = cnt[tid * LSEG + g]; cnt[tid * LSEG + g] = run; run += v; }
        }
        __syncthreads();
        each_pair(a, p0, pe, glo, ghi, nq, seed, pmask, [&](u32 q, u32 seg, bool m, const Start& st) {
            if (!__any(m)) return;                             // (the same for the whole wave)
            const uint8_t* P; u64 L;
            pattern(q, P, L);
            u32 flg = 0;
            const u64 c = m ? dfs(a, st, P, L, stk, a.max_hits, flg, [](u64, u32, u64) {}) : 0;
            u64 incl = c;
            for (int o = 1; o < 64; o <<= 1) { const u64 x = __shfl_up(incl, o, 64); if ((int)(tid & 63) >= o) incl += x; }
            // index of this start's first hit among the pattern's
            const u64 first = a.counts[(q0 + q) * a.ntiles + tile] - a.counts[(q0 + q) * a.ntiles] + cnt[q * LSEG + seg] + incl - c;
            if (c == 0 || first >= a.max_hits) return;
            const u64 h0 = a.hoff[q0 + q] + first, hend = a.hoff[q0 + q + 1];
            dfs(a, st, P, L, stk, min(c, a.max_hits - first), flg, [&](u64 i, u32 k, u64 T) {
                if (h0 + i >= hend) return;                    // (never: the counts of the two passes agree)
                if (MODE == M_HITS) {
                    a.hits[h0 + i] = LocateHit{a.size[st.s] > 1 ? Q_NONE : a.cc[st.s] + st.o, st.s, st.g - a.ent_off[st.s], st.o};
                    a.hit_k[h0 + i] = k;
                } else {
                    int32_t* out = a.choices + a.coff[h0 + i];
                    u32 d = 0;
                    for (u64 sym = st.s + 1; sym < st.s + T && d < k; sym++)
                        if (a.size[sym] > 1) { out[d] = (int32_t)(a.cd[sym] + stk[(u64)d * LNT]); d++; }
                }
            });
        });
        __syncthreads();
    }
}

// per pattern: the sum of its tiles, what the cap keeps of it, and flag bit 0 when the cap left something out
__global__ void k_loc_kept(const u64* __restrict__ scanned, u64 ntiles, u64 np, u64 max_hits, u64* __restrict__ totals,
                           u64* __restrict__ kept, u32* __restrict__ flags)
{
    for (u64 q = blockIdx.x * (u64)blockDim.x + threadIdx.x; q < np; q += (u64)gridDim.x * blockDim.x) {
        const u64 raw = scanned[(q + 1) * ntiles] - scanned[q * ntiles];
        totals[q] = raw;
        kept[q] = min(raw, max_hits);
        if (raw > max_hits) flags[q] |= 1;
    }
}

} // namespace

void LocatePipeline::run(QueryPipeline& qp, DeviceEds& de, const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n,
                         size_t n, const u64* pattern_off, const uint8_t* patterns, u64 max_hits, bool common_only, LocateOut& out,
                         hipStream_t st)
{
    QueryInfo& info = qp.info();
    info = QueryInfo{};
    if (max_hits == 0) throw ParamError("max_hits must be at least 1");
    for (size_t q = 0; q < n; q++) {
        if (pattern_off[q + 1] < pattern_off[q]) throw ParamError("pattern_off decreases at pattern " + std::to_string(q));
        if (pattern_off[q + 1] == pattern_off[q]) throw ParamError("Pattern " + std::to_string(q) + " is empty");
    }
    max_hits = std::min(max_hits, MAX_HITS_CEILING);
    const u64 ns = qp.tables(de, eds, eds_n, seds, seds_n, st);
    out = LocateOut{};
    out.hit_off.assign(n + 1, 0);
    out.choice_off.assign(1, 0);
    out.totals.assign(n, 0);
    out.flags.assign(n, 0);
    const u64 N = de.n_chars(), m = de.m();
    if (n == 0 || ns == 0 || N == 0) return;                   // an empty EDS, or one without a character: no hits
    const EdsView v = de.view();

    const u64 ntiles = (N + LTILE - 1) / LTILE;
    str_sym_.ensure(8 * m);
    ctl_.ensure(8 * 4);
    u64* ctl = ctl_.as<u64>();                                  // scan lengths: [0] counters  [1] patterns  [2] hits
    TimedRuns timed(st, nullptr);
    timed.run("k_loc_str_sym", [&] {
        hipLaunchKernelGGL(k_loc_str_sym, dim3(grid_for(ns, 4096)), dim3(256), 0, st, v.sym.size, v.sym.ent_off, ns, str_sym_.as<u64>());
    }, &info.tables_ms);
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    timed.harvest();

    // patterns per launch: whole chunks, within the counter budget
    const u64 group = std::max<u64>(LCHUNK, COUNT_ENTRIES / ntiles / LCHUNK * LCHUNK);
    LocArgs a{};
    a.size = v.sym.size; a.ent_off = v.sym.ent_off; a.str_off = v.str_off; a.chars = v.chars; a.bits = v.bits; a.W = v.W;
    a.cc = qp.cum_common(); a.cd = qp.cum_deg(); a.str_sym = str_sym_.as<u64>();
    a.n = ns; a.m = m; a.N = N; a.max_hits = max_hits; a.common_only = common_only ? 1 : 0; a.ntiles = ntiles;
    std::vector<u64> seed, pmask, poff, hoff, coff;
    std::vector<u32> flg;
    for (u64 g0 = 0; g0 < n; g0 += group) {
        const u64 np = std::min<u64>(group, n - g0), len = np * ntiles, pbase = pattern_off[g0], pbytes = pattern_off[g0 + np] - pbase;
        seed.assign(np, 0); pmask.assign(np, 0); poff.resize(np + 1);
        for (u64 q = 0; q <= np; q++) poff[q] = pattern_off[g0 + q] - pbase;
        for (u64 q = 0; q < np; q++) {
            const u64 l8 = std::min<u64>(poff[q + 1] - poff[q], 8);
            std::memcpy(&seed[q], patterns + pbase + poff[q], l8);
            pmask[q] = ~0ull >> (64 - 8 * l8);
        }
        pat_.ensure(pbytes); poff_.ensure(8 * (np + 1)); seed_.ensure(8 * np); pmask_.ensure(8 * np);
        counts_.ensure(8 * (len + 1)); flags_.ensure(4 * np); kept_.ensure(8 * np); totals_.ensure(8 * np); hoff_.ensure(8 * (np + 1));
        scan_tmp_.ensure(8 * (len / SCAN_TILE + 4));
        EDSX_HIP(hipMemcpyAsync(pat_.ptr, patterns + pbase, pbytes, hipMemcpyHostToDevice, st));
        EDSX_HIP(hipMemcpyAsync(poff_.ptr, poff.data(), 8 * (np + 1), hipMemcpyHostToDevice, st));
        EDSX_HIP(hipMemcpyAsync(seed_.ptr, seed.data(), 8 * np, hipMemcpyHostToDevice, st));
        EDSX_HIP(hipMemcpyAsync(pmask_.ptr, pmask.data(), 8 * np, hipMemcpyHostToDevice, st));
        EDSX_HIP(hipMemsetAsync(flags_.ptr, 0, 4 * np, st));
        u64 hctl[3] = {len, np, 0};
        EDSX_HIP(hipMemcpyAsync(ctl, hctl, sizeof(hctl), hipMemcpyHostToDevice, st));
        a.np = np; a.poff = poff_.as<u64>(); a.pat = pat_.as<uint8_t>(); a.seed = seed_.as<u64>(); a.pmask = pmask_.as<u64>();
        a.counts = counts_.as<u64>(); a.flags = flags_.as<u32>(); a.hoff = hoff_.as<u64>();
        // about 4096 blocks in flight, whatever the number of chunks; a block strides over the tiles
        const u64 chunks = (np + LCHUNK - 1) / LCHUNK;
        const dim3 grid((unsigned)std::min<u64>(ntiles, std::max<u64>(256, 4096 / chunks)), (unsigned)chunks);
        timed.run("count", [&] {
            hipLaunchKernelGGL(k_locate<M_COUNT>, grid, dim3(LNT), 0, st, a);
            exclusive_scan_u64(a.counts, a.counts, ctl, a.counts + len, scan_tmp_.as<u64>(), st);
            hipLaunchKernelGGL(k_loc_kept, dim3(grid_for(np, 4096)), dim3(256), 0, st, a.counts, ntiles, np, max_hits, totals_.as<u64>(),
                               kept_.as<u64>(), a.flags);
            exclusive_scan_u64(kept_.as<u64>(), hoff_.as<u64>(), ctl + 1, hoff_.as<u64>() + np, scan_tmp_.as<u64>(), st);
        }, &info.kernel_ms);
        hoff.resize(np + 1); flg.resize(np);
        EDSX_HIP(hipMemcpyAsync(hoff.data(), hoff_.ptr, 8 * (np + 1), hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipMemcpyAsync(out.totals.data() + g0, totals_.ptr, 8 * np, hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipMemcpyAsync(flg.data(), flags_.ptr, 4 * np, hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        EDSX_HIP(hipGetLastError());
        timed.harvest();
        const u64 H = hoff[np], h0 = out.hits.size();
        for (u64 q = 0; q < np; q++) { out.flags[g0 + q] = (uint8_t)flg[q]; out.hit_off[g0 + q + 1] = h0 + hoff[q + 1]; }
        if (H == 0) continue;

        hits_.ensure(sizeof(LocateHit) * H); hit_k_.ensure(8 * H); coff_.ensure(8 * (H + 1));
        scan_tmp_.ensure(8 * (std::max(len, H) / SCAN_TILE + 4));
        EDSX_HIP(hipMemcpyAsync(ctl + 2, &H, 8, hipMemcpyHostToDevice, st));
        a.hits = hits_.as<LocateHit>(); a.hit_k = hit_k_.as<u64>(); a.coff = coff_.as<u64>();
        timed.run("hits", [&] {
            hipLaunchKernelGGL(k_locate<M_HITS>, grid, dim3(LNT), 0, st, a);
            exclusive_scan_u64(a.hit_k, coff_.as<u64>(), ctl + 2, coff_.as<u64>() + H, scan_tmp_.as<u64>(), st);
        }, &info.kernel_ms);
        u64 K = 0;
        EDSX_HIP(hipMemcpyAsync(&K, coff_.as<u64>() + H, 8, hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        EDSX_HIP(hipGetLastError());
        timed.harvest();
        if (K) {
            choices_.ensure(4 * K);
            a.choices = choices_.as<int32_t>();
            timed.run("choices", [&] { hipLaunchKernelGGL(k_locate<M_CHOICES>, grid, dim3(LNT), 0, st, a); }, &info.kernel_ms);
            EDSX_HIP(hipStreamSynchronize(st));
            EDSX_HIP(hipGetLastError());
            timed.harvest();
        }
        const auto t0 = std::chrono::steady_clock::now();
        const u64 k0 = out.choices.size();
        out.hits.resize(h0 + H);
        coff.resize(H + 1);
        out.choices.resize(k0 + K);
        EDSX_HIP(hipMemcpyAsync(out.hits.data() + h0, hits_.ptr, sizeof(LocateHit) * H, hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipMemcpyAsync(coff.data(), coff_.ptr, 8 * (H + 1), hipMemcpyDeviceToHost, st));
        if (K) EDSX_HIP(hipMemcpyAsync(out.choices.data() + k0, choices_.ptr, 4 * K, hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        for (u64 h = 1; h <= H; h++) out.choice_off.push_back(k0 + coff[h]);
        info.download_ms += since_ms(t0);
    }
}

} // namespace edsx
