// merge_scan.hip — device scans of one rank's slice of an .eds / .seds text for the symbol-range partition of the merge
// (merge_multi.hip).  Ports of edsparser_amd/multigpu.py, eds_scan_range / seds_scan_range, whose results are the spec.
//
// .eds, bytes [lo, hi): the window [w0, w1) goes to HBM - w0 the last '{' in front of lo (one group back), w1 up to
// min(end, hi + 65536 + 4 l) - and is read in 4 KB blocks (256 threads x 16 bytes, the tokenisers' geometry):
//   count   per block: '{' minus '}' and string starts inside the slice, braces and commas of the window; whitespace
//   scan    of the four block counters (exclusive_scan_multi)
//   fill    every slice byte gets its brace depth (the state at lo + the '{' - '}' in front of it) and is checked: depth
//           0 or 1 behind it, no ',' at depth 0, no '{' at depth 1; every brace of the window goes to a compact list
//           (position, kind, commas and slice string starts in front of it)
//   check   one thread per brace: the '}' of a COMPACT `}p{x,y}` or FULL `}{p}{x,y}` sentinel whose neighbouring groups
//           hold a comma and whose p has at least max(l, 1) characters; atomicMin keeps the first
// .seds, bytes [lo, hi): '{' per block, scanned; the prefixes stay in HBM, and locating the k-th source set is a binary
// search over them followed by a scan inside one block.  Positions are 64-bit throughout.
#include "merge_scan.hpp"

#include <algorithm>
#include <cstring>

namespace edsx {

namespace {

constexpr u32 SC_BLOCK = 4096;
constexpr u64 SC_MARGIN = 1ull << 16;              // look-ahead of the sentinel search (eds_scan_range's margin)
constexpr u64 SC_CLOSE_LOOK = 1ull << 16;          // bytes the device searches for the '}' of a located source set
constexpr u64 NO_HIT = ~0ull;

struct ScanCtl { u64 nblk, tot[4], ws_slice, ws_win, bad, hit, pad[7]; };
struct BraceEnt { u64 pos_kind, commas, starts; };    // window position << 1 | (is '{'); commas / slice starts in front

__device__ __forceinline__ bool sc_ws(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }

// the 16 bytes of this thread (nb of them exist) and the byte in front of them (prev0 in front of the window)
__device__ __forceinline__ void sc_load(const uint8_t* raw, u64 n, u64 i0, uint8_t prev0, uint8_t (&c)[16], int& nb, uint8_t& prev)
{
    nb = i0 < n ? (n - i0 < 16 ? (int)(n - i0) : 16) : 0;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (nb > 0) v = *reinterpret_cast<const uint4*>(raw + i0);       // (the buffer has 16 bytes of slack behind the text)
    __builtin_memcpy(c, &v, 16);
    prev = i0 == 0 ? prev0 : (nb > 0 ? raw[i0 - 1] : 0);
}

// exclusive prefix of K counters over the 256 threads of the workgroup; total = their sums over the workgroup
template <int K>
__device__ __forceinline__ void sc_block_scan(const u64 (&mine)[K], u64 (&ex)[K], u64 (&total)[K], u64 (*wsum)[K])
{
    const u32 lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    u64 inc[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        inc[j] = mine[j];
        for (int o = 1; o < 64; o <<= 1) {
            const u64 t = __shfl_up(inc[j], o, 64);
            if (lane >= (u32)o) inc[j] += t;
        }
    }
    __syncthreads();                                          // (wsum of the previous block has been read)
    if (lane == 63)
        for (int j = 0; j < K; j++) wsum[wv][j] = inc[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < K; j++) {
        ex[j] = inc[j] - mine[j];
        total[j] = 0;
        for (u32 w = 0; w < 4; w++) {
            const u64 t = wsum[w][j];
            if (w < wv) ex[j] += t;
            total[j] += t;
        }
    }
}

// .eds window [0, n), slice [a, b) of it.  Block counters: D = '{' - '}' in the slice (mod 2^64), S = string starts in the
// slice, B = braces of the window, C = commas of the window.  FILL: validate the slice, write the brace list (br != null).
template <bool FILL>
__global__ void __launch_bounds__(256) k_eds_scan(const uint8_t* __restrict__ raw, u64 n, u64 a, u64 b, uint8_t prev0, u64 inside0,
                                                  u64* __restrict__ D, u64* __restrict__ S, u64* __restrict__ B, u64* __restrict__ C,
                                                  BraceEnt* __restrict__ br, ScanCtl* ctl)
{
    __shared__ u64 wsum[4][4];
    const u64 nblk = (n + SC_BLOCK - 1) / SC_BLOCK;
    bool ws_s = false, ws_w = false, bad = false;
    for (u64 blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const u64 i0 = blk * SC_BLOCK + (u64)threadIdx.x * 16;
        uint8_t c[16], prev;
        int nb;
        sc_load(raw, n, i0, prev0, c, nb, prev);
        u64 mine[4] = {0, 0, 0, 0};
        uint8_t pv = prev;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            if (k < nb) {
                const uint8_t ch = c[k];
                const u64 i = i0 + k;
                const bool in = i >= a && i < b, o = ch == '{', cl = ch == '}', cm = ch == ',';
                if (in) {
                    mine[0] += o ? 1ull : (cl ? ~0ull : 0ull);
                    // a bare run starts behind a '}' (its depth is 0 in any slice that passes the checks below)
                    mine[1] += (o || cm || (!cl && pv == '}')) ? 1 : 0;
                }
                mine[2] += (o || cl) ? 1 : 0;
                mine[3] += cm ? 1 : 0;
                if (!FILL && sc_ws(ch)) { ws_w = true; ws_s |= in; }
                pv = ch;
            }
        }
        u64 ex[4], total[4];
        sc_block_scan<4>(mine, ex, total, wsum);
        if constexpr (!FILL) {
            if (threadIdx.x == 0) { D[blk] = total[0]; S[blk] = total[1]; B[blk] = total[2]; C[blk] = total[3]; }
        } else {
            u64 d = inside0 + D[blk] + ex[0], s = S[blk] + ex[1], e = B[blk] + ex[2], cc = C[blk] + ex[3];
            pv = prev;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                if (k < nb) {
                    const uint8_t ch = c[k];
                    const u64 i = i0 + k;
                    const bool in = i >= a && i < b, o = ch == '{', cl = ch == '}', cm = ch == ',';
                    if (in) {
                        const long long db = (long long)d, da = db + (o ? 1 : (cl ? -1 : 0));
                        if (da < 0 || da > 1 || (cm && db == 0) || (o && db == 1)) bad = true;
                    }
                    if (o || cl) {
                        if (br) br[e] = BraceEnt{(i << 1) | (o ? 1ull : 0ull), cc, s};
                        e++;
                    }
                    if (cm) cc++;
                    if (in) {
                        d += o ? 1ull : (cl ? ~0ull : 0ull);
                        s += (o || cm || (!cl && pv == '}')) ? 1 : 0;
                    }
                    pv = ch;
                }
            }
        }
    }
    if (ws_s) ctl->ws_slice = 1;
    if (ws_w) ctl->ws_win = 1;
    if (bad) ctl->bad = 1;
}

// brace k (1 <= k < nb - 1) is the '}' in front of a sentinel: the first such k whose '}' lies in the slice [a, b)
__global__ void __launch_bounds__(256) k_eds_sentinel(const BraceEnt* __restrict__ br, u64 nb, u64 a, u64 b, u64 need, ScanCtl* ctl)
{
    auto pos = [&](u64 j) { return br[j].pos_kind >> 1; };
    auto open = [&](u64 j) { return (br[j].pos_kind & 1) != 0; };
    auto commas = [&](u64 x, u64 y) { return br[y].commas - br[x].commas; };     // strictly between braces x < y
    for (u64 k = 1 + blockIdx.x * (u64)blockDim.x + threadIdx.x; k + 1 < nb; k += (u64)gridDim.x * blockDim.x) {
        const u64 pk = pos(k);
        if (open(k) || !open(k - 1) || commas(k - 1, k) == 0 || pk < a || pk >= b || !open(k + 1)) continue;
        const u64 p1 = pos(k + 1);
        // COMPACT: } p {x,y}
        const bool compact = p1 - pk - 1 >= need && commas(k, k + 1) == 0 && k + 2 < nb && !open(k + 2) && commas(k + 1, k + 2) > 0;
        // FULL: }{p}{x,y}
        const bool full = !compact && p1 == pk + 1 && k + 4 < nb && !open(k + 2) && pos(k + 2) - p1 - 1 >= need &&
                          commas(k + 1, k + 2) == 0 && open(k + 3) && pos(k + 3) == pos(k + 2) + 1 && !open(k + 4) &&
                          commas(k + 3, k + 4) > 0;
        if (compact || full) atomicMin((unsigned long long*)&ctl->hit, (unsigned long long)k);
    }
}

// .seds slice [0, n): '{' per block, whitespace
__global__ void __launch_bounds__(256) k_seds_count(const uint8_t* __restrict__ raw, u64 n, u64* __restrict__ P, ScanCtl* ctl)
{
    __shared__ u64 wsum[4][1];
    const u64 nblk = (n + SC_BLOCK - 1) / SC_BLOCK;
    bool ws = false;
    for (u64 blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const u64 i0 = blk * SC_BLOCK + (u64)threadIdx.x * 16;
        uint8_t c[16], prev;
        int nb;
        sc_load(raw, n, i0, 0, c, nb, prev);
        u64 mine[1] = {0}, ex[1], total[1];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            if (k < nb) {
                mine[0] += c[k] == '{' ? 1 : 0;
                ws |= sc_ws(c[k]);
            }
        }
        sc_block_scan<1>(mine, ex, total, wsum);
        if (threadIdx.x == 0) P[blk] = total[0];
    }
    if (ws) ctl->ws_slice = 1;
}

// one workgroup per ordinal k: the block whose prefix range holds it (binary search over the exclusive prefixes P), then
// the byte inside the block.  out: slice positions of the k-th '{' and one past the '}' behind it (0: not within reach)
__global__ void __launch_bounds__(256) k_seds_locate(const uint8_t* __restrict__ raw, u64 n, const u64* __restrict__ P, u64 nblk,
                                                     const u64* __restrict__ ord, u64* __restrict__ out)
{
    __shared__ u64 wsum[4][1];
    __shared__ u64 sblk;
    const u64 k = ord[blockIdx.x];
    if (threadIdx.x == 0) {
        u64 lo = 0, hi = nblk;                                 // the last block with P[blk] <= k (P[0] = 0)
        while (hi - lo > 1) {
            const u64 mid = lo + (hi - lo) / 2;
            if (P[mid] <= k) lo = mid; else hi = mid;
        }
        sblk = lo;
    }
    __syncthreads();
    const u64 blk = sblk, i0 = blk * SC_BLOCK + (u64)threadIdx.x * 16;
    uint8_t c[16], prev;
    int nb;
    sc_load(raw, n, i0, 0, c, nb, prev);
    u64 mine[1] = {0}, ex[1], total[1];
    for (int j = 0; j < nb; j++) mine[0] += c[j] == '{' ? 1 : 0;
    sc_block_scan<1>(mine, ex, total, wsum);
    const u64 want = k - P[blk];
    if (want < ex[0] || want >= ex[0] + mine[0]) return;
    u64 seen = ex[0], p = i0;
    for (int j = 0; j < nb; j++) {
        if (c[j] != '{') continue;
        if (seen == want) { p = i0 + j; break; }
        seen++;
    }
    const u64 stop = n - p - 1 < SC_CLOSE_LOOK ? n : p + 1 + SC_CLOSE_LOOK;
    u64 q = p + 1;
    while (q < stop && raw[q] != '}') q++;
    out[2 * blockIdx.x] = p;
    out[2 * blockIdx.x + 1] = q < stop ? q + 1 : 0;
}

unsigned grid_for(u64 nblk) { return (unsigned)std::max<u64>(1, std::min<u64>(nblk, 8192)); }

} // namespace

u64 text_end(const uint8_t* p, u64 n)
{
    while (n && (p[n - 1] == ' ' || (p[n - 1] >= 9 && p[n - 1] <= 13))) n--;
    return n;
}

EdsRangeScan RangeScanner::eds(const uint8_t* eds, u64 n, u64 end, u64 lo, u64 hi, u32 l, hipStream_t st)
{
    EdsRangeScan res;
    if (hi > n) throw ParamError("eds range scan: slice ends behind the text");
    if (hi <= lo) return res;
    // the state at lo and the look-behind: the last '{' in front of lo, and whether a '}' follows it before lo
    u64 w0 = lo, w1 = hi;
    u64 inside0 = 0;
    if (lo > 0) {
        u64 q = lo;
        while (q > 0 && eds[q - 1] != '{') q--;
        if (q > 0) {
            w0 = q - 1;
            inside0 = std::memchr(eds + q, '}', lo - q) ? 0 : 1;
        }
        w1 = std::max(hi, std::min(end, hi + SC_MARGIN + 4ull * l));
    }
    const u64 nw = w1 - w0, a = lo - w0, b = hi - w0;
    const u64 nblk = (nw + SC_BLOCK - 1) / SC_BLOCK;
    raw_.ensure(nw + 16);
    cnt_.ensure(8 * 4 * (nblk + 1));
    tmp_.ensure(8 * 4 * (nblk / SCAN_TILE + 4));
    ctl_.ensure(sizeof(ScanCtl));
    ScanCtl h{};
    h.nblk = nblk;
    h.hit = NO_HIT;
    ScanCtl* ctl = ctl_.as<ScanCtl>();
    EDSX_HIP(hipMemcpyAsync(ctl, &h, sizeof(h), hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemcpyAsync(raw_.ptr, eds + w0, nw, hipMemcpyHostToDevice, st));
    eds_h2d_ += nw;
    const uint8_t* raw = raw_.as<uint8_t>();
    u64* D = cnt_.as<u64>();
    u64 *S = D + (nblk + 1), *B = S + (nblk + 1), *C = B + (nblk + 1);
    const uint8_t prev0 = w0 > 0 ? eds[w0 - 1] : (uint8_t)'}';
    const unsigned grid = grid_for(nblk);
    hipLaunchKernelGGL(k_eds_scan<false>, dim3(grid), dim3(256), 0, st, raw, nw, a, b, prev0, inside0, D, S, B, C,
                       (BraceEnt*)nullptr, ctl);
    {
        ScanSet<4> ss{{D, S, B, C}, {D, S, B, C}, {&ctl->tot[0], &ctl->tot[1], &ctl->tot[2], &ctl->tot[3]}};
        exclusive_scan_multi<4>(ss, &ctl->nblk, tmp_.as<u64>(), st);
    }
    EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    if (h.ws_slice) { res.ok = false; return res; }
    // the sentinel search needs the window without whitespace (some rank reports it otherwise) and four braces
    const u64 nbr = h.tot[2];
    BraceEnt* br = nullptr;
    if (lo > 0 && !h.ws_win && nbr >= 4) {
        br_.ensure(sizeof(BraceEnt) * nbr);
        br = br_.as<BraceEnt>();
    }
    hipLaunchKernelGGL(k_eds_scan<true>, dim3(grid), dim3(256), 0, st, raw, nw, a, b, prev0, inside0, D, S, B, C, br, ctl);
    if (br) {
        const unsigned g = (unsigned)std::min<u64>((nbr + 255) / 256, 4096);
        hipLaunchKernelGGL(k_eds_sentinel, dim3(g), dim3(256), 0, st, (const BraceEnt*)br, nbr, a, b,
                           (u64)std::max<u32>(l, 1), ctl);
    }
    EDSX_HIP(hipGetLastError());
    EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    if (h.bad) { res.ok = false; return res; }
    res.strings = h.tot[1];
    if (br && h.hit != NO_HIT) {
        BraceEnt e[3];                                          // (a hit has at least two braces behind it)
        EDSX_HIP(hipMemcpyAsync(e, br + h.hit, sizeof(e), hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        const u64 p0 = e[0].pos_kind >> 1, p1 = e[1].pos_kind >> 1, p2 = e[2].pos_kind >> 1;
        res.has_cut = true;
        if (p1 != p0 + 1) { res.sym_start = p0 + 1 + w0; res.sym_end = p1 + w0; res.strings_before = e[0].starts; }   // }p{
        else { res.sym_start = p1 + w0; res.sym_end = p2 + 1 + w0; res.strings_before = e[1].starts; }               // }{p}
    }
    return res;
}

bool RangeScanner::seds_count(const uint8_t* seds, u64 n, u64 lo, u64 hi, u64& braces, hipStream_t st)
{
    if (hi > n) throw ParamError("seds range scan: slice ends behind the text");
    s_host_ = seds; s_n_ = n; s_lo_ = lo; s_hi_ = std::max(lo, hi); s_braces_ = 0; s_ok_ = true;
    braces = 0;
    if (hi <= lo) return true;
    const u64 nw = hi - lo, nblk = (nw + SC_BLOCK - 1) / SC_BLOCK;
    sraw_.ensure(nw + 16);
    scnt_.ensure(8 * (nblk + 1));
    stmp_.ensure(8 * (nblk / SCAN_TILE + 4));
    sctl_.ensure(sizeof(ScanCtl));
    ScanCtl h{};
    h.nblk = nblk;
    ScanCtl* ctl = sctl_.as<ScanCtl>();
    EDSX_HIP(hipMemcpyAsync(ctl, &h, sizeof(h), hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemcpyAsync(sraw_.ptr, seds + lo, nw, hipMemcpyHostToDevice, st));
    seds_h2d_ += nw;
    u64* P = scnt_.as<u64>();
    hipLaunchKernelGGL(k_seds_count, dim3(grid_for(nblk)), dim3(256), 0, st, sraw_.as<uint8_t>(), nw, P, ctl);
    {
        ScanSet<1> ss{{P}, {P}, {&ctl->tot[0]}};
        exclusive_scan_multi<1>(ss, &ctl->nblk, stmp_.as<u64>(), st);
    }
    EDSX_HIP(hipGetLastError());
    EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    if (h.ws_slice) { s_ok_ = false; return false; }
    s_braces_ = braces = h.tot[0];
    return true;
}

void RangeScanner::seds_locate(const u64* ordinals, size_t k, u64* p0, u64* p1, hipStream_t st)
{
    if (!k) return;
    if (!s_ok_) throw ParamError("seds range scan: the slice is not plain text");
    for (size_t i = 0; i < k; i++)
        if (ordinals[i] >= s_braces_) throw ParamError("seds range scan: ordinal out of range");
    const u64 nw = s_hi_ - s_lo_, nblk = (nw + SC_BLOCK - 1) / SC_BLOCK;
    sout_.ensure(8 * 3 * k);
    u64* d_ord = sout_.as<u64>();
    u64* d_out = d_ord + k;
    std::vector<u64> out(2 * k);
    EDSX_HIP(hipMemcpyAsync(d_ord, ordinals, 8 * k, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_seds_locate, dim3((unsigned)k), dim3(256), 0, st, sraw_.as<uint8_t>(), nw, (const u64*)scnt_.as<u64>(), nblk,
                       (const u64*)d_ord, d_out);
    EDSX_HIP(hipGetLastError());
    EDSX_HIP(hipMemcpyAsync(out.data(), d_out, 16 * k, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i < k; i++) {
        p0[i] = out[2 * i] + s_lo_;
        if (out[2 * i + 1]) { p1[i] = out[2 * i + 1] + s_lo_; continue; }
        // the '}' lies behind the slice (or far into it): find('}') over the rest of the buffer, like the Python spec
        const void* q = std::memchr(s_host_ + p0[i] + 1, '}', s_n_ - p0[i] - 1);
        p1[i] = q ? (u64)(static_cast<const uint8_t*>(q) - s_host_) + 1 : 0;
    }
}

} // namespace edsx
