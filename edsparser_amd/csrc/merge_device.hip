// merge_device.hip — EDS -> l-EDS merge (LINEAR with sources / CARTESIAN) on gfx950.
//
// Replaces the reference's round loop (src/cpp/lib/transforms/eds_transforms.cpp):
//   is_leds :439-468 + select_independent_merge_pairs :46-107  -> k_should, max-scan, k_select
//   merge_multiple_pairs :120-196 -> EDS::merge_adjacent (eds.cpp:1425-1695) -> k_pair_count / k_pair_fill
//   reconstruct_eds :207-296 (text round trip, an identity)            -> index compaction (scan)
//   EDS::save / save_sources (eds.cpp:600-631, :641-659)               -> k_fin_* kernels
// The reference rebuilds the whole container for every merged pair (quadratic); here a round
// touches each symbol once and strings are materialised once, at the end.
//
// Data layout in HBM
//   chars/str_off     all original strings back to back, and the round-0 symbol arrays: DeviceEds (eds_device.hip)
//   entry pool        one entry per string of every symbol that ever existed: leaves are the
//                     original strings; an entry made by a merge points to its (left, right)
//                     parents, carries its length and, for LINEAR, its source set as a bitset of
//                     W 64-bit words (bit 0 = the universal path "0").  A symbol's entries are
//                     contiguous in the pool, in the reference's product order (left outer).
//                     elen / bits are the DeviceEds's arrays, taken over through DeviceEds::consume and
//                     grown here; left / right are the merge's own.
//   symbols           size[i], ent_off[i], len1[i] (length of the only string when size == 1)
//                     for the current round, double buffered: the DeviceEds's arrays and a second set.
#include "merge_device.hpp"

#include <algorithm>
#include <cstring>

namespace edsx {

constexpr u32 LEAF = 0xffffffffu;
constexpr u64 NO_ERR = ~0ull;

struct Pool { u32* left; u32* right; u32* elen; u64* bits; u32 W; };

// ---- per round -------------------------------------------------------------------------------
// should[i] for the pair (i, i+1): eds_transforms.cpp:75-97
__global__ void k_should(SymArrays s, u64 n, u64 l, u64* __restrict__ runmark, u64* __restrict__ any)
{
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        bool sh = false;
        if (i + 1 < n) {
            const bool degA = s.size[i] > 1, degB = s.size[i + 1] > 1;
            if (!degA && i > 0 && s.len1[i] < l) sh = true;
            if (!degB && i + 1 < n - 1 && s.len1[i + 1] < l) sh = true;
            if (degA && degB) sh = true;
        }
        // run mark for the max-scan: start of a run of consecutive `should` -> i+1, a gap -> 0 is
        // not enough (a gap must cut the run), so gaps publish their own index with bit 63 set
        u64 prev_sh = 0;
        if (i > 0) {
            const bool degP = s.size[i - 1] > 1, degA = s.size[i] > 1;
            bool p = false;
            if (!degP && i - 1 > 0 && s.len1[i - 1] < l) p = true;
            if (!degA && i < n - 1 && s.len1[i] < l) p = true;
            if (degP && degA) p = true;
            prev_sh = p;
        }
        // value = 2*(position of the latest event)+kind, kind 1 = run start, 0 = gap; monotone in i
        u64 v = 0;
        if (!sh) v = 2 * (i + 1);
        else if (!prev_sh) v = 2 * (i + 1) + 1;
        runmark[i] = v;
        if (sh) *any = 1;
    }
}

// selected pairs: even offsets inside every run of consecutive `should` (:63-66, :99-103 greedy)
__global__ void k_select(const u64* __restrict__ runscan, u64 n, u64* __restrict__ sel, u64* __restrict__ keep)
{
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 v = runscan[i];
        bool s = false;
        if (v & 1) {                                   // inside a run that started at (v>>1)-1
            const u64 start = (v >> 1) - 1;
            s = ((i - start) & 1) == 0;
        }
        sel[i] = s;
    }
}
__global__ void k_keep(const u64* __restrict__ sel, u64 n, u64* __restrict__ keep)
{
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
        keep[i] = !(i > 0 && sel[i - 1]);
}

// source-set intersection with the universal path 0 (eds.cpp:1481-1500); returns non-empty?
__device__ __forceinline__ bool src_intersect(const u64* a, const u64* b, u32 W, u64* out)
{
    const bool ua = a[0] & 1, ub = b[0] & 1;
    bool any = false;
    for (u32 w = 0; w < W; w++) {
        u64 v;
        if (ua && ub) v = w == 0 ? 1ull : 0ull;
        else if (ua) v = b[w];
        else if (ub) v = a[w];
        else v = a[w] & b[w];
        if (out) out[w] = v;
        any |= v != 0;
    }
    return any;
}

struct RoundParams {
    SymArrays cur, nxt; Pool pool; u64 n; const u64* sel; const u64* keep; const u64* newidx;
    u64* newcnt; const u64* newoff; u64 pool_used; u64* err_pos; u64* err_big; int linear;
};

// survivors of every selected pair (0 for symbols that are copied)
__global__ void k_pair_count(RoundParams p)
{
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < p.n; i += (u64)gridDim.x * blockDim.x) {
        if (!p.keep[i]) continue;
        u64 cnt = 0;
        if (p.sel[i]) {
            const u64 na = p.cur.size[i], nb = p.cur.size[i + 1];
            if (!p.linear) {
                if (na != 0 && nb > 0xffffffffull / na) { atomicMin(p.err_big, i); cnt = 0; }
                else cnt = na * nb;
            } else {
                const u64 a0 = p.cur.ent_off[i], b0 = p.cur.ent_off[i + 1];
                for (u64 x = 0; x < na; x++)
                    for (u64 y = 0; y < nb; y++)
                        cnt += src_intersect(p.pool.bits + (a0 + x) * p.pool.W, p.pool.bits + (b0 + y) * p.pool.W,
                                             p.pool.W, nullptr);
                if (cnt == 0) atomicMin(p.err_pos, i);           // eds.cpp:1513-1519
            }
        }
        p.newcnt[p.newidx[i]] = cnt;
    }
}

// new symbol list + the entries of the merged symbols (product order: left outer, right inner)
__global__ void k_pair_fill(RoundParams p)
{
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < p.n; i += (u64)gridDim.x * blockDim.x) {
        if (!p.keep[i]) continue;
        const u64 j = p.newidx[i];
        if (!p.sel[i]) {
            p.nxt.size[j] = p.cur.size[i]; p.nxt.ent_off[j] = p.cur.ent_off[i]; p.nxt.len1[j] = p.cur.len1[i];
            continue;
        }
        const u64 na = p.cur.size[i], nb = p.cur.size[i + 1];
        const u64 a0 = p.cur.ent_off[i], b0 = p.cur.ent_off[i + 1];
        u64 o = p.pool_used + p.newoff[j];
        const u64 first = o;
        for (u64 x = 0; x < na; x++)
            for (u64 y = 0; y < nb; y++) {
                if (p.linear) {
                    const u64* sa = p.pool.bits + (a0 + x) * p.pool.W;
                    const u64* sb = p.pool.bits + (b0 + y) * p.pool.W;
                    // test first: slot o belongs to the next symbol once this one's survivors are written
                    if (!src_intersect(sa, sb, p.pool.W, nullptr)) continue;
                    src_intersect(sa, sb, p.pool.W, p.pool.bits + o * p.pool.W);
                }
                p.pool.left[o] = (u32)(a0 + x);
                p.pool.right[o] = (u32)(b0 + y);
                p.pool.elen[o] = p.pool.elen[a0 + x] + p.pool.elen[b0 + y];
                o++;
            }
        const u64 cnt = o - first;
        p.nxt.size[j] = cnt; p.nxt.ent_off[j] = first; p.nxt.len1[j] = cnt == 1 ? p.pool.elen[first] : 0;
    }
}

// ---- final text --------------------------------------------------------------------------------
struct FinParams {
    SymArrays sym; Pool pool; u64 n; const u64* cum;     // cum = exclusive scan of sym.size
    u32* fin_ent; uint8_t* fin_flag;                      // per final string: entry, 1 = first | 2 = last | 4 = brackets
    u64* bytes; u64* sbytes;                              // per final string: eds bytes / seds bytes (-> offsets)
    const uint8_t* chars; const u64* str_off;
    uint8_t* out; uint8_t* sout; u64* err; int compact, linear;
    u32* spill = nullptr; u32 spill_depth = 0;            // serial walk after more than FIN_STACK - 2 rounds: a stack per string in HBM
};

__global__ void k_fin_list(FinParams p)
{
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < p.n; i += (u64)gridDim.x * blockDim.x) {
        const u64 k = p.sym.size[i], e0 = p.sym.ent_off[i], t0 = p.cum[i];
        const bool br = !p.compact || k > 1;                   // eds.cpp:613
        for (u64 x = 0; x < k; x++) {
            const u64 t = t0 + x;
            p.fin_ent[t] = (u32)(e0 + x);
            uint8_t fl = (x == 0 ? 1 : 0) | (x + 1 == k ? 2 : 0) | (br ? 4 : 0);
            p.fin_flag[t] = fl;
            p.bytes[t] = (u64)p.pool.elen[e0 + x] + ((x == 0) ? (br ? 1 : 0) : 1) + ((x + 1 == k && br) ? 1 : 0);
            if (p.linear) {
                const u64* b = p.pool.bits + (e0 + x) * p.pool.W;
                u64 sb = 1;                                    // '{' ; every id is followed by ',' or '}'
                for (u32 w = 0; w < p.pool.W; w++) {
                    u64 v = b[w];
                    while (v) { u32 id = w * 64 + __builtin_ctzll(v); v &= v - 1; sb += ndigits(id ? id : 1) + 1; }
                }
                p.sbytes[t] = sb;
            }
        }
    }
}

// ---- final text ---------------------------------------------------------------------------------------
// A string of the result is the left-to-right concatenation of the leaves of its entry's merge tree.  Walking that tree
// with one thread per string is a chain of dependent loads as long as the string has leaves (l = 32 on a 10 % EDS:
// strings of several hundred leaves, 1.8 ms for the longest one alone).  Every entry carries its length, so a node's
// output offset follows from its parent's (right child = offset + length of the left one) and the subtrees can be
// expanded side by side: a workgroup takes a batch of `ns` consecutive strings, keeps (entry, offset) items on a stack
// in LDS, and in every round each thread pops one item - a leaf is copied to its place, an inner entry pushes its two
// children (empty subtrees are dropped, so the items of one level cover disjoint bytes).  The latency per string is its
// tree's depth, not its number of leaves.  Leaves of 256 bytes and more are copied by the whole workgroup.  A stack that
// would overflow (far beyond 256 x depth items) sends the batch to the serial walk below, which also has the only
// depth limit left.
#if defined(EDSX_EXPERIMENTS) && defined(EDSX_FW_STACK)
constexpr u32 FW_STACK = EDSX_FW_STACK;                   // (test builds: see build.py)
#else
constexpr u32 FW_STACK = 4096;
#endif
constexpr u32 FW_LONG = 32, FW_LONG_MIN = 256;

// Depth of an entry's merge tree <= number of rounds that were run (an entry made in round k has children from earlier
// rounds).  Every round merges at least half of each run of mergeable pairs (greedy non-overlapping pairs,
// eds_transforms.cpp:63-66), so trees are normally ~log2(run length) deep; only products that collapse and reopen a run
// round after round make deeper ones.  A merge of up to FIN_STACK - 2 rounds walks with the stack in registers /
// scratch below; after more rounds (the reference allows 10 000, eds_transforms.cpp:335) the host hands every string a
// stack of rounds + 2 entries in HBM (FinParams::spill), so no depth is refused.
#if defined(EDSX_EXPERIMENTS) && defined(EDSX_FIN_STACK)
constexpr int FIN_STACK = EDSX_FIN_STACK;                 // (test builds: a tiny stack sends ordinary inputs through the spill path)
#else
constexpr int FIN_STACK = 96;
#endif

// the serial walk: one thread, one string (fallback of k_fin_write)
__device__ void fin_eds_direct(const FinParams& p, u64 t)
{
    const uint8_t fl = p.fin_flag[t];
    uint8_t* o = p.out + p.bytes[t];
    {   // opening bracket of the symbol's first string, else the separator (kept branch-free:
        // hipcc 7.2 lost the pointer increment when this was written as nested ifs)
        const bool first = (fl & 1) != 0, wr = !first || (fl & 4) != 0;
        if (wr) *o = first ? '{' : ',';
        o += wr ? 1 : 0;
    }
    u32 local[FIN_STACK];
    u32* stack = p.spill ? p.spill + t * (u64)p.spill_depth : local;
    const int cap = p.spill ? (int)p.spill_depth : FIN_STACK;
    int sp = 0;
    stack[sp++] = p.fin_ent[t];
    while (sp) {
        const u32 e = stack[--sp];
        if (p.pool.left[e] == LEAF) {
            const u64 s0 = p.str_off[p.pool.right[e]], s1 = p.str_off[p.pool.right[e] + 1];
            for (u64 c = s0; c < s1; c++) *o++ = p.chars[c];
        } else {
            if (sp + 2 > cap) { *p.err = 1; break; }
            stack[sp++] = p.pool.right[e];
            stack[sp++] = p.pool.left[e];
        }
    }
    if ((fl & 2) && (fl & 4)) *o++ = '}';
}

// n bytes, any alignment, 16 at a time
__device__ __forceinline__ void fin_copy(uint8_t* dst, const uint8_t* src, u64 n)
{
    u64 i = 0;
    for (; i + 16 <= n; i += 16) {
        const uint4 v = load16u(src + i);
        U128u w{v.x, v.y, v.z, v.w};
        __builtin_memcpy(dst + i, &w, 16);
    }
    for (; i < n; i++) dst[i] = src[i];
}

__global__ void __launch_bounds__(256) k_fin_write(FinParams p, u64 nstr, u64 E, u32 ns)
{
    __shared__ u32 s_ent[FW_STACK];
    __shared__ u32 s_dst[FW_STACK];                    // offset from the batch's first byte
    __shared__ u64 l_src[FW_LONG];
    __shared__ u32 l_dst[FW_LONG], l_len[FW_LONG];
    __shared__ u32 top, nlong, ovf;
    const u32 tid = threadIdx.x;
    const u64 nbatch = (nstr + ns - 1) / ns;
    for (u64 bt = blockIdx.x; bt < nbatch; bt += gridDim.x) {
        const u64 t0 = bt * ns, t = t0 + tid;
        const bool owner = tid < ns && t < nstr;
        const u64 g0 = p.bytes[t0], g1 = t0 + ns < nstr ? p.bytes[t0 + ns] : E;
        uint8_t* gout = p.out + g0;
        __syncthreads();                                   // (the previous batch is done with the stack)
        if (tid == 0) { top = 0; nlong = 0; ovf = g1 - g0 > 0xffffffffull ? 1u : 0u; }
        __syncthreads();
        if (owner && !ovf) {
            const uint8_t fl = p.fin_flag[t];
            u32 o = (u32)(p.bytes[t] - g0);
            const bool first = (fl & 1) != 0, wr = !first || (fl & 4) != 0;
            if (wr) gout[o] = first ? '{' : ',';
            o += wr ? 1u : 0u;
            const u32 e = p.fin_ent[t], len = p.pool.elen[e];
            if (len) { const u32 slot = atomicAdd(&top, 1u); s_ent[slot] = e; s_dst[slot] = o; }   // ns <= 256 < FW_STACK
            if ((fl & 2) && (fl & 4)) gout[o + len] = '}';
        }
        __syncthreads();
        while (!ovf) {
            const u32 n = top;
            if (n == 0) break;
            const u32 take = n < 256u ? n : 256u, base = n - take;
            u32 e = 0, d = 0;
            if (tid < take) { e = s_ent[base + tid]; d = s_dst[base + tid]; }
            __syncthreads();                               // every thread has its item and has seen `top`
            if (tid == 0) top = base;
            __syncthreads();
            if (tid < take) {
                const u32 l = p.pool.left[e], r = p.pool.right[e];
                if (l == LEAF) {
                    const u64 s0 = p.str_off[r], s1 = p.str_off[r + 1];
                    if (s1 - s0 >= FW_LONG_MIN) {
                        const u32 slot = atomicAdd(&nlong, 1u);
                        if (slot < FW_LONG) { l_src[slot] = s0; l_dst[slot] = d; l_len[slot] = (u32)(s1 - s0); }
                        else fin_copy(gout + d, p.chars + s0, s1 - s0);
                    } else fin_copy(gout + d, p.chars + s0, s1 - s0);
                } else {
                    const u32 el = p.pool.elen[l], er = p.pool.elen[r];
                    const u32 cnt = (el ? 1u : 0u) + (er ? 1u : 0u);
                    if (cnt) {
                        u32 slot = atomicAdd(&top, cnt);
                        if (slot + cnt > FW_STACK) ovf = 1u;
                        else {
                            if (er) { s_ent[slot] = r; s_dst[slot] = d + el; slot++; }      // left on top: popped first
                            if (el) { s_ent[slot] = l; s_dst[slot] = d; }
                        }
                    }
                }
            }
            __syncthreads();
            const u32 nl = nlong < FW_LONG ? nlong : FW_LONG;
            if (nl) {                                       // the long leaves of this round: the whole workgroup copies
                for (u32 i = 0; i < nl; i++) {
                    const uint8_t* src = p.chars + l_src[i];
                    uint8_t* dst = gout + l_dst[i];
                    const u32 len = l_len[i], full = len & ~15u;
                    for (u32 c = tid * 16u; c < full; c += 4096u) {
                        const uint4 v = load16u(src + c);
                        U128u w{v.x, v.y, v.z, v.w};
                        __builtin_memcpy(dst + c, &w, 16);
                    }
                    if (tid < len - full) dst[full + tid] = src[full + tid];
                }
                __syncthreads();
                if (tid == 0) nlong = 0;
                __syncthreads();
            }
        }
        if (ovf && owner) fin_eds_direct(p, t);            // (rewrites what the stack had placed already: same bytes)
    }
}

// "{id,id,...}" of every string's source set (eds.cpp:641-659), a thread per string
__global__ void k_fin_write_sources(FinParams p, u64 nstr)
{
    for (u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x; t < nstr; t += (u64)gridDim.x * blockDim.x) {
        uint8_t* so = p.sout + p.sbytes[t];
        *so++ = '{';
        const u64* b = p.pool.bits + (u64)p.fin_ent[t] * p.pool.W;
        for (u32 w = 0; w < p.pool.W; w++) {
            u64 v = b[w];
            while (v) {
                u32 id = w * 64 + __builtin_ctzll(v);
                v &= v - 1;
                u32 nd = ndigits(id ? id : 1);
                u32 x = id;
                for (int d = (int)nd - 1; d >= 0; d--) { so[d] = (uint8_t)('0' + x % 10); x /= 10; }
                so += nd;
                *so++ = ',';
            }
        }
        so[-1] = '}';
    }
}

// the leaves of the entry pool: the original strings (their lengths are the DeviceEds's elen)
__global__ void k_leaf_links(u64 m, u32* __restrict__ left, u32* __restrict__ right)
{
    for (u64 s = blockIdx.x * (u64)blockDim.x + threadIdx.x; s < m; s += (u64)gridDim.x * blockDim.x) {
        left[s] = LEAF; right[s] = (u32)s;
    }
}

// ---- host ---------------------------------------------------------------------------------------
static void grow_keep(DevBuf& b, size_t used, size_t need, hipStream_t st)
{
    if (need <= b.cap) return;
    DevBuf nb;
    nb.ensure(std::max(need, b.cap * 2));
    if (used) EDSX_HIP(hipMemcpyAsync(nb.ptr, b.ptr, used, hipMemcpyDeviceToDevice, st));
    EDSX_HIP(hipStreamSynchronize(st));
    std::swap(b.ptr, nb.ptr);
    std::swap(b.cap, nb.cap);
}

void MergePipeline::run(DeviceEds& de, const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, uint32_t l,
                        bool compact, HostBytes& out, HostBytes& seds_out, hipStream_t st, MergeShard* shard)
{
    if (l == 0) throw ParamError("context_length must be > 0 for l-EDS transformation");   // :322-324
    const bool linear = seds != nullptr;

    de.load(eds, eds_n, seds, seds_n, linear, st, true);
    StageTrace trace;
    const u64 n0 = de.n(), m = de.m(), head_len = de.head_len();
    const u32 W = de.W();
    if (n0 == 0) {                                           // empty EDS: save() prints "\n" (quirk 19)
        out.take(1);
        out.data[0] = '\n';
        seds_out.take(0);
        return;
    }
    if (shard) {
        shard->head_intact = shard->tail_intact = true;
        if ((shard->head_sentinel && !de.head_single()) || (shard->tail_sentinel && !de.tail_single()) ||
            ((shard->head_sentinel && shard->tail_sentinel) && n0 < 3))
            throw ParamError("a sentinel of a symbol range must be a single-string symbol of its own");
    }
    // the pool: the text's elen / bits (with the headroom asked for above) + the leaf links; the second symbol buffers
    const DeviceEds::Pool dp = de.consume();
    DevBuf &elen_ = dp.elen, &bits_ = dp.bits;
    const size_t pool_cap = std::max<size_t>(2 * m + 1024, 4096);
    left_.ensure(4 * pool_cap); right_.ensure(4 * pool_cap);
    hipLaunchKernelGGL(k_leaf_links, dim3(2048), dim3(256), 0, st, m, left_.as<u32>(), right_.as<u32>());
    for (DevBuf* b : {&size2_, &ent_off2_, &len12_}) b->ensure(8 * (n0 + 1));
    const SymArrays sym[2] = {dp.sym, SymArrays{size2_.as<u64>(), ent_off2_.as<u64>(), len12_.as<u64>()}};
    ctl_.ensure(8 * 16);
    a_.ensure(8 * (n0 + 2)); b_.ensure(8 * (n0 + 2)); c_.ensure(8 * (n0 + 2)); d_.ensure(8 * (n0 + 2)); e_.ensure(8 * (n0 + 2));
    scan_tmp_.ensure(8 * ((n0 + 2) / SCAN_TILE + 2));
    u64* ctl = ctl_.as<u64>();         // [0]=n  [1]=any  [2]=n_new  [3]=total_new  [4]=err_pos  [5]=err_big  [6]=scratch

    u64 n = n0, pool_used = m;
    int cur = 0;
    size_t iteration = 0;
    const size_t MAX_ITERATIONS = 10000;                     // eds_transforms.cpp:335
    while (iteration < MAX_ITERATIONS) {
        if (n < 2) break;
        u64 hctl[8] = {n, 0, 0, 0, NO_ERR, NO_ERR, 0, 0};
        EDSX_HIP(hipMemcpyAsync(ctl, hctl, sizeof(hctl), hipMemcpyHostToDevice, st));
        const SymArrays sc = sym[cur], sn = sym[cur ^ 1];
        Pool pool{left_.as<u32>(), right_.as<u32>(), elen_.as<u32>(), bits_.as<u64>(), W};
        u64 *runmark = a_.as<u64>(), *sel = b_.as<u64>(), *keep = c_.as<u64>(), *newidx = d_.as<u64>(), *newcnt = e_.as<u64>();
        hipLaunchKernelGGL(k_should, dim3(1024), dim3(256), 0, st, sc, n, (u64)l, runmark, ctl + 1);
        inclusive_max_scan_u64(runmark, runmark, ctl + 0, ctl + 6, scan_tmp_.as<u64>(), st);
        hipLaunchKernelGGL(k_select, dim3(1024), dim3(256), 0, st, runmark, n, sel, keep);
        hipLaunchKernelGGL(k_keep, dim3(1024), dim3(256), 0, st, sel, n, keep);
        exclusive_scan_u64(keep, newidx, ctl + 0, ctl + 2, scan_tmp_.as<u64>(), st);
        RoundParams rp{sc, sn, pool, n, sel, keep, newidx, newcnt, newcnt, pool_used, ctl + 4, ctl + 5, linear ? 1 : 0};
        hipLaunchKernelGGL(k_pair_count, dim3(1024), dim3(256), 0, st, rp);
        exclusive_scan_u64(newcnt, newcnt, ctl + 2, ctl + 3, scan_tmp_.as<u64>(), st);
        EDSX_HIP(hipMemcpyAsync(hctl, ctl, sizeof(hctl), hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        if (!hctl[1]) break;                                 // is_leds: nothing left to merge
        if (hctl[4] != NO_ERR)
            throw FormatError("Merging positions " + std::to_string(hctl[4]) + " and " + std::to_string(hctl[4] + 1) +
                              " results in empty set (no valid source intersections)");
        if (hctl[5] != NO_ERR || pool_used + hctl[3] >= 0xfffffff0ull)
            throw FormatError("l-EDS merge produces more than 2^32 strings; refusing (the reference would exhaust memory)");
        const u64 n_new = hctl[2], total_new = hctl[3];
        const size_t need = pool_used + total_new + 16;
        grow_keep(left_, 4 * pool_used, 4 * need, st);
        grow_keep(right_, 4 * pool_used, 4 * need, st);
        grow_keep(elen_, 4 * pool_used, 4 * need, st);
        if (linear) grow_keep(bits_, 8 * pool_used * W, 8 * need * W, st);
        rp.pool = Pool{left_.as<u32>(), right_.as<u32>(), elen_.as<u32>(), bits_.as<u64>(), W};
        hipLaunchKernelGGL(k_pair_fill, dim3(1024), dim3(256), 0, st, rp);
        pool_used += total_new;
        n = n_new;
        cur ^= 1;
        iteration++;
    }
    if (iteration >= MAX_ITERATIONS) throw FormatError("Maximum iterations reached without convergence");
    rounds_run_ = iteration;
    trace.mark("merge rounds");

    // ---- symbol range of a partitioned merge: did the sentinels stay out of every merge?  Merged symbols get
    // fresh pool entries (>= m), an untouched sentinel still points at its leaf.
    if (shard && (shard->head_sentinel || shard->tail_sentinel)) {
        u64 h[4] = {0, 0, 0, 0};
        EDSX_HIP(hipMemcpyAsync(h + 0, sym[cur].size, 8, hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipMemcpyAsync(h + 1, sym[cur].ent_off, 8, hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipMemcpyAsync(h + 2, sym[cur].size + (n - 1), 8, hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipMemcpyAsync(h + 3, sym[cur].ent_off + (n - 1), 8, hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        if (shard->head_sentinel) shard->head_intact = h[0] == 1 && h[1] == 0 && n >= 2;
        if (shard->tail_sentinel) shard->tail_intact = h[2] == 1 && h[3] == m - 1 && n >= 2;
    }

    // ---- final text
    const SymArrays sf = sym[cur];
    Pool pool{left_.as<u32>(), right_.as<u32>(), elen_.as<u32>(), bits_.as<u64>(), W};
    u64 hctl[8] = {n, 0, 0, 0, 0, 0, 0, 0};
    EDSX_HIP(hipMemcpyAsync(ctl, hctl, sizeof(hctl), hipMemcpyHostToDevice, st));
    u64* cum = a_.as<u64>();
    exclusive_scan_u64(sf.size, cum, ctl + 0, ctl + 1, scan_tmp_.as<u64>(), st);
    EDSX_HIP(hipMemcpyAsync(hctl, ctl, sizeof(hctl), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    const u64 nstr = hctl[1];
    if (nstr >= 0xfffffff0ull) throw FormatError("l-EDS output has too many strings");
    fin_ent_.ensure(4 * (nstr + 1)); fin_flag_.ensure(nstr + 16); fbytes_.ensure(8 * (nstr + 2)); fsbytes_.ensure(8 * (nstr + 2));
    scan_tmp_.ensure(8 * ((nstr + 2) / SCAN_TILE + 2));
    FinParams fp{sf, pool, n, cum, fin_ent_.as<u32>(), fin_flag_.as<uint8_t>(), fbytes_.as<u64>(), fsbytes_.as<u64>(),
                 dp.chars, dp.str_off, nullptr, nullptr, ctl + 4, compact ? 1 : 0, linear ? 1 : 0};
    hipLaunchKernelGGL(k_fin_list, dim3(1024), dim3(256), 0, st, fp);
    hctl[0] = nstr; hctl[4] = 0;
    EDSX_HIP(hipMemcpyAsync(ctl, hctl, sizeof(hctl), hipMemcpyHostToDevice, st));
    exclusive_scan_u64(fbytes_.as<u64>(), fbytes_.as<u64>(), ctl + 0, ctl + 2, scan_tmp_.as<u64>(), st);
    if (linear) exclusive_scan_u64(fsbytes_.as<u64>(), fsbytes_.as<u64>(), ctl + 0, ctl + 3, scan_tmp_.as<u64>(), st);
    EDSX_HIP(hipMemcpyAsync(hctl, ctl, sizeof(hctl), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    const u64 E = hctl[2], Q = linear ? hctl[3] : 0;
    d_out_.ensure(E + 16);
    if (linear) d_sout_.ensure(Q + 16);
    fp.out = d_out_.as<uint8_t>(); fp.sout = d_sout_.as<uint8_t>();
    if (rounds_run_ + 2 > (u64)FIN_STACK && nstr) {          // trees may be deeper than the serial walk's own stack
        fin_spill_.ensure(4 * nstr * (rounds_run_ + 2));
        fp.spill = fin_spill_.as<u32>(); fp.spill_depth = (u32)(rounds_run_ + 2);
    }
    {
        // strings per workgroup: about 16 KB of text (a power of two, at most one string per thread)
        const u64 mean = nstr ? std::max<u64>(1, E / nstr) : 1;
        u32 ns = 256;
        while (ns > 1 && (u64)ns * mean > 16384) ns >>= 1;
        if (nstr) hipLaunchKernelGGL(k_fin_write, dim3((unsigned)std::min<u64>((nstr + ns - 1) / ns, 1u << 20)), dim3(256), 0, st, fp, nstr, E, ns);
        if (linear && nstr) hipLaunchKernelGGL(k_fin_write_sources, dim3(2048), dim3(256), 0, st, fp, nstr);
    }
    trace.mark("final sizes");
    // malloc'ed, not value-initialised (see HostBytes): the pages are first touched by the copy
    out.take(E + 1);
    PinnedDownload::copy(out.data, d_out_.ptr, E, st);
    if (linear) {
        seds_out.take(Q + 1);
        PinnedDownload::copy(seds_out.data, d_sout_.ptr, Q, st);
    } else seds_out.take(0);
    EDSX_HIP(hipMemcpyAsync(hctl, ctl, sizeof(hctl), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    if (hctl[4]) throw FormatError("l-EDS merge nesting deeper than this build supports");
    trace.mark("text kernel + download");
    out.data[E] = '\n';                                      // eds.cpp:630
    if (linear) seds_out.data[Q] = '\n';                     // eds.cpp:658
    if (shard && shard->tail_sentinel) {                     // not the last range: the text goes on
        out.size--;
        if (linear) seds_out.size--;
    }
    if (shard && shard->head_sentinel && shard->head_intact) {   // the left neighbour prints the shared sentinel
        out.drop_front((size_t)head_len + (compact ? 0 : 2));
        if (linear) {
            const void* b = memchr(seds_out.data, '}', seds_out.size);
            seds_out.drop_front(b ? static_cast<size_t>(static_cast<const uint8_t*>(b) - seds_out.data) + 1 : 0);
        }
    }
}

} // namespace edsx
