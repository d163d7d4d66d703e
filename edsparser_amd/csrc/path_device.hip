// path_device.hip — spell the sequence of every path of an EDS with sources on gfx950 (eds2fasta).
//
// The chosen string of path p at symbol i is the first string of the symbol, in file order, whose source set holds p
// or 0; the sequence of p is the concatenation over the symbols, and a symbol without such a string adds one to
// missing[p].  The kernels read a DeviceEds of the session's own through its view (eds_device.hpp: per symbol size,
// first string, single-string length; per string str_off into the character pool, its path bitset of W words, bit 0 =
// universal).
//
//   open      k_path_flags   a symbol is FIXED when its one string is universal: every path takes it, so one shared
//                            exclusive scan (cum_fixed) gives its share of every path's offsets; all other symbols
//                            are CHOICE symbols, numbered by a second scan (rank) and listed by k_path_cidx
//             k_path_or      OR of all sets: P is its highest bit
//   per batch of K paths (K from free HBM: the tables are K x n_choice, never P x n)
//             k_path_choose  one lane per (path, choice symbol): the chosen string and its length, missing counts
//             one exclusive scan over the K rows laid end to end (row k's offsets are differences to its first entry)
//             k_path_copy    one workgroup per (16 KiB of a path's FASTA body, path), paths fastest, so the K
//                            workgroups that need the same stretch of the character pool run next to each other and
//                            the pool comes from HBM about once per batch.  A workgroup finds its first symbol by a
//                            256-way search, keeps the offsets and pool bases of its (up to 3072) symbols in LDS, and
//                            every lane writes 16 bytes of OUTPUT at a time: the line feeds of the FASTA wrapping are
//                            put in on the way (output byte o of a body holds sequence character
//                            o - o / (line_width + 1)), one 16-byte load where the 16 bytes come out of one string,
//                            and always one 16-byte store.
//
// GFA walks (edsx_paths_gfa_walks): the P line of a path lists the segment ids of its non-empty chosen
// strings.  Its token text ("<id>+," per step) is laid out like the sequence above with token bytes in place of
// characters (gfa_text.hpp), so the same tables carry it:
//   first call k_path_tokfixed seg_rank (segment_ranks, shared with gfa_device.hip) and the token bytes of the fixed
//                              symbols, scanned once (cum_tok) and kept with the session
//   per batch  k_path_tok      after k_path_choose: token bytes per (path, choice symbol), scanned like the lengths; the
//                              steps of a row are counted with one atomic per wave
//              k_path_walk     the shape of k_path_copy: a workgroup per (16 KiB of a line, path), the symbol range by the
//                              256-way search, 16 bytes per lane assembled in registers and stored at once; the last
//                              comma of a line is a tab and "*\n" follows.  No LDS cache of the stretch's offsets
//
// Alignment rows (edsx_paths_align): symbol i owns w[i] columns, the length of its longest string; a row holds
// the chosen strings left-justified in their columns and the gap byte elsewhere, so every row has W = sum w[i] characters:
//   first call k_align_width   w, scanned once (col) and kept with the session
//   per batch  k_path_choose   as above (the chosen strings and the missing counts; the scanned lengths are not used)
//              k_path_align    the shape of k_path_copy over columns instead of characters: col does not depend on the
//                              path, so the symbol range of a step needs no table row; 2000 symbols per step in LDS,
//                              those behind them from global memory; gap runs are stores without a load
//
// spell, align and walks write records - a header text and a body - through one driver, emit_records: the arithmetic of
// the records and of their batches is path_records.hpp; each of the three brings its tables and its body kernel.  The
// coordinate lift, the region slice, the path distances, the linkage disequilibrium, the shared segments and the mosaics
// of the session: lift_device.hip, slice_device.hip, dist_device.hip, ld_device.hip, ibs_device.hip, mosaic_device.hip.
#include "path_device.hpp"
#include "gfa_device.hpp"

#include <chrono>
#include <cstdlib>
#include <cstring>

namespace edsx {

namespace {

constexpr u64 NONE = ~0ull;
constexpr int CP_THREADS = 256;
constexpr u32 CP_TILE = 16384;       // output bytes per workgroup step: 4 chunks of 16 bytes per lane
constexpr u32 CP_SYMS = 3072;        // symbols whose offsets and pool bases are kept in LDS per step (36 KiB)

__global__ void k_path_flags(const u64* __restrict__ size, const u64* __restrict__ ent_off, const u64* __restrict__ len1,
                             const u64* __restrict__ bits, u32 W, u64 n, u64* __restrict__ fx, u64* __restrict__ ch)
{
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const bool fixed = size[i] == 1 && (bits[ent_off[i] * W] & 1);
        fx[i] = fixed ? len1[i] : 0;
        ch[i] = fixed ? 0 : 1;
    }
}

__global__ void k_path_cidx(const u64* __restrict__ rank, u64 n, u64* __restrict__ cidx)
{
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 r = rank[i];
        if (rank[i + 1] != r) cidx[r] = i;
    }
}

__global__ void __launch_bounds__(256) k_path_or(const u64* __restrict__ bits, u32 W, u64 m, u64* __restrict__ orbits)
{
    const u64 t0 = blockIdx.x * (u64)blockDim.x + threadIdx.x, step = (u64)gridDim.x * blockDim.x;
    for (u32 w = 0; w < W; w++) {
        u64 o = 0;
        for (u64 k = t0; k < m; k += step) o |= bits[k * W + w];
        for (int sh = 32; sh > 0; sh >>= 1) o |= __shfl_xor(o, sh, 64);
        if ((threadIdx.x & 63) == 0 && o) atomicOr((unsigned long long*)&orbits[w], (unsigned long long)o);
    }
}

// csid / clen: K rows of nc entries; lanes run along a row, so the table writes and the reads of neighbouring symbols'
// sets are contiguous
__global__ void __launch_bounds__(256) k_path_choose(const u64* __restrict__ size, const u64* __restrict__ ent_off,
                                                     const u64* __restrict__ str_off, const u64* __restrict__ bits, u32 W,
                                                     const u64* __restrict__ cidx, u64 nc, const u64* __restrict__ ids, u64 K,
                                                     u64* __restrict__ csid, u64* __restrict__ clen, u64* __restrict__ missing)
{
    const u64 total = K * nc;
    for (u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x; t < total; t += (u64)gridDim.x * blockDim.x) {
        const u64 k = t / nc, i = cidx[t - k * nc], p = ids[k];
        const u64 e0 = ent_off[i], sz = size[i], w = p >> 6, bit = 1ull << (p & 63);
        u64 sid = NONE;
        for (u64 q = 0; q < sz; q++) {
            const u64* b = bits + (e0 + q) * W;
            if ((b[0] & 1) || (b[w] & bit)) { sid = e0 + q; break; }
        }
        csid[t] = sid;
        clen[t] = sid == NONE ? 0 : str_off[sid + 1] - str_off[sid];
        if (sid == NONE) atomicAdd((unsigned long long*)&missing[k], 1ull);
    }
}

// S: the scanned rows (K * nc + 1 entries)
__global__ void k_path_totals(const u64* __restrict__ S, u64 nc, u64 F, u64 K, u64* __restrict__ tot)
{
    const u64 k = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (k < K) tot[k] = F + (nc ? S[(k + 1) * nc] - S[k * nc] : 0);
}

__global__ void k_path_headers(const uint8_t* __restrict__ blob, const PathRec* __restrict__ rec, uint8_t* __restrict__ out)
{
    const PathRec r = rec[blockIdx.x];
    const u64 len = r.body_off - r.rec_off;
    for (u64 j = threadIdx.x; j < len; j += blockDim.x) out[r.rec_off + j] = blob[r.hdr_src + j];
}

struct CopyArgs {
    const u64* ent_off; const u64* str_off; const uint8_t* chars;
    const u64* cf; const u64* rank;            // n + 1 entries each
    const u64* csid; const u64* S; u64 n, nc;  // choice tables (null when nc == 0)
    const PathRec* rec; u64 nrec, max_tiles;
    uint8_t* out;
};

// sequence offset of symbol i (0 <= i <= n) on the path of table row kb / nc
__device__ __forceinline__ u64 sym_pos(const CopyArgs& a, u64 kb, u64 i)
{
    return a.cf[i] + (a.nc ? a.S[kb + a.rank[i]] - a.S[kb] : 0);
}

__device__ __forceinline__ void sym_load(const CopyArgs& a, u64 kb, u64 i, u64& pos, u64& s0, u64& len)
{
    const u64 r = a.rank[i];
    const bool choice = a.rank[i + 1] != r;
    pos = a.cf[i] + (a.nc ? a.S[kb + r] - a.S[kb] : 0);
    const u64 sid = choice ? a.csid[kb + r] : a.ent_off[i];
    if (sid == NONE) { s0 = 0; len = 0; return; }
    s0 = a.str_off[sid];
    len = a.str_off[sid + 1] - s0;
}

// largest i in [0, n) with sym_pos(i) <= q (sym_pos(0) = 0): the whole workgroup probes 256 points per round
__device__ u64 block_find(const CopyArgs& a, u64 kb, u64 q)
{
    u64 lo = 0, hi = a.n;
    while (hi - lo > 1) {
        const u64 step = (hi - lo + CP_THREADS - 1) / CP_THREADS;
        const u64 i = lo + threadIdx.x * step;
        const int ok = i < hi && sym_pos(a, kb, i) <= q;
        const int cnt = __syncthreads_count(ok);                 // the offsets ascend: the lanes that hold are a prefix
        lo += (u64)(cnt - 1) * step;
        hi = min(hi, lo + step);
    }
    return lo;
}

typedef unsigned __int128 u128;

__global__ void __launch_bounds__(CP_THREADS) k_path_copy(CopyArgs a)
{
    // per step: for the symbols iA .. iA + cnt, where each begins on the path (relative to q0, saturated) and where
    // its chosen string lies in the pool (pool offset minus path offset: character q of the path is chars[sbase + q])
    __shared__ u32 spos[CP_SYMS + 1];
    __shared__ u64 sbase[CP_SYMS];
    const u64 work = a.max_tiles * a.nrec;
    for (u64 wi = blockIdx.x; wi < work; wi += gridDim.x) {
        const PathRec rc = a.rec[wi % a.nrec];
        const u64 o0 = (wi / a.nrec) * CP_TILE;
        if (o0 >= rc.body) continue;
        const u64 o1 = min(rc.body, o0 + (u64)CP_TILE), per = rc.lw + 1, kb = rc.row * a.nc, last = rc.body - 1;
        const u64 q0 = o0 - o0 / per, q1 = min(rc.L, o1 - o1 / per);      // this step spells characters [q0, q1)
        u64 iA = 0, iB = 0;
        u32 cnt = 0;
        __syncthreads();                                                  // the last step's readers of the tables are through
        if (q0 < q1) {
            iA = block_find(a, kb, q0);
            iB = block_find(a, kb, q1 - 1);
            cnt = (u32)min((u64)CP_SYMS, iB - iA + 1);                    // (symbols behind the cached ones: from HBM)
            for (u32 j = threadIdx.x; j <= cnt; j += CP_THREADS) {
                u64 p, s0, len;
                if (j < cnt) { sym_load(a, kb, iA + j, p, s0, len); sbase[j] = s0 - p; }
                else p = sym_pos(a, kb, iA + j);
                spos[j] = p <= q0 ? 0u : (u32)min(p - q0, 0xffffffffull);
            }
            __syncthreads();
        }
        auto find = [&](u64 q) -> u64 {                                    // symbol of character q, q0 <= q < q1
            const u64 rel = q - q0;
            if (rel < (u64)spos[cnt]) {
                u32 lo = 0, hi = cnt;
                while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if ((u64)spos[mid] <= rel) lo = mid; else hi = mid; }
                return iA + lo;
            }
            u64 lo = iA + cnt, hi = iB + 1;
            while (hi - lo > 1) { const u64 mid = lo + ((hi - lo) >> 1); if (sym_pos(a, kb, mid) <= q) lo = mid; else hi = mid; }
            return lo;
        };
        auto sym = [&](u64 i, u64& end, u64& base) {                       // where symbol i's string ends on the path; its base
            const u64 j = i - iA;
            if (j < cnt) { end = q0 + spos[j + 1]; base = sbase[j]; return; }
            u64 p, s0, len;
            sym_load(a, kb, i, p, s0, len);
            end = p + len; base = s0 - p;
        };
        for (u64 o = o0 + (u64)threadIdx.x * 16; o < o1; o += (u64)CP_THREADS * 16) {
            const u32 nb = (u32)min((u64)16, o1 - o);
            uint8_t* dst = a.out + rc.body_off + o;
            u64 q = o - o / per;                                           // first character at or behind output byte o
            const u64 nl1 = min((o / per + 1) * per - 1, last);            // first line feed at or behind o
            u32 nn = 0;
            if (nl1 < o + nb) {
                nn = 1;
                if (nl1 < last && min(nl1 + per, last) < o + nb) nn = 2;
            }
            if (nn == 1 && nb == 1) { dst[0] = '\n'; continue; }
            u64 i = find(q), end, base;
            sym(i, end, base);
            if (nn <= 1 && q + (nb - nn) <= end) {                         // the chunk comes out of one string
                const uint4 v = load16u(a.chars + (base + q));               // (the pool ends in 16 bytes of slack)
                u128 x = ((u128)(((u64)v.w << 32) | v.z) << 64) | (((u64)v.y << 32) | v.x);
                if (nn) {
                    const u32 sh = 8u * (u32)(nl1 - o);
                    const u128 mask = ((u128)1 << sh) - 1;
                    x = (x & mask) | ((u128)'\n' << sh) | ((x & ~mask) << 8);
                }
                if (nb == 16) {
                    const u64 lo = (u64)x, hi = (u64)(x >> 64);
                    store16u(dst, make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32)));
                } else {
                    for (u32 b = 0; b < nb; b++) dst[b] = (uint8_t)(x >> (8u * b));
                }
                continue;
            }
            u64 nl = nl1;                                                  // byte by byte across strings and short lines
            u128 x = 0;
            for (u32 b = 0; b < nb; b++) {
                u32 c = '\n';
                if (o + b == nl) nl = nl == last ? NONE : min(nl + per, last);
                else {
                    while (q >= end && i + 1 < a.n) { i++; sym(i, end, base); }
                    c = q < end ? a.chars[(u64)(base + q)] : (u32)'?';
                    q++;
                }
                x |= (u128)c << (8u * b);
            }
            if (nb == 16) {
                const u64 lo = (u64)x, hi = (u64)(x >> 64);
                store16u(dst, make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32)));
            } else {
                for (u32 b = 0; b < nb; b++) dst[b] = (uint8_t)(x >> (8u * b));
            }
        }
    }
}

// ---- alignment rows (eds2msa): every symbol owns as many columns as its longest string has characters --------
// w[i] into col[i] (scanned in place afterwards; col[n] = 0 becomes W); stat[0]: symbols of width 0, stat[1]: the widest
__global__ void __launch_bounds__(256) k_align_width(const u64* __restrict__ size, const u64* __restrict__ ent_off,
                                                     const u64* __restrict__ str_off, u64 n, u64* __restrict__ col,
                                                     u64* __restrict__ stat)
{
    u64 zero = 0, widest = 0;
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i <= n; i += (u64)gridDim.x * blockDim.x) {
        u64 w = 0;
        if (i < n) {
            const u64 e0 = ent_off[i], e1 = e0 + size[i];
            for (u64 j = e0; j < e1; j++) w = max(w, str_off[j + 1] - str_off[j]);
            if (w == 0) zero++;
            widest = max(widest, w);
        }
        col[i] = w;
    }
    for (int sh = 32; sh > 0; sh >>= 1) {
        zero += __shfl_xor(zero, sh, 64);
        widest = max(widest, (u64)__shfl_xor(widest, sh, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (zero) atomicAdd((unsigned long long*)&stat[0], (unsigned long long)zero);
        if (widest) atomicMax((unsigned long long*)&stat[1], (unsigned long long)widest);
    }
}

constexpr u32 AL_SYMS = 2000;        // symbols whose columns, string ends and pool bases are kept in LDS per step: 16 B each,
                                     // 2000 so that five workgroups fit the 160 KiB of a CU (2048 leaves room for four)

struct AlignArgs {
    const u64* ent_off; const u64* str_off; const uint8_t* chars;
    const u64* col; const u64* rank;           // n + 1 entries each
    const u64* csid; u64 n, nc;                // the chosen strings (null when nc == 0)
    const PathRec* rec; u64 nrec, max_tiles;
    uint8_t* out; u32 gap;
};

// symbol i on the path of table row kb / nc: its first column, where its chosen string ends (no string: at once), and the
// pool offset of the string minus the first column (column c of the string is chars[base + c])
__device__ __forceinline__ void align_load(const AlignArgs& a, u64 kb, u64 i, u64& c0, u64& send, u64& base)
{
    const u64 r = a.rank[i];
    c0 = a.col[i];
    const u64 sid = a.rank[i + 1] != r ? a.csid[kb + r] : a.ent_off[i];
    if (sid == NONE) { send = c0; base = 0; return; }
    const u64 s0 = a.str_off[sid];
    send = c0 + (a.str_off[sid + 1] - s0);
    base = s0 - c0;
}

// largest i in [0, n) with col[i] <= q (col[0] = 0), as block_find.  For q < W that symbol has a column: symbols of
// width 0 share their col with the next one, which is then the larger i
__device__ u64 align_block_find(const u64* __restrict__ col, u64 n, u64 q)
{
    u64 lo = 0, hi = n;
    while (hi - lo > 1) {
        const u64 step = (hi - lo + CP_THREADS - 1) / CP_THREADS;
        const u64 i = lo + threadIdx.x * step;
        const int ok = i < hi && col[i] <= q;
        const int cnt = __syncthreads_count(ok);
        lo += (u64)(cnt - 1) * step;
        hi = min(hi, lo + step);
    }
    return lo;
}

__device__ __forceinline__ void put16(uint8_t* dst, u128 x, u32 nb)
{
    if (nb == 16) {
        const u64 lo = (u64)x, hi = (u64)(x >> 64);
        store16u(dst, make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32)));
    } else {
        for (u32 b = 0; b < nb; b++) dst[b] = (uint8_t)(x >> (8u * b));
    }
}

// One workgroup per (16 KiB of a row's FASTA body, path), paths fastest as in k_path_copy.  The columns do not depend on
// the path: the symbol range of a step comes from col alone, and the step keeps, for its first AL_SYMS symbols, the first
// column (relative to the step's first, saturated), the end of the chosen string (the same) and the pool base in LDS;
// symbols behind those are looked up in global memory.  A lane assembles 16 output bytes: where they lie inside one
// symbol, one 16-byte load out of the string (the pool ends in 16 bytes of slack) with the bytes behind the string's
// end replaced by the gap byte, or no load at all when they lie behind it; otherwise byte by byte.
__global__ void __launch_bounds__(CP_THREADS) k_path_align(AlignArgs a)
{
    __shared__ u32 scol[AL_SYMS + 1];
    __shared__ u32 send[AL_SYMS];
    __shared__ u64 sbase[AL_SYMS];
    const u64 work = a.max_tiles * a.nrec;
    const u128 gaps = (u128)(0x0101010101010101ull * a.gap) << 64 | (u128)(0x0101010101010101ull * a.gap);
    for (u64 wi = blockIdx.x; wi < work; wi += gridDim.x) {
        const PathRec rc = a.rec[wi % a.nrec];
        const u64 o0 = (wi / a.nrec) * CP_TILE;
        if (o0 >= rc.body) continue;
        const u64 o1 = min(rc.body, o0 + (u64)CP_TILE), per = rc.lw + 1, kb = rc.row * a.nc, last = rc.body - 1;
        const u64 q0 = o0 - o0 / per, q1 = min(rc.L, o1 - o1 / per);      // this step writes columns [q0, q1)
        u64 iA = 0, iB = 0;
        u32 cnt = 0;
        __syncthreads();                                                  // the last step's readers of the tables are through
        if (q0 < q1) {
            iA = align_block_find(a.col, a.n, q0);
            iB = align_block_find(a.col, a.n, q1 - 1);
            cnt = (u32)min((u64)AL_SYMS, iB - iA + 1);
            for (u32 j = threadIdx.x; j <= cnt; j += CP_THREADS) {
                u64 c0;
                if (j < cnt) {
                    u64 se, base;
                    align_load(a, kb, iA + j, c0, se, base);
                    send[j] = se <= q0 ? 0u : (u32)min(se - q0, 0xffffffffull);
                    sbase[j] = base;
                } else c0 = a.col[iA + j];
                scol[j] = c0 <= q0 ? 0u : (u32)min(c0 - q0, 0xffffffffull);
            }
            __syncthreads();
        }
        auto find = [&](u64 q) -> u64 {                                    // symbol of column q, q0 <= q < q1
            const u64 rel = q - q0;
            if (rel < (u64)scol[cnt]) {
                u32 lo = 0, hi = cnt;
                while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if ((u64)scol[mid] <= rel) lo = mid; else hi = mid; }
                return iA + lo;
            }
            u64 lo = iA + cnt, hi = iB + 1;
            while (hi - lo > 1) { const u64 mid = lo + ((hi - lo) >> 1); if (a.col[mid] <= q) lo = mid; else hi = mid; }
            return lo;
        };
        auto sym = [&](u64 i, u64& end, u64& se, u64& base) {              // symbol i: behind its last column, behind its string
            const u64 j = i - iA;
            if (j < cnt) { end = q0 + scol[j + 1]; se = q0 + send[j]; base = sbase[j]; return; }
            u64 c0;
            align_load(a, kb, i, c0, se, base);
            end = a.col[i + 1];
        };
        for (u64 o = o0 + (u64)threadIdx.x * 16; o < o1; o += (u64)CP_THREADS * 16) {
            const u32 nb = (u32)min((u64)16, o1 - o);
            uint8_t* dst = a.out + rc.body_off + o;
            u64 q = o - o / per;                                           // first column at or behind output byte o
            const u64 nl1 = min((o / per + 1) * per - 1, last);            // first line feed at or behind o
            u32 nn = 0;
            if (nl1 < o + nb) {
                nn = 1;
                if (nl1 < last && min(nl1 + per, last) < o + nb) nn = 2;
            }
            if (nn == 1 && nb == 1) { dst[0] = '\n'; continue; }
            u64 i = find(q), end, se, base;
            sym(i, end, se, base);
            if (nn <= 1 && q + (nb - nn) <= end) {                         // the chunk lies in one symbol
                u128 x = gaps;
                if (q < se) {
                    const uint4 v = load16u(a.chars + (base + q));
                    x = ((u128)(((u64)v.w << 32) | v.z) << 64) | (((u64)v.y << 32) | v.x);
                    if (se - q < 16) {                                     // the string ends inside: gaps behind it
                        const u128 keep = ((u128)1 << (8u * (u32)(se - q))) - 1;
                        x = (x & keep) | (gaps & ~keep);
                    }
                }
                if (nn) {
                    const u32 sh = 8u * (u32)(nl1 - o);
                    const u128 mask = ((u128)1 << sh) - 1;
                    x = (x & mask) | ((u128)'\n' << sh) | ((x & ~mask) << 8);
                }
                put16(dst, x, nb);
                continue;
            }
            u64 nl = nl1;                                                  // byte by byte across symbols and short lines
            u128 x = 0;
            for (u32 b = 0; b < nb; b++) {
                u32 c = '\n';
                if (o + b == nl) nl = nl == last ? NONE : min(nl + per, last);
                else {
                    while (q >= end && i + 1 < a.n) { i++; sym(i, end, se, base); }
                    c = q < se ? a.chars[(u64)(base + q)] : a.gap;
                    q++;
                }
                x |= (u128)c << (8u * b);
            }
            put16(dst, x, nb);
        }
    }
}

// ---- GFA walks (P lines): the same tables over token bytes instead of characters (gfa_text.hpp) -----------------------
// token bytes ("<id>+,") of every fixed symbol whose string is not empty, and a 1 for each such symbol
__global__ void k_path_tokfixed(const u64* __restrict__ ent_off, const u32* __restrict__ elen, const u64* __restrict__ seg_rank,
                                const u64* __restrict__ rank, u64 n, u64* __restrict__ tok, u64* __restrict__ cnt)
{
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i <= n; i += (u64)gridDim.x * blockDim.x) {
        u64 t = 0;
        if (i < n && rank[i + 1] == rank[i]) { const u64 j = ent_off[i]; if (elen[j]) t = gfa::digits(seg_rank[j] + 1) + 2; }
        tok[i] = t;
        cnt[i] = t ? 1 : 0;
    }
}

// token bytes per (path, choice symbol); cnt[k]: the tokens of row k (one atomic per wave where a wave lies in one row)
__global__ void __launch_bounds__(256) k_path_tok(const u64* __restrict__ csid, u64 nc, u64 K, const u32* __restrict__ elen,
                                                  const u64* __restrict__ seg_rank, u64* __restrict__ tlen, u64* __restrict__ cnt)
{
    const u64 total = K * nc;
    for (u64 base = blockIdx.x * (u64)blockDim.x; base < total; base += (u64)gridDim.x * blockDim.x) {   // block-uniform
        const u64 t = base + threadIdx.x;
        const bool act = t < total;
        u64 k = NONE, tl = 0;
        if (act) {
            k = t / nc;
            const u64 sid = csid[t];
            if (sid != NONE && elen[sid]) tl = gfa::digits(seg_rank[sid] + 1) + 2;
            tlen[t] = tl;
        }
        const u64 k0 = __shfl(k, 0, 64);                              // (t ascends: lane 0 is active when any lane is)
        const u64 has = ballot64(tl != 0);
        if (__all(!act || k == k0)) {
            if ((threadIdx.x & 63) == 0 && has) atomicAdd((unsigned long long*)&cnt[k0], (unsigned long long)__popcll(has));
        } else if (tl) atomicAdd((unsigned long long*)&cnt[k], 1ull);
    }
}

// T: the scanned token bytes of the rows (K * nc + 1 entries)
__global__ void k_path_toktotals(const u64* __restrict__ T, u64 nc, u64 F, u64 K, u64* __restrict__ tot)
{
    const u64 k = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (k < K) tot[k] = F + (nc ? T[(k + 1) * nc] - T[k * nc] : 0);
}

struct WalkArgs { gfa::WalkTab tab; const PathRec* rec; u64 nrec, max_tiles; uint8_t* out; };

// largest i in [0, n) with walk_pos(i) <= q, as block_find
__device__ u64 walk_block_find(const gfa::WalkTab& a, u64 kb, u64 q)
{
    u64 lo = 0, hi = a.n;
    while (hi - lo > 1) {
        const u64 step = (hi - lo + CP_THREADS - 1) / CP_THREADS;
        const u64 i = lo + threadIdx.x * step;
        const int ok = i < hi && gfa::walk_pos(a, kb, i) <= q;
        const int cnt = __syncthreads_count(ok);
        lo += (u64)(cnt - 1) * step;
        hi = min(hi, lo + step);
    }
    return lo;
}

// One workgroup per (16 KiB of a path's line behind its name, path), paths fastest as in k_path_copy.  The workgroup finds
// the first and last symbol of its stretch by the 256-way search; a lane finds the token its 16 bytes start in by
// bisection between them, assembles the 16 bytes in registers (rec.L: the token bytes T; the body is T + 2 bytes, the
// last comma a tab, then "*\n") and stores them at once.
__global__ void __launch_bounds__(CP_THREADS) k_path_walk(WalkArgs a)
{
    const u64 work = a.max_tiles * a.nrec;
    for (u64 wi = blockIdx.x; wi < work; wi += gridDim.x) {
        const PathRec rc = a.rec[wi % a.nrec];
        const u64 o0 = (wi / a.nrec) * CP_TILE;
        if (o0 >= rc.body) continue;
        const u64 o1 = min(rc.body, o0 + (u64)CP_TILE), kb = rc.row * a.tab.nc, T = rc.L;
        u64 iA = 0, iB = 0;
        if (o0 < T) {
            iA = walk_block_find(a.tab, kb, o0);
            iB = walk_block_find(a.tab, kb, min(o1, T) - 1);
        }
        for (u64 o = o0 + (u64)threadIdx.x * 16; o < o1; o += (u64)CP_THREADS * 16) {
            const u32 nb = (u32)min((u64)16, o1 - o);
            const gfa::B16 x = gfa::walk_chunk(a.tab, kb, iA, iB, T, o, nb);
            uint8_t* dst = a.out + rc.body_off + o;
            if (nb == 16) store16u(dst, make_uint4((u32)x.lo, (u32)(x.lo >> 32), (u32)x.hi, (u32)(x.hi >> 32)));
            else for (u32 b = 0; b < nb; b++) dst[b] = (uint8_t)((b < 8 ? x.lo >> (8u * b) : x.hi >> (8u * (b - 8u))) & 0xffu);
        }
    }
}

u64 free_hbm()
{
    size_t free_b = 0, total_b = 0;
    EDSX_HIP(hipMemGetInfo(&free_b, &total_b));
    return free_b;
}

// the grid of a body kernel: a workgroup per (tile, record), capped
unsigned body_grid(u64 nrec, u64 max_tiles) { return (unsigned)std::min<u64>(max_tiles * nrec, 1u << 20); }

} // namespace

void PathPipeline::open(const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, hipStream_t st)
{
    if (!seds) throw ParamError("Path spelling needs sources (.seds)");
    info_ = PathInfo{};
    timing_ = PathTiming{};
    walk_.ready = align_.ready = lift_.ready = slice_.ready = dist_.ready = dist_.cls[0].ready = dist_.cls[1].ready = ld_.ready = ibs_.ready = mosaic_.ready = false;
    const auto t0 = std::chrono::steady_clock::now();
    eds_.load(eds, eds_n, seds, seds_n, true, st);
    eds_.drop_scratch();                                                      // the session may live long
    n_ = eds_.n(); nc_ = 0; F_ = 0;
    info_.tokenised_on_device = eds_.tokenised_on_device();
    if (n_ == 0) { timing_.tokenise_ms = since_ms(t0); return; }              // empty EDS: P = 0
    const EdsView v = eds_.view();
    const u32 W = v.W;
    cum_fixed_.ensure(8 * (n_ + 1));
    rank_.ensure(8 * (n_ + 1));
    ctl_.ensure(8 * 8);
    scan_tmp_.ensure(8 * 2 * (n_ / SCAN_TILE + 4));
    tot_.ensure(8 * (size_t)W);
    u64 hn = n_;
    EDSX_HIP(hipMemcpyAsync(ctl_.ptr, &hn, 8, hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemsetAsync(tot_.ptr, 0, 8 * (size_t)W, st));
    u64 *cf = cum_fixed_.as<u64>(), *rk = rank_.as<u64>();
    hipLaunchKernelGGL(k_path_flags, dim3(grid_for(n_, 8192)), dim3(256), 0, st, v.sym.size, v.sym.ent_off, v.sym.len1, v.bits, W,
                       n_, cf, rk);
    ScanSet<2> ss{{cf, rk}, {cf, rk}, {cf + n_, rk + n_}};
    exclusive_scan_multi<2>(ss, ctl_.as<u64>(), scan_tmp_.as<u64>(), st);
    hipLaunchKernelGGL(k_path_or, dim3(1024), dim3(256), 0, st, v.bits, W, v.m, tot_.as<u64>());
    u64 h[2] = {0, 0};
    std::vector<u64> orb(W, 0);
    EDSX_HIP(hipMemcpyAsync(&h[0], cf + n_, 8, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipMemcpyAsync(&h[1], rk + n_, 8, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipMemcpyAsync(orb.data(), tot_.ptr, 8 * (size_t)W, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    F_ = h[0]; nc_ = h[1];
    if (nc_) {
        cidx_.ensure(8 * nc_);
        hipLaunchKernelGGL(k_path_cidx, dim3(grid_for(n_, 8192)), dim3(256), 0, st, rk, n_, cidx_.as<u64>());
        EDSX_HIP(hipStreamSynchronize(st));
        EDSX_HIP(hipGetLastError());
    }
    u64 P = 0;
    for (u32 w = 0; w < W; w++)
        if (orb[w]) P = 64ull * w + 63 - (u64)__builtin_clzll(orb[w]);
    info_.n_symbols = n_; info_.n_strings = v.m; info_.n_chars = v.n_chars; info_.num_paths = P; info_.n_choice_symbols = nc_;
    timing_.tokenise_ms = since_ms(t0);
}

void PathPipeline::check_ids(const u64* ids, size_t n) const
{
    for (size_t k = 0; k < n; k++)
        if (ids[k] == 0 || ids[k] > info_.num_paths)
            throw ParamError("Path id " + std::to_string(ids[k]) + " out of range (1.." + std::to_string(info_.num_paths) + ")");
}

void PathPipeline::begin_call()
{
    const double tok = timing_.tokenise_ms;
    timing_ = PathTiming{};
    timing_.tokenise_ms = tok;
}

// the bytes a batch may take: EDSX_PATHS_BUDGET when set (the tests force several batches), else that part of the free HBM
u64 PathPipeline::budget(u64 part)
{
    const char* e = getenv("EDSX_PATHS_BUDGET");
    const u64 ov = e ? std::strtoull(e, nullptr, 10) : 0;
    return ov ? ov : free_hbm() / part;
}

// paths per choice table: 16 bytes per (path, choice symbol) within a quarter of the free HBM (24 with the token bytes)
u64 PathPipeline::table_batch(size_t n, u64 cell_bytes) const
{
    return std::max<u64>(1, std::min<u64>(n, budget(4) / (cell_bytes * nc_ + 64)));
}

void PathPipeline::tables(const u64* ids, u64 K, std::vector<u64>& len, std::vector<u64>& miss, hipStream_t st)
{
    len.assign(K, 0); miss.assign(K, 0);
    ids_.ensure(8 * K); miss_.ensure(8 * K); tot_.ensure(8 * K);
    EDSX_HIP(hipMemcpyAsync(ids_.ptr, ids, 8 * K, hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemsetAsync(miss_.ptr, 0, 8 * K, st));
    TimedRuns timed(st, nullptr);
    const u64 cells = K * nc_;
    if (nc_) {
        csid_.ensure(8 * cells);
        clen_.ensure(8 * (cells + 1));
        scan_tmp_.ensure(8 * (cells / SCAN_TILE + 4));
        ctl_.ensure(8 * 8);
        EDSX_HIP(hipMemcpyAsync(ctl_.ptr, &cells, 8, hipMemcpyHostToDevice, st));
        const EdsView v = eds_.view();
        timed.run("k_path_choose", [&] {
            hipLaunchKernelGGL(k_path_choose, dim3(grid_for(cells, 8192)), dim3(256), 0, st, v.sym.size, v.sym.ent_off, v.str_off, v.bits,
                               v.W, cidx_.as<u64>(), nc_, ids_.as<u64>(), K, csid_.as<u64>(), clen_.as<u64>(), miss_.as<u64>());
        }, &timing_.choose_ms);
        timed.run("scan_cells", [&] {
            exclusive_scan_u64(clen_.as<u64>(), clen_.as<u64>(), ctl_.as<u64>(), clen_.as<u64>() + cells, scan_tmp_.as<u64>(), st);
        }, &timing_.scan_ms);
    }
    hipLaunchKernelGGL(k_path_totals, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, clen_.as<u64>(), nc_, F_, K, tot_.as<u64>());
    EDSX_HIP(hipMemcpyAsync(len.data(), tot_.ptr, 8 * K, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipMemcpyAsync(miss.data(), miss_.ptr, 8 * K, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    timed.harvest();
}

void PathPipeline::lengths(const u64* ids, size_t n, u64* length, u64* missing, hipStream_t st)
{
    check_ids(ids, n);
    begin_call();
    if (n == 0) return;
    const u64 KT = table_batch(n);
    std::vector<u64> len, miss;
    for (size_t i0 = 0; i0 < n; i0 += KT) {
        const u64 K = std::min<u64>(KT, n - i0);
        tables(ids + i0, K, len, miss, st);
        std::memcpy(length + i0, len.data(), 8 * K);
        if (missing) std::memcpy(missing + i0, miss.data(), 8 * K);
    }
}

template <class Tables, class Body>
void PathPipeline::emit_records(records::Rule rule, size_t n, const records::Headers& hdr, u64 line_width, u64 cell_bytes,
                                HostBytes& out, u64* missing, Tables&& make_tables, Body&& launch_body, hipStream_t st)
{
    // lengths and missing counts of all requested paths; one table batch: its tables stay for the bodies
    const u64 KT = table_batch(n, cell_bytes);
    const bool single = KT >= n;
    std::vector<u64> len(n), miss(n), bl, bm;
    for (size_t i0 = 0; i0 < n; i0 += KT) {
        const u64 K = std::min<u64>(KT, n - i0);
        make_tables(i0, K, bl, bm);
        std::memcpy(len.data() + i0, bl.data(), 8 * K);
        std::memcpy(miss.data() + i0, bm.data(), 8 * K);
    }
    if (missing) std::memcpy(missing, miss.data(), 8 * n);
    const records::Layout lay = records::layout(rule, len.data(), n, hdr.off.data(), line_width, KT);
    const u64 total = lay.start[n];
    out.take(total);
    timing_.bytes_written = total;
    if (total == 0) return;
    hdr_.ensure(hdr.blob.size());
    EDSX_HIP(hipMemcpyAsync(hdr_.ptr, hdr.blob.data(), hdr.blob.size(), hipMemcpyHostToDevice, st));
    const u64 out_budget = budget(2);
    std::vector<PathRec> batch;
    for (size_t i0 = 0; i0 < n; i0 += KT) {
        const size_t i1 = std::min<size_t>(n, i0 + KT);
        if (!single) make_tables(i0, i1 - i0, bl, bm);
        for (size_t r0 = i0, r1; r0 < i1; r0 = r1) {
            r1 = records::batch_end(lay.start, r0, i1, out_budget);
            const u64 bytes = lay.start[r1] - lay.start[r0], max_body = records::batch_records(lay, hdr.off.data(), r0, r1, batch);
            if (batch.empty()) continue;
            const u64 nrec = batch.size(), max_tiles = (max_body + CP_TILE - 1) / CP_TILE;
            out_.ensure(bytes + 16);                             // 16 bytes of slack behind the text, as every output buffer here
            rec_.ensure(sizeof(PathRec) * nrec);
            EDSX_HIP(hipMemcpyAsync(rec_.ptr, batch.data(), sizeof(PathRec) * nrec, hipMemcpyHostToDevice, st));
            TimedRuns timed(st, nullptr);
            timed.run("records", [&] {
                hipLaunchKernelGGL(k_path_headers, dim3((unsigned)nrec), dim3(64), 0, st, hdr_.as<uint8_t>(), rec_.as<PathRec>(), out_.as<uint8_t>());
                if (max_tiles) launch_body(rec_.as<PathRec>(), nrec, max_tiles, out_.as<uint8_t>());
            }, &timing_.copy_ms);
            EDSX_HIP(hipStreamSynchronize(st));
            EDSX_HIP(hipGetLastError());
            timed.harvest();
            const auto t0 = std::chrono::steady_clock::now();
            PinnedDownload::copy(out.data + lay.start[r0], out_.ptr, bytes, st);
            timing_.download_ms += since_ms(t0);
        }
    }
}

void PathPipeline::spell(const u64* ids, size_t n, const char* const* names, const char* prefix, u64 line_width, HostBytes& out,
                         u64* missing, hipStream_t st)
{
    check_ids(ids, n);
    begin_call();
    out.take(0);
    if (n == 0) return;
    const EdsView v = eds_.view();
    emit_records(records::FASTA, n, records::fasta_headers(ids, n, names, prefix), line_width, 16, out, missing,
        [&](size_t i0, u64 K, std::vector<u64>& len, std::vector<u64>& miss) { tables(ids + i0, K, len, miss, st); },
        [&](const PathRec* rec, u64 nrec, u64 max_tiles, uint8_t* dst) {
            const CopyArgs a{v.sym.ent_off, v.str_off, v.chars, cum_fixed_.as<u64>(), rank_.as<u64>(), nc_ ? csid_.as<u64>() : nullptr,
                             nc_ ? clen_.as<u64>() : nullptr, n_, nc_, rec, nrec, max_tiles, dst};
            hipLaunchKernelGGL(k_path_copy, dim3(body_grid(nrec, max_tiles)), dim3(CP_THREADS), 0, st, a);
        }, st);
}

void PathPipeline::align_open(hipStream_t st)
{
    if (align_.ready) return;
    AlignInfo& ai = align_.info;
    ai = AlignInfo{};
    ai.n_symbols = n_; ai.num_paths = info_.num_paths;
    if (n_) {
        const EdsView v = eds_.view();
        align_.col.ensure(8 * (n_ + 1));
        ctl_.ensure(8 * 8);
        scan_tmp_.ensure(8 * (n_ / SCAN_TILE + 4));
        u64 h[4] = {n_ + 1, 0, 0, 0};                            // count; W; symbols of width 0; the widest
        u64 *ctl = ctl_.as<u64>(), *col = align_.col.as<u64>();
        EDSX_HIP(hipMemcpyAsync(ctl, h, sizeof(h), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_align_width, dim3(grid_for(n_ + 1, 8192)), dim3(256), 0, st, v.sym.size, v.sym.ent_off, v.str_off, n_, col,
                           ctl + 2);
        exclusive_scan_u64(col, col, ctl, ctl + 1, scan_tmp_.as<u64>(), st);
        EDSX_HIP(hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        EDSX_HIP(hipGetLastError());
        ai.n_columns = h[1]; ai.n_zero_width_symbols = h[2]; ai.widest_symbol = h[3];
    }
    align_.ready = true;
}

void PathPipeline::align(const u64* ids, size_t n, const char* const* names, const char* prefix, u64 line_width, uint8_t gap,
                         u64 max_bytes, HostBytes& out, u64* missing, hipStream_t st)
{
    check_ids(ids, n);
    if (std::strchr(">\n\r {},", gap)) throw ParamError("Gap character is not usable in an alignment");   // (and 0)
    begin_call();
    out.take(0);
    if (n == 0) return;
    align_open(st);
    // header texts, and the size of the whole: every row has W columns, so the counts give it before any table is made
    const u64 W = align_.info.n_columns;
    const records::Headers hdr = records::fasta_headers(ids, n, names, prefix);
    u64 lw, body;
    records::body_of(records::FASTA, W, line_width, lw, body);
    const unsigned __int128 total128 = (unsigned __int128)body * n + hdr.blob.size();
    if ((max_bytes && total128 > max_bytes) || total128 > ~0ull) {
        const std::string cap = std::to_string(max_bytes ? max_bytes : ~0ull);
        const std::string have = total128 > ~0ull ? "more than " + std::to_string(~0ull) : std::to_string((u64)total128);
        throw ParamError("Alignment has " + have + " bytes, above the limit of " + cap);
    }
    const EdsView v = eds_.view();
    emit_records(records::FASTA, n, hdr, line_width, 16, out, missing,
        [&](size_t i0, u64 K, std::vector<u64>& len, std::vector<u64>& miss) {   // the chosen strings and the missing counts
            tables(ids + i0, K, len, miss, st);
            len.assign(K, W);
        },
        [&](const PathRec* rec, u64 nrec, u64 max_tiles, uint8_t* dst) {
            const AlignArgs a{v.sym.ent_off, v.str_off, v.chars, align_.col.as<u64>(), rank_.as<u64>(), nc_ ? csid_.as<u64>() : nullptr, n_, nc_,
                              rec, nrec, max_tiles, dst, gap};
            hipLaunchKernelGGL(k_path_align, dim3(body_grid(nrec, max_tiles)), dim3(CP_THREADS), 0, st, a);
        }, st);
}

void PathPipeline::walk_open(hipStream_t st)
{
    if (walk_.ready || n_ == 0) return;
    const EdsView v = eds_.view();
    walk_.seg_rank.ensure(8 * (v.m + 1));
    walk_.cum_tok.ensure(8 * (n_ + 1));
    walk_.cnt.ensure(8 * (n_ + 1));
    ctl_.ensure(8 * 8);
    scan_tmp_.ensure(8 * 2 * (v.m / SCAN_TILE + n_ / SCAN_TILE + 8));
    u64 h[6] = {v.m + 1, n_ + 1, 0, 0, 0, 0};
    u64* ctl = ctl_.as<u64>();
    EDSX_HIP(hipMemcpyAsync(ctl, h, sizeof(h), hipMemcpyHostToDevice, st));
    segment_ranks(v, walk_.seg_rank.as<u64>(), ctl, ctl + 2, scan_tmp_.as<u64>(), st);
    u64 *ct = walk_.cum_tok.as<u64>(), *cn = walk_.cnt.as<u64>();
    hipLaunchKernelGGL(k_path_tokfixed, dim3(grid_for(n_ + 1, 8192)), dim3(256), 0, st, v.sym.ent_off, v.elen, walk_.seg_rank.as<u64>(),
                       rank_.as<u64>(), n_, ct, cn);
    ScanSet<2> ss{{ct, cn}, {ct, cn}, {ctl + 3, ctl + 4}};
    exclusive_scan_multi<2>(ss, ctl + 1, scan_tmp_.as<u64>(), st);
    EDSX_HIP(hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    walk_.Ftok = h[3]; walk_.Fcnt = h[4];
    walk_.ready = true;
}

void PathPipeline::walk_tables(const u64* ids, u64 K, std::vector<u64>& tok, std::vector<u64>& miss, std::vector<u64>& cnt, hipStream_t st)
{
    std::vector<u64> len;
    tables(ids, K, len, miss, st);                               // csid_, the missing counts (and the lengths, not used here)
    tok.assign(K, 0); cnt.assign(K, 0);
    const u64 cells = K * nc_;
    walk_.cnt.ensure(8 * std::max<u64>(K, n_ + 1));
    u64* cn = walk_.cnt.as<u64>();
    EDSX_HIP(hipMemsetAsync(cn, 0, 8 * K, st));
    TimedRuns timed(st, nullptr);
    if (nc_) {
        walk_.tlen.ensure(8 * (cells + 1));
        u64* tlen = walk_.tlen.as<u64>();
        EDSX_HIP(hipMemcpyAsync(ctl_.ptr, &cells, 8, hipMemcpyHostToDevice, st));
        const EdsView v = eds_.view();
        timed.run("k_path_tok", [&] {
            hipLaunchKernelGGL(k_path_tok, dim3(grid_for(cells, 8192)), dim3(256), 0, st, csid_.as<u64>(), nc_, K, v.elen,
                               walk_.seg_rank.as<u64>(), tlen, cn);
            exclusive_scan_u64(tlen, tlen, ctl_.as<u64>(), tlen + cells, scan_tmp_.as<u64>(), st);
        }, &timing_.scan_ms);
    }
    hipLaunchKernelGGL(k_path_toktotals, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, walk_.tlen.as<u64>(), nc_, walk_.Ftok, K, tot_.as<u64>());
    EDSX_HIP(hipMemcpyAsync(tok.data(), tot_.ptr, 8 * K, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipMemcpyAsync(cnt.data(), cn, 8 * K, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    timed.harvest();
    for (u64 k = 0; k < K; k++) cnt[k] += walk_.Fcnt;
}

void PathPipeline::walks(const u64* ids, size_t n, const char* const* names, const char* prefix, HostBytes& out, u64* missing,
                         u64* steps, hipStream_t st)
{
    check_ids(ids, n);
    begin_call();
    out.take(0);
    if (n == 0) return;
    size_t bad = n;
    const records::Headers hdr = records::walk_headers(ids, n, names, prefix, bad);   // the texts in front of the walks: "P\t<name>\t"
    if (bad < n) throw ParamError("Path name " + std::to_string(bad) + " is not a GFA name");
    walk_open(st);
    const EdsView v = eds_.view();
    std::vector<u64> cnt;
    emit_records(records::WALK, n, hdr, 0, 24, out, missing,
        [&](size_t i0, u64 K, std::vector<u64>& tok, std::vector<u64>& miss) {
            walk_tables(ids + i0, K, tok, miss, cnt, st);
            if (steps) std::memcpy(steps + i0, cnt.data(), 8 * K);
        },
        [&](const PathRec* rec, u64 nrec, u64 max_tiles, uint8_t* dst) {
            const WalkArgs a{gfa::WalkTab{v.sym.ent_off, walk_.seg_rank.as<u64>(), walk_.cum_tok.as<u64>(), rank_.as<u64>(),
                                          nc_ ? csid_.as<u64>() : nullptr, nc_ ? walk_.tlen.as<u64>() : nullptr, n_, nc_},
                             rec, nrec, max_tiles, dst};
            hipLaunchKernelGGL(k_path_walk, dim3(body_grid(nrec, max_tiles)), dim3(CP_THREADS), 0, st, a);
        }, st);
}

} // namespace edsx
