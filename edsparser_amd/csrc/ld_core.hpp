// ld_core.hpp — the per-item arithmetic of the linkage disequilibrium between the alleles of an EDS (ld_device.hip, DESIGN
// 8m): the walk over the strings of a choice symbol for one row word, the listing rule, the partner range of an allele,
// the column tiles of a row tile, the validity of a pair and r².  Plain functions over plain arrays, as dist_core.hpp and
// slice_core.hpp: hipcc compiles them into the k_ld_* kernels, and g++ compiles them for tests/cpp/test_ld_core.cpp, which
// runs them on heap tables of exactly the sizes below under the address and undefined-behaviour sanitizers.
//
// Rows.  The source set of a string is a bitset of W = P / 64 + 1 words, bit 0 the universal path and bit p path p.  A
// row has WP = ceil(P / 64) words and holds path p at bit p - 1: row word w is the set shifted down by one across the
// word seam, all ones for a universal set.  mask: the row of the requested paths M, padding bits zero, so every row that
// went through it has zero padding as well.
//
// Carriers.  T(r, j) is the row of the paths of M that take string j of choice symbol r: the set of j without the paths
// an earlier string of the symbol has taken (`seen`, the OR of the rows so far); U(r), the paths present at r, is `seen`
// behind the last string.
//
// Tables: afirst, nc + 1 entries: the first listed allele of every choice symbol, afirst[nc] = A; tstart, RT + 1: the
// first column tile of every row tile in the list of all tiles, tstart[RT] = their number.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define LD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LD_HD inline __attribute__((always_inline))
#endif

namespace edsx {
namespace ld {

typedef unsigned long long u64;
typedef unsigned int u32;
typedef long long i64;

constexpr u64 NONE = ~0ull;
constexpr u32 TILE = 64, STAGE_WORDS = 32;

// ---- the symbol walk
// word w (w < WP) of the row of the set b (W words)
LD_HD u64 row_word(const u64* b, u32 W, u64 w)
{
    if (b[0] & 1) return ~0ull;
    return b[w] >> 1 | (w + 1 < W ? b[w + 1] << 63 : 0);
}
// word w of T(r, j) for the next string of a symbol: seen takes its paths
LD_HD u64 walk_step(const u64* b, u32 W, u64 w, u64 mask_word, u64& seen)
{
    const u64 t = row_word(b, W, w) & mask_word & ~seen;
    seen |= t;
    return t;
}

// ---- the listing rule: string j of a symbol with `present` paths, `count` of which take it
LD_HD bool listed(u64 j, bool all_strings, u64 count, u64 present, u64 min_count)
{
    if (j == 0 && !all_strings) return false;
    return min_count <= present && min_count <= count && count <= present - min_count;
}

// ---- the band: the partners of an allele of choice symbol r are the listed alleles [lo, hi) of the symbols r + 1 .. r + window
LD_HD u64 partner_lo(const u64* afirst, u64 r) { return afirst[r + 1]; }
LD_HD u64 partner_hi(const u64* afirst, u64 nc, u64 r, u64 window) { return afirst[window < nc - r ? r + window + 1 : nc]; }

// the column tiles [c0, c1) a row tile touches, whose first allele lies in symbol r_first and whose last in r_last
LD_HD void tile_columns(const u64* afirst, u64 nc, u64 r_first, u64 r_last, u64 window, u64& c0, u64& c1)
{
    const u64 lo = partner_lo(afirst, r_first), hi = partner_hi(afirst, nc, r_last, window);
    if (hi <= lo) { c0 = c1 = 0; return; }
    c0 = lo / TILE;
    c1 = (hi + TILE - 1) / TILE;
}
// tile q of the list (q < tstart[RT]): its row tile, the last t with tstart[t] <= q
LD_HD u64 tile_row(const u64* tstart, u64 RT, u64 q)
{
    u64 lo = 0, hi = RT - 1;
    while (lo < hi) { const u64 mid = lo + ((hi - lo + 1) >> 1); if (tstart[mid] <= q) lo = mid; else hi = mid - 1; }
    return lo;
}
// where the counter of (row xi of row tile t, column tile c0 + c) lies: allele-major, so one scan gives the (x, y) order
LD_HD u64 counter_slot(u64 tstart_t, u64 ntile_t, u64 xi, u64 c) { return TILE * tstart_t + xi * ntile_t + c; }

// alleles of the symbols rx and ry form a candidate pair
LD_HD bool pair_valid(u64 rx, u64 ry, u64 window) { return rx < ry && ry - rx <= window; }

// ---- r² from the four counts; false: undefined (an allele that all or none of the n paths carry)
LD_HD bool r2(u64 n, u64 n_a, u64 n_b, u64 n_ab, double& out)
{
    const u64 da = n_a * (n - n_a), db = n_b * (n - n_b);
    if (da == 0 || db == 0) return false;
    const i64 D = (i64)(n * n_ab) - (i64)(n_a * n_b);
    out = ((double)D / (double)da) * ((double)D / (double)db);
    return true;
}

} // namespace ld
} // namespace edsx
