// div_core.hpp — the per-item arithmetic of the windowed diversity between groups of paths of an EDS (div_device.hip,
// DESIGN 8p): the group counts of one row word, the sums of a choice symbol over its strings, the closed forms of diff and
// comp, the windows of both units, the rank bisection of the COLUMNS unit and the bin rule of the site frequency spectrum.
// Plain functions over plain arrays, as ld_core.hpp: hipcc compiles them into the k_div_* kernels, and g++ compiles them
// for tests/cpp/test_div_core.cpp, which runs them on heap tables of exactly the sizes below under the address and
// undefined-behaviour sanitizers.
//
// Rows and carriers are those of ld_core.hpp: T(r, j) comes from ld::walk_step over the row of ALL paths (valid_word), and
// the count of group g is popcount(T & mask_g), mask_g the row of the paths of g with zero padding.
//
// Arrays.  Per choice symbol the device keeps NA = 2 G + 2 NP numbers, array-major with a stride of nc + 1 (entry nc is 0,
// so that an exclusive scan leaves the total there): seg_g, present_g, diff_q, comp_q (arr_* below), q the pair (g, h),
// g <= h, in row-major order.
#pragma once

#include "ld_core.hpp"

namespace edsx {
namespace diversity {

typedef ld::u64 u64;
typedef ld::u32 u32;

constexpr u32 MAX_GROUPS = 16;
enum Unit { SYMBOLS = 0, COLUMNS = 1 };

// ---- groups and pairs
LD_HD u64 num_pairs(u64 G) { return G * (G + 1) / 2; }
LD_HD u64 pair_index(u64 G, u64 g, u64 h) { return g * G - g * (g + 1) / 2 + h; }      // g <= h < G
LD_HD u64 arr_seg(u64, u64 g) { return g; }
LD_HD u64 arr_present(u64 G, u64 g) { return G + g; }
LD_HD u64 arr_diff(u64 G, u64 q) { return 2 * G + q; }
LD_HD u64 arr_comp(u64 G, u64 q) { return 2 * G + num_pairs(G) + q; }
LD_HD u64 num_arrays(u64 G) { return 2 * G + 2 * num_pairs(G); }

// word w (w < WP) of the row of all P paths
LD_HD u64 valid_word(u64 P, u64 WP, u64 w) { return w + 1 < WP || (P & 63) == 0 ? ~0ull : (1ull << (P & 63)) - 1; }
// the paths of a group among the carriers t of one row word
LD_HD u32 group_count(u64 t, u64 mask_word) { return (u32)__builtin_popcountll(t & mask_word); }

// ---- a choice symbol: n_g = sum_j c_gj, s_gh = sum_j c_gj c_hj, strings_g = the strings with a carrier in g
struct GroupSums { u64 n, strings; };
LD_HD void add_string(GroupSums& s, u64 c) { s.n += c; s.strings += c ? 1 : 0; }
LD_HD u64 segregating(const GroupSums& s) { return s.strings >= 2 ? 1 : 0; }
// the closed forms: pairs of paths that both take a string, and those of them whose strings differ
LD_HD u64 comp_within(u64 n) { return n * (n - (n ? 1 : 0)) / 2; }
LD_HD u64 diff_within(u64 n, u64 s_gg) { return (n * n - s_gg) / 2; }
LD_HD u64 comp_between(u64 n_g, u64 n_h) { return n_g * n_h; }
LD_HD u64 diff_between(u64 n_g, u64 n_h, u64 s_gh) { return n_g * n_h - s_gh; }
// nc * kmax^2 stays below 2^63: every window sum fits 64 bits
LD_HD bool sums_fit(u64 nc, u64 kmax)
{
    const unsigned __int128 v = (unsigned __int128)nc * kmax * kmax;
    return v < ((unsigned __int128)1 << 63);
}

// ---- the site frequency spectrum: string j of a symbol at which n of the K paths of the group are present, c of them on j
LD_HD bool sfs_counts(u64 j, u64 n, u64 K) { return j >= 1 && n == K; }

// ---- windows over the extent E: window k covers [k step, min(k step + size, E))
LD_HD u64 window_count(u64 E, u64 size, u64 step)
{
    if (E == 0) return 0;
    if (size == 0) return 1;
    if (step == 0) step = size;
    return (E - 1) / step + 1;
}
LD_HD void window_bounds(u64 k, u64 E, u64 size, u64 step, u64& start, u64& end)
{
    if (size == 0) { start = 0; end = E; return; }
    if (step == 0) step = size;
    start = k * step;
    end = size >= E - start ? E : start + size;
}
// the coordinate of choice symbol r; col: the exclusive scan of the symbol widths, E = max(W, 1)
LD_HD u64 coordinate(int unit, u64 r, const u64* cidx, const u64* col, u64 E)
{
    if (unit == SYMBOLS) return r;
    const u64 c = col[cidx[r]];
    return c < E - 1 ? c : E - 1;
}
// the first r in [0, nc] whose coordinate is at least x (nc: none); coordinates do not decrease with r
LD_HD u64 rank_at(int unit, u64 nc, const u64* cidx, const u64* col, u64 E, u64 x)
{
    if (unit == SYMBOLS) return x < nc ? x : nc;
    u64 lo = 0, hi = nc;
    while (lo < hi) { const u64 mid = lo + ((hi - lo) >> 1); if (coordinate(unit, mid, cidx, col, E) >= x) hi = mid; else lo = mid + 1; }
    return lo;
}

} // namespace diversity
} // namespace edsx
