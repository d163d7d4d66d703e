// ibs_core.hpp — the per-item arithmetic of the shared segments of two paths (ibs_device.hip): the walk over
// the set bits of one xor word of two `strings` bit rows (dist_core.hpp), the segment between two differing choice ranks
// with its head and tail cases, the reporting test, the index of a pair in upper-triangle order, and the walk of one
// pair over its chunk edges that adds the segments no chunk can see.  Plain functions over plain arrays, as dist_core.hpp
// and ld_core.hpp: hipcc compiles them into the k_ibs_* kernels, and g++ compiles them for tests/cpp/test_ibs_core.cpp,
// which runs them on heap tables of exactly the sizes below under the address and undefined-behaviour sanitizers.
//
// Rows.  Under the STRINGS class list every path has exactly one bit per listed choice symbol, so R[a] ^ R[b] has two set
// bits at every symbol where the two paths take different strings and none elsewhere.  desc[c] >> 24 is the choice rank
// of class column c; descriptors ascend, so the set bits of a pair come in rank order and the two bits of one symbol
// follow each other - in one word, in two neighbouring words or in two chunks.  `last` is the rank of the last bit seen:
// a bit of the same rank is the same difference.
//
// Tables (IbsTab) and their sizes: cidx: nc (the symbol of choice rank r); col: n + 1 (the first column of every symbol
// in the alignment view, col[n] = W); desc: C.  Scratch of a call over `pairs` pairs and `chunks` chunks: icnt, first,
// last: pairs x chunks (the reported interior segments of a chunk, its first and last differing rank, NONE without one);
// tot: pairs x (chunks + 1) + 1 (icnt plus the seam segment that ends in the chunk; slot `chunks` is the tail; one more
// entry so that the exclusive scan leaves the total behind the last).
#pragma once

#include "dist_core.hpp"

#define IBS_HD DIST_HD

namespace edsx {
namespace ibs {

typedef dist::u64 u64;
typedef dist::u32 u32;

constexpr u64 NONE = dist::NONE;

// edsx_ibs_segment (include/edsx.h)
struct Segment { u64 x, y, symbol_first, symbol_last, sites, column_first, column_end; };

struct IbsTab { const u64* cidx; const u64* col; u64 n, nc; };
struct Rule { u64 min_sites, min_columns; };

// ---- the segment between the differing ranks r_prev < r_next; r_prev NONE: from the head of the EDS, r_next NONE: to its
// tail, both NONE: the whole EDS.  false: the interval is empty (adjacent differing symbols, a difference at an end, n = 0)
IBS_HD bool gap(const IbsTab& t, u64 r_prev, u64 r_next, Segment& s)
{
    const u64 first = r_prev == NONE ? 0 : t.cidx[r_prev] + 1, end = r_next == NONE ? t.n : t.cidx[r_next];
    if (first >= end) return false;
    s.symbol_first = first; s.symbol_last = end - 1;
    s.sites = (r_next == NONE ? t.nc : r_next) - (r_prev == NONE ? 0 : r_prev + 1);
    s.column_first = t.col[first]; s.column_end = t.col[end];
    return true;
}
IBS_HD bool reported(const Rule& q, const Segment& s) { return s.sites >= q.min_sites && s.column_end - s.column_first >= q.min_columns; }

// ---- pair (x, y), x < y < K, in row-major order over the upper triangle without the diagonal
// (one factor of each product is even: halved first, so that K up to 2^32 and beyond stays within 64 bits)
IBS_HD u64 pair_index(u64 K, u64 x, u64 y)
{
    const u64 f = 2 * K - x - 1;
    return (x & 1 ? x * (f / 2) : x / 2 * f) + (y - x - 1);
}
IBS_HD u64 pair_count(u64 K) { return K & 1 ? (K - 1) / 2 * K : K / 2 * (K - 1); }

// ---- the walk over one xor word: word index gw of the row, `last` the rank of the last bit seen in this chunk (NONE at the
// chunk's start).  on_first(r): the chunk's first difference; on_gap(r_prev, r_next): two differences of the chunk in a row
template <class First, class Gap>
IBS_HD void walk_word(const u64* desc, u64 gw, u64 word, u64& last, First&& on_first, Gap&& on_gap)
{
    for (u64 x = word; x; x &= x - 1) {
        const u64 r = desc[64 * gw + (u64)__builtin_ctzll(x)] >> dist::INDEX_BITS;
        if (r == last) continue;
        if (last == NONE) on_first(r); else on_gap(last, r);
        last = r;
    }
}

// ---- the stitch of one pair over its chunk edges, in chunk order: first, last: the `chunks` edges of the pair.
// seam(c, r_prev, r_next): a segment no chunk sees - c < chunks: it ends at the first difference of chunk c (r_prev NONE: the
// head); c == chunks: the tail (r_next NONE), or the whole EDS for a pair without a difference
template <class Seam>
IBS_HD void stitch(const u64* first, const u64* last, u64 chunks, Seam&& seam)
{
    u64 prev = NONE;
    for (u64 c = 0; c < chunks; c++) {
        const u64 f = first[c];
        if (f == NONE) continue;
        if (f != prev) seam(c, prev, f);                          // (equal ranks: one symbol's two bits in two chunks)
        prev = last[c];
    }
    seam(chunks, prev, NONE);
}

} // namespace ibs
} // namespace edsx
