// mosaic_core.hpp — the per-item arithmetic of the minimal mosaic of a path (mosaic_device.hip): a target path
// written as the fewest copies from donor paths plus the symbols nobody shares.  Plain functions over plain arrays, as
// ibs_core.hpp: hipcc compiles them into the k_mosaic_* kernels, and g++ compiles them for tests/cpp/test_mosaic_core.cpp,
// which runs the march on heap tables of exactly the sizes below under the address and undefined-behaviour sanitizers.
//
// Rows.  Under the STRINGS class list (dist_core.hpp) every path has exactly one bit per listed choice symbol, so of the
// two set bits R[t] ^ R[d] has at a symbol where target and donor differ, one is the target's own: R[t] & ~R[d] keeps that
// one.  It has exactly one set bit per differing listed rank, at the column where the target has its bit, so the bits of
// all donors of one target at one rank lie in the same column of the same word (a bit of the rank seen last is the same
// difference: it is never seen twice), their order is the order of the ranks, and "donor d differs from t at the rank of
// column c" is one bit test of R[d] at c, wherever the other class columns of that symbol lie - in this word, the one
// before or the one behind.  desc[c] >> 24 is the choice rank of class column c and cidx[rank] its symbol.
//
// The march of one target goes along the class words with a set of alive donors: those that have agreed with the target
// since the segment's start.  Bits below the column `from` belong to ranks that are done.  Tables (Tab) and their sizes:
// cidx: nc; col: n + 1; desc: C.  Scratch of a call: alive: targets x alive_words(D, lanes) x lanes words, bit b of word
// kk of a lane is its donor donor_of(kk, b, lane, lanes); cnt: targets + 1.
#pragma once

#include "ibs_core.hpp"

#define MOSAIC_HD DIST_HD

namespace edsx {
namespace mosaic {

typedef dist::u64 u64;
typedef dist::u32 u32;

constexpr u64 NONE = dist::NONE;

// edsx_mosaic_segment (include/edsx.h)
struct Segment { u64 target, donor, symbol_first, symbol_last, sites, column_first, column_end; };

typedef ibs::IbsTab Tab;                       // cidx, col, n, nc

// ---- donors across lanes: lane l of `lanes` holds the donors l, l + lanes, l + 2 lanes, ..; 64 of them per alive word
MOSAIC_HD u64 alive_words(u64 D, u64 lanes) { return ((D + lanes - 1) / lanes + 63) / 64; }
MOSAIC_HD u64 donor_of(u64 kk, u32 b, u64 lane, u64 lanes) { return (64 * kk + b) * lanes + lane; }

// ---- the bits of class word w at or behind column `from`
MOSAIC_HD u64 mask_from(u64 from, u64 w)
{
    if (from <= 64 * w) return ~0ull;
    if (from >= 64 * w + 64) return 0;
    return ~0ull << (from - 64 * w);
}
// the ranks of word w at which the donor (word dw) differs from the target (word tw), one bit each
MOSAIC_HD u64 differ_word(u64 tw, u64 dw, u64 mask) { return tw & ~dw & mask; }
// does the donor agree with the target at the rank of class column c, a column where the target has its bit
MOSAIC_HD bool agrees_at(u64 dw, u64 c) { return (dw >> (c & 63)) & 1; }

// ---- where the last alive donors die inside one word: the furthest column wins, then the smallest request position
constexpr u32 POS_BITS = 58;
MOSAIC_HD u64 death_key(u32 bit, u64 pos) { return (u64)bit << POS_BITS | (((1ull << POS_BITS) - 1) - pos); }
MOSAIC_HD u32 key_bit(u64 key) { return (u32)(key >> POS_BITS); }
MOSAIC_HD u64 key_pos(u64 key) { return ((1ull << POS_BITS) - 1) - (key & ((1ull << POS_BITS) - 1)); }

MOSAIC_HD u64 symbol_of(const Tab& t, const u64* desc, u64 c) { return t.cidx[desc[c] >> dist::INDEX_BITS]; }

// ---- the record of the symbols [first, end), end > first: ibs::gap's columns; its sites are counted between two symbols,
// not between two differing ranks: the choice symbols below `end` less those below `first`
MOSAIC_HD u64 choice_below(const Tab& t, u64 sym)
{
    u64 lo = 0, hi = t.nc;
    while (lo < hi) { const u64 mid = lo + ((hi - lo) >> 1); if (t.cidx[mid] < sym) lo = mid + 1; else hi = mid; }
    return lo;
}
MOSAIC_HD Segment segment(const Tab& t, u64 target, u64 donor, u64 first, u64 end)
{
    Segment s;
    s.target = target; s.donor = donor; s.symbol_first = first; s.symbol_last = end - 1;
    s.sites = choice_below(t, end) - choice_below(t, first);
    s.column_first = t.col[first]; s.column_end = t.col[end];
    return s;
}

// ---- the private-run rule.  The run holds the symbols [s, prev]; the target's next listed symbol is `sym` > prev.  A symbol
// between them is not listed: every path takes the same string there, so every eligible donor agrees and the run ends at
// prev + 1 (GAP).  Else sym == prev + 1 and the run goes on through it unless a donor agrees there (NEXT: ask the donors)
enum Private { GAP = 0, NEXT = 1 };
MOSAIC_HD Private private_step(u64 prev, u64 sym) { return sym > prev + 1 ? GAP : NEXT; }

// ---- the state of one target's march, the same in every lane
struct March {
    u64 s = 0;                                 // the open segment's first symbol
    u64 prev = 0;                              // private run: its last symbol so far
    u64 from = 0;                              // class columns below it are done
    bool priv = false;
    u64 segments = 0, private_segments = 0, private_symbols = 0;
};

// closes [m.s, end) and opens the next segment at `end`
template <class Emit>
MOSAIC_HD void close(March& m, u64 donor, u64 end, Emit&& emit)
{
    emit(m.segments, donor, m.s, end);
    m.segments++;
    if (donor == NONE) { m.private_segments++; m.private_symbols += end - m.s; }
    m.s = end;
}

// ---- the march of one target over its RW class words (trow), n > 0 and at least one eligible donor.  Everything in it is
// the same in every lane; what goes over the donors is the caller's (a workgroup's lanes, or a loop):
//   ops.reset()               alive = every eligible donor
//   ops.survive(w, tw, mask)  true: some alive donor has no difference in word w at or behind the mask; then alive loses
//                             those that have one.  false: alive is unchanged
//   ops.death(w, tw, mask)    all alive donors differ in word w: the largest death_key(first differing bit, position)
//   ops.agree(w, c)           alive = the eligible donors that agree at class column c of word w; true: there is one
//   ops.first()               the smallest alive request position
//   emit(k, donor, first, end)   segment k of the target: the symbols [first, end)
template <class Ops, class Emit>
MOSAIC_HD March march(const Tab& t, const u64* desc, const u64* trow, u64 RW, Ops&& ops, Emit&& emit)
{
    March m;
    ops.reset();
    for (u64 w = 0; w < RW;) {
        const u64 tw = trow[w], mask = mask_from(m.from, w);
        if (!m.priv) {
            if (ops.survive(w, tw, mask)) { w++; continue; }
            const u64 key = ops.death(w, tw, mask), c = 64 * w + key_bit(key), sym = symbol_of(t, desc, c);
            if (sym > m.s) close(m, key_pos(key), sym, emit);     // (sym == s: a segment opened on trust, and nobody agrees at s)
            if (!ops.agree(w, c)) { m.priv = true; m.prev = sym; }
            m.from = c + 1;
            continue;
        }
        const u64 own = tw & mask;                               // the target's next listed symbol
        if (!own) { w++; continue; }
        const u64 c = 64 * w + (u64)__builtin_ctzll(own), sym = symbol_of(t, desc, c);
        if (private_step(m.prev, sym) == GAP) {                  // opened on trust: all eligible donors, column c is still to come
            close(m, NONE, m.prev + 1, emit);
            m.priv = false;
            ops.reset();
            continue;
        }
        if (ops.agree(w, c)) { close(m, NONE, sym, emit); m.priv = false; }
        else m.prev = sym;
        m.from = c + 1;
    }
    if (m.priv) {
        if (m.prev + 1 < t.n) { close(m, NONE, m.prev + 1, emit); m.priv = false; ops.reset(); }
        else close(m, NONE, t.n, emit);
    }
    if (!m.priv) close(m, ops.first(), t.n, emit);
    return m;
}

} // namespace mosaic
} // namespace edsx
