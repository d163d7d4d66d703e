// slice_core.hpp — the per-region arithmetic of the region slice (slice_device.hip): the ends of a column
// region, the cut of a string, the byte counts of a region and the place of a string inside its region.  Plain functions
// over plain arrays, as lift_core.hpp: hipcc compiles them into the k_slice_* kernels, and g++ compiles them for
// tests/cpp/test_slice_core.cpp, which runs them on heap tables of exactly the sizes below under the address and
// undefined-behaviour sanitizers.
//
// The tables (SliceTab) and their sizes, in entries of 8 bytes: size, ent_off: n; str_off, sb: m + 1; col: n + 1.  sb is
// the exclusive scan of the .seds bytes of every string ("{ids}").
//
// A region holds the symbols i0 .. i1.  Every string of symbol i0 loses its first o0 characters, every string of symbol
// i1 keeps at most its first o1e (o0 < o1e when i0 == i1); `removed` of a string is what the two cuts take from it.  With
//   A = sum over the strings of i0 of min(len, o0)        B = sum over the strings of i1 of min(len, o1e)
// the region has chars = span - A - (L(i1) - B) characters, span the characters of all its strings uncut, L(i1) those of
// symbol i1.  String j of symbol i begins at
//   dst = (str_off[j] - str_off[e0]) - R(j) + (j - e0) + (i - i0) + 1
// inside the region's .eds text, R(j) the characters removed from the strings e0 .. j - 1 (e0 = ent_off[i0]): one byte of
// punctuation in front of every string up to j, one closing brace per symbol in front of i.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SLICE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SLICE_HD inline __attribute__((always_inline))
#endif

namespace edsx {
namespace slice {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr u64 NONE = ~0ull;
enum : uint8_t { OK = 0, RANGE = 4 };

struct SliceTab {
    const u64* size; const u64* ent_off; const u64* str_off;
    const u64* sb;                             // scanned .seds bytes per string
    const u64* col;                            // first alignment column of symbol i; col[n] = W
    u64 n, m;
};

// the resolved ends of a region: symbols, cut offsets, column window
struct Ends { u64 i0, i1, o0, o1e, c0, c1e; };

// edsx_slice_region without the four offsets and lengths
struct Counts { u64 strings, chars, eds_len, seds_len, edge_strings; };

SLICE_HD u64 min64(u64 a, u64 b) { return a < b ? a : b; }
SLICE_HD u64 ent_end(const SliceTab& t, u64 i) { return t.ent_off[i] + t.size[i]; }

// the largest symbol i < n with col[i] <= x, for x < col[n] (symbols of width 0 share a column with the one behind them)
SLICE_HD u64 col_symbol(const SliceTab& t, u64 x)
{
    u64 lo = 0, hi = t.n;
    while (hi - lo > 1) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (t.col[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// ends of the column region [start, end): false when it is empty or leaves [0, W)
SLICE_HD bool column_ends(const SliceTab& t, u64 start, u64 end, Ends& e)
{
    if (t.n == 0 || start >= end || end > t.col[t.n]) return false;
    e.i0 = col_symbol(t, start);
    e.i1 = col_symbol(t, end - 1);
    e.o0 = start - t.col[e.i0];
    e.o1e = end - t.col[e.i1];
    e.c0 = start;
    e.c1e = end;
    return true;
}

// ends of a path region from the lift sites of (path, start) and (path, end - 1)
SLICE_HD void path_ends(u64 i0, u64 o0, u64 c0, u64 i1, u64 o1, u64 c1, Ends& e)
{
    e.i0 = i0; e.i1 = i1; e.o0 = o0; e.o1e = o1 + 1; e.c0 = c0; e.c1e = c1 + 1;
}

// what is left of a string of length len in symbol i: characters [begin, begin + kept)
SLICE_HD void cut(const Ends& e, u64 i, u64 len, u64& begin, u64& kept)
{
    const u64 a = i == e.i0 ? min64(len, e.o0) : 0;
    const u64 b = i == e.i1 ? min64(len, e.o1e) : len;
    begin = a;
    kept = b > a ? b - a : 0;
}

SLICE_HD u64 removed(const Ends& e, u64 i, u64 len)
{
    u64 begin, kept;
    cut(e, i, len, begin, kept);
    return len - kept;
}

// the sizes of a region from its two edge sums
SLICE_HD void counts(const SliceTab& t, const Ends& e, u64 A, u64 B, Counts& c)
{
    const u64 e0 = t.ent_off[e.i0], e1 = ent_end(t, e.i1);
    const u64 span = t.str_off[e1] - t.str_off[e0];
    const u64 last = t.str_off[e1] - t.str_off[t.ent_off[e.i1]];
    c.strings = e1 - e0;
    c.chars = span - A - (last - B);
    c.eds_len = c.chars + c.strings + (e.i1 - e.i0 + 1) + 1;             // commas and braces, then the line feed
    c.seds_len = t.sb[e1] - t.sb[e0] + 1;
    c.edge_strings = t.size[e.i0] + (e.i1 != e.i0 ? t.size[e.i1] : 0);
}

// first byte of string j of symbol i inside the region's .eds text, R the characters removed in front of it
SLICE_HD u64 string_dst(const SliceTab& t, const Ends& e, u64 i, u64 j, u64 R)
{
    const u64 e0 = t.ent_off[e.i0];
    return (t.str_off[j] - t.str_off[e0]) - R + (j - e0) + (i - e.i0) + 1;
}

// the stretch [lo, hi) of the character pool that holds every kept character of the region: from the cut of its first
// string to the cut of its last one
SLICE_HD void copy_span(const SliceTab& t, const Ends& e, u64& lo, u64& hi)
{
    const u64 ja = t.ent_off[e.i0], jb = ent_end(t, e.i1) - 1;
    u64 begin, kept;
    cut(e, e.i0, t.str_off[ja + 1] - t.str_off[ja], begin, kept);
    lo = t.str_off[ja] + begin;
    cut(e, e.i1, t.str_off[jb + 1] - t.str_off[jb], begin, kept);
    hi = t.str_off[jb] + begin + kept;
}

// first byte of the set of string j inside the region's .seds text
SLICE_HD u64 set_dst(const SliceTab& t, const Ends& e, u64 j) { return t.sb[j] - t.sb[t.ent_off[e.i0]]; }

// slot of string j in the table of the edge strings of its region (the strings of i0, then those of i1), NONE inside
SLICE_HD u64 edge_slot(const SliceTab& t, const Ends& e, u64 i, u64 j)
{
    if (i == e.i0) return j - t.ent_off[i];
    if (i == e.i1) return t.size[e.i0] + (j - t.ent_off[i]);
    return NONE;
}

SLICE_HD u32 digits10(u64 v) { u32 d = 1; while (v >= 10) { v /= 10; d++; } return d; }

// bytes of the ids of word w of a set (x, bit 0 of word 0 already cleared), each with the comma or brace behind it
SLICE_HD u64 word_bytes(u32 w, u64 x)
{
    if (!x) return 0;
    const u32 lo = digits10(64ull * w), hi = digits10(64ull * w + 63);
    if (lo == hi) return (u64)__builtin_popcountll(x) * (lo + 1);
    u64 n = 0;
    while (x) {
        const u32 b = (u32)__builtin_ctzll(x);
        x &= x - 1;
        n += digits10(64ull * w + b) + 1;
    }
    return n;
}

// bytes of "{ids}" from the sum of word_bytes: a set that holds 0 is "{0}", an empty one "{}"
SLICE_HD u64 set_bytes(bool universal, u64 sum) { return universal ? 3 : sum ? sum + 1 : 2; }

} // namespace slice
} // namespace edsx
