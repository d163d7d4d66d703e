// dist_core.hpp — the per-descriptor arithmetic of the path distances (dist_device.hip): the classes of a
// compared unit, the 8-byte descriptor of a class column, and the bit a path gets in that column.  Plain functions over
// plain arrays, as lift_core.hpp and slice_core.hpp: hipcc compiles them into the k_dist_* kernels, and g++ compiles them
// for tests/cpp/test_dist_core.cpp, which runs them on heap tables of exactly the sizes below under the address and
// undefined-behaviour sanitizers.
//
// A unit is what two paths are compared at: a choice symbol (metric STRINGS) or one alignment column of a choice symbol
// (metric COLUMNS).  Every path has exactly one class per unit - STRINGS: the string it takes, or none; COLUMNS: the byte
// it shows there, or no character - so two paths agree at a unit iff they share a class, and with one bit per (path,
// class) the number of units at which they agree is popcount(row a & row b).  A unit with fewer than two classes cannot
// tell two paths apart and is not listed.
//
// The tables (DistTab) and their sizes: size, ent_off: n entries of 8 bytes; str_off: m + 1; chars: the character pool;
// cidx: nc (the symbol of choice rank r); ccol: nc + 1 (the exclusive scan of the widths of the choice symbols, ccol[nc] =
// their columns); may_miss: nc bytes.  csid_row: the nc chosen strings of one path (NONE: it takes none).
//
// Descriptors.  COLUMNS: unit << 9 | value, unit = ccol[r] + offset (below 2^55), value a byte or NOCHAR.  STRINGS:
// r << 24 | index of the string within its symbol, NOSTRING for "none" (a symbol holds fewer than 2^24 - 1 strings).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define DIST_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DIST_HD inline __attribute__((always_inline))
#endif

namespace edsx {
namespace dist {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr u64 NONE = ~0ull;
enum Metric : int { COLUMNS = 0, STRINGS = 1 };
constexpr u32 VALUE_BITS = 9, NOCHAR = 256;
constexpr u32 INDEX_BITS = 24;
constexpr u64 NOSTRING = (1ull << INDEX_BITS) - 1;

struct DistTab {
    const u64* size; const u64* ent_off; const u64* str_off; const uint8_t* chars;
    const u64* cidx; const u64* ccol; const uint8_t* may_miss;
    u64 nc;
};

// ---- the bytes present in a column: 256 bits
struct Present { u64 w[4]; };

DIST_HD void present_clear(Present& m) { m.w[0] = m.w[1] = m.w[2] = m.w[3] = 0; }
DIST_HD void present_add(Present& m, u32 byte) { m.w[byte >> 6] |= 1ull << (byte & 63); }
DIST_HD bool present_has(const Present& m, u32 byte) { return (m.w[byte >> 6] >> (byte & 63)) & 1; }
DIST_HD u32 present_count(const Present& m)
{
    return (u32)(__builtin_popcountll(m.w[0]) + __builtin_popcountll(m.w[1]) + __builtin_popcountll(m.w[2]) + __builtin_popcountll(m.w[3]));
}
// how many present bytes are smaller than `byte`: the place of its class among the classes of the unit
DIST_HD u32 present_rank(const Present& m, u32 byte)
{
    u32 r = 0;
    for (u32 k = 0; k < (byte >> 6); k++) r += (u32)__builtin_popcountll(m.w[k]);
    return r + (u32)__builtin_popcountll(m.w[byte >> 6] & ((1ull << (byte & 63)) - 1));
}

// ---- descriptors
DIST_HD u64 pack_column(u64 unit, u32 value) { return unit << VALUE_BITS | value; }
DIST_HD void unpack_column(u64 d, u64& unit, u32& value) { unit = d >> VALUE_BITS; value = (u32)(d & ((1u << VALUE_BITS) - 1)); }
DIST_HD u64 pack_string(u64 r, u64 index) { return r << INDEX_BITS | index; }
DIST_HD void unpack_string(u64 d, u64& r, u64& index) { r = d >> INDEX_BITS; index = d & NOSTRING; }

// ---- a symbol may leave a path without a string: none of its sets is universal and their OR lacks an id of 1..P
// bits: W words per string, bit 0 of word 0 = universal; the strings e0 .. e0 + sz - 1
DIST_HD bool may_miss(const u64* bits, u32 W, u64 e0, u64 sz, u64 P)
{
    bool lacks = false;
    for (u32 w = 0; w < W; w++) {
        u64 o = 0;
        for (u64 q = 0; q < sz; q++) o |= bits[(e0 + q) * W + w];
        if (w == 0 && (o & 1)) return false;
        const u64 lo = w == 0 ? 1 : 64ull * w, hi = 64ull * w + 63 < P ? 64ull * w + 63 : P;     // the ids of this word within 1..P
        if (lo > hi) continue;
        const u64 need = (hi - lo == 63 ? ~0ull : ((1ull << (hi - lo + 1)) - 1)) << (lo & 63);
        if ((o & need) != need) lacks = true;
    }
    return lacks;
}

// the choice rank whose columns hold unit (unit < ccol[nc]): the largest r with ccol[r] <= unit, which has a column
DIST_HD u64 unit_symbol(const DistTab& t, u64 unit)
{
    u64 lo = 0, hi = t.nc - 1;
    while (lo < hi) { const u64 mid = lo + ((hi - lo + 1) >> 1); if (t.ccol[mid] <= unit) lo = mid; else hi = mid - 1; }
    return lo;
}

// ---- classes of a unit
// COLUMNS: the bytes the strings of choice symbol r show at offset off; nochar: a string ends in front of off, or the
// symbol may leave a path without a string
DIST_HD void column_classes(const DistTab& t, u64 r, u64 off, Present& m, bool& nochar)
{
    const u64 i = t.cidx[r], e0 = t.ent_off[i], e1 = e0 + t.size[i];
    present_clear(m);
    nochar = t.may_miss[r] != 0;
    for (u64 j = e0; j < e1; j++) {
        const u64 s0 = t.str_off[j];
        if (off < t.str_off[j + 1] - s0) present_add(m, t.chars[s0 + off]); else nochar = true;
    }
}
// the class columns of a unit: none when it has fewer than two classes
DIST_HD u64 listed(u64 classes) { return classes >= 2 ? classes : 0; }
DIST_HD u64 column_count(const Present& m, bool nochar) { return listed(present_count(m) + (nochar ? 1 : 0)); }
DIST_HD u64 string_count(const DistTab& t, u64 r) { return listed(t.size[t.cidx[r]] + (t.may_miss[r] ? 1 : 0)); }

// the descriptors of a listed unit, column_count / string_count of them: bytes ascending, then no character; strings in
// file order, then none
DIST_HD void column_fill(const Present& m, bool nochar, u64 unit, u64* desc)
{
    u64 k = 0;
    for (u32 w = 0; w < 4; w++)
        for (u64 x = m.w[w]; x; x &= x - 1) desc[k++] = pack_column(unit, 64 * w + (u32)__builtin_ctzll(x));
    if (nochar) desc[k] = pack_column(unit, NOCHAR);
}
DIST_HD void string_fill(const DistTab& t, u64 r, u64* desc)
{
    const u64 sz = t.size[t.cidx[r]];
    for (u64 j = 0; j < sz; j++) desc[j] = pack_string(r, j);
    if (t.may_miss[r]) desc[sz] = pack_string(r, NOSTRING);
}

// ---- the bit of a path in a class column
// what the path shows at offset off of choice symbol r: a byte, or NOCHAR
DIST_HD u32 shown(const DistTab& t, const u64* csid_row, u64 r, u64 off)
{
    const u64 sid = csid_row[r];
    if (sid == NONE) return NOCHAR;
    const u64 s0 = t.str_off[sid];
    return off < t.str_off[sid + 1] - s0 ? t.chars[s0 + off] : NOCHAR;
}
DIST_HD bool string_bit(const DistTab& t, const u64* csid_row, u64 d)
{
    u64 r, index;
    unpack_string(d, r, index);
    const u64 sid = csid_row[r];
    return index == NOSTRING ? sid == NONE : sid == t.ent_off[t.cidx[r]] + index;
}

// word wd of the bit row of a path: the class columns 64 * wd .. 64 * wd + 63 below C, bit b for column 64 * wd + b; the
// bits of columns at or above C are zero.  Descriptors ascend by unit, so the symbol is searched for once and then followed.
DIST_HD u64 row_word(const DistTab& t, Metric metric, const u64* desc, u64 C, const u64* csid_row, u64 wd)
{
    const u64 c0 = 64 * wd, c1 = c0 + 64 < C ? c0 + 64 : C;
    u64 word = 0;
    if (metric == STRINGS) {
        for (u64 c = c0; c < c1; c++) word |= (u64)string_bit(t, csid_row, desc[c]) << (c - c0);
        return word;
    }
    u64 r = 0, last = NONE;
    u32 have = NOCHAR;
    for (u64 c = c0; c < c1; c++) {
        u64 unit;
        u32 value;
        unpack_column(desc[c], unit, value);
        if (unit != last) {
            if (last == NONE) r = unit_symbol(t, unit);
            else while (unit >= t.ccol[r + 1]) r++;
            have = shown(t, csid_row, r, unit - t.ccol[r]);
            last = unit;
        }
        word |= (u64)(have == value) << (c - c0);
    }
    return word;
}

// ---- the launch geometry of the pair kernel: 64 x 64 path pairs per tile, tile row <= tile column, chunks of class words
constexpr u32 TILE = 64, STAGE_WORDS = 32, MIN_CHUNK_WORDS = 64, MAX_WORKGROUPS = 8192;
struct Plan { u64 tiles, tile_pairs, row_words, chunk_words, chunks; };

// chunk_words is MIN_CHUNK_WORDS until that would make more than MAX_WORKGROUPS workgroups; then the chunks grow, in steps
// of MIN_CHUNK_WORDS, and a lane's 32-bit sums hold a chunk of up to 2^26 words
DIST_HD Plan plan(u64 K, u64 C)
{
    Plan p;
    p.tiles = (K + TILE - 1) / TILE;
    p.tile_pairs = p.tiles * (p.tiles + 1) / 2;
    p.row_words = (C + 63) / 64;
    const u64 most = p.tile_pairs >= MAX_WORKGROUPS ? 1 : MAX_WORKGROUPS / (p.tile_pairs ? p.tile_pairs : 1);
    p.chunk_words = MIN_CHUNK_WORDS;
    if ((p.row_words + MIN_CHUNK_WORDS - 1) / MIN_CHUNK_WORDS > most)
        p.chunk_words = ((p.row_words + most - 1) / most + MIN_CHUNK_WORDS - 1) / MIN_CHUNK_WORDS * MIN_CHUNK_WORDS;
    p.chunks = (p.row_words + p.chunk_words - 1) / p.chunk_words;
    return p;
}
// tile pair q (0 <= q < tile_pairs) in row-major order over the upper triangle: its tile row and tile column
DIST_HD void tile_of(u64 tiles, u64 q, u64& tr, u64& tc)
{
    tr = 0;
    while (q >= tiles - tr) { q -= tiles - tr; tr++; }
    tc = tr + q;
}

} // namespace dist
} // namespace edsx
