// vcf_text.hpp — where every byte of a VCF record of an EDS lies (see vcf_export_device.hip, include/edsx.h "eds2vcf").
// Plain functions over plain arrays, compiled for the device by the kernels and for the host by
// tests/cpp/test_vcf_text.cpp, which runs them against tests/vcf_export_spec.py without a GPU.
//
// A record is a symbol with two strings or more.  Its line is a FIXED PART
//   <chrom> \t <POS> \t . \t <REF> \t <ALT1>,<ALT2>,... \t . \t . \t . [\t GT]
// followed, with sources, by one CELL per path 1..P, "\t" and the numbers of the alleles the path takes joined by '/'
// ("." when it takes none), and a line feed.  Allele 0 is the reference string (index r among the symbol's strings), the
// others follow in file order: allele a is string r (a == 0), a - 1 (a <= r) or a (a > r).  An anchored record (one with
// an empty string) carries one reference base in front of every allele, or behind it when the record lies at position 1.
// The strings of a symbol lie back to back in the pool, so allele a starts
//   A(a) = (reflen + anc + 1) + (characters of the strings before it, less the reference) + (a - 1) * (anc + 1)
// bytes into the alleles (A(0) = 0): the fixed part's length is a closed form and any byte of it is found by bisection
// over a, which is what lets a record with one very long allele spread over many lanes.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define VCF_HD __host__ __device__ inline
#else
#define VCF_HD inline
#endif

namespace edsx {

typedef unsigned long long u64;
typedef unsigned int u32;

namespace vcf {

constexpr u64 NONE = ~0ull;
constexpr u32 TILE_PATHS = 256;                        // path ids [256 t, 256 t + 256) form tile t: four bitset words

// decimal digits of v (v >= 0; 0 has one)
VCF_HD u32 digits(u64 v)
{
    u32 d = 1;
    while (v >= 10ull) { v /= 10ull; d++; }
    return d;
}
// character t (0: most significant) of the d digits of v
VCF_HD u32 digit_char(u64 v, u32 d, u32 t)
{
    for (u32 k = t + 1; k < d; k++) v /= 10ull;
    return '0' + (u32)(v % 10ull);
}

// 16 bytes of text, byte k in bits 8k of lo (k < 8) or hi
struct B16 { u64 lo, hi; };
VCF_HD void put(B16& x, u32 k, u32 c)
{
    if (k < 8) x.lo |= (u64)c << (8u * k);
    else x.hi |= (u64)c << (8u * (k - 8u));
}

// anchor word of a symbol: 0 = not anchored, else the base in bits 8.., ANC_FRONT or ANC_BACK below
constexpr u64 ANC_FRONT = 1, ANC_BACK = 2;

struct Tab {
    const u64* size; const u64* ent_off; const u64* str_off; const uint8_t* chars;
    const u64* bits; u32 W;                            // null / 0 without sources
    const u64* refidx;                                 // per symbol: index of its reference string among its strings
    const u64* refpos;                                 // n + 1: where the symbol's reference string begins in the reference
    const u64* anchor;                                 // per symbol: the anchor word
    u64 n, P;
    const uint8_t* chrom; u32 chrom_len; u32 with_gt;
};

struct Rec {
    u64 e0, k, r, reflen, sum, pos;                    // first string, strings, reference index, characters of all strings, POS
    u32 anc, back, base;                               // anchored (0 / 1), the base goes behind the alleles, the base
};

VCF_HD Rec rec_of(const Tab& t, u64 i)
{
    Rec c;
    c.e0 = t.ent_off[i]; c.k = t.size[i]; c.r = t.refidx[i];
    c.reflen = t.str_off[c.e0 + c.r + 1] - t.str_off[c.e0 + c.r];
    c.sum = t.str_off[c.e0 + c.k] - t.str_off[c.e0];
    const u64 a = t.anchor[i];
    c.anc = a ? 1u : 0u; c.back = (a & 3) == ANC_BACK; c.base = (u32)(a >> 8);
    c.pos = a ? (c.back ? 1 : t.refpos[i]) : t.refpos[i] + 1;
    return c;
}

// bytes of the alleles with their separators: REF \t ALT , ALT ... \t
VCF_HD u64 allele_bytes(const Rec& c) { return c.sum + c.k * (c.anc + 1); }

// the fixed part; nl: the line feed belongs to it (no cell follows)
VCF_HD u64 fixed_bytes(const Tab& t, const Rec& c, bool nl)
{
    return t.chrom_len + 1 + digits(c.pos) + 3 + allele_bytes(c) + 5 + (t.with_gt ? 3 : 0) + (nl ? 1 : 0);
}

// string (index among the symbol's) of allele a, 0 <= a < k
VCF_HD u64 allele_string(const Rec& c, u64 a) { return a == 0 ? c.r : (a <= c.r ? a - 1 : a); }

// where allele a begins among the alleles, 0 <= a <= k
VCF_HD u64 allele_start(const Tab& t, const Rec& c, u64 a)
{
    if (a == 0) return 0;
    const u64 j = a <= c.r ? a - 1 : a;                                   // (a == k: behind the last string)
    const u64 before = t.str_off[c.e0 + j] - t.str_off[c.e0] - (j > c.r ? c.reflen : 0);
    return c.reflen + c.anc + 1 + before + (a - 1) * (c.anc + 1);
}

// Byte x of the alleles.  When it is a character of a string: true, pool = where it lies in the pool and room = the
// characters of that string from there on; else false and ch = the byte.
VCF_HD bool allele_byte(const Tab& t, const Rec& c, u64 x, u64& pool, u64& room, u32& ch)
{
    u64 lo = 0, hi = c.k - 1;
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo + 1) >> 1);
        if (allele_start(t, c, mid) <= x) lo = mid; else hi = mid - 1;
    }
    const u64 a = lo, j = allele_string(c, a), s0 = t.str_off[c.e0 + j], len = t.str_off[c.e0 + j + 1] - s0;
    u64 y = x - allele_start(t, c, a);
    if (c.anc && !c.back) { if (y == 0) { ch = c.base; return false; } y--; }
    if (y < len) { pool = s0 + y; room = len - y; return true; }
    y -= len;
    if (c.anc && c.back) { if (y == 0) { ch = c.base; return false; } y--; }
    ch = (a == 0 || a == c.k - 1) ? '\t' : ',';
    return false;
}

// byte x of the fixed part
VCF_HD u32 fixed_byte(const Tab& t, const Rec& c, u64 x)
{
    if (x < t.chrom_len) return t.chrom[x];
    x -= t.chrom_len;
    if (x == 0) return '\t';
    x--;
    const u32 d = digits(c.pos);
    if (x < d) return digit_char(c.pos, d, (u32)x);
    x -= d;
    if (x < 3) return x == 1 ? '.' : '\t';
    x -= 3;
    const u64 ab = allele_bytes(c);
    if (x < ab) {
        u64 pool, room;
        u32 ch;
        return allele_byte(t, c, x, pool, room, ch) ? t.chars[pool] : ch;
    }
    x -= ab;
    if (x < 5) return (x & 1) ? '\t' : '.';
    x -= 5;
    if (t.with_gt && x < 3) return x == 0 ? '\t' : (x == 1 ? 'G' : 'T');
    return '\n';
}

// Bytes [o, o + nb) of the fixed part (nb <= 16, all inside it).  When the whole chunk is characters of one string nothing
// is assembled: true, and `pool` says where the characters lie in the pool (which ends in 16 bytes of slack).
VCF_HD bool fixed_chunk(const Tab& t, const Rec& c, u64 o, u32 nb, B16& x, u64& pool)
{
    x.lo = 0; x.hi = 0;
    const u64 pre = t.chrom_len + 1 + digits(c.pos) + 3;
    if (o >= pre && o + nb <= pre + allele_bytes(c)) {
        u64 room;
        u32 ch;
        if (allele_byte(t, c, o - pre, pool, room, ch) && room >= nb) return true;
    }
    for (u32 b = 0; b < nb; b++) put(x, b, fixed_byte(t, c, o + b));
    return false;
}

// ---- cells ---------------------------------------------------------------------------------------------------------
// the paths of word w that take string j (absolute index): its set, or all of them when it holds 0
VCF_HD u64 cell_word(const Tab& t, u64 j, u32 w) { return t.bits[j * t.W + w] | (0ull - (t.bits[j * t.W] & 1ull)); }

// bytes of the cell of path 64 w + l, the tab in front included
VCF_HD u32 cell_bytes(const Tab& t, const Rec& c, u32 w, u32 l)
{
    u32 nb = 0;
    for (u64 a = 0; a < c.k; a++)
        if ((cell_word(t, c.e0 + allele_string(c, a), w) >> l) & 1ull) nb += 1 + digits(a);     // '\t' or '/' and the number
    return nb ? nb : 2;
}

// writes the cell (cell_bytes of them) to dst
VCF_HD void cell_write(const Tab& t, const Rec& c, u32 w, u32 l, uint8_t* dst)
{
    u32 nb = 0;
    for (u64 a = 0; a < c.k; a++)
        if ((cell_word(t, c.e0 + allele_string(c, a), w) >> l) & 1ull) {
            dst[nb] = nb ? '/' : '\t';
            nb++;
            const u32 d = digits(a);
            for (u32 q = 0; q < d; q++) dst[nb++] = (uint8_t)digit_char(a, d, q);
        }
    if (!nb) { dst[0] = '\t'; dst[1] = '.'; }
}

// ---- reference FASTA -------------------------------------------------------------------------------------------------
// the last i in [lo, hi] with refpos[i] <= q (refpos[lo] <= q); for q < refpos[n] and hi = n - 1 the symbol whose
// reference string holds character q
VCF_HD u64 ref_find(const u64* refpos, u64 lo, u64 hi, u64 q)
{
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo + 1) >> 1);
        if (refpos[mid] <= q) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// character q of the reference (q < refpos[n])
VCF_HD u32 ref_char(const Tab& t, u64 q)
{
    const u64 i = ref_find(t.refpos, 0, t.n - 1, q);
    return t.chars[t.str_off[t.ent_off[i] + t.refidx[i]] + (q - t.refpos[i])];
}

} // namespace vcf
} // namespace edsx
