// gfa_text.hpp — where every byte of the GFA text of an EDS lies, as closed forms (see gfa_device.hip).  Plain functions
// over plain arrays, compiled for the device by the kernels and for the host by tests/cpp/test_gfa_text.cpp, which runs
// them against a line-by-line writer without a GPU.
//
// Segment ids are the 1-based ranks of the non-empty strings, so the ids of a symbol, of a run of symbols and of all
// strings before one are ranges of consecutive integers, and the decimal digits of a range are a ten-step function:
//   dsum(x) = sum of digits(k) for 1 <= k <= x
// S line of id r with len characters: "S\t<r>\t<seq>\n", 4 + digits(r) + len bytes; the pool holds the strings back to back,
//   so the line of string j starts 4 * rank + dsum(rank) + str_off[j] bytes into the S lines (rank = seg_rank[j])
// L line: "L\t<u>\t+\t<v>\t+\t0M\n", 11 + digits(u) + digits(v) bytes; symbol i links u in [a, b) to v in [b, d), ordered by
//   (u, v): row u starts (u - a) * (11 * nv + Dv) + nv * (dsum(u - 1) - dsum(a - 1)) bytes into the symbol's block, with
//   nv = d - b and Dv = dsum(d - 1) - dsum(b - 1), and v lies (v - b) * (11 + digits(u)) + dsum(v - 1) - dsum(b - 1) into it
// P line: tokens "<id>+," of the non-empty chosen strings; the last ',' becomes '\t' and "*\n" follows
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define GFA_HD __host__ __device__ inline
#else
#define GFA_HD inline
#endif

namespace edsx {

typedef unsigned long long u64;
typedef unsigned int u32;

namespace gfa {

constexpr u64 NONE = ~0ull;
constexpr u32 HEADER_BYTES = 11;                       // "H\tVN:Z:1.0\n"

// decimal digits of v (1 <= v < 10^10)
GFA_HD u32 digits(u64 v)
{
    return 1u + (v >= 10ull) + (v >= 100ull) + (v >= 1000ull) + (v >= 10000ull) + (v >= 100000ull) + (v >= 1000000ull) +
           (v >= 10000000ull) + (v >= 100000000ull) + (v >= 1000000000ull);
}

// sum of digits(k) over 1 <= k <= x (x < 10^10): every k >= 10^p adds one digit
GFA_HD u64 dsum(u64 x)
{
    u64 s = 0, p = 1;
    for (int k = 0; k < 10; k++) {
        if (x >= p) s += x - p + 1;
        p *= 10;
    }
    return s;
}

// the decimal digits of v, least significant in the lowest nibble
GFA_HD u64 bcd(u64 v)
{
    u64 r = 0;
    for (u32 k = 0; k < 40 && v; k += 4) { r |= (v % 10ull) << k; v /= 10ull; }
    return r;
}
// character t (0: most significant) of the d digits held in b
GFA_HD u32 digit_char(u64 b, u32 d, u32 t) { return '0' + (u32)((b >> (4u * (d - 1u - t))) & 15ull); }

// 16 bytes of text, byte k in bits 8k of lo (k < 8) or hi
struct B16 { u64 lo, hi; };
GFA_HD void put(B16& x, u32 k, u32 c)
{
    if (k < 8) x.lo |= (u64)c << (8u * k);
    else x.hi |= (u64)c << (8u * (k - 8u));
}

// ---- S lines -------------------------------------------------------------------------------------------------------
struct SegTab { const u64* seg_rank; const u64* str_off; const u32* elen; const uint8_t* chars; u64 m; };

GFA_HD u64 seg_off(const SegTab& t, u64 j)              // 0 <= j <= m; [m]: all S bytes
{
    const u64 r = t.seg_rank[j];
    return 4 * r + dsum(r) + t.str_off[j];
}

// the last j in [lo, hi] with seg_off(j) <= o (seg_off(lo) <= o); for o inside the S lines and hi = m - 1 a non-empty string
GFA_HD u64 seg_find(const SegTab& t, u64 lo, u64 hi, u64 o)
{
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo + 1) >> 1);
        if (seg_off(t, mid) <= o) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Bytes [o, o + nb) of the S lines (nb <= 16, all inside them); the string of o lies in [jlo, jhi].  When the whole chunk
// is sequence of one string, nothing is assembled: true, and `pool` says where the 16 characters lie in the pool.
GFA_HD bool seg_chunk(const SegTab& t, u64 jlo, u64 jhi, u64 o, u32 nb, B16& out, u64& pool)
{
    u64 j = seg_find(t, jlo, jhi, o);
    u64 s0 = seg_off(t, j), id = t.seg_rank[j] + 1, len = t.elen[j], dg = bcd(id);
    u32 d = digits(id);
    {
        const u64 rel = o - s0, h = 3 + d;
        if (nb == 16 && rel >= h && rel + 16 <= h + len) { pool = t.str_off[j] + (rel - h); return true; }
    }
    out.lo = out.hi = 0;
    for (u32 b = 0; b < nb; b++) {
        u64 rel = o + b - s0;
        if (rel >= 4 + d + len) {                                   // the next line starts here
            s0 += 4 + d + len;
            do j++; while (j + 1 < t.m && t.elen[j] == 0);
            id = t.seg_rank[j] + 1; len = t.elen[j]; dg = bcd(id); d = digits(id);
            rel = 0;
        }
        u32 c;
        if (rel == 0) c = 'S';
        else if (rel == 1 || rel == 2 + d) c = '\t';
        else if (rel < 2 + d) c = digit_char(dg, d, (u32)rel - 2);
        else if (rel < 3 + d + len) c = t.chars[t.str_off[j] + (rel - 3 - d)];
        else c = '\n';
        put(out, b, c);
    }
    return false;
}

// ---- L lines -------------------------------------------------------------------------------------------------------
// per symbol i: its segments are the ids [seg_rank[e0] + 1, seg_rank[e1] + 1) (e0 = ent_off[i], e1 = e0 + size[i]); it links
// them to the ids [seg_rank[e1] + 1, vend[i]); loff[i]: where its lines start (n + 1 entries)
struct LinkTab { const u64* size; const u64* ent_off; const u64* seg_rank; const u64* vend; const u64* loff; u64 n; };

// bytes of the links u in [a, b) x v in [c, d)
GFA_HD u64 link_block_bytes(u64 a, u64 b, u64 c, u64 d)
{
    if (a >= b || c >= d) return 0;
    return (d - c) * (dsum(b - 1) - dsum(a - 1)) + (b - a) * (dsum(d - 1) - dsum(c - 1)) + 11 * (b - a) * (d - c);
}

struct Link { u64 u, v, start, b, c, d; };              // line u -> v starts at `start`; its symbol's u end at b, its v are [c, d)

// the link whose line holds byte o of the L lines; its symbol lies in [ilo, ihi]
GFA_HD Link link_at(const LinkTab& t, u64 ilo, u64 ihi, u64 o)
{
    u64 lo = ilo, hi = ihi;
    while (lo < hi) {                                               // the last i with loff[i] <= o: the one with bytes there
        const u64 mid = lo + ((hi - lo + 1) >> 1);
        if (t.loff[mid] <= o) lo = mid; else hi = mid - 1;
    }
    const u64 i = lo, e0 = t.ent_off[i], e1 = e0 + t.size[i];
    const u64 a = t.seg_rank[e0] + 1, b = t.seg_rank[e1] + 1, c = b, d = t.vend[i];
    const u64 nv = d - c, Dc = dsum(c - 1), Dv = dsum(d - 1) - Dc, Da = dsum(a - 1), row = 11 * nv + Dv, rel = o - t.loff[i];
    lo = a; hi = b - 1;
    while (lo < hi) {                                               // the last u whose row starts at or before rel
        const u64 mid = lo + ((hi - lo + 1) >> 1);
        if ((mid - a) * row + nv * (dsum(mid - 1) - Da) <= rel) lo = mid; else hi = mid - 1;
    }
    const u64 u = lo, ro = (u - a) * row + nv * (dsum(u - 1) - Da), r2 = rel - ro, per = 11 + digits(u);
    lo = c; hi = d - 1;
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo + 1) >> 1);
        if ((mid - c) * per + dsum(mid - 1) - Dc <= r2) lo = mid; else hi = mid - 1;
    }
    const u64 v = lo;
    return Link{u, v, t.loff[i] + ro + (v - c) * per + dsum(v - 1) - Dc, b, c, d};
}

// bytes [o, o + nb) of the L lines (nb <= 16, all inside them)
GFA_HD B16 link_chunk(const LinkTab& t, u64 ilo, u64 ihi, u64 o, u32 nb)
{
    Link k = link_at(t, ilo, ihi, o);
    u32 du = digits(k.u), dv = digits(k.v);
    u64 bu = bcd(k.u), bv = bcd(k.v);
    B16 out{0, 0};
    for (u32 b = 0; b < nb; b++) {
        u64 rel = o + b - k.start;
        if (rel >= 11 + du + dv) {                                  // the next line: the next v, the next u, or the next symbol
            k.start += 11 + du + dv;
            if (++k.v == k.d) {
                k.v = k.c;
                if (++k.u == k.b) k = link_at(t, ilo, ihi, o + b);
                du = digits(k.u); bu = bcd(k.u);
            }
            dv = digits(k.v); bv = bcd(k.v);
            rel = 0;
        }
        const u32 r = (u32)rel;
        u32 c;
        if (r == 0) c = 'L';
        else if (r == 1 || r == 2 + du || r == 4 + du) c = '\t';
        else if (r < 2 + du) c = digit_char(bu, du, r - 2);
        else if (r == 3 + du) c = '+';
        else if (r < 5 + du + dv) c = digit_char(bv, dv, r - 5 - du);
        else {
            const u32 q = r - 5 - du - dv;                          // "\t+\t0M\n"
            c = q == 0 || q == 2 ? '\t' : q == 1 ? '+' : q == 3 ? '0' : q == 4 ? 'M' : '\n';
        }
        put(out, b, c);
    }
    return out;
}

// ---- P lines -------------------------------------------------------------------------------------------------------
// The token text of a path: symbol i's token starts at ct[i] + (TS[kb + rank[i]] - TS[kb]) (ct: the token bytes of the
// fixed symbols before i, n + 1 entries; rank: the choice symbols before i, n + 1 entries; TS: the scanned token bytes of
// the table rows, kb = row * nc).  csid: the chosen string of every (row, choice symbol).
struct WalkTab { const u64* ent_off; const u64* seg_rank; const u64* ct; const u64* rank; const u64* csid; const u64* TS; u64 n, nc; };

GFA_HD u64 walk_pos(const WalkTab& a, u64 kb, u64 i) { return a.ct[i] + (a.nc ? a.TS[kb + a.rank[i]] - a.TS[kb] : 0); }

GFA_HD u64 walk_id(const WalkTab& a, u64 kb, u64 i)     // of a symbol that has a token
{
    const u64 r = a.rank[i];
    return a.seg_rank[a.rank[i + 1] != r ? a.csid[kb + r] : a.ent_off[i]] + 1;
}

// Bytes [o, o + nb) of the body of a P line with T > 0 token bytes (nb <= 16, o + nb <= T + 2): the tokens, the last comma
// as a tab, then "*\n".  The symbol of o (when o < T) lies in [ilo, ihi].
GFA_HD B16 walk_chunk(const WalkTab& a, u64 kb, u64 ilo, u64 ihi, u64 T, u64 o, u32 nb)
{
    B16 out{0, 0};
    u64 i = 0, start = 0, end = 0, dg = 0;
    u32 d = 0;
    if (o < T) {
        u64 lo = ilo, hi = ihi;
        while (lo < hi) {                                           // the last i with walk_pos(i) <= o: the one with bytes there
            const u64 mid = lo + ((hi - lo + 1) >> 1);
            if (walk_pos(a, kb, mid) <= o) lo = mid; else hi = mid - 1;
        }
        i = lo; start = walk_pos(a, kb, i); end = walk_pos(a, kb, i + 1);
        d = (u32)(end - start) - 2; dg = bcd(walk_id(a, kb, i));
    }
    for (u32 b = 0; b < nb; b++) {
        const u64 q = o + b;
        u32 c;
        if (q >= T) c = q == T ? '*' : '\n';
        else {
            if (q >= end) {
                do { i++; start = end; end = walk_pos(a, kb, i + 1); } while (q >= end);
                d = (u32)(end - start) - 2; dg = bcd(walk_id(a, kb, i));
            }
            const u32 r = (u32)(q - start);
            c = r < d ? digit_char(dg, d, r) : r == d ? '+' : q + 1 == T ? '\t' : ',';
        }
        put(out, b, c);
    }
    return out;
}

} // namespace gfa
} // namespace edsx
