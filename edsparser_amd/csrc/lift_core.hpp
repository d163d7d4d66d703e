// lift_core.hpp — the per-query code of the coordinate lift (path_device.hip): the search step over the
// sequence offsets of the symbols on one path, the site of a found symbol, and the place of a site on a path.  Plain
// functions over plain arrays, as vcf_walk.hpp and gfa_text.hpp: hipcc compiles them into k_lift_find / k_lift_place,
// and g++ compiles them for tests/cpp/test_lift_core.cpp, which runs them on heap tables of exactly the sizes below under
// the address and undefined-behaviour sanitizers.
//
// The tables (LiftTab) and their sizes, in entries of 8 bytes: size, ent_off: n; str_off: m + 1; cf, rank, col, cc:
// n + 1; csid: rows * nc; S: rows * nc + 1 (both null when nc == 0).  kb = row * nc is the first cell of a path's row.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define LIFT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LIFT_HD inline __attribute__((always_inline))
#endif

namespace edsx {
namespace lift {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr u64 NONE = ~0ull;
enum : uint8_t { SAME = 0, ALIGNED = 1, GAP = 2, MISSING = 3, RANGE = 4 };

// symbol, local string index, offset in the string, alignment column, common position (NONE inside a degenerate symbol)
struct Site { u64 symbol, string, offset, column, common_pos; };

struct LiftTab {
    const u64* size; const u64* ent_off; const u64* str_off;
    const u64* cf; const u64* rank;            // fixed characters / choice symbols in front of symbol i
    const u64* csid; const u64* S;             // chosen string per (row, choice symbol); its scanned lengths
    const u64* col; const u64* cc;             // first alignment column / common characters in front of symbol i
    u64 n, nc;
};

// sequence offset of symbol i (0 <= i <= n) on the path of row kb / nc; i == n: the length of the path
LIFT_HD u64 sym_pos(const LiftTab& t, u64 kb, u64 i)
{
    return t.cf[i] + (t.nc ? t.S[kb + t.rank[i]] - t.S[kb] : 0);
}

// the string the path takes in symbol i < n (a global string number), NONE when it takes none
LIFT_HD u64 chosen(const LiftTab& t, u64 kb, u64 i)
{
    const u64 r = t.rank[i];
    return t.rank[i + 1] != r ? t.csid[kb + r] : t.ent_off[i];
}

// largest i in [lo, hi) with sym_pos(i) <= x, given sym_pos(lo) <= x: the offsets ascend, runs of symbols that add
// nothing to the path share one, and the last of a run is the answer
LIFT_HD u64 search(const LiftTab& t, u64 kb, u64 lo, u64 hi, u64 x)
{
    while (hi - lo > 1) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (sym_pos(t, kb, mid) <= x) lo = mid; else hi = mid;
    }
    return lo;
}

LIFT_HD void no_site(Site& s) { s.symbol = s.string = s.offset = s.column = s.common_pos = NONE; }

// the site of character x of the path, i the symbol search() found for x < sym_pos(n)
LIFT_HD void site_at(const LiftTab& t, u64 kb, u64 i, u64 x, Site& s)
{
    const u64 o = x - sym_pos(t, kb, i);
    s.symbol = i;
    s.string = chosen(t, kb, i) - t.ent_off[i];
    s.offset = o;
    s.column = t.col[i] + o;
    s.common_pos = t.size[i] == 1 ? t.cc[i] + o : NONE;
}

// site of (row, x): 0, or RANGE with every field NONE when the path has no character x
LIFT_HD uint8_t find_site(const LiftTab& t, u64 kb, u64 lo, u64 hi, u64 x, Site& s)
{
    if (t.n == 0 || x >= sym_pos(t, kb, t.n)) { no_site(s); return RANGE; }
    site_at(t, kb, search(t, kb, lo, hi, x), x, s);
    return 0;
}

// where (symbol i, string j, offset o) lies on the path of the row
LIFT_HD uint8_t place(const LiftTab& t, u64 kb, u64 i, u64 j, u64 o, u64& pos)
{
    pos = NONE;
    if (i >= t.n || j >= t.size[i]) return RANGE;
    const u64 e0 = t.ent_off[i], sj = e0 + j;
    if (o >= t.str_off[sj + 1] - t.str_off[sj]) return RANGE;
    const u64 start = sym_pos(t, kb, i), c = chosen(t, kb, i);
    if (c == NONE) { pos = start; return MISSING; }
    const u64 len = t.str_off[c + 1] - t.str_off[c];
    if (o >= len) { pos = start + len; return GAP; }
    pos = start + o;
    return c == sj ? SAME : ALIGNED;
}

} // namespace lift
} // namespace edsx
