// test_lift_core.cpp — the per-query code of the coordinate lift on the CPU: edsparser_amd/csrc/lift_core.hpp (what
// k_lift_find and k_lift_place run per lane) over a case file written by tests/test_lift_cpu.py; meant to be built with
// -fsanitize=address,undefined.  Every table is a heap block of its own of exactly the size the header names, so the
// first entry nobody asked for is a redzone.  The search runs twice per query: over all symbols, and inside the stretch a
// sampled table of TOP entries gives, as the kernel does with its LDS table; the two must agree.
//
// Case (u64, little endian): n, m, nc, rows, top; size[n], ent_off[n], str_off[m + 1], cf[n + 1], rank[n + 1], col[n + 1],
// cc[n + 1], csid[rows * nc], S[rows * nc + 1] (the last two only when nc > 0); nf, nf x (row, x); np, np x (row, i, j, o).
// Result: per find query status, symbol, string, offset, column, common_pos; per place query status, pos.
#include "lift_core.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

using namespace edsx::lift;

namespace {

struct Reader {
    const std::vector<uint8_t>& f;
    size_t at = 0;
    u64 one()
    {
        if (at + 8 > f.size()) { std::fprintf(stderr, "case file cut short\n"); std::exit(2); }
        u64 v; std::memcpy(&v, f.data() + at, 8); at += 8; return v;
    }
    u64* block(u64 count)                                   // exact size: count entries (count 0: one byte nobody reads)
    {
        u64* p = static_cast<u64*>(std::malloc(count ? 8 * count : 1));
        if (!p) std::abort();
        for (u64 k = 0; k < count; k++) p[k] = one();
        return p;
    }
};

} // namespace

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: test_lift_core cases.bin results.bin\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::ofstream out(argv[2], std::ios::binary);
    auto put = [&](u64 v) { out.write(reinterpret_cast<const char*>(&v), 8); };
    Reader r{file};
    size_t cases = 0, queries = 0;
    while (r.at < file.size()) {
        const u64 n = r.one(), m = r.one(), nc = r.one(), rows = r.one(), top = r.one();
        u64 *size = r.block(n), *ent_off = r.block(n), *str_off = r.block(m + 1), *cf = r.block(n + 1), *rank = r.block(n + 1);
        u64 *col = r.block(n + 1), *cc = r.block(n + 1);
        u64 *csid = nc ? r.block(rows * nc) : nullptr, *S = nc ? r.block(rows * nc + 1) : nullptr;
        const LiftTab t{size, ent_off, str_off, cf, rank, csid, S, col, cc, n, nc};
        const u64 stride = (n + top - 1) / top;
        std::vector<u64> tops(top);
        for (u64 nf = r.one(); nf; nf--) {
            const u64 row = r.one(), x = r.one(), kb = row * nc;
            Site a, b;
            const uint8_t sa = find_site(t, kb, 0, n, x, a);
            for (u64 j = 0; j < top; j++) tops[j] = j * stride < n ? sym_pos(t, kb, j * stride) : NONE;
            u64 lo = 0, hi = top;
            while (hi - lo > 1) { const u64 mid = (lo + hi) >> 1; if (tops[mid] <= x) lo = mid; else hi = mid; }
            const uint8_t sb = find_site(t, kb, lo * stride, lo * stride + stride < n ? lo * stride + stride : n, x, b);
            if (sa != sb || std::memcmp(&a, &b, sizeof(a))) { std::fprintf(stderr, "sampled search differs: row %llu x %llu\n", row, x); return 1; }
            put(sa); put(a.symbol); put(a.string); put(a.offset); put(a.column); put(a.common_pos);
            queries++;
        }
        for (u64 np = r.one(); np; np--) {
            const u64 row = r.one(), i = r.one(), j = r.one(), o = r.one();
            u64 pos = 0;
            const uint8_t st = place(t, row * nc, i, j, o, pos);
            put(st); put(pos);
            queries++;
        }
        for (u64* p : {size, ent_off, str_off, cf, rank, col, cc, csid, S}) std::free(p);
        cases++;
    }
    out.close();
    std::fprintf(stderr, "%zu cases, %zu queries\n", cases, queries);
    return out ? 0 : 1;
}
