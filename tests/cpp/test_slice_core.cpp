// test_slice_core.cpp — the per-region code of the region slice on the CPU: edsparser_amd/csrc/slice_core.hpp (what the
// k_slice_* kernels run per lane), with lift_core.hpp for the ends of path regions as on the device, over a case file
// written by tests/test_slice_cpu.py; meant to be built with -fsanitize=address,undefined.  Every table is a heap block of
// its own of exactly the size the headers name, so the first entry nobody asked for is a redzone.  Where a kernel sums
// over lanes or scans inside a wave, this program walks the strings in order; the functions are the same.
//
// Case (u64, little endian): n, m, nc, rows, W; size[n], ent_off[n], str_off[m + 1], cf[n + 1], rank[n + 1], col[n + 1],
// cc[n + 1], csid[rows * nc], S[rows * nc + 1] (the last two only when nc > 0), bits[m * W]; nr, nr x (path, start, end),
// path 0 for columns, else row + 1.
// Result: sb[m + 1] as computed from the bitsets; per region the status and, unless it is RANGE, i0 i1 o0 o1e c0 c1e
// strings chars eds_len seds_len edge_strings lo hi, then per string dst begin kept set_dst edge_slot.
#include "lift_core.hpp"
#include "slice_core.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

using namespace edsx;
using slice::u64;

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

int fail(const char* what, u64 r) { std::fprintf(stderr, "%s (region %llu)\n", what, r); return 1; }

} // namespace

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: test_slice_core cases.bin results.bin\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::ofstream out(argv[2], std::ios::binary);
    auto put = [&](u64 v) { out.write(reinterpret_cast<const char*>(&v), 8); };
    Reader r{file};
    size_t cases = 0, regions = 0;
    while (r.at < file.size()) {
        const u64 n = r.one(), m = r.one(), nc = r.one(), rows = r.one(), W = r.one();
        u64 *size = r.block(n), *ent_off = r.block(n), *str_off = r.block(m + 1), *cf = r.block(n + 1), *rank = r.block(n + 1);
        u64 *col = r.block(n + 1), *cc = r.block(n + 1);
        u64 *csid = nc ? r.block(rows * nc) : nullptr, *S = nc ? r.block(rows * nc + 1) : nullptr;
        u64* bits = r.block(m * W);
        u64* sb = static_cast<u64*>(std::malloc(8 * (m + 1)));
        if (!sb) std::abort();
        // the session table: bytes of every set, scanned
        u64 run = 0;
        for (u64 j = 0; j < m; j++) {
            u64 sum = 0;
            for (u64 w = 0; w < W; w++) sum += slice::word_bytes((slice::u32)w, w == 0 ? bits[j * W] & ~1ull : bits[j * W + w]);
            sb[j] = run;
            run += slice::set_bytes(bits[j * W] & 1, sum);
        }
        sb[m] = run;
        for (u64 j = 0; j <= m; j++) put(sb[j]);
        const lift::LiftTab lt{size, ent_off, str_off, cf, rank, csid, S, col, cc, n, nc};
        const slice::SliceTab t{size, ent_off, str_off, sb, col, n, m};
        for (u64 nr = r.one(), q = 0; q < nr; q++) {
            const u64 path = r.one(), start = r.one(), end = r.one();
            slice::Ends e;
            bool ok;
            if (path == 0) ok = slice::column_ends(t, start, end, e);
            else {
                lift::Site a, b;
                const u64 kb = (path - 1) * nc;
                const uint8_t sa = lift::find_site(lt, kb, 0, n, start, a), sb2 = lift::find_site(lt, kb, 0, n, end - 1, b);
                ok = start < end && sa == 0 && sb2 == 0;
                if (ok) slice::path_ends(a.symbol, a.offset, a.column, b.symbol, b.offset, b.column, e);
            }
            regions++;
            put(ok ? slice::OK : slice::RANGE);
            if (!ok) continue;
            u64 A = 0, B = 0;
            for (u64 j = ent_off[e.i0]; j < slice::ent_end(t, e.i0); j++) A += slice::min64(str_off[j + 1] - str_off[j], e.o0);
            for (u64 j = ent_off[e.i1]; j < slice::ent_end(t, e.i1); j++) B += slice::min64(str_off[j + 1] - str_off[j], e.o1e);
            slice::Counts c;
            slice::counts(t, e, A, B, c);
            u64 lo, hi;
            slice::copy_span(t, e, lo, hi);
            for (u64 v : {e.i0, e.i1, e.o0, e.o1e, e.c0, e.c1e, c.strings, c.chars, c.eds_len, c.seds_len, c.edge_strings, lo, hi}) put(v);
            u64 R = 0, chars = 0, last_end = 0, first_kept = slice::NONE, end_kept = 0;
            for (u64 i = e.i0; i <= e.i1; i++)
                for (u64 j = ent_off[i]; j < slice::ent_end(t, i); j++) {
                    const u64 len = str_off[j + 1] - str_off[j];
                    u64 begin, kept;
                    slice::cut(e, i, len, begin, kept);
                    if (i != e.i0 && i != e.i1 && R != A) return fail("inner strings do not have A in front of them", q);
                    const u64 d = slice::string_dst(t, e, i, j, R), slot = slice::edge_slot(t, e, i, j);
                    if (d != last_end + 1 + (i != e.i0 && j == ent_off[i] ? 1 : 0)) return fail("strings do not follow each other", q);
                    if ((slot == slice::NONE) != (i != e.i0 && i != e.i1) || (slot != slice::NONE && slot >= c.edge_strings)) return fail("edge slot", q);
                    if (kept) {
                        if (first_kept == slice::NONE) first_kept = str_off[j] + begin;
                        end_kept = str_off[j] + begin + kept;
                        if (str_off[j] + begin < lo || end_kept > hi) return fail("a kept character outside the copy span", q);
                    }
                    for (u64 v : {d, begin, kept, slice::set_dst(t, e, j), slot}) put(v);
                    last_end = d + kept;
                    R += slice::removed(e, i, len);
                    chars += kept;
                }
            if (chars != c.chars || last_end + 2 != c.eds_len) return fail("the strings do not fill the region", q);
        }
        for (u64* p : {size, ent_off, str_off, cf, rank, col, cc, csid, S, bits, sb}) std::free(p);
        cases++;
    }
    out.close();
    std::fprintf(stderr, "%zu cases, %zu regions\n", cases, regions);
    return out ? 0 : 1;
}
