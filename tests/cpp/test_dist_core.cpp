// test_dist_core.cpp — the per-descriptor code of the path distances on the CPU: edsparser_amd/csrc/dist_core.hpp (what the
// k_dist_* kernels run per lane) over a case file written by tests/test_dist_cpu.py; meant to be built with
// -fsanitize=address,undefined.  Every table is a heap block of its own of exactly the size the header names, so the first
// entry nobody asked for is a redzone.  Where a kernel scans, this program walks the units in order; the functions are
// the same.
//
// Records (u64, little endian), each led by its kind:
//   0  an EDS: n, m, nc, P, W, nchars; size[n], ent_off[n], str_off[m + 1], chars (nchars bytes, padded to 8), cidx[nc],
//      bits[m * W].  Result: may_miss[nc], ccol[nc + 1]; then per metric (COLUMNS, STRINGS) V, C, desc[C], and the bit rows
//      of the paths 1..P, ceil(C / 64) words each.  The chosen strings come from the session's rule, restated here.
//   1  descriptors as numbers: q, then q x (unit, value, r, index).  Result per entry: the packed column descriptor, its
//      unit and value again, the packed string descriptor, its r and index again.
//   2  a ccol table as numbers: nc, ccol[nc + 1], q, q units.  Result: unit_symbol of each.
//   3  geometry: K, C, q, q tile pairs.  Result: tiles, tile_pairs, row_words, chunk_words, chunks, then (tr, tc) of each.
//   4  a present mask: q bytes that are present, then 256 x (has, rank).
#include "dist_core.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

using namespace edsx;
using dist::u64;

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
    uint8_t* bytes(u64 count)
    {
        uint8_t* p = static_cast<uint8_t*>(std::malloc(count ? count : 1));
        if (!p) std::abort();
        if (at + count > f.size()) { std::fprintf(stderr, "case file cut short\n"); std::exit(2); }
        std::memcpy(p, f.data() + at, count);
        at += (count + 7) / 8 * 8;
        return p;
    }
};

template <class T> T* heap(u64 count)
{
    T* p = static_cast<T*>(std::malloc(count ? sizeof(T) * count : 1));
    if (!p) std::abort();
    return p;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: test_dist_core cases.bin results.bin\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::ofstream out(argv[2], std::ios::binary);
    auto put = [&](u64 v) { out.write(reinterpret_cast<const char*>(&v), 8); };
    Reader r{file};
    size_t records = 0;
    while (r.at < file.size()) {
        const u64 kind = r.one();
        records++;
        if (kind == 1) {
            for (u64 q = r.one(); q; q--) {
                const u64 unit = r.one(), value = r.one(), rank = r.one(), index = r.one();
                u64 u2, r2, i2;
                dist::u32 v2;
                const u64 dc = dist::pack_column(unit, (dist::u32)value), ds = dist::pack_string(rank, index);
                dist::unpack_column(dc, u2, v2);
                dist::unpack_string(ds, r2, i2);
                for (u64 v : {dc, u2, (u64)v2, ds, r2, i2}) put(v);
            }
            continue;
        }
        if (kind == 2) {
            const u64 nc = r.one();
            u64* ccol = r.block(nc + 1);
            const dist::DistTab t{nullptr, nullptr, nullptr, nullptr, nullptr, ccol, nullptr, nc};
            for (u64 q = r.one(); q; q--) put(dist::unit_symbol(t, r.one()));
            std::free(ccol);
            continue;
        }
        if (kind == 3) {
            const u64 K = r.one(), C = r.one();
            const dist::Plan p = dist::plan(K, C);
            for (u64 v : {p.tiles, p.tile_pairs, p.row_words, p.chunk_words, p.chunks}) put(v);
            for (u64 q = r.one(); q; q--) {
                u64 tr, tc;
                dist::tile_of(p.tiles, r.one(), tr, tc);
                put(tr); put(tc);
            }
            continue;
        }
        if (kind == 4) {
            dist::Present m;
            dist::present_clear(m);
            for (u64 q = r.one(); q; q--) dist::present_add(m, (dist::u32)r.one());
            put(dist::present_count(m));
            for (dist::u32 b = 0; b < 256; b++) { put(dist::present_has(m, b)); put(dist::present_rank(m, b)); }
            continue;
        }
        if (kind != 0) { std::fprintf(stderr, "unknown record kind\n"); return 2; }
        const u64 n = r.one(), m = r.one(), nc = r.one(), P = r.one(), W = r.one(), nchars = r.one();
        u64 *size = r.block(n), *ent_off = r.block(n), *str_off = r.block(m + 1);
        uint8_t* chars = r.bytes(nchars);
        u64 *cidx = r.block(nc), *bits = r.block(m * W);
        uint8_t* mm = heap<uint8_t>(nc);
        u64* ccol = heap<u64>(nc + 1);
        u64 run = 0;
        for (u64 c = 0; c < nc; c++) {
            const u64 i = cidx[c];
            u64 w = 0;
            for (u64 j = ent_off[i]; j < ent_off[i] + size[i]; j++) w = w > str_off[j + 1] - str_off[j] ? w : str_off[j + 1] - str_off[j];
            mm[c] = dist::may_miss(bits, (dist::u32)W, ent_off[i], size[i], P) ? 1 : 0;
            ccol[c] = run;
            run += w;
        }
        ccol[nc] = run;
        for (u64 c = 0; c < nc; c++) put(mm[c]);
        for (u64 c = 0; c <= nc; c++) put(ccol[c]);
        const dist::DistTab t{size, ent_off, str_off, chars, cidx, ccol, mm, nc};
        // the chosen strings: the first string of the symbol whose set holds p or 0
        u64* csid = heap<u64>(P * nc);
        for (u64 p = 1; p <= P; p++)
            for (u64 c = 0; c < nc; c++) {
                const u64 i = cidx[c];
                u64 sid = dist::NONE;
                for (u64 j = ent_off[i]; j < ent_off[i] + size[i]; j++)
                    if ((bits[j * W] & 1) || (bits[j * W + (p >> 6)] >> (p & 63) & 1)) { sid = j; break; }
                csid[(p - 1) * nc + c] = sid;
            }
        for (dist::Metric metric : {dist::COLUMNS, dist::STRINGS}) {
            const u64 U = metric == dist::STRINGS ? nc : ccol[nc];
            u64* cnt = heap<u64>(U + 1);
            u64 C = 0, V = 0;
            for (u64 u = 0; u < U; u++) {
                u64 c;
                if (metric == dist::STRINGS) c = dist::string_count(t, u);
                else {
                    const u64 s = dist::unit_symbol(t, u);
                    dist::Present pm;
                    bool nochar;
                    dist::column_classes(t, s, u - ccol[s], pm, nochar);
                    c = dist::column_count(pm, nochar);
                }
                cnt[u] = C;
                C += c;
                V += c ? 1 : 0;
            }
            cnt[U] = C;
            u64* desc = heap<u64>(C);
            for (u64 u = 0; u < U; u++) {
                if (cnt[u + 1] == cnt[u]) continue;
                if (metric == dist::STRINGS) dist::string_fill(t, u, desc + cnt[u]);
                else {
                    const u64 s = dist::unit_symbol(t, u);
                    dist::Present pm;
                    bool nochar;
                    dist::column_classes(t, s, u - ccol[s], pm, nochar);
                    dist::column_fill(pm, nochar, u, desc + cnt[u]);
                }
            }
            put(V); put(C);
            for (u64 c = 0; c < C; c++) put(desc[c]);
            const u64 words = (C + 63) / 64;
            for (u64 p = 0; p < P; p++)
                for (u64 wd = 0; wd < words; wd++) put(dist::row_word(t, metric, desc, C, csid + p * nc, wd));
            std::free(cnt); std::free(desc);
        }
        for (u64* p : {size, ent_off, str_off, cidx, bits, ccol, csid}) std::free(p);
        std::free(chars); std::free(mm);
    }
    out.close();
    std::fprintf(stderr, "%zu records\n", records);
    return out ? 0 : 1;
}
