// test_ibs_core.cpp — the per-item code of the shared segments on the CPU: edsparser_amd/csrc/ibs_core.hpp (what the
// k_ibs_* kernels run per lane) over a case file written by tests/test_ibs_cpu.py; meant to be built with
// -fsanitize=address,undefined.  Every table is a heap block of its own of exactly the size the header names, so the first
// entry nobody asked for is a redzone.  The scan and the stitch are emulated as the kernels run them: COUNT over every
// (tile pair, chunk) and every pair x < y of the tile, the stitch per pair over its chunk edges, one exclusive scan over
// [pair][chunk + 1], then FILL; so the seams between words and between chunks are what is checked.
//
// Records (u64, little endian):
//   0, n, m, nc, P, W, nchars; size[n], ent_off[n], str_off[m + 1], chars (nchars bytes, padded to 8), cidx[nc], bits[m * W]
//      (the EDS record of tests/cpp/test_dist_core.cpp), then K, ids[K], min_sites, min_columns, chunk_words (0: the
//      geometry of dist::plan; else chunks of that many words, so that a small EDS has many).
//      Result: C, chunks, candidate segments, segments, pair_off[K (K - 1) / 2 + 1], then seven numbers per record.
//   1, q, then q x (K, x, y).  Result: pair_index of each and pair_count(K).
#include "ibs_core.hpp"

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

enum { COUNT = 0, FILL = 1 };

struct Call {
    ibs::IbsTab t; ibs::Rule rule;
    const u64* rows; const u64* desc;
    u64 K, pairs; dist::Plan pl;
    u64 *icnt, *first, *last, *tot; ibs::Segment* out;
    u64 cand = 0;
};

// what one lane of k_ibs_scan does for one of its pairs in one chunk
void scan_pair(Call& c, int mode, u64 ra, u64 rb, u64 chunk)
{
    const u64 w0 = chunk * c.pl.chunk_words, w1 = c.pl.row_words < w0 + c.pl.chunk_words ? c.pl.row_words : w0 + c.pl.chunk_words;
    const u64 p = ibs::pair_index(c.K, ra, rb), slot = p * c.pl.chunks + chunk;
    u64 last = ibs::NONE, aux = mode == FILL ? c.tot[p * (c.pl.chunks + 1) + chunk + 1] - c.icnt[slot] : 0;
    for (u64 gw = w0; gw < w1; gw++) {
        const u64 d = c.rows[ra * c.pl.row_words + gw] ^ c.rows[rb * c.pl.row_words + gw];
        if (!d) continue;
        ibs::walk_word(c.desc, gw, d, last,
            [&](u64 r) { if (mode == COUNT) c.first[slot] = r; },
            [&](u64 r_prev, u64 r_next) {
                ibs::Segment s;
                if (!ibs::gap(c.t, r_prev, r_next, s)) return;
                if (mode == COUNT) c.cand++;
                if (!ibs::reported(c.rule, s)) return;
                if (mode == FILL) { s.x = ra; s.y = rb; c.out[aux] = s; }
                aux++;
            });
    }
    if (mode == FILL) return;
    c.icnt[slot] = aux;
    c.last[slot] = last;
    if (last == ibs::NONE) c.first[slot] = ibs::NONE;
}

void scan(Call& c, int mode)
{
    for (u64 q = 0; q < c.pl.tile_pairs; q++) {
        u64 tr, tc;
        dist::tile_of(c.pl.tiles, q, tr, tc);
        for (u64 chunk = 0; chunk < c.pl.chunks; chunk++)
            for (u64 a = 0; a < dist::TILE; a++)
                for (u64 b = 0; b < dist::TILE; b++) {
                    const u64 ra = tr * dist::TILE + a, rb = tc * dist::TILE + b;
                    if (ra < rb && rb < c.K) scan_pair(c, mode, ra, rb, chunk);
                }
    }
}

void stitch(Call& c, int mode, u64* pair_off)
{
    const u64 ch = c.pl.chunks;
    for (u64 x = 0; x < c.K; x++)
        for (u64 y = x + 1; y < c.K; y++) {
            const u64 p = ibs::pair_index(c.K, x, y);
            u64* tot = c.tot + p * (ch + 1);
            if (mode == COUNT) {
                for (u64 k = 0; k < ch; k++) tot[k] = c.icnt[p * ch + k];
                tot[ch] = 0;
            } else {
                pair_off[p] = tot[0];
                if (p + 1 == c.pairs) pair_off[c.pairs] = tot[ch + 1];
            }
            ibs::stitch(c.first + p * ch, c.last + p * ch, ch, [&](u64 k, u64 r_prev, u64 r_next) {
                ibs::Segment s;
                if (!ibs::gap(c.t, r_prev, r_next, s)) return;
                if (mode == COUNT) c.cand++;
                if (!ibs::reported(c.rule, s)) return;
                if (mode == COUNT) tot[k]++;
                else { s.x = x; s.y = y; c.out[tot[k]] = s; }
            });
        }
}

} // namespace

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: test_ibs_core cases.bin results.bin\n"); return 2; }
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
                const u64 K = r.one(), x = r.one(), y = r.one();
                put(ibs::pair_index(K, x, y)); put(ibs::pair_count(K));
            }
            continue;
        }
        if (kind != 0) { std::fprintf(stderr, "unknown record kind\n"); return 2; }
        const u64 n = r.one(), m = r.one(), nc = r.one(), P = r.one(), W = r.one(), nchars = r.one();
        u64 *size = r.block(n), *ent_off = r.block(n), *str_off = r.block(m + 1);
        uint8_t* chars = r.bytes(nchars);
        u64 *cidx = r.block(nc), *bits = r.block(m * W);
        const u64 K = r.one();
        u64* ids = r.block(K);
        const u64 min_sites = r.one(), min_columns = r.one(), chunk_words = r.one();

        // the session's tables: col over all symbols, may_miss per choice symbol, the STRINGS class list
        u64* col = heap<u64>(n + 1);
        col[0] = 0;
        for (u64 i = 0; i < n; i++) {
            u64 w = 0;
            for (u64 j = ent_off[i]; j < ent_off[i] + size[i]; j++) w = w > str_off[j + 1] - str_off[j] ? w : str_off[j + 1] - str_off[j];
            col[i + 1] = col[i] + w;
        }
        uint8_t* mm = heap<uint8_t>(nc);
        for (u64 c = 0; c < nc; c++) mm[c] = dist::may_miss(bits, (dist::u32)W, ent_off[cidx[c]], size[cidx[c]], P) ? 1 : 0;
        const dist::DistTab dt{size, ent_off, str_off, chars, cidx, nullptr, mm, nc};
        u64* cnt = heap<u64>(nc + 1);
        u64 C = 0;
        for (u64 u = 0; u < nc; u++) { cnt[u] = C; C += dist::string_count(dt, u); }
        cnt[nc] = C;
        u64* desc = heap<u64>(C);
        for (u64 u = 0; u < nc; u++) if (cnt[u + 1] != cnt[u]) dist::string_fill(dt, u, desc + cnt[u]);

        Call c;
        c.K = K; c.pairs = ibs::pair_count(K);
        c.pl = dist::plan(K, C);
        if (chunk_words) { c.pl.chunk_words = chunk_words; c.pl.chunks = (c.pl.row_words + chunk_words - 1) / chunk_words; }
        // the chosen strings of the requested paths and their bit rows
        u64* csid = heap<u64>(K * nc);
        for (u64 k = 0; k < K; k++)
            for (u64 q = 0; q < nc; q++) {
                const u64 i = cidx[q], p = ids[k];
                u64 sid = dist::NONE;
                for (u64 j = ent_off[i]; j < ent_off[i] + size[i]; j++)
                    if ((bits[j * W] & 1) || (bits[j * W + (p >> 6)] >> (p & 63) & 1)) { sid = j; break; }
                csid[k * nc + q] = sid;
            }
        u64* rows = heap<u64>(K * c.pl.row_words);
        for (u64 k = 0; k < K; k++)
            for (u64 wd = 0; wd < c.pl.row_words; wd++) rows[k * c.pl.row_words + wd] = dist::row_word(dt, dist::STRINGS, desc, C, csid + k * nc, wd);

        const u64 slots = c.pairs * c.pl.chunks, N = c.pairs * (c.pl.chunks + 1) + 1;
        c.t = ibs::IbsTab{cidx, col, n, nc};
        c.rule = ibs::Rule{min_sites, min_columns};
        c.rows = rows; c.desc = desc;
        c.icnt = heap<u64>(slots); c.first = heap<u64>(slots); c.last = heap<u64>(slots); c.tot = heap<u64>(N);
        c.out = nullptr;
        u64* pair_off = heap<u64>(c.pairs + 1);
        scan(c, COUNT);
        stitch(c, COUNT, pair_off);
        c.tot[N - 1] = 0;
        u64 total = 0;
        for (u64 k = 0; k < N; k++) { const u64 v = c.tot[k]; c.tot[k] = total; total += v; }
        c.out = heap<ibs::Segment>(total);
        for (u64 k = 0; k <= c.pairs; k++) pair_off[k] = 0;
        if (c.pairs) { scan(c, FILL); stitch(c, FILL, pair_off); }
        put(C); put(c.pl.chunks); put(c.cand); put(total);
        for (u64 k = 0; k <= c.pairs; k++) put(pair_off[k]);
        for (u64 k = 0; k < total; k++)
            for (u64 v : {c.out[k].x, c.out[k].y, c.out[k].symbol_first, c.out[k].symbol_last, c.out[k].sites, c.out[k].column_first, c.out[k].column_end})
                put(v);
        for (u64* p : {size, ent_off, str_off, cidx, bits, ids, col, cnt, desc, csid, rows, c.icnt, c.first, c.last, c.tot, pair_off}) std::free(p);
        std::free(chars); std::free(mm); std::free(c.out);
    }
    out.close();
    std::fprintf(stderr, "%zu records\n", records);
    return out ? 0 : 1;
}
