// test_mosaic_core.cpp — the per-item code of the mosaics on the CPU: edsparser_amd/csrc/mosaic_core.hpp (what k_mosaic runs)
// over a case file written by tests/test_mosaic_cpu.py; meant to be built with -fsanitize=address,undefined.  Every table is
// a heap block of its own of exactly the size the header names, so the first entry nobody asked for is a redzone.  The march
// is emulated word by word as the kernel runs it: the donors go across `lanes` lanes (1: one donor per alive bit of one
// lane, 64: a wave's worth), every lane keeps its alive words where the kernel keeps them, the donor rows are word-major
// in request order, and what a workgroup agrees on with a barrier is a loop over the lanes here.  COUNT, one exclusive scan
// over the targets, FILL.
//
// Records (u64, little endian):
//   0, n, m, nc, P, W, nchars; size[n], ent_off[n], str_off[m + 1], chars (nchars bytes, padded to 8), cidx[nc], bits[m * W]
//      (the EDS record of tests/cpp/test_dist_core.cpp), then T, targets[T], D, donors[D], lanes.
//      Result: C, segments, private segments, private symbols, target_off[T + 1], then seven numbers per record.
#include "mosaic_core.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

using namespace edsx;
using dist::u64;
using dist::u32;

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

// the workgroup of one target: what k_mosaic's lanes do, lane after lane
struct Lanes {
    const u64* rt; const u64* drow;
    u64 D, L, KW, tr;
    u64* al;                                   // KW x L, word kk of lane l at al[kk * L + l]

    bool eligible(u64 y) const { return y < D && drow[y] != tr; }
    void reset() const
    {
        for (u64 l = 0; l < L; l++)
            for (u64 kk = 0; kk < KW; kk++) {
                u64 m = 0;
                for (u32 b = 0; b < 64; b++) m |= (u64)eligible(mosaic::donor_of(kk, b, l, L)) << b;
                al[kk * L + l] = m;
            }
    }
    u64 clean(u64 l, u64 kk, u64 am, u64 w, u64 tw, u64 mask) const
    {
        u64 nm = 0;
        for (u64 x = am; x; x &= x - 1) {
            const u32 b = (u32)__builtin_ctzll(x);
            if (!mosaic::differ_word(tw, rt[w * D + mosaic::donor_of(kk, b, l, L)], mask)) nm |= 1ull << b;
        }
        return nm;
    }
    bool survive(u64 w, u64 tw, u64 mask) const
    {
        bool some = false;
        for (u64 l = 0; l < L; l++)
            for (u64 kk = 0; kk < KW; kk++) some |= clean(l, kk, al[kk * L + l], w, tw, mask) != 0;
        if (!some) return false;
        for (u64 l = 0; l < L; l++)
            for (u64 kk = 0; kk < KW; kk++) al[kk * L + l] = clean(l, kk, al[kk * L + l], w, tw, mask);
        return true;
    }
    u64 death(u64 w, u64 tw, u64 mask) const
    {
        u64 best = 0;
        for (u64 l = 0; l < L; l++)
            for (u64 kk = 0; kk < KW; kk++)
                for (u64 x = al[kk * L + l]; x; x &= x - 1) {
                    const u64 y = mosaic::donor_of(kk, (u32)__builtin_ctzll(x), l, L);
                    const u64 d = mosaic::differ_word(tw, rt[w * D + y], mask);
                    if (!d) { std::fprintf(stderr, "a survivor in death()\n"); std::exit(3); }
                    const u64 key = mosaic::death_key((u32)__builtin_ctzll(d), y);
                    best = best > key ? best : key;
                }
        return best;
    }
    bool agree(u64 w, u64 c) const
    {
        bool some = false;
        for (u64 l = 0; l < L; l++)
            for (u64 kk = 0; kk < KW; kk++) {
                u64 m = 0;
                for (u32 b = 0; b < 64; b++) {
                    const u64 y = mosaic::donor_of(kk, b, l, L);
                    if (eligible(y) && mosaic::agrees_at(rt[w * D + y], c)) m |= 1ull << b;
                }
                al[kk * L + l] = m;
                some |= m != 0;
            }
        return some;
    }
    u64 first() const
    {
        u64 y = mosaic::NONE;
        for (u64 l = 0; l < L; l++)
            for (u64 kk = 0; kk < KW; kk++) {
                const u64 am = al[kk * L + l];
                if (!am) continue;
                const u64 mine = mosaic::donor_of(kk, (u32)__builtin_ctzll(am), l, L);
                y = y < mine ? y : mine;
                break;
            }
        return y;
    }
};

} // namespace

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: test_mosaic_core cases.bin results.bin\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::ofstream out(argv[2], std::ios::binary);
    auto put = [&](u64 v) { out.write(reinterpret_cast<const char*>(&v), 8); };
    Reader r{file};
    size_t records = 0;
    while (r.at < file.size()) {
        const u64 kind = r.one();
        records++;
        if (kind != 0) { std::fprintf(stderr, "unknown record kind\n"); return 2; }
        const u64 n = r.one(), m = r.one(), nc = r.one(), P = r.one(), W = r.one(), nchars = r.one();
        u64 *size = r.block(n), *ent_off = r.block(n), *str_off = r.block(m + 1);
        uint8_t* chars = r.bytes(nchars);
        u64 *cidx = r.block(nc), *bits = r.block(m * W);
        const u64 T = r.one();
        u64* targets = r.block(T);
        const u64 D = r.one();
        u64* donors = r.block(D);
        const u64 L = r.one();

        // the session's tables: col over all symbols, may_miss per choice symbol, the STRINGS class list
        u64* col = heap<u64>(n + 1);
        col[0] = 0;
        for (u64 i = 0; i < n; i++) {
            u64 w = 0;
            for (u64 j = ent_off[i]; j < ent_off[i] + size[i]; j++) w = w > str_off[j + 1] - str_off[j] ? w : str_off[j + 1] - str_off[j];
            col[i + 1] = col[i] + w;
        }
        uint8_t* mm = heap<uint8_t>(nc);
        for (u64 c = 0; c < nc; c++) mm[c] = dist::may_miss(bits, (u32)W, ent_off[cidx[c]], size[cidx[c]], P) ? 1 : 0;
        const dist::DistTab dt{size, ent_off, str_off, chars, cidx, nullptr, mm, nc};
        u64* cnt = heap<u64>(nc + 1);
        u64 C = 0;
        for (u64 u = 0; u < nc; u++) { cnt[u] = C; C += dist::string_count(dt, u); }
        cnt[nc] = C;
        u64* desc = heap<u64>(C);
        for (u64 u = 0; u < nc; u++) if (cnt[u + 1] != cnt[u]) dist::string_fill(dt, u, desc + cnt[u]);
        const u64 RW = (C + 63) / 64;

        // one bit row per path 1..P (the device: per distinct requested path), the donor rows word-major in request order
        u64* csid = heap<u64>(nc);
        u64* rows = heap<u64>(P * RW);
        for (u64 p = 1; p <= P; p++) {
            for (u64 q = 0; q < nc; q++) {
                const u64 i = cidx[q];
                u64 sid = dist::NONE;
                for (u64 j = ent_off[i]; j < ent_off[i] + size[i]; j++)
                    if ((bits[j * W] & 1) || (bits[j * W + (p >> 6)] >> (p & 63) & 1)) { sid = j; break; }
                csid[q] = sid;
            }
            for (u64 wd = 0; wd < RW; wd++) rows[(p - 1) * RW + wd] = dist::row_word(dt, dist::STRINGS, desc, C, csid, wd);
        }
        u64* drow = heap<u64>(D);
        for (u64 y = 0; y < D; y++) drow[y] = donors[y] - 1;
        u64* rt = heap<u64>(D * RW);
        for (u64 w = 0; w < RW; w++)
            for (u64 y = 0; y < D; y++) rt[w * D + y] = rows[drow[y] * RW + w];

        const mosaic::Tab t{cidx, col, n, nc};
        const u64 KW = mosaic::alive_words(D, L);
        u64* alive = heap<u64>(KW * L);
        u64* off = heap<u64>(T + 1);
        mosaic::Segment* segs = nullptr;
        u64 total = 0, priv_segs = 0, priv_syms = 0;
        for (int mode = 0; mode < 2; mode++) {
            for (u64 x = 0; x < T; x++) {
                if (n == 0) { if (mode == 0) off[x] = 0; continue; }
                const Lanes lanes{rt, drow, D, L, KW, targets[x] - 1, alive};
                const u64 base = mode ? off[x] : 0;
                auto emit = [&](u64 k, u64 donor, u64 first, u64 end) {
                    if (mode) segs[base + k] = mosaic::segment(t, x, donor, first, end);
                };
                bool some = false;
                for (u64 y = 0; y < D; y++) some |= lanes.eligible(y);
                mosaic::March mch;
                if (some) mch = mosaic::march(t, desc, rows + lanes.tr * RW, RW, lanes, emit);
                else mosaic::close(mch, mosaic::NONE, n, emit);
                if (mode) continue;
                off[x] = mch.segments;
                priv_segs += mch.private_segments; priv_syms += mch.private_symbols;
            }
            if (mode) break;
            for (u64 x = 0; x < T; x++) { const u64 v = off[x]; off[x] = total; total += v; }
            off[T] = total;
            segs = heap<mosaic::Segment>(total);
        }
        put(C); put(total); put(priv_segs); put(priv_syms);
        for (u64 x = 0; x <= T; x++) put(off[x]);
        for (u64 k = 0; k < total; k++)
            for (u64 v : {segs[k].target, segs[k].donor, segs[k].symbol_first, segs[k].symbol_last, segs[k].sites, segs[k].column_first, segs[k].column_end})
                put(v);
        for (u64* p : {size, ent_off, str_off, cidx, bits, targets, donors, col, cnt, desc, csid, rows, drow, rt, alive, off}) std::free(p);
        std::free(chars); std::free(mm); std::free(segs);
    }
    out.close();
    std::fprintf(stderr, "%zu records\n", records);
    return out ? 0 : 1;
}
