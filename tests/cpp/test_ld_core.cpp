// test_ld_core — edsparser_amd/csrc/ld_core.hpp as host code, driven by tests/test_ld_cpu.py under the address and
// undefined-behaviour sanitizers.  argv[1]: a file of 64-bit little-endian numbers, records laid end to end; argv[2]: the
// answers, the same way.  Every table is copied into a heap array of exactly its size, so a read past one is found.
//   0  n m nc P W  size[n] ent_off[n] cidx[nc] bits[m * W]  WP mask[WP]  min_count all_strings  nwin window[nwin]
//        the two walks of k_ld_count / k_ld_rows and the tile list of k_ld_tiles / k_ld_pairs:
//        per choice symbol: present, then per string count and listed;  A;  afirst[nc + 1];  the T rows (A x WP);  per
//        choice symbol its U row (WP);  per window: per allele lo hi;  RT;  per row tile c0 c1;  NT;  per tile its row tile;
//        the pairs (x, y) that pair_valid accepts
//   1  count, then count x (n n_a n_b n_ab)
//        per item: defined, the bits of r2 (0 when undefined)
#include "ld_core.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace edsx::ld;

static std::vector<u64> in, out;
static size_t at = 0;

static u64 next()
{
    if (at >= in.size()) { std::fprintf(stderr, "the case file ends inside a record\n"); std::exit(3); }
    return in[at++];
}
static std::vector<u64> take(u64 n)
{
    std::vector<u64> v(n);
    for (u64 k = 0; k < n; k++) v[k] = next();
    return v;
}

static void eds_record()
{
    const u64 n = next(), m = next(), nc = next(), P = next(), W = next();
    const std::vector<u64> size = take(n), ent_off = take(n), cidx = take(nc), bits = take(m * W);
    const u64 WP = next();
    const std::vector<u64> mask = take(WP);
    const u64 min_count = next();
    const bool all_strings = next() != 0;
    const std::vector<u64> windows = take(next());
    if (WP != (P + 63) / 64) { std::fprintf(stderr, "WP\n"); std::exit(3); }
    std::vector<std::vector<u64>> cnt(nc);
    std::vector<u64> pres(nc), afirst(nc + 1, 0);
    for (u64 r = 0; r < nc; r++) {                               // k_ld_count
        const u64 i = cidx[r], e0 = ent_off[i], sz = size[i];
        cnt[r].assign(sz, 0);
        u64 present = 0;
        for (u64 w = 0; w < WP; w++) {
            u64 seen = 0;
            for (u64 j = 0; j < sz; j++) cnt[r][j] += (u64)__builtin_popcountll(walk_step(&bits[(e0 + j) * W], (u32)W, w, mask[w], seen));
            present += (u64)__builtin_popcountll(seen);
        }
        pres[r] = present;
        out.push_back(present);
        u64 l = 0;
        for (u64 j = 0; j < sz; j++) {
            const bool is = listed(j, all_strings, cnt[r][j], present, min_count);
            out.push_back(cnt[r][j]);
            out.push_back(is);
            l += is;
        }
        afirst[r + 1] = afirst[r] + l;
    }
    const u64 A = afirst[nc];
    out.push_back(A);
    out.insert(out.end(), afirst.begin(), afirst.end());
    std::vector<u64> trows(A * WP), urows(nc * WP), ar(A);
    for (u64 r = 0; r < nc; r++) {                               // k_ld_rows
        const u64 i = cidx[r], e0 = ent_off[i], sz = size[i];
        for (u64 w = 0; w < WP; w++) {
            u64 seen = 0, x = afirst[r];
            for (u64 j = 0; j < sz; j++) {
                const u64 t = walk_step(&bits[(e0 + j) * W], (u32)W, w, mask[w], seen);
                if (!listed(j, all_strings, cnt[r][j], pres[r], min_count)) continue;
                trows[x * WP + w] = t;
                ar[x] = r;
                x++;
            }
            urows[r * WP + w] = seen;
        }
    }
    out.insert(out.end(), trows.begin(), trows.end());
    out.insert(out.end(), urows.begin(), urows.end());
    for (const u64 window : windows) {                           // k_ld_tiles and the tile search of k_ld_pairs
        for (u64 x = 0; x < A; x++) { out.push_back(partner_lo(afirst.data(), ar[x])); out.push_back(partner_hi(afirst.data(), nc, ar[x], window)); }
        const u64 RT = (A + TILE - 1) / TILE;
        out.push_back(RT);
        std::vector<u64> tstart(RT + 1, 0);
        for (u64 t = 0; t < RT; t++) {
            u64 c0, c1;
            tile_columns(afirst.data(), nc, ar[t * TILE], ar[(A < (t + 1) * TILE ? A : (t + 1) * TILE) - 1], window, c0, c1);
            out.push_back(c0);
            out.push_back(c1);
            tstart[t + 1] = tstart[t] + (c1 - c0);
        }
        out.push_back(tstart[RT]);
        for (u64 q = 0; q < tstart[RT]; q++) out.push_back(tile_row(tstart.data(), RT, q));
        u64 valid = 0;
        for (u64 x = 0; x < A; x++)
            for (u64 y = 0; y < A; y++) valid += pair_valid(ar[x], ar[y], window);
        out.push_back(valid);
    }
}

static void r2_record()
{
    const u64 count = next();
    for (u64 k = 0; k < count; k++) {
        const u64 n = next(), n_a = next(), n_b = next(), n_ab = next();
        double v = 0;
        const bool defined = r2(n, n_a, n_b, n_ab, v);
        u64 b = 0;
        if (defined) std::memcpy(&b, &v, 8);
        out.push_back(defined);
        out.push_back(b);
    }
}

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: test_ld_core <cases> <answers>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    u64 v;
    while (std::fread(&v, 8, 1, f) == 1) in.push_back(v);
    std::fclose(f);
    while (at < in.size()) {
        const u64 kind = next();
        if (kind == 0) eds_record();
        else if (kind == 1) r2_record();
        else { std::fprintf(stderr, "unknown record %llu\n", kind); return 3; }
    }
    f = std::fopen(argv[2], "wb");
    if (!f) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    if (!out.empty() && std::fwrite(out.data(), 8, out.size(), f) != out.size()) { std::fclose(f); return 2; }
    std::fclose(f);
    return 0;
}
