// test_div_core — the per-item device code of the diversity (edsparser_amd/csrc/div_core.hpp, with ld_core.hpp's walk) as
// host code under the address and undefined-behaviour sanitizers, driven by tests/test_div_cpu.py.  Every table lives in a
// heap block of exactly its size, so that a read or write past an end is reported.
//   argv[1]: records of u64, argv[2]: the answers as u64
//   record: n_symbols, n_strings, nc, P, W, size[n_symbols], ent_off[n_symbols], cidx[nc], bits[n_strings * W],
//           col[n_symbols + 1], E_columns, WP, G, masks[G * WP], n_requests, then per request: unit, size, step
//   answer: per choice symbol: per group seg, present, then per pair diff, comp; per group the K_g + 1 bins of the spectrum;
//           per request: NW, then per window start, end, rank_first, rank_end, per group seg, present, per pair diff, comp
#include "div_core.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

using namespace edsx;
namespace dv = edsx::diversity;
typedef dv::u64 u64;

struct Reader {
    std::vector<u64> v;
    size_t at = 0;
    u64 next() { if (at >= v.size()) { std::fprintf(stderr, "short input\n"); std::exit(2); } return v[at++]; }
    std::unique_ptr<u64[]> block(size_t n) { std::unique_ptr<u64[]> b(new u64[n]); for (size_t k = 0; k < n; k++) b[k] = next(); return b; }
};

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    if (!dv::sums_fit(1ull << 20, 1ull << 21) || dv::sums_fit(1ull << 21, 1ull << 21) || dv::sums_fit(~0ull, ~0ull) || !dv::sums_fit(0, ~0ull)) return 3;
    Reader in;
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        u64 x;
        while (std::fread(&x, 8, 1, f) == 1) in.v.push_back(x);
        std::fclose(f);
    }
    std::vector<u64> out;
    while (in.at < in.v.size()) {
        const u64 n = in.next(), m = in.next(), nc = in.next(), P = in.next(), W = in.next();
        auto size = in.block(n), ent_off = in.block(n), cidx = in.block(nc), bits = in.block(m * W), col = in.block(n + 1);
        const u64 Ecol = in.next(), WP = in.next(), G = in.next();
        auto masks = in.block(G * WP);
        const u64 NP = dv::num_pairs(G), NA = dv::num_arrays(G), stride = nc + 1;
        std::unique_ptr<u64[]> K(new u64[G]), off(new u64[G + 1]);
        u64 bins = 0;
        for (u64 g = 0; g < G; g++) {
            K[g] = 0;
            for (u64 w = 0; w < WP; w++) K[g] += (u64)__builtin_popcountll(masks[g * WP + w]);
            off[g] = bins;
            bins += K[g] + 1;
        }
        off[G] = bins;
        std::unique_ptr<u64[]> arr(new u64[NA * stride]), sfs(new u64[bins]), seen(new u64[WP ? WP : 1]), c(new u64[G]), s(new u64[NP]);
        std::unique_ptr<dv::GroupSums[]> gs(new dv::GroupSums[G]);
        for (u64 k = 0; k < bins; k++) sfs[k] = 0;
        for (u64 a = 0; a < NA; a++) arr[a * stride + nc] = 0;
        for (u64 r = 0; r < nc; r++) {
            const u64 i = cidx[r], e0 = ent_off[i], sz = size[i];
            for (int pass = 0; pass < 2; pass++) {               // the second walk: the spectrum of the complete groups
                for (u64 w = 0; w < WP; w++) seen[w] = 0;
                if (pass == 0) { for (u64 g = 0; g < G; g++) gs[g] = dv::GroupSums{0, 0}; for (u64 q = 0; q < NP; q++) s[q] = 0; }
                for (u64 j = 0; j < sz; j++) {
                    for (u64 g = 0; g < G; g++) c[g] = 0;
                    for (u64 w = 0; w < WP; w++) {
                        const u64 t = ld::walk_step(bits.get() + (e0 + j) * W, (ld::u32)W, w, dv::valid_word(P, WP, w), seen[w]);
                        for (u64 g = 0; g < G; g++) c[g] += dv::group_count(t, masks[g * WP + w]);
                    }
                    if (pass == 0) {
                        for (u64 g = 0; g < G; g++) dv::add_string(gs[g], c[g]);
                        for (u64 g = 0; g < G; g++) for (u64 h = g; h < G; h++) s[dv::pair_index(G, g, h)] += c[g] * c[h];
                    } else {
                        for (u64 g = 0; g < G; g++) if (dv::sfs_counts(j, gs[g].n, K[g])) sfs[off[g] + c[g]]++;
                    }
                }
            }
            for (u64 g = 0; g < G; g++) {
                arr[dv::arr_seg(G, g) * stride + r] = dv::segregating(gs[g]);
                arr[dv::arr_present(G, g) * stride + r] = gs[g].n;
                out.push_back(dv::segregating(gs[g])); out.push_back(gs[g].n);
            }
            for (u64 g = 0; g < G; g++)
                for (u64 h = g; h < G; h++) {
                    const u64 q = dv::pair_index(G, g, h);
                    const u64 d = g == h ? dv::diff_within(gs[g].n, s[q]) : dv::diff_between(gs[g].n, gs[h].n, s[q]);
                    const u64 cm = g == h ? dv::comp_within(gs[g].n) : dv::comp_between(gs[g].n, gs[h].n);
                    arr[dv::arr_diff(G, q) * stride + r] = d;
                    arr[dv::arr_comp(G, q) * stride + r] = cm;
                }
            for (u64 q = 0; q < NP; q++) { out.push_back(arr[dv::arr_diff(G, q) * stride + r]); out.push_back(arr[dv::arr_comp(G, q) * stride + r]); }
        }
        for (u64 k = 0; k < bins; k++) out.push_back(sfs[k]);
        for (u64 a = 0; a < NA; a++) {                           // the exclusive scans
            u64 run = 0;
            for (u64 r = 0; r <= nc; r++) { const u64 v = arr[a * stride + r]; arr[a * stride + r] = run; run += v; }
        }
        const u64 nreq = in.next();
        for (u64 q = 0; q < nreq; q++) {
            const int unit = (int)in.next();
            const u64 wsize = in.next(), step = in.next();
            const u64 E = unit == dv::SYMBOLS ? nc : Ecol;
            const u64 NW = nc ? dv::window_count(E, wsize, step) : 0;
            out.push_back(NW);
            for (u64 k = 0; k < NW; k++) {
                u64 start, end;
                dv::window_bounds(k, E, wsize, step, start, end);
                const u64 r0 = dv::rank_at(unit, nc, cidx.get(), col.get(), E, start), r1 = dv::rank_at(unit, nc, cidx.get(), col.get(), E, end);
                out.push_back(start); out.push_back(end); out.push_back(r0); out.push_back(r1);
                for (u64 g = 0; g < G; g++) {
                    out.push_back(arr[dv::arr_seg(G, g) * stride + r1] - arr[dv::arr_seg(G, g) * stride + r0]);
                    out.push_back(arr[dv::arr_present(G, g) * stride + r1] - arr[dv::arr_present(G, g) * stride + r0]);
                }
                for (u64 p = 0; p < NP; p++) {
                    out.push_back(arr[dv::arr_diff(G, p) * stride + r1] - arr[dv::arr_diff(G, p) * stride + r0]);
                    out.push_back(arr[dv::arr_comp(G, p) * stride + r1] - arr[dv::arr_comp(G, p) * stride + r0]);
                }
            }
        }
    }
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    if (!out.empty()) std::fwrite(out.data(), 8, out.size(), f);
    std::fclose(f);
    return 0;
}
