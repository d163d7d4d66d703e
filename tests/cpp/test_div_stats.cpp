// test_div_stats — the derived statistics of the diversity (edsparser_amd/host/div_stats.hpp) as the tool computes them,
// driven by tests/test_div_cpu.py, which holds every result against tests/div_spec.py bit for bit.
//   argv[1]: items of ten u64: K, seg, diff, comp, present, sites, diff_h, comp_h, diff_xy, comp_xy
//   argv[2]: per item eight u64: defined (0 | 1) and the bits of the double for pi, theta_w, tajima_d and fst (of the
//            group itself, a second group with diff_h / comp_h, and diff_xy / comp_xy between them)
#include "div_stats.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace edsparser;

static void put(std::vector<uint64_t>& out, bool defined, double v)
{
    uint64_t bits = 0;
    if (defined) std::memcpy(&bits, &v, 8);
    out.push_back(defined ? 1 : 0);
    out.push_back(bits);
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    std::vector<uint64_t> in, out;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t x;
    while (std::fread(&x, 8, 1, f) == 1) in.push_back(x);
    std::fclose(f);
    for (size_t at = 0; at + 10 <= in.size(); at += 10) {
        const uint64_t K = in[at], seg = in[at + 1], diff = in[at + 2], comp = in[at + 3], present = in[at + 4], sites = in[at + 5];
        const divstats::Harmonic h = divstats::harmonic(K);
        double pi = 0, th = 0, td = 0, pih = 0, dxy = 0, fs = 0;
        const bool has_pi = divstats::ratio(diff, comp, pi);
        put(out, has_pi, pi);
        const bool has_th = divstats::theta_w(seg, h, th), has_td = divstats::tajima_d(K, seg, diff, present, sites, h, td);
        put(out, has_th, th);
        put(out, has_td, td);
        const bool has_h = divstats::ratio(in[at + 6], in[at + 7], pih), has_xy = divstats::ratio(in[at + 8], in[at + 9], dxy);
        const bool has_fs = divstats::fst(has_pi, pi, has_h, pih, has_xy, dxy, fs);
        put(out, has_fs, fs);
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    if (!out.empty()) std::fwrite(out.data(), 8, out.size(), f);
    std::fclose(f);
    return 0;
}
