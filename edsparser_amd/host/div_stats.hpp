// div_stats.hpp — the statistics derived from the integer sums of edsx_paths_diversity: pi, d_xy, Hudson's F_ST, Watterson's
// theta and Tajima's D.  Host code only, shared by edsparser-diversity, edsparser::path_diversity's callers and
// tests/cpp/test_div_stats.cpp; never compiled into a kernel.  Every function is a fixed sequence of IEEE double
// operations, written one operation per expression node below, and is built without floating-point contraction
// (-ffp-contract=off), so that tests/div_spec.py, which performs the same operations in the same order, agrees bit for bit.
// A statistic whose denominator is zero is undefined: the functions return false and the tool prints NA.
#pragma once

#include <cmath>
#include <cstdint>

namespace edsparser {
namespace divstats {

// pi_g = diff_gg / comp_gg and d_xy = diff_gh / comp_gh: one division of the two converted integers
inline bool ratio(uint64_t diff, uint64_t comp, double& out)
{
    if (comp == 0) return false;
    out = static_cast<double>(diff) / static_cast<double>(comp);
    return true;
}

// Hudson's F_ST = 1.0 - ((pi_g + pi_h) * 0.5) / dxy: an addition, a multiplication, a division, a subtraction
inline bool fst(bool has_g, double pi_g, bool has_h, double pi_h, bool has_xy, double dxy, double& out)
{
    if (!has_g || !has_h || !has_xy || dxy == 0.0) return false;
    out = 1.0 - ((pi_g + pi_h) * 0.5) / dxy;
    return true;
}

// a1 = sum 1 / i and a2 = sum 1 / (i * i) over i = 1 .. K - 1, added in ascending order
struct Harmonic { double a1 = 0.0, a2 = 0.0; };
inline Harmonic harmonic(uint64_t K)
{
    Harmonic h;
    for (uint64_t i = 1; i < K; i++) {
        const double d = static_cast<double>(i);
        h.a1 += 1.0 / d;
        h.a2 += 1.0 / (d * d);
    }
    return h;
}

// Watterson's theta_W = seg / a1
inline bool theta_w(uint64_t seg, const Harmonic& h, double& out)
{
    if (h.a1 == 0.0) return false;
    out = static_cast<double>(seg) / h.a1;
    return true;
}

// Tajima's D of a window of `sites` choice symbols, defined only where no path of the group is missing (present == sites K).
// With n = K and S = seg, in this order:
//   b1 = (n + 1) / (3 (n - 1))                 b2 = (2 (n n + n + 3)) / (9 n (n - 1))
//   c1 = b1 - 1 / a1                           c2 = b2 - (n + 2) / (a1 n) + a2 / (a1 a1)
//   e1 = c1 / a1                               e2 = c2 / (a1 a1 + a2)
//   k  = diff / C(K, 2)  (C(K, 2) = K (K - 1) / 2 as an integer, then converted)
//   var = e1 S + e2 S (S - 1);  D = (k - S / a1) / sqrt(var);  undefined unless var > 0
inline bool tajima_d(uint64_t K, uint64_t seg, uint64_t diff, uint64_t present, uint64_t sites, const Harmonic& h, double& out)
{
    if (K < 2 || seg == 0 || present != sites * K) return false;
    const double n = static_cast<double>(K), a1 = h.a1, a2 = h.a2;
    const double b1 = (n + 1.0) / (3.0 * (n - 1.0));
    const double b2 = (2.0 * (n * n + n + 3.0)) / (9.0 * n * (n - 1.0));
    const double c1 = b1 - 1.0 / a1;
    const double c2 = b2 - (n + 2.0) / (a1 * n) + a2 / (a1 * a1);
    const double e1 = c1 / a1;
    const double e2 = c2 / (a1 * a1 + a2);
    const double S = static_cast<double>(seg);
    const double k = static_cast<double>(diff) / static_cast<double>(K * (K - 1) / 2);
    const double var = e1 * S + e2 * S * (S - 1.0);
    if (!(var > 0.0)) return false;
    out = (k - S / a1) / std::sqrt(var);
    return true;
}

} // namespace divstats
} // namespace edsparser
