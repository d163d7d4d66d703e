// test_vcf_text — the closed forms of csrc/vcf_text.hpp on the host, without a GPU: the record lines of an EDS are produced
// by the functions the kernels call (rec_of, fixed_bytes, fixed_chunk, cell_bytes, cell_write, ref_char), from tables built
// here the way the count kernels build them, and written out for tests/test_vcf_export_cpu.py to compare with the
// specification.  Only inputs the export accepts.
// stdin: one case per line, "<eds> <seds or -> <ref_path> <lead> <chrom>": FULL-form texts without blanks; lead: the bytes
// in front of the body (where the 16-byte chunks fall).  stdout per case: "<bytes>\n" and the body.
#include "../../edsparser_amd/csrc/vcf_text.hpp"

#include <algorithm>
#include <cstdio>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

using namespace edsx;

namespace {

struct Eds {
    std::vector<u64> size, ent_off, str_off, bits;
    std::string chars;
    u64 P = 0;
    u32 W = 0;
};

Eds parse(const std::string& eds, const std::string& seds)
{
    Eds e;
    size_t k = 0;
    u64 m = 0;
    while (k < eds.size()) {
        if (eds[k] != '{') throw std::runtime_error("full form expected");
        const size_t close = eds.find('}', k);
        e.ent_off.push_back(m);
        u64 cnt = 0;
        size_t a = k + 1;
        for (;;) {
            size_t b = eds.find(',', a);
            if (b == std::string::npos || b > close) b = close;
            e.str_off.push_back(e.chars.size());
            e.chars += eds.substr(a, b - a);
            cnt++; m++;
            if (b == close) break;
            a = b + 1;
        }
        e.size.push_back(cnt);
        k = close + 1;
    }
    e.str_off.push_back(e.chars.size());
    e.chars += std::string(16, '#');
    if (seds != "-") {
        std::vector<std::vector<u64>> sets;
        k = 0;
        while (k < seds.size()) {
            const size_t close = seds.find('}', k);
            std::vector<u64> s;
            size_t a = k + 1;
            while (a < close) {
                size_t b = seds.find(',', a);
                if (b == std::string::npos || b > close) b = close;
                s.push_back(std::stoull(seds.substr(a, b - a)));
                a = b + 1;
            }
            for (u64 p : s) e.P = std::max(e.P, p);
            sets.push_back(s);
            k = close + 1;
        }
        if (sets.size() != m) throw std::runtime_error("cardinality");
        e.W = (u32)(e.P / 64 + 1);
        e.bits.assign(m * e.W, 0);
        for (u64 j = 0; j < m; j++)
            for (u64 p : sets[j]) e.bits[j * e.W + p / 64] |= 1ull << (p % 64);
    }
    return e;
}

} // namespace

int main()
{
    std::string eds, seds, chrom;
    u64 ref_path, lead;
    while (std::cin >> eds >> seds >> ref_path >> lead >> chrom) {
        const Eds e = parse(eds, seds);
        const u64 n = e.size.size();
        const bool with_gt = seds != "-";
        // ---- as k_vcf_sym, its scan and k_vcf_anchor
        std::vector<u64> refidx(n + 1, 0), refpos(n + 1, 0), anchor(n + 1, 0), recsym;
        for (u64 i = 0; i < n; i++) {
            u64 r = 0;
            if (ref_path) {
                r = vcf::NONE;
                for (u64 q = 0; q < e.size[i] && r == vcf::NONE; q++) {
                    const u64* b = e.bits.data() + (e.ent_off[i] + q) * e.W;
                    if ((b[0] & 1) || (b[ref_path >> 6] >> (ref_path & 63) & 1)) r = q;
                }
                if (r == vcf::NONE) throw std::runtime_error("reference path takes no string");
            }
            refidx[i] = r;
            refpos[i + 1] = refpos[i] + e.str_off[e.ent_off[i] + r + 1] - e.str_off[e.ent_off[i] + r];
            if (e.size[i] >= 2) recsym.push_back(i);
        }
        vcf::Tab t{e.size.data(), e.ent_off.data(), e.str_off.data(), reinterpret_cast<const uint8_t*>(e.chars.data()),
                   with_gt ? e.bits.data() : nullptr, e.W, refidx.data(), refpos.data(), anchor.data(), n, e.P,
                   reinterpret_cast<const uint8_t*>(chrom.data()), (u32)chrom.size(), with_gt ? 1u : 0u};
        const u64 L = refpos[n];
        for (u64 i : recsym) {
            bool empty = false;
            for (u64 q = 0; q < e.size[i]; q++) empty = empty || e.str_off[e.ent_off[i] + q + 1] == e.str_off[e.ent_off[i] + q];
            if (!empty) continue;
            const u64 q = refpos[i] > 0 ? refpos[i] - 1 : refpos[i + 1];
            if (q >= L) throw std::runtime_error("no anchor base");
            anchor[i] = ((u64)vcf::ref_char(t, q) << 8) | (refpos[i] > 0 ? vcf::ANC_FRONT : vcf::ANC_BACK);
        }
        // ---- count and fill, a record at a time: the fixed part chunk by chunk, the cells tile by tile, word by word
        const u64 NT = with_gt && e.P ? e.P / vcf::TILE_PATHS + 1 : 0;
        std::string text;
        for (u64 i : recsym) {
            const vcf::Rec c = vcf::rec_of(t, i);
            const u64 d0 = lead + text.size(), d1 = d0 + vcf::fixed_bytes(t, c, NT == 0);
            for (u64 c0 = d0 / 16 * 16; c0 < d1; c0 += 16) {
                const u64 lo = std::max(c0, d0), hi = std::min(c0 + 16, d1);
                vcf::B16 x;
                u64 pool = 0;
                if (vcf::fixed_chunk(t, c, lo - d0, (u32)(hi - lo), x, pool)) text += e.chars.substr(pool, hi - lo);
                else for (u32 b = 0; b < hi - lo; b++) text += (char)((b < 8 ? x.lo >> (8 * b) : x.hi >> (8 * (b - 8))) & 0xff);
            }
            for (u64 tile = 0; tile < NT; tile++) {
                for (u64 w = 4 * tile; w < 4 * tile + 4; w++)
                    for (u32 l = 0; l < 64; l++) {
                        const u64 p = 64 * w + l;
                        if (p < 1 || p > e.P) continue;
                        std::string cell(vcf::cell_bytes(t, c, (u32)w, l), '?');
                        vcf::cell_write(t, c, (u32)w, l, reinterpret_cast<uint8_t*>(&cell[0]));
                        text += cell;
                    }
                if (tile == NT - 1) text += '\n';
            }
        }
        std::printf("%zu\n", text.size());
        std::fwrite(text.data(), 1, text.size(), stdout);
    }
    return 0;
}
