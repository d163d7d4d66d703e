// test_gfa_text — the closed forms of csrc/gfa_text.hpp on the host, without a GPU: every 16-byte chunk of the S, L and P
// text of an EDS is produced by the functions the kernels call (seg_chunk, link_chunk, walk_chunk), from tables built here
// the way the count kernels build them, and written out for tests/test_gfa_cpu.py to compare with the specification.
// stdin: one case per line, "<eds> <seds or -> <lead>": FULL-form texts without blanks; lead: the bytes in front of the S
// lines (where the 16-byte chunks fall).  stdout per case: "<bytes>\n" and the text.
#include "../../edsparser_amd/csrc/gfa_text.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

using namespace edsx;

namespace {

struct Eds {
    std::vector<u64> size, ent_off, str_off;
    std::vector<u32> elen;
    std::string chars;
    std::vector<std::set<u64>> sets;
    u64 P = 0;
};

Eds parse(const std::string& eds, const std::string& seds)
{
    Eds e;
    size_t k = 0;
    while (k < eds.size()) {
        if (eds[k] != '{') throw std::runtime_error("full form expected");
        const size_t close = eds.find('}', k);
        e.ent_off.push_back(e.elen.size());
        u64 cnt = 0;
        size_t a = k + 1;
        for (;;) {
            size_t b = eds.find(',', a);
            if (b == std::string::npos || b > close) b = close;
            e.str_off.push_back(e.chars.size());
            e.elen.push_back((u32)(b - a));
            e.chars += eds.substr(a, b - a);
            cnt++;
            if (b == close) break;
            a = b + 1;
        }
        e.size.push_back(cnt);
        k = close + 1;
    }
    e.str_off.push_back(e.chars.size());
    e.chars += std::string(16, '#');
    if (seds != "-") {
        k = 0;
        while (k < seds.size()) {
            const size_t close = seds.find('}', k);
            std::set<u64> s;
            size_t a = k + 1;
            while (a < close) {
                size_t b = seds.find(',', a);
                if (b == std::string::npos || b > close) b = close;
                s.insert(std::stoull(seds.substr(a, b - a)));
                a = b + 1;
            }
            for (u64 p : s) e.P = std::max(e.P, p);
            e.sets.push_back(s);
            k = close + 1;
        }
        if (e.sets.size() != e.elen.size()) throw std::runtime_error("cardinality");
    }
    return e;
}

void append(std::string& out, const gfa::B16& x, u32 nb)
{
    for (u32 b = 0; b < nb; b++) out += (char)((b < 8 ? x.lo >> (8 * b) : x.hi >> (8 * (b - 8))) & 0xff);
}

} // namespace

int main()
{
    std::string eds, seds;
    u64 lead;
    while (std::cin >> eds >> seds >> lead) {
        const Eds e = parse(eds, seds);
        const u64 n = e.size.size(), m = e.elen.size();
        std::string text;
        // ---- counts, as k_gfa_flags / k_gfa_closed / k_gfa_compact / k_gfa_reach and their scans
        std::vector<u64> seg_rank(m + 1, 0), C(n + 1, 0), closed, vend(n + 1, 0), loff(n + 1, 0);
        for (u64 j = 0; j < m; j++) seg_rank[j + 1] = seg_rank[j] + (e.elen[j] ? 1 : 0);
        for (u64 i = 0; i < n; i++) {
            const bool c = seg_rank[e.ent_off[i] + e.size[i]] - seg_rank[e.ent_off[i]] == e.size[i];
            C[i + 1] = C[i] + (c ? 1 : 0);
            if (c) closed.push_back(i);
        }
        u64 lbytes = 0;
        for (u64 i = 0; i < n; i++) {
            const u64 R = C[i + 1] < closed.size() ? closed[C[i + 1]] : n - 1;
            const u64 a = seg_rank[e.ent_off[i]] + 1, b = seg_rank[e.ent_off[i] + e.size[i]] + 1, d = seg_rank[e.ent_off[R] + e.size[R]] + 1;
            vend[i] = d;
            loff[i] = lbytes;
            lbytes += gfa::link_block_bytes(a, b, b, d);
        }
        loff[n] = lbytes;
        const u64 M = seg_rank[m], N = e.str_off[m], sbytes = 4 * M + gfa::dsum(M) + (M ? N : 0);
        // ---- fill, chunk by chunk as the emitters tile their section
        auto section = [&](u64 sec0, u64 bytes, auto&& chunk) {
            const u64 sec1 = sec0 + bytes;
            for (u64 c0 = sec0 / 16 * 16; c0 < sec1; c0 += 16) {
                const u64 lo = std::max(c0, sec0), hi = std::min(c0 + 16, sec1);
                chunk(lo - sec0, (u32)(hi - lo));
            }
        };
        if (sbytes) {
            const gfa::SegTab t{seg_rank.data(), e.str_off.data(), e.elen.data(), reinterpret_cast<const uint8_t*>(e.chars.data()), m};
            section(lead, sbytes, [&](u64 o, u32 nb) {
                gfa::B16 x{0, 0};
                u64 pool = 0;
                if (gfa::seg_chunk(t, 0, m - 1, o, nb, x, pool)) text += e.chars.substr(pool, 16);
                else append(text, x, nb);
            });
        }
        if (lbytes) {
            const gfa::LinkTab t{e.size.data(), e.ent_off.data(), seg_rank.data(), vend.data(), loff.data(), n};
            section(lead + sbytes, lbytes, [&](u64 o, u32 nb) { append(text, gfa::link_chunk(t, 0, n - 1, o, nb), nb); });
        }
        // ---- walks of all paths, one table row per path, as k_path_flags / k_path_choose / k_path_tokfixed / k_path_tok
        if (seds != "-" && n) {
            std::vector<u64> rank(n + 1, 0), ct(n + 1, 0), cidx;
            for (u64 i = 0; i < n; i++) {
                const bool fixed = e.size[i] == 1 && e.sets[e.ent_off[i]].count(0);
                rank[i + 1] = rank[i] + (fixed ? 0 : 1);
                if (!fixed) cidx.push_back(i);
                const u64 j = e.ent_off[i];
                ct[i + 1] = ct[i] + (fixed && e.elen[j] ? gfa::digits(seg_rank[j] + 1) + 2 : 0);
            }
            const u64 nc = cidx.size(), K = e.P;
            std::vector<u64> csid(K * nc + 1, gfa::NONE), TS(K * nc + 1, 0);
            for (u64 k = 0; k < K; k++)
                for (u64 r = 0; r < nc; r++) {
                    const u64 i = cidx[r], t = k * nc + r;
                    for (u64 q = 0; q < e.size[i]; q++) {
                        const auto& s = e.sets[e.ent_off[i] + q];
                        if (s.count(0) || s.count(k + 1)) { csid[t] = e.ent_off[i] + q; break; }
                    }
                    const u64 sid = csid[t];
                    TS[t + 1] = TS[t] + (sid != gfa::NONE && e.elen[sid] ? gfa::digits(seg_rank[sid] + 1) + 2 : 0);
                }
            const gfa::WalkTab a{e.ent_off.data(), seg_rank.data(), ct.data(), rank.data(), csid.data(), TS.data(), n, nc};
            for (u64 k = 0; k < K; k++) {
                const u64 kb = k * nc, T = ct[n] + (nc ? TS[kb + nc] - TS[kb] : 0);
                if (!T) continue;
                text += "P\tpath" + std::to_string(k + 1) + "\t";
                for (u64 o = 0; o < T + 2; o += 16) append(text, gfa::walk_chunk(a, kb, 0, n - 1, T, o, (u32)std::min<u64>(16, T + 2 - o)), (u32)std::min<u64>(16, T + 2 - o));
            }
        }
        std::printf("%zu\n", text.size());
        std::fwrite(text.data(), 1, text.size(), stdout);
    }
    return 0;
}
