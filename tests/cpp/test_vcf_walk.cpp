// test_vcf_walk.cpp — the VCF -> EDS overlay on the CPU: the per-thread device code of edsparser_amd/csrc/vcf_walk.hpp run
// one "thread" after another over a case file written by tests/vcf_walk_cases.py; meant to be built with
// -fsanitize=address,undefined.  Every buffer is a heap block of its own, of exactly the size VcfPipeline asks for
// (vcf_size::*), filled with a byte the case chooses, so the first byte nobody asked for is a redzone; the two texts are
// 256-byte aligned as on the device.  The steps the device does with wave operations (line starts, reference compaction,
// scans, the sort of distinct positions, the common-text copy) are the plain loops below.
//
// Case records (little endian): u32 mode, u32 nfills, nfills bytes, u32 name_len, name, u64 vcf_len, vcf, u64 fasta_len,
// fasta, u64 up0, u64 up1.   mode 0: whole transform   1: up to the count pass   2: fa_cpos over the window [up0, up1)
// 3: fa_cpos over the whole file.   One result per (case, fill): u32 name_len, name, u32 fill, u32 verdict, u64 detail,
// u64 eds_len, eds, u64 seds_len, seds.   verdict 0: accepted (mode 0: texts follow)   1: not plain, the host tokeniser's
// 2: equal positions (out of scope here)   3: a byte index outside the text was reported (detail)   4: refused input
// 5: fa_cpos differs from the byte-by-byte count at file offset `detail`
#include "vcf_walk.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <utility>
#include <vector>

using namespace edsx;

namespace {

constexpr u64 THREADS = 3;       // "threads" of every body: more than one, so that the strides are walked

struct Arena {                   // the DevBufs of one call
    uint8_t fill;
    std::vector<void*> blocks;
    explicit Arena(uint8_t f) : fill(f) {}
    ~Arena() { for (void* p : blocks) std::free(p); }
    template <class T> T* get(u64 bytes, bool text = false)
    {
        void* p = nullptr;
        if (text) { if (posix_memalign(&p, 256, bytes)) std::abort(); }
        else p = std::malloc(bytes);
        if (!p) std::abort();
        std::memset(p, fill, bytes);                        // contents are undefined on the device: the case's byte here
        blocks.push_back(p);
        return static_cast<T*>(p);
    }
};

template <class F> void each_thread(F f) { for (u64 t = 0; t < THREADS; t++) f(HostGrid{t, THREADS}); }

void exclusive_scan(const u64* in, u64* out, u64 n, u64* total)       // out[0..n) only, as the device scan
{
    u64 s = 0;
    for (u64 i = 0; i < n; i++) { const u64 v = in[i]; out[i] = s; s += v; }
    *total = s;
}
void inclusive_max_scan(const u64* in, u64* out, u64 n, u64* total)
{
    u64 m = 0;
    for (u64 i = 0; i < n; i++) { m = in[i] > m ? in[i] : m; out[i] = m; }
    *total = m;
}

struct Result { u32 verdict = 0; u64 detail = 0; std::vector<uint8_t> eds, seds; };

struct Tokens {                   // what tokenize_device leaves behind
    u64 nrec = 0, max_samples = 0;
    u64 *start = nullptr, *reflen = nullptr, *alt0 = nullptr, *altoff = nullptr, *pair0 = nullptr, *pa0 = nullptr;
    uint8_t* altchars = nullptr; int* alleles = nullptr;
};

// VcfPipeline::tokenize_device + tokenize_lines.  false: r.verdict says why
bool tokenise(Arena& A, const std::vector<uint8_t>& vcf, bool count_only, u64* ctlbuf, Tokens& tk, Result& r)
{
    const u64 n = vcf.size();
    if (n == 0) { r.verdict = 1; return false; }
    uint8_t* raw = A.get<uint8_t>(vcf_size::text(n), true);
    std::memcpy(raw, vcf.data(), n);
    const u64 nblk = vcf_size::line_blocks(n);
    u64* idx = A.get<u64>(vcf_size::line_counts(nblk));
    VtCtl* ctl = reinterpret_cast<VtCtl*>(ctlbuf + 16);
    *ctl = VtCtl{};
    ctl->n = nblk;
    bool cr = false;
    for (u64 b = 0; b < nblk; b++) {                                   // k_vt_line_count
        u64 c = 0;
        for (u64 lane = 0; lane < 64; lane++) c += (u64)__builtin_popcount(vt_line_start_mask(raw, n, b * VT_BLOCK + lane * 16, cr));
        idx[b] = c;
    }
    if (cr) ctl->bad = 1;
    exclusive_scan(idx, idx, ctl->n, &ctl->nrec);
    if (ctl->bad || ctl->nrec >= 0xffffffffull) { r.verdict = 1; return false; }
    const u64 nr = ctl->nrec;
    if (nr == 0) return true;
    u64* lstart = A.get<u64>(vcf_size::line_starts(nr));
    for (u64 b = 0; b < nblk; b++) {                                   // k_vt_line_fill
        u64 at = idx[b];
        for (u64 lane = 0; lane < 64; lane++) {
            const u64 i0 = b * VT_BLOCK + lane * 16;
            u32 m = vt_line_start_mask(raw, n, i0, cr);
            while (m) { lstart[at++] = i0 + (u32)__builtin_ctz(m); m &= m - 1; }
        }
    }
    // tokenize_lines
    *ctl = VtCtl{};
    u64* rec[10];
    for (u64*& p : rec) p = A.get<u64>(vcf_size::per_record(nr));
    const VtRec vr{rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], nullptr};
    u64 *s1 = rec[6], *s2 = rec[7], *s3 = rec[8], *s4 = rec[9];
    each_thread([&](HostGrid g) { vt_count_body(raw, n, lstart, nr, vr, ctl, g); });
    each_thread([&](HostGrid g) { vt_ascending_body(vr.pos, nr, ctl, g); });
    if (ctl->oob) { r.verdict = 3; r.detail = ctl->oob; return false; }
    if (ctl->bad) { r.verdict = 1; return false; }
    if (count_only) return true;
    const u32* order = nullptr;
    if (ctl->t_alt) {                                                  // not ascending: the radix sort's result for distinct keys
        std::vector<std::pair<u64, u32>> ord(nr);
        for (u64 i = 0; i < nr; i++) ord[i] = {vr.pos[i], (u32)i};
        std::sort(ord.begin(), ord.end());
        for (u64 i = 0; i + 1 < nr; i++) if (ord[i].first == ord[i + 1].first) { r.verdict = 2; return false; }
        u32* o = A.get<u32>(vcf_size::order(nr));
        for (u64 i = 0; i < nr; i++) o[i] = ord[i].second;
        order = o;
        ctl->t_alt = 0;
    }
    ctl->n = nr;
    each_thread([&](HostGrid g) { vt_gather_body(vr, order, nr, s1, s2, s3, s4, g); });
    tk.alt0 = A.get<u64>(vcf_size::per_record(nr)); tk.pair0 = A.get<u64>(vcf_size::per_record(nr));
    tk.start = A.get<u64>(vcf_size::per_record(nr)); tk.reflen = A.get<u64>(vcf_size::per_record(nr));
    exclusive_scan(s1, tk.alt0, ctl->n, &ctl->t_alt);
    exclusive_scan(s2, s2, ctl->n, &ctl->t_altc);
    exclusive_scan(s3, tk.pair0, ctl->n, &ctl->t_pair);
    exclusive_scan(s4, s4, ctl->n, &ctl->t_all);
    tk.altoff = A.get<u64>(vcf_size::altoff(ctl->t_alt)); tk.altchars = A.get<uint8_t>(vcf_size::altchars(ctl->t_altc));
    tk.pa0 = A.get<u64>(vcf_size::pa0(ctl->t_pair)); tk.alleles = A.get<int>(vcf_size::alleles(ctl->t_all));
    const VtOut o{tk.start, tk.reflen, tk.alt0, tk.altoff, tk.altchars, tk.pair0, tk.pa0, tk.alleles, s2, s4};
    each_thread([&](HostGrid g) { vt_fill_body(raw, n, lstart, order, nr, o, ctl, g); });
    if (ctl->oob) { r.verdict = 3; r.detail = ctl->oob; return false; }
    tk.nrec = nr; tk.max_samples = ctl->max_samples;
    return true;
}

// fasta_head of vcf_device.hip: header line, first sequence line
bool fasta_head(const std::vector<uint8_t>& fa, u64& seq_start, u64& lw, u64& rest_from)
{
    const u64 n = fa.size();
    if (n == 0 || fa[0] != '>') return false;
    u64 e = 0;
    while (e < n && fa[e] != '\n') e++;
    if (e == n) { seq_start = n; return false; }                       // no second line: "FASTA file is empty"
    seq_start = e + 1;
    if (seq_start >= n) return false;
    u64 e2 = seq_start;
    while (e2 < n && fa[e2] != '\n') e2++;
    lw = e2 - seq_start;
    rest_from = e2 < n ? e2 + 1 : n;
    return lw != 0;
}

// the reference stream of run(): text [up0, up1) of the file on the "device", blkpre / refc from file offset cbase on
struct RefStream { uint8_t* dfa; u64* blkpre; uint8_t* refc; u64 refc_n; };
RefStream reference_stream(Arena& A, const std::vector<uint8_t>& fa, u64 up0, u64 up1, bool window, u64 seq_start, u64* ctl)
{
    RefStream s{};
    const u64 fasta_n = fa.size(), up_n = up1 - up0;
    s.dfa = A.get<uint8_t>(vcf_size::fasta(up_n), true);
    if (up_n) std::memcpy(s.dfa, fa.data() + up0, up_n);
    const u64 body = window ? up_n : fasta_n > seq_start ? fasta_n - seq_start : 0;
    const u64 nblk = vcf_size::ref_blocks(body);
    s.blkpre = A.get<u64>(vcf_size::blkpre(nblk));
    s.refc = A.get<uint8_t>(vcf_size::refc(body));
    ctl[0] = nblk;
    const u64 kn = window ? up_n : fasta_n, ks = window ? 0 : seq_start;
    auto kept = [](uint8_t ch) { return ch != '\n' && ch != '\r'; };
    for (u64 b = 0; b < nblk; b++) {                                   // k_fa_count
        u64 c = 0;
        for (u64 i = ks + b * 256; i < ks + b * 256 + 256 && i < kn; i++) c += kept(s.dfa[i]);
        s.blkpre[b] = c;
    }
    if (nblk) exclusive_scan(s.blkpre, s.blkpre, ctl[0], &ctl[1]);
    for (u64 b = 0; b < nblk; b++) {                                   // k_fa_compact
        u64 o = s.blkpre[b];
        for (u64 i = ks + b * 256; i < ks + b * 256 + 256 && i < kn; i++) if (kept(s.dfa[i])) s.refc[o++] = s.dfa[i];
    }
    s.refc_n = nblk ? ctl[1] : 0;
    return s;
}

// VcfPipeline::run on the whole file (no position range, nothing resident)
Result transform(uint8_t fill, const std::vector<uint8_t>& vcf, const std::vector<uint8_t>& fa, bool count_only)
{
    Result r;
    Arena A(fill);
    u64* ctl = A.get<u64>(vcf_size::ctl());
    u64 seq_start = 0, lw = 0, rest_from = 0;
    const bool fasta_ok = fasta_head(fa, seq_start, lw, rest_from);
    if (!count_only && !fasta_ok) { r.verdict = 4; return r; }
    Tokens tk;
    if (!tokenise(A, vcf, count_only, ctl, tk, r) || count_only) return r;
    const u64 fasta_n = fa.size(), nrec = tk.nrec;
    std::memset(ctl, 0, vcf_size::ctl());
    ctl[10] = ~0ull; ctl[12] = fasta_n;
    const RefStream rs = reference_stream(A, fa, 0, fasta_n, false, seq_start, ctl);
    if (rest_from < fasta_n) {
        each_thread([&](HostGrid g) { fa_record_end_body(rs.dfa, fasta_n, rest_from, ctl + 12, g); });
        for (u64 i = rest_from; i < ctl[12]; i++) ctl[13] += rs.dfa[i] != '\n';        // k_fa_seq_bytes
    }
    const u64 seq_size = lw + ctl[13];

    VcfDev d{};
    d.fasta = rs.dfa + seq_start; d.fasta_n = fasta_n; d.seq_start = seq_start; d.seq_size = seq_size; d.lw = lw;
    d.refc = rs.refc; d.refc_n = rs.refc_n; d.blkpre = rs.blkpre;
    d.cbase = seq_start; d.wend = fasta_n; d.oob = nullptr;
    d.nrec = nrec; d.cur0 = 0;
    u64 cur = 0, ngrp = 0, E = 0, Q = 0;
    GrpArrays ga{};
    HapArrays ha{};
    if (nrec) {
        d.start = tk.start; d.reflen = tk.reflen; d.alt0 = tk.alt0; d.altstr_off = tk.altoff; d.altchars = tk.altchars;
        d.pair0 = tk.pair0; d.pair_a0 = tk.pa0; d.alleles = tk.alleles;
        u64* ends = A.get<u64>(vcf_size::per_record(nrec)); u64* flag = A.get<u64>(vcf_size::per_record(nrec));
        u64* gidx = A.get<u64>(vcf_size::per_record(nrec)); u64* grp_r0 = A.get<u64>(vcf_size::per_record(nrec));
        ctl[0] = nrec;
        each_thread([&](HostGrid g) { rec_ends_body(d.start, d.reflen, nrec, ends, g); });
        inclusive_max_scan(ends, ends, ctl[0], ctl + 2);
        each_thread([&](HostGrid g) { mark_groups_body(d.start, ends, nrec, flag, g); });
        exclusive_scan(flag, gidx, ctl[0], ctl + 3);
        each_thread([&](HostGrid g) { group_firsts_body(flag, gidx, nrec, grp_r0, ctl + 3, g); });
        ngrp = ctl[3];
        d.ngrp = ngrp; d.grp_r0 = grp_r0; d.incl_end = ends;
        u64* gb[14];
        for (u64*& p : gb) p = A.get<u64>(vcf_size::per_group(ngrp));
        ga = GrpArrays{gb[0], gb[1], gb[2], gb[3], gb[4], gb[5], gb[6], gb[7], gb[8], gb[9], gb[10], ctl + 10};
        u64 *raw0 = gb[11], *rawc0 = gb[12], *bit0 = gb[13];
        ctl[0] = ngrp;
        each_thread([&](HostGrid g) { grp_count_body(d, ga, g); });
        exclusive_scan(ga.nraw, raw0, ctl[0], ctl + 4);
        exclusive_scan(ga.rawchars, rawc0, ctl[0], ctl + 5);
        const u64 nraw_total = ctl[4], rawchars_total = ctl[5];
        const u32 sw = (u32)std::max<u64>(1, (tk.max_samples + 63) / 64);
        ha = HapArrays{raw0, rawc0, A.get<u64>(vcf_size::per_raw(nraw_total)), A.get<u64>(vcf_size::per_raw(nraw_total)),
                       A.get<u32>(vcf_size::canon(nraw_total)), A.get<uint8_t>(vcf_size::hapchars(rawchars_total)), bit0, nullptr, sw};
        each_thread([&](HostGrid g) { grp_haps_body(d, ga, ha, g); });
        exclusive_scan(ga.bitwords, bit0, ctl[0], ctl + 6);
        ha.carried = A.get<u64>(vcf_size::carried(ctl[6]));
        each_thread([&](HostGrid g) { grp_samples_body(d, ga, ha, g); });
        each_thread([&](HostGrid g) { grp_common_body(d, ga, g); });
        exclusive_scan(ga.eds_len, ga.eds_len, ctl[0], ctl + 7);
        exclusive_scan(ga.seds_len, ga.seds_len, ctl[0], ctl + 8);
        E = ctl[7]; Q = ctl[8]; cur = ga.cur_after[ngrp - 1];
    }
    u64 tail = 0;
    if (cur < seq_size) {
        const u64 length = seq_size - cur;
        cpos_body(d, seq_start + cur + cur / lw, ctl + 11, HostGrid{0, 1});
        tail = std::min<u64>(length, rs.refc_n - ctl[11]);
    }
    const u64 Etot = E + (tail ? tail + 2 : 0), Qtot = Q + (tail ? 3 : 0);
    uint8_t* eds = A.get<uint8_t>(vcf_size::eds(Etot)); uint8_t* seds = A.get<uint8_t>(vcf_size::eds(Qtot));
    if (ngrp) {
        const EmitArrays ea{ga.eds_len, ga.seds_len, eds, seds};
        for (u64 g = 0; g < ngrp; g++) {                               // k_grp_emit_common
            const u64 clen = ga.commonlen[g];
            if (!clen) continue;
            uint8_t* eo = eds + ea.eds_off[g]; uint8_t* so = seds + ea.seds_off[g];
            const u64 c = g ? ga.cur_after[g - 1] : d.cur0;
            const u64 c0 = fa_cpos(d, d.seq_start + c + c / d.lw);
            eo[0] = '{'; eo[clen + 1] = '}'; so[0] = '{'; so[1] = '0'; so[2] = '}';
            for (u64 i = 0; i < clen; i++) eo[1 + i] = d.refc[c0 + i];
        }
        each_thread([&](HostGrid g) { grp_emit_body(d, ga, ha, ea, g); });
    }
    if (tail) each_thread([&](HostGrid g) { tail_body(d, cur, tail, eds + E, seds + Q, g); });
    r.eds.assign(eds, eds + Etot); r.seds.assign(seds, seds + Qtot);
    return r;
}

// fa_cpos alone: every file offset from cbase to fasta_n + 2 against a byte-by-byte count
Result cpos_sweep(uint8_t fill, const std::vector<uint8_t>& fa, u64 up0, u64 up1, bool window)
{
    Result r;
    Arena A(fill);
    u64* ctl = A.get<u64>(vcf_size::ctl());
    std::memset(ctl, 0, vcf_size::ctl());
    u64 seq_start = 0, lw = 0, rest_from = 0;
    const u64 fasta_n = fa.size();
    if (!fasta_head(fa, seq_start, lw, rest_from) || up0 > up1 || up1 > fasta_n || (window && up0 < seq_start)) { r.verdict = 4; return r; }
    if (!window) { up0 = 0; up1 = fasta_n; }
    const RefStream rs = reference_stream(A, fa, up0, up1, window, seq_start, ctl);
    const u64 cbase = window ? up0 : seq_start;
    VcfDev d{};
    d.fasta = rs.dfa + (cbase - up0); d.fasta_n = fasta_n; d.seq_start = seq_start; d.lw = lw;
    d.refc = rs.refc; d.refc_n = rs.refc_n; d.blkpre = rs.blkpre; d.cbase = cbase; d.wend = up1; d.oob = window ? ctl + 20 : nullptr;
    u64 want = 0;                                                      // kept bytes in [cbase, off)
    for (u64 off = cbase; off < fasta_n + 2; off++) {
        ctl[20] = 0;
        cpos_body(d, off, ctl + 11, HostGrid{0, 1});
        const bool outside = off >= fasta_n || off >= up1;
        const u64 expect = outside ? rs.refc_n : want;
        const u64 expect_oob = window && off < fasta_n && off > up1 ? (off | (1ull << 63)) : 0;
        if (ctl[11] != expect || ctl[20] != expect_oob) { r.verdict = 5; r.detail = off; return r; }
        if (off < up1) want += fa[off] != '\n' && fa[off] != '\r';
    }
    return r;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: test_vcf_walk cases.bin results.bin\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::ofstream out(argv[2], std::ios::binary);
    size_t at = 0, runs = 0;
    auto u32at = [&]() { uint32_t v; std::memcpy(&v, file.data() + at, 4); at += 4; return v; };
    auto u64at = [&]() { uint64_t v; std::memcpy(&v, file.data() + at, 8); at += 8; return v; };
    auto bytes = [&](u64 n) { std::vector<uint8_t> v(file.begin() + at, file.begin() + at + n); at += n; return v; };
    auto put32 = [&](uint32_t v) { out.write(reinterpret_cast<const char*>(&v), 4); };
    auto put64 = [&](uint64_t v) { out.write(reinterpret_cast<const char*>(&v), 8); };
    while (at < file.size()) {
        const uint32_t mode = u32at(), nfills = u32at();
        const std::vector<uint8_t> fills = bytes(nfills);
        const std::vector<uint8_t> name = bytes(u32at());
        const std::vector<uint8_t> vcf = bytes(u64at());
        const std::vector<uint8_t> fa = bytes(u64at());
        const u64 up0 = u64at(), up1 = u64at();
        for (uint8_t fill : fills) {
            const Result r = mode <= 1 ? transform(fill, vcf, fa, mode == 1) : cpos_sweep(fill, fa, up0, up1, mode == 2);
            put32((uint32_t)name.size()); out.write(reinterpret_cast<const char*>(name.data()), name.size());
            put32(fill); put32(r.verdict); put64(r.detail);
            put64(r.eds.size()); out.write(reinterpret_cast<const char*>(r.eds.data()), r.eds.size());
            put64(r.seds.size()); out.write(reinterpret_cast<const char*>(r.seds.data()), r.seds.size());
            runs++;
        }
    }
    out.close();
    std::fprintf(stderr, "%zu runs\n", runs);
    return out ? 0 : 1;
}
