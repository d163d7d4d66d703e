// vcf_walk_twin.hpp — what the host twins of the VCF path share (test_vcf_walk.cpp, test_contig_walk.cpp): the "HBM" arena,
// the device tokeniser, the reference stream and the whole transform of VcfPipeline::run as loops over the per-thread code of
// csrc/vcf_walk.hpp and the host code of csrc/vcf_host.hpp.  See test_vcf_walk.cpp for the rules (buffer sizes, fills).
#pragma once

#include "vcf_host.hpp"

#include <cstdlib>
#include <fstream>
#include <iterator>

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
    template <class T> T* upload(const std::vector<T>& v)  // upload() of vcf_device.hip
    {
        T* p = get<T>(sizeof(T) * (v.size() + 1) + 16);
        if (!v.empty()) std::memcpy(p, v.data(), sizeof(T) * v.size());
        return p;
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

struct Result { u32 verdict = 0; u64 detail = 0; std::vector<uint8_t> eds, seds; bool host_tokeniser = false; };

struct Tokens {                   // the record SoA in "HBM", from either tokeniser
    u64 nrec = 0, max_samples = 0;
    u64 *start = nullptr, *reflen = nullptr, *alt0 = nullptr, *altoff = nullptr, *pair0 = nullptr, *pa0 = nullptr;
    uint8_t* altchars = nullptr; int* alleles = nullptr;
    VcfSoA host;                  // host tokeniser: the arrays on the host (grouping looks at them for wrapped positions)
    bool from_host = false;
};

// What a VcfSession hands VcfPipeline::run (VcfResident): the FASTA record where it lies inside a larger "device" buffer,
// with the seq_size the index counted, and the VCF text with a slice of regrouped line starts (d_vcf null: no lines).
struct Resident { const uint8_t* d_fasta = nullptr; u64 seq_size = 0; const uint8_t* d_vcf = nullptr; u64 vcf_n = 0; const u64* d_lstart = nullptr; u64 nrec = 0; };

bool tokenise_lines(Arena& A, const uint8_t* raw, u64 n, const u64* lstart, u64 nr, bool count_only, bool presorted, VtCtl* ctl,
                    Tokens& tk, Result& r);

// vt_line_starts of vcf_text_kernels.hpp over the text raw[0, n) in a buffer of vcf_size::text(n) bytes: the record-line
// starts and their number in ctl->nrec.  false: a '\r' somewhere, or too many lines
bool line_starts(Arena& A, const uint8_t* raw, u64 n, VtCtl* ctl, u64*& lstart)
{
    const u64 nblk = vcf_size::line_blocks(n);
    u64* idx = A.get<u64>(vcf_size::line_counts(nblk));
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
    if (ctl->bad || ctl->nrec >= 0xffffffffull) return false;
    const u64 nr = ctl->nrec;
    lstart = nullptr;
    if (nr == 0) return true;
    lstart = A.get<u64>(vcf_size::line_starts(nr));
    for (u64 b = 0; b < nblk; b++) {                                   // k_vt_line_fill
        u64 at = idx[b];
        for (u64 lane = 0; lane < 64; lane++) {
            const u64 i0 = b * VT_BLOCK + lane * 16;
            u32 m = vt_line_start_mask(raw, n, i0, cr);
            while (m) { lstart[at++] = i0 + (u32)__builtin_ctz(m); m &= m - 1; }
        }
    }
    return true;
}

// VcfPipeline::tokenize_device + tokenize_lines.  false: r.verdict says why
bool device_tokenise(Arena& A, const std::vector<uint8_t>& vcf, bool count_only, bool presorted, VtCtl* ctl, Tokens& tk, Result& r)
{
    const u64 n = vcf.size();
    if (n == 0) { r.verdict = 1; return false; }
    uint8_t* raw = A.get<uint8_t>(vcf_size::text(n), true);
    std::memcpy(raw, vcf.data(), n);
    u64* lstart = nullptr;
    if (!line_starts(A, raw, n, ctl, lstart)) { r.verdict = 1; return false; }
    const u64 nr = ctl->nrec;
    return tokenise_lines(A, raw, n, lstart, nr, count_only, presorted, ctl, tk, r);
}

// VcfPipeline::tokenize_lines: record lines [lstart[j], ...) of the text raw[0, n)
bool tokenise_lines(Arena& A, const uint8_t* raw, u64 n, const u64* lstart, u64 nr, bool count_only, bool presorted, VtCtl* ctl,
                    Tokens& tk, Result& r)
{
    if (nr == 0) return true;
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
    if (ctl->t_alt && !presorted) {            // not ascending: the radix sort's result for distinct keys, else the host's sort
        std::vector<std::pair<u64, u32>> ord(nr);
        for (u64 i = 0; i < nr; i++) ord[i] = {vr.pos[i], (u32)i};
        std::sort(ord.begin(), ord.end());
        bool equal = false;
        for (u64 i = 0; i + 1 < nr; i++) equal |= ord[i].first == ord[i + 1].first;
        u32* o = A.get<u32>(vcf_size::order(nr));
        if (equal) vcf_sort_order(vr.pos, nr, o);
        else for (u64 i = 0; i < nr; i++) o[i] = ord[i].second;
        order = o;
    }
    ctl->t_alt = 0;
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

// the host tokeniser's way of VcfPipeline::run: tokenise -> order -> SoA -> the eight uploads
void host_tokenise(Arena& A, const std::vector<uint8_t>& vcf, bool presorted, Tokens& tk)
{
    static const uint8_t none = 0;
    std::vector<VcfPart> parts;
    std::vector<u64> part_base;
    VcfCounters stats;
    tokenise(vcf.empty() ? &none : vcf.data(), vcf.size(), parts, part_base, stats, false);
    tk.host = build_soa(parts, part_base, host_order(parts, part_base, presorted));
    const VcfSoA& s = tk.host;
    tk.from_host = true;
    tk.nrec = s.start.size(); tk.max_samples = s.max_samples;
    tk.start = A.upload(s.start); tk.reflen = A.upload(s.reflen); tk.alt0 = A.upload(s.alt0); tk.altoff = A.upload(s.altoff);
    tk.altchars = A.upload(s.altchars); tk.pair0 = A.upload(s.pair0); tk.pa0 = A.upload(s.pa0); tk.alleles = A.upload(s.alleles);
}

// the reference stream of run(): text [up0, up1) of the file on the "device", blkpre / refc from file offset cbase on
struct RefStream { const uint8_t* dfa; u64* blkpre; uint8_t* refc; u64 refc_n; };
// resident: the file is on the "device" already, at any alignment (a record of a session's FASTA), and is not copied
RefStream reference_stream(Arena& A, const std::vector<uint8_t>& fa, const RefWindow& w, u64 seq_start, VcfCtl* ctl,
                           const uint8_t* resident = nullptr)
{
    RefStream s{};
    const u64 fasta_n = fa.size(), up_n = w.up1 - w.up0;
    if (resident) s.dfa = resident;
    else {
        uint8_t* up = A.get<uint8_t>(vcf_size::fasta(up_n), true);
        if (up_n) std::memcpy(up, fa.data() + w.up0, up_n);
        s.dfa = up;
    }
    const u64 body = w.window ? up_n : fasta_n > seq_start ? fasta_n - seq_start : 0;
    const u64 nblk = vcf_size::ref_blocks(body);
    s.blkpre = A.get<u64>(vcf_size::blkpre(nblk));
    s.refc = A.get<uint8_t>(vcf_size::refc(body));
    ctl->n = nblk;
    const u64 kn = w.window ? up_n : fasta_n, ks = w.window ? 0 : seq_start;
    auto kept = [](uint8_t ch) { return ch != '\n' && ch != '\r'; };
    for (u64 b = 0; b < nblk; b++) {                                   // k_fa_count
        u64 c = 0;
        for (u64 i = ks + b * 256; i < ks + b * 256 + 256 && i < kn; i++) c += kept(s.dfa[i]);
        s.blkpre[b] = c;
    }
    if (nblk) exclusive_scan(s.blkpre, s.blkpre, ctl->n, &ctl->refc_n);
    for (u64 b = 0; b < nblk; b++) {                                   // k_fa_compact
        u64 o = s.blkpre[b];
        for (u64 i = ks + b * 256; i < ks + b * 256 + 256 && i < kn; i++) if (kept(s.dfa[i])) s.refc[o++] = s.dfa[i];
    }
    s.refc_n = nblk ? ctl->refc_n : 0;
    return s;
}

bool head_of(const std::vector<uint8_t>& fa, u64& seq_start, u64& lw, u64& rest_from)      // false: the library refuses the file
{
    static const uint8_t none = 0;
    try { fasta_head(fa.empty() ? &none : fa.data(), fa.size(), seq_start, lw, rest_from); } catch (const FormatError&) { return false; }
    return lw != 0;
}

// VcfPipeline::run.  host: take the host tokeniser where the device tokeniser says "not plain".  res: what a session has
// resident; fa is then the record's bytes on the host (run() parses its head there), and resident lines the count pass
// refuses end the call with verdict 1 (the session builds the contig's text on the host and calls again)
Result transform(uint8_t fill, const std::vector<uint8_t>& vcf, const std::vector<uint8_t>& fa, bool count_only, bool host,
                 const VcfRange& range = VcfRange(), const Resident* res = nullptr)
{
    Result r;
    Arena A(fill);
    VcfCtl* ctl = A.get<VcfCtl>(vcf_size::ctl());
    u64 seq_start = 0, lw = 0, rest_from = 0;
    const bool fasta_ok = head_of(fa, seq_start, lw, rest_from);
    if (!count_only && !fasta_ok) { r.verdict = 4; return r; }
    Tokens tk;
    const bool lines_resident = res && res->d_vcf;
    if (!(lines_resident ? tokenise_lines(A, res->d_vcf, res->vcf_n, res->d_lstart, res->nrec, count_only, range.presorted, &ctl->vt, tk, r)
                         : device_tokenise(A, vcf, count_only, range.presorted, &ctl->vt, tk, r))) {
        if (lines_resident || !(host && r.verdict == 1)) return r;
        r = Result();
        try { host_tokenise(A, vcf, range.presorted, tk); } catch (const FormatError&) { r.verdict = 4; return r; }
    }
    if (count_only) return r;
    r.host_tokeniser = tk.from_host;
    const u64 fasta_n = fa.size(), nrec = tk.nrec;
    const FastaMeta* meta = range.fasta;
    FastaMeta res_meta;
    if (res && res->d_fasta) { res_meta.seq_size = res->seq_size; res_meta.regular = false; meta = &res_meta; }   // (the index counted it)
    // reference stream
    const RefWindow w = reference_window(range, meta, seq_start, lw, fasta_n);
    *ctl = VcfCtl{};
    ctl->rec_end = fasta_n;
    const RefStream rs = reference_stream(A, fa, w, seq_start, ctl, res ? res->d_fasta : nullptr);
    if (!meta && rest_from < fasta_n) {
        each_thread([&](HostGrid g) { fa_record_end_body(rs.dfa, fasta_n, rest_from, &ctl->rec_end, g); });
        for (u64 i = rest_from; i < ctl->rec_end; i++) ctl->rest_bytes += rs.dfa[i] != '\n';      // k_fa_seq_bytes
    }
    const u64 seq_size = meta ? meta->seq_size : lw + ctl->rest_bytes;

    VcfDev d{};
    d.fasta = rs.dfa + (w.cbase - w.up0); d.fasta_n = fasta_n; d.seq_start = seq_start; d.seq_size = seq_size; d.lw = lw;
    d.refc = rs.refc; d.refc_n = rs.refc_n; d.blkpre = rs.blkpre;
    d.cbase = w.cbase; d.wend = w.up1; d.oob = w.window ? &ctl->oob : nullptr;
    d.nrec = nrec; d.cur0 = range.cur0;
    auto window_check = [&](u64 v) { if (v) { r.verdict = 3; r.detail = v; } return v != 0; };
    u64 cur = range.cur0, ngrp = 0, E = 0, Q = 0;
    GrpArrays ga{};
    HapArrays ha{};
    if (nrec) {
        // grouping
        d.start = tk.start; d.reflen = tk.reflen; d.alt0 = tk.alt0; d.altstr_off = tk.altoff; d.altchars = tk.altchars;
        d.pair0 = tk.pair0; d.pair_a0 = tk.pa0; d.alleles = tk.alleles;
        u64* ends = A.get<u64>(vcf_size::per_record(nrec)); u64* flag = A.get<u64>(vcf_size::per_record(nrec));
        u64* gidx = A.get<u64>(vcf_size::per_record(nrec)); u64* grp_r0 = A.get<u64>(vcf_size::per_record(nrec));
        ctl->n = nrec;
        if (!(tk.from_host && positions_wrap(tk.host.start, tk.host.reflen))) {
            each_thread([&](HostGrid g) { rec_ends_body(d.start, d.reflen, nrec, ends, g); });
            inclusive_max_scan(ends, ends, ctl->n, &ctl->max_end);
            each_thread([&](HostGrid g) { mark_groups_body(d.start, ends, nrec, flag, g); });
        } else {
            std::vector<u64> hflag, hend;
            sweep_groups(tk.host.start, tk.host.reflen, hflag, hend);
            std::memcpy(flag, hflag.data(), 8 * nrec);
            std::memcpy(ends, hend.data(), 8 * nrec);
        }
        exclusive_scan(flag, gidx, ctl->n, &ctl->ngrp);
        each_thread([&](HostGrid g) { group_firsts_body(flag, gidx, nrec, grp_r0, &ctl->ngrp, g); });
        ngrp = ctl->ngrp;
        d.ngrp = ngrp; d.grp_r0 = grp_r0; d.incl_end = ends;
        // haplotypes and sizes
        u64* gb[14];
        for (u64*& p : gb) p = A.get<u64>(vcf_size::per_group(ngrp));
        ga = GrpArrays{gb[0], gb[1], gb[2], gb[3], gb[4], gb[5], gb[6], gb[7], gb[8], gb[9], gb[10]};
        u64 *raw0 = gb[11], *rawc0 = gb[12], *bit0 = gb[13];
        ctl->n = ngrp;
        each_thread([&](HostGrid g) { grp_count_body(d, ga, g); });
        exclusive_scan(ga.nraw, raw0, ctl->n, &ctl->nraw);
        exclusive_scan(ga.rawchars, rawc0, ctl->n, &ctl->rawchars);
        const u64 nraw_total = ctl->nraw, rawchars_total = ctl->rawchars;
        const u32 sw = (u32)std::max<u64>(1, (tk.max_samples + 63) / 64);
        ha = HapArrays{raw0, rawc0, A.get<u64>(vcf_size::per_raw(nraw_total)), A.get<u64>(vcf_size::per_raw(nraw_total)),
                       A.get<u32>(vcf_size::canon(nraw_total)), A.get<uint8_t>(vcf_size::hapchars(rawchars_total)), bit0, nullptr, sw};
        each_thread([&](HostGrid g) { grp_haps_body(d, ga, ha, g); });
        exclusive_scan(ga.bitwords, bit0, ctl->n, &ctl->bitwords);
        ha.carried = A.get<u64>(vcf_size::carried(ctl->bitwords));
        each_thread([&](HostGrid g) { grp_samples_body(d, ga, ha, g); });
        each_thread([&](HostGrid g) { grp_common_body(d, ga, g); });
        exclusive_scan(ga.eds_len, ga.eds_len, ctl->n, &ctl->eds);
        exclusive_scan(ga.seds_len, ga.seds_len, ctl->n, &ctl->seds);
        E = ctl->eds; Q = ctl->seds; cur = ga.cur_after[ngrp - 1];
        if (w.window && window_check(ctl->oob)) return r;
    }
    // tail
    u64 tail = 0;
    if (const u64 length = tail_length(cur, seq_size, range.next_start)) {
        const u64 off = seq_start + cur + cur / lw;
        cpos_body(d, off, &ctl->cpos, HostGrid{0, 1});
        tail = tail_clamp(length, rs.refc_n, ctl->cpos);
        if (w.window && tail < length && window_check(off | (1ull << 62))) return r;
    }
    // emit
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
    if (w.window && window_check(ctl->oob)) return r;
    r.eds.assign(eds, eds + Etot); r.seds.assign(seds, seds + Qtot);
    return r;
}

} // namespace
