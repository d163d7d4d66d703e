// test_vcf_walk.cpp — the VCF -> EDS overlay on the CPU: the per-thread device code of edsparser_amd/csrc/vcf_walk.hpp run
// one "thread" after another, and the host code of the path (csrc/vcf_host.hpp: FASTA head, host tokeniser, records -> SoA,
// the sweep for wrapped positions, window and tail arithmetic, the planner of a partitioned run) as the library compiles
// it, over a case file written by tests/vcf_walk_cases.py; meant to be built with -fsanitize=address,undefined.  Every
// buffer is a heap block of its own, of exactly the size VcfPipeline asks for (vcf_size::*, and upload()'s for the host
// tokeniser's arrays), filled with a byte the case chooses, so the first byte nobody asked for is a redzone; the two texts
// are 256-byte aligned as on the device.  The steps the device does with wave operations (line starts, reference
// compaction, scans, the sort of distinct positions, the common-text copy, the FASTA slice scan) are the plain loops below.
//
// Case records (little endian): u32 mode, u32 nfills, nfills bytes, u32 name_len, name, u64 vcf_len, vcf, u64 fasta_len,
// fasta, u64 a0, a1, a2, a3.
//   mode 0: whole transform, device tokeniser only   1: up to the count pass   2: fa_cpos over the window [a0, a1)
//   3: fa_cpos over the whole file   4: whole transform as the library runs it: the host tokeniser where the count pass
//   says "not plain"   5: one position range: the lines are presorted, cur0 = a0, next_start = a1, FastaMeta{a2, a3}
//   6: the planner of a partitioned run over a0 ranks (result: u64 words in `eds`, the runs' text in `seds`, see plan())
// One result per (case, fill): u32 name_len, name, u32 fill, u32 verdict, u64 detail, u64 eds_len, eds, u64 seds_len,
// seds.   verdict 0: accepted (texts follow)   1: not plain, the host tokeniser's   3: a byte index outside the text or
// the window was reported (detail)   4: refused input (the library throws)   5: fa_cpos differs from the byte-by-byte
// count at file offset `detail`
// The arena, the tokenisers, the reference stream and the whole transform are in vcf_walk_twin.hpp, which
// test_contig_walk.cpp shares.
#include "vcf_walk_twin.hpp"

namespace {

// fa_cpos alone: every file offset from cbase to fasta_n + 2 against a byte-by-byte count
Result cpos_sweep(uint8_t fill, const std::vector<uint8_t>& fa, u64 up0, u64 up1, bool window)
{
    Result r;
    Arena A(fill);
    VcfCtl* ctl = A.get<VcfCtl>(vcf_size::ctl());
    *ctl = VcfCtl{};
    u64 seq_start = 0, lw = 0, rest_from = 0;
    const u64 fasta_n = fa.size();
    if (!head_of(fa, seq_start, lw, rest_from) || up0 > up1 || up1 > fasta_n || (window && up0 < seq_start)) { r.verdict = 4; return r; }
    if (!window) { up0 = 0; up1 = fasta_n; }
    const RefWindow w{window, up0, up1, window ? up0 : seq_start};
    const RefStream rs = reference_stream(A, fa, w, seq_start, ctl);
    VcfDev d{};
    d.fasta = rs.dfa + (w.cbase - up0); d.fasta_n = fasta_n; d.seq_start = seq_start; d.lw = lw;
    d.refc = rs.refc; d.refc_n = rs.refc_n; d.blkpre = rs.blkpre; d.cbase = w.cbase; d.wend = up1; d.oob = window ? &ctl->oob : nullptr;
    u64 want = 0;                                                      // kept bytes in [cbase, off)
    for (u64 off = w.cbase; off < fasta_n + 2; off++) {
        ctl->oob = 0;
        cpos_body(d, off, &ctl->cpos, HostGrid{0, 1});
        const bool outside = off >= fasta_n || off >= up1;
        const u64 expect = outside ? rs.refc_n : want;
        const u64 expect_oob = window && off < fasta_n && off > up1 ? (off | (1ull << 63)) : 0;
        if (ctl->cpos != expect || ctl->oob != expect_oob) { r.verdict = 5; r.detail = off; return r; }
        if (off < up1) want += fa[off] != '\n' && fa[off] != '\r';
    }
    return r;
}

// VcfPipeline::fasta_slice with its two kernels as loops: slice [a, b) of the FASTA body
FaSlice fasta_slice(const std::vector<uint8_t>& fa, u64 a, u64 b, u64 seq_start, u64 rest_from, u64 lw)
{
    FaSlice r{~0ull, 0, 0, ~0ull};
    if (a >= b) return r;
    for (u64 i = std::max(a, rest_from); i < b; i++) if (fa[i] == '>' && fa[i - 1] == '\n') { r.rec_end = i; break; }   // k_fa_slice_end
    const u64 hi = std::min(r.rec_end, b), period = lw + 1;                                                           // k_fa_slice_scan
    for (u64 i = a; i < hi; i++) {
        const bool grid = (i - seq_start) % period == lw;
        r.count += fa[i] != '\n';
        if (fa[i] == '\r') r.flags |= 1;
        if (grid && fa[i] != '\n') r.flags |= 2;
        if (!grid && fa[i] == '\n' && i < r.offgrid) r.offgrid = i;
    }
    return r;
}

// Phases 1 to 4 of MultiMsa::run_rank_vcf for all N ranks at once, without the exchanges.  Words: has_meta, seq_size,
// regular; per rank lo, hi; n, wraps, cuts[N + 1], order[n], start[n]; unless wraps, per (rank, destination): the number of
// runs, their k, their byte counts - and their text, back to back, in `seds`.
Result plan(const std::vector<uint8_t>& vcf, const std::vector<uint8_t>& fa, int N)
{
    static const uint8_t none = 0;
    Result r;
    std::vector<u64> words;
    const uint8_t* v = vcf.empty() ? &none : vcf.data();
    u64 seq_start = 0, lw = 0, rest_from = 0;
    FastaMeta meta;
    const bool has_meta = head_of(fa, seq_start, lw, rest_from);
    if (has_meta) {
        std::vector<FaSlice> slices(N);
        const u64 body = fa.size() - seq_start;
        for (int k = 0; k < N; k++)
            slices[k] = fasta_slice(fa, seq_start + (u64)((unsigned __int128)body * (unsigned)k / (unsigned)N),
                                    seq_start + (u64)((unsigned __int128)body * (unsigned)(k + 1) / (unsigned)N), seq_start, rest_from, lw);
        meta = fasta_meta(slices.data(), N, seq_start, lw, fa.size());
    }
    words.insert(words.end(), {(u64)has_meta, meta.seq_size, (u64)meta.regular});
    std::vector<u64> gpos, gref, base(N + 1, 0), lo(N), hi(N);
    std::vector<std::vector<u64>> loff(N), llen(N);
    for (int k = 0; k < N; k++) {
        lo[k] = vcf_cut(v, vcf.size(), k, N); hi[k] = vcf_cut(v, vcf.size(), k + 1, N);
        words.push_back(lo[k]); words.push_back(hi[k]);
        std::vector<u64> pos, reflen;
        VcfCounters c;
        vcf_index(hi[k] > lo[k] ? v + lo[k] : &none, hi[k] - lo[k], pos, reflen, loff[k], llen[k], c);
        gpos.insert(gpos.end(), pos.begin(), pos.end()); gref.insert(gref.end(), reflen.begin(), reflen.end());
        base[k + 1] = gpos.size();
    }
    const VcfPlan p = plan_vcf_cuts(gpos, gref, N);
    words.push_back(gpos.size()); words.push_back(p.wraps);
    words.insert(words.end(), p.cuts.begin(), p.cuts.end());
    words.insert(words.end(), p.order.begin(), p.order.end());
    words.insert(words.end(), p.start.begin(), p.start.end());
    if (!p.wraps)
        for (int k = 0; k < N; k++)
            for (int d = 0; d < N; d++) {
                const std::vector<Run> runs = line_runs(p.order, p.cuts[d], p.cuts[d + 1], base[k], base[k + 1], v, lo[k], loff[k], llen[k]);
                words.push_back(runs.size());
                for (const Run& x : runs) words.push_back(x.k);
                for (const Run& x : runs) words.push_back(x.n);
                for (const Run& x : runs) r.seds.insert(r.seds.end(), x.p, x.p + x.n);
            }
    r.eds.resize(8 * words.size());
    if (!words.empty()) std::memcpy(r.eds.data(), words.data(), r.eds.size());
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
        u64 a[4];
        for (u64& x : a) x = u64at();
        for (uint8_t fill : fills) {
            Result r;
            if (mode <= 1) r = transform(fill, vcf, fa, mode == 1, false);
            else if (mode <= 3) r = cpos_sweep(fill, fa, a[0], a[1], mode == 2);
            else if (mode == 4) r = transform(fill, vcf, fa, false, true);
            else if (mode == 5) {
                const FastaMeta meta{a[2], a[3] != 0};
                VcfRange range;
                range.presorted = true; range.cur0 = a[0]; range.next_start = a[1]; range.fasta = &meta;
                r = transform(fill, vcf, fa, false, true, range);
            } else r = plan(vcf, fa, (int)a[0]);
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
