// vcf_multi.hip — vcf2eds over several GPUs of one node from C++: position ranges (the C++ port of
// edsparser_amd/multigpu.py, VcfSharder), host code on the rank threads and exchanges of multi_gpu.hip.
//
// Groups of overlapping records (vcf_transforms.cpp:482-534) never span a cut placed at a group start, so every rank
// walks its own range of reference positions and the pieces concatenate to the whole file's text.  Every phase ends in
// the rank barrier (rank_barrier.hpp):
//   1. rank r indexes its byte range of the VCF (cut at line starts; VcfPipeline::index_device, or the host vcf_index
//      for files the device tokeniser does not take) and scans slice r of the FASTA body (VcfPipeline::fasta_slice);
//   2. all-gather of the counts, counters and slice results: every rank knows seq_size and whether the FASTA is regular;
//   3. all-gather of the (POS, REF length) arrays, 16 bytes per record;
//   4. every rank derives the same order (strictly ascending: the identity; distinct positions: a stable sort; equal
//      positions: vcf_sort_order over the whole array, the reference's std::sort) and cuts the sorted records at group
//      starts (start[j] >= max end[< j]).  Wrapped positions (POS 0): not partitioned, rank 0 transforms the whole file;
//   5. record lines move to the rank that owns them, as runs of lines adjacent in the file and in the sorted order;
//   6. every rank runs VcfPipeline::run on its lines (presorted, cur0 = its first group start, next_start = the next
//      rank's) with the FASTA window of its range (a regular FASTA) or the whole FASTA;
//   7. all-gather of the piece sizes; 8. every rank copies its piece to its offset of the output.
#include "multi_gpu.hpp"

#include <algorithm>
#include <cstring>

namespace edsx {

namespace {

// vcf_cut, fasta_meta, plan_vcf_cuts, line_runs and Run: vcf_host.hpp (plain host code, tested on the CPU)

struct VcfHead {                // exchanged as it is
    u64 nrec, total, processed, malformed, unsupported;
    FaSlice slice;
};

} // namespace

struct MultiMsa::VcfShared {
    const uint8_t* vcf; u64 vcf_n; const uint8_t* fasta; u64 fasta_n;
    u64 seq_start, lw, rest_from;
    HostBytes* eds; HostBytes* seds;
    VcfCounters* stats;                         // the caller's: written by rank 0 as soon as known
    std::vector<std::exception_ptr> error;      // per rank
};

void MultiMsa::run_rank_vcf(int r, VcfShared& sh)
{
    const int N = world();
    Rank& me = *ranks_[r];
    std::string fail;
    auto phase = [&](auto&& body) -> bool { return rank_phase(*bar_, r, fail, body, &sh.error[r]); };
    hipStream_t st = nullptr;
    static const uint8_t none = 0;
    const u64 lo = vcf_cut(sh.vcf, sh.vcf_n, r, N), hi = vcf_cut(sh.vcf, sh.vcf_n, r + 1, N);
    const u64 body = sh.fasta_n - sh.seq_start;
    const u64 sa = sh.seq_start + (u64)((unsigned __int128)body * (unsigned)r / (unsigned)N);
    const u64 sb = sh.seq_start + (u64)((unsigned __int128)body * (unsigned)(r + 1) / (unsigned)N);
    std::vector<u64> pos, reflen, loff, llen;
    VcfHead mine{};
    u64 h2d = 0;
    std::vector<uint8_t> pr;

    // ---- 1. index of my byte range, my slice of the FASTA body
    if (!phase([&] {
            EDSX_HIP(hipSetDevice(me.device));
            if (!me.vcf) me.vcf.reset(new VcfPipeline());
            VcfCounters c;
            const uint8_t* v = hi > lo ? sh.vcf + lo : &none;
            if (!me.vcf->index_device(v, hi - lo, st, pos, reflen, loff, llen, c)) vcf_index(v, hi - lo, pos, reflen, loff, llen, c);
            mine.nrec = pos.size();
            mine.total = c.total_variants; mine.processed = c.processed_variants;
            mine.malformed = c.skipped_malformed; mine.unsupported = c.skipped_unsupported_sv;
            mine.slice = me.vcf->fasta_slice(sh.fasta, sa, sb, sh.seq_start, sh.rest_from, sh.lw, st, h2d);
            pr.resize(16 * pos.size());
            if (!pos.empty()) {
                std::memcpy(pr.data(), pos.data(), 8 * pos.size());
                std::memcpy(pr.data() + 8 * pos.size(), reflen.data(), 8 * pos.size());
            }
        })) return;

    // ---- 2. counts, counters, FASTA slices
    std::vector<VcfHead> heads(N);
    if (!phase([&] { xch_->all_gather(r, &mine, sizeof(VcfHead), heads.data()); })) return;
    std::vector<u64> base(N + 1, 0);
    VcfCounters tot;
    std::vector<FaSlice> slices(N);
    for (int k = 0; k < N; k++) {
        base[k + 1] = base[k] + heads[k].nrec;
        tot.total_variants += heads[k].total; tot.processed_variants += heads[k].processed;
        tot.skipped_malformed += heads[k].malformed; tot.skipped_unsupported_sv += heads[k].unsupported;
        slices[k] = heads[k].slice;
    }
    const FastaMeta meta = fasta_meta(slices.data(), N, sh.seq_start, sh.lw, sh.fasta_n);
    const u64 n = base[N];
    if (r == 0) *sh.stats = tot;
    if (!phase([&] {
            // the single transform refuses this after its tokeniser has counted the records (vcf_device.hip)
            if (sh.lw == 0) throw FormatError("Invalid FASTA format: empty first sequence line");
            if (n >= 0xffffffffull) throw FormatError("VCF has too many records for this build");
        })) return;

    // ---- 3. (POS, REF length) of every record
    std::vector<uint8_t> all;
    std::vector<u64> sizes;
    if (!phase([&] { xch_->all_gather_v(r, N, pr.data(), pr.size(), all, sizes); })) return;

    // ---- 4. the same order and cuts on every rank; 5. (local) my lines for every destination
    VcfPlan plan;                                              // order, sorted record starts (POS - 1), cuts, wraps
    std::vector<Run> keep;                                     // my lines that stay here
    std::vector<uint8_t> payload;                              // per destination: nruns, nbytes, k[], nbytes[], text
    u64 moved = 0;
    if (!phase([&] {
            const size_t cap = all.size() / (size_t)N;
            std::vector<u64> gpos(n), gref(n);
            for (int k = 0; k < N; k++) {
                const u64 m = heads[k].nrec;
                if (!m) continue;
                std::memcpy(gpos.data() + base[k], all.data() + (size_t)k * cap, 8 * m);
                std::memcpy(gref.data() + base[k], all.data() + (size_t)k * cap + 8 * m, 8 * m);
            }
            std::vector<uint8_t>().swap(all);
            plan = plan_vcf_cuts(gpos, gref, N);
            if (plan.wraps) return;
            // my records of every destination's range, as runs of lines
            for (int d = 0; d < N; d++) {
                std::vector<Run> runs = line_runs(plan.order, plan.cuts[d], plan.cuts[d + 1], base[r], base[r + 1], sh.vcf, lo, loff, llen);
                if (d == r) { keep = std::move(runs); continue; }
                u64 nb = 0;
                for (const Run& x : runs) nb += x.n;
                moved += nb;
                const u64 hdr[2] = {runs.size(), nb};
                const size_t at = payload.size();
                payload.resize(at + 16 + 16 * runs.size() + nb);
                uint8_t* p = payload.data() + at;
                std::memcpy(p, hdr, 16); p += 16;
                for (const Run& x : runs) { std::memcpy(p, &x.k, 8); p += 8; }
                for (const Run& x : runs) { std::memcpy(p, &x.n, 8); p += 8; }
                for (const Run& x : runs) { std::memcpy(p, x.p, x.n); p += x.n; }
            }
        })) return;

    // ---- wrapped positions: not partitioned, rank 0 runs the unpartitioned transform on the whole file
    if (plan.wraps) {
        if (!phase([&] {
                if (r != 0) return;
                VcfCounters c;
                me.vcf->run(sh.vcf_n ? sh.vcf : &none, sh.vcf_n, sh.fasta, sh.fasta_n, *sh.eds, *sh.seds, c, st);
                *sh.stats = c;
            })) return;
        const u64 mine_h2d = r == 0 ? h2d + me.vcf->fasta_h2d_bytes() : h2d;
        std::vector<u64> h2ds(N);
        if (!phase([&] { xch_->all_gather(r, &mine_h2d, 8, h2ds.data()); })) return;
        if (r == 0) {
            vcf_info_.fasta_h2d_bytes_max = *std::max_element(h2ds.begin(), h2ds.end());
            vcf_info_.records_min = vcf_info_.records_max = n;
        }
        return;
    }

    // ---- 5. record lines that change rank
    std::vector<uint8_t> got;
    std::vector<u64> got_sizes;
    if (!phase([&] { xch_->all_gather_v(r, N, payload.data(), payload.size(), got, got_sizes); })) return;

    // ---- 6. my lines in sorted order -> my range of the transform
    const std::vector<u64>&cuts = plan.cuts, &start = plan.start;
    std::vector<int> nonempty;
    for (int k = 0; k < N; k++) if (cuts[k] < cuts[k + 1]) nonempty.push_back(k);
    const u64 n_mine = cuts[r + 1] - cuts[r];
    HostBytes pe, ps;
    VcfCounters rc;
    if (!phase([&] {
            const size_t cap = got.size() / (size_t)N;
            std::vector<Run> runs = keep;
            for (int k = 0; k < N; k++) {
                if (k == r) continue;
                const uint8_t* p = got.data() + (size_t)k * cap;
                for (int d = 0; d < N; d++) {
                    if (d == k) continue;
                    u64 hdr[2];
                    std::memcpy(hdr, p, 16);
                    const uint8_t* ks = p + 16;
                    const uint8_t* ns = ks + 8 * hdr[0];
                    const uint8_t* text = ns + 8 * hdr[0];
                    if (d == r)
                        for (u64 i = 0; i < hdr[0]; i++) {
                            Run x;
                            std::memcpy(&x.k, ks + 8 * i, 8);
                            std::memcpy(&x.n, ns + 8 * i, 8);
                            x.p = text;
                            text += x.n;
                            runs.push_back(x);
                        }
                    p += 16 + 16 * hdr[0] + hdr[1];
                }
            }
            std::sort(runs.begin(), runs.end(), [](const Run& x, const Run& y) { return x.k < y.k; });
            std::vector<uint8_t> lines;
            u64 total = 0;
            for (const Run& x : runs) total += x.n + 1;
            lines.reserve(total);
            for (size_t i = 0; i < runs.size(); i++) {
                if (i) lines.push_back('\n');
                lines.insert(lines.end(), runs[i].p, runs[i].p + runs[i].n);
            }
            const bool runs_here = n_mine > 0 || (nonempty.empty() && r == 0);   // an empty VCF: rank 0, the bare reference
            if (!runs_here) return;
            EDSX_HIP(hipSetDevice(me.device));
            const bool first = nonempty.empty() || r == nonempty[0];
            VcfRange range;
            range.presorted = true;
            range.cur0 = first ? 0 : start[cuts[r]];
            for (int k : nonempty) if (k > r) { range.next_start = start[cuts[k]]; break; }
            range.fasta = &meta;
            me.vcf->run(lines.empty() ? &none : lines.data(), lines.size(), sh.fasta, sh.fasta_n, pe, ps, rc, st, range);
            h2d += me.vcf->fasta_h2d_bytes();
        })) return;

    // ---- 7. piece sizes, groups, moved bytes, FASTA bytes copied
    const u64 my[5] = {pe.size, ps.size, rc.variant_groups, moved, h2d};
    std::vector<u64> piece(5 * (size_t)N);
    if (!phase([&] { xch_->all_gather(r, my, sizeof(my), piece.data()); })) return;
    u64 eoff, soff, etot, stot;
    piece_offsets(piece, 5, r, eoff, soff, etot, stot);
    if (!phase([&] {
            if (r != 0) return;
            sh.eds->take(etot); sh.seds->take(stot);
            VcfMultiInfo& info = vcf_info_;
            info.partitioned = nonempty.size() >= 2;
            info.fasta_windowed = meta.regular;
            for (int k = 0; k < N; k++) {
                sh.stats->variant_groups += piece[5 * k + 2];
                info.moved_line_bytes += piece[5 * k + 3];
                info.fasta_h2d_bytes_max = std::max(info.fasta_h2d_bytes_max, piece[5 * k + 4]);
            }
            for (size_t i = 0; i < nonempty.size(); i++) {
                const u64 m = cuts[nonempty[i] + 1] - cuts[nonempty[i]];
                info.records_min = i ? std::min(info.records_min, m) : m;
                info.records_max = std::max(info.records_max, m);
            }
        })) return;

    // ---- 8. every rank copies its piece to its offset
    phase([&] {
        if (pe.size) std::memcpy(sh.eds->data + eoff, pe.data, pe.size);
        if (ps.size) std::memcpy(sh.seds->data + soff, ps.data, ps.size);
    });
}

void MultiMsa::vcf_transform(const uint8_t* vcf, size_t vcf_n, const uint8_t* fasta, size_t fasta_n, HostBytes& eds, HostBytes& seds,
                             VcfCounters& stats)
{
    static const uint8_t none = 0;
    const int N = world();
    stats = VcfCounters();
    vcf_info_ = VcfMultiInfo();
    VcfShared sh;
    sh.vcf = vcf_n ? vcf : &none; sh.vcf_n = vcf_n; sh.fasta = fasta_n ? fasta : &none; sh.fasta_n = fasta_n;
    // header and first line on the host, with the unpartitioned transform's error texts (and, like it, no counters yet)
    fasta_head(sh.fasta, fasta_n, sh.seq_start, sh.lw, sh.rest_from);
    sh.eds = &eds; sh.seds = &seds; sh.stats = &stats;
    sh.error.assign(N, nullptr);
    run_ranks([&](int r) { run_rank_vcf(r, sh); }, &sh.error);
}

void MultiMsa::leds_merge(HostBytes& eds, HostBytes& seds, uint32_t context_len)
{
    Rank& r0 = *ranks_[0];
    EDSX_HIP(hipSetDevice(r0.device));
    if (!r0.merge) r0.merge.reset(new MergePipeline());
    HostBytes lo, so;
    r0.merge->run(r0.merge_eds, eds.data, eds.size, seds.data, seds.size, context_len, true, lo, so, nullptr);
    std::swap(eds.data, lo.data); std::swap(eds.size, lo.size);
    std::swap(seds.data, so.data); std::swap(seds.size, so.size);
}

} // namespace edsx
