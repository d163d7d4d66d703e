// vcf_host.hpp — the host code of the VCF -> EDS overlay, without a HIP include (as path_records.hpp, lift_core.hpp and
// slice_core.hpp): FASTA head, the tokeniser for files the device tokeniser does not accept and the reference's sort —
// the text-parsing front end of src/cpp/lib/transforms/vcf_transforms.cpp (:51-86, :142-326, :715-718) —, the records
// -> SoA build, the host sweep for wrapped positions, the window and tail arithmetic of a position range
// (VcfPipeline::run, vcf_device.hip) and the planning of a partitioned run (MultiMsa::run_rank_vcf, vcf_multi.hip).
// hipcc compiles it into the library, g++ into tests/cpp/test_vcf_walk.cpp, which runs it under the sanitizers.
#pragma once

#include "errors.hpp"
#include "vcf_walk.hpp"

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace edsx {

struct VcfCounters {   // vcf_transforms.hpp:24-35
    u64 total_variants = 0, processed_variants = 0, skipped_malformed = 0, skipped_unsupported_sv = 0, variant_groups = 0;
};

// FASTA metadata of a partitioned run, found once over the slices of all ranks (VcfPipeline::fasta_slice, fasta_meta below).
// regular: the file is one record without '\r' or blank lines, and every line but its last (non-empty) one has exactly the first
// line's width lw, so position p sits at file offset seq_start + p + p / lw (vcf_transforms.cpp:98-129 read it there)
// and a range of positions can be read from a window of the file.
struct FastaMeta { u64 seq_size = 0; bool regular = false; };
// one rank's slice [a, b) of the FASTA body, exchanged as it is: the first "\n>" in it (its '>', ~0: none), and in front of
// that: the bytes that are not '\n', flags (1: '\r', 2: a byte on the line grid of width lw + 1 that is not '\n'), the
// first '\n' off that grid (~0: none)
struct FaSlice { u64 rec_end, count, flags, offgrid; };

// One position range of a partitioned run: the records are handed over in their final order, the
// walk starts at cur0 (no common text in front of the first group when cur0 is its start) and the closing common
// text stops at the first group of the next range.
struct VcfRange {
    bool presorted = false;
    u64 cur0 = 0;
    u64 next_start = ~0ull;        // ~0: last (or only) range, flush to the end of the reference
    // set: seq_size comes from here, and a regular file is read from the window [off(cur0), off(end)) only (end =
    // next_start, or seq_size for the last range; 16 bytes of slack, clipped to the file); otherwise the whole file
    const FastaMeta* fasta = nullptr;
};

inline bool next_line(const uint8_t* f, size_t n, size_t& pos, std::string& line, bool* hit_eof = nullptr)
{
    if (pos >= n) return false;
    const uint8_t* nl = static_cast<const uint8_t*>(memchr(f + pos, '\n', n - pos));
    size_t end = nl ? static_cast<size_t>(nl - f) : n;
    line.assign(reinterpret_cast<const char*>(f + pos), end - pos);
    if (hit_eof) *hit_eof = (nl == nullptr);
    pos = nl ? end + 1 : n;
    return true;
}

// header line and first sequence line (:51-86) with the reference's error texts: sequence start, width of the first
// line, offset of the second line
inline void fasta_head(const uint8_t* fasta, size_t fasta_n, u64& seq_start, u64& lw, u64& rest_from)
{
    size_t pos = 0;
    std::string line;
    bool eof = false;
    if (!next_line(fasta, fasta_n, pos, line, &eof) || line.empty() || line[0] != '>')
        throw FormatError("Invalid FASTA format: expected header line starting with '>'");
    seq_start = eof ? fasta_n : pos;
    if (!next_line(fasta, fasta_n, pos, line)) throw FormatError("FASTA file is empty");
    lw = line.size();
    rest_from = pos;
}

enum class Skip { NONE, HEADER, MALFORMED, UNSUPPORTED_SV };

// Records of one stretch of the file, flat (no allocation per record): record i has alts
// [alt0[i], alt0[i+1]) with characters altoff[..] .. altoff[..+1], and samples [gt0[i], gt0[i+1]) with
// alleles gtoff[..] .. gtoff[..+1].
struct VcfPart {
    std::vector<u64> pos, reflen;
    std::vector<u64> alt0{0}, altoff{0};
    std::vector<uint8_t> altchars;
    std::vector<u64> gt0{0}, gtoff{0};
    std::vector<int> alleles;
    std::vector<u64> loff, llen;                             // line of every accepted record (index pass only)
    VcfCounters st;
    std::vector<std::string> warns;
    size_t size() const { return pos.size(); }
    void drop_open_record()                                  // undo a record that turned out unsupported
    {
        altoff.resize(alt0.back() + 1); altchars.resize(altoff.back());
        gtoff.resize(gt0.back() + 1); alleles.resize(gtoff.back());
    }
};

struct Span { const char* p; size_t n; };

// parse_genotype :190-216 — tokens between delimiters as std::getline yields them (a trailing empty one
// is not produced), "." skipped, std::stoi decides what a number is (exceptions -> token ignored)
inline void parse_gt_flat(Span gt, VcfPart& out)
{
    const char delim = memchr(gt.p, '/', gt.n) ? '/' : '|';
    size_t i = 0;
    while (i < gt.n) {
        const char* e = static_cast<const char*>(memchr(gt.p + i, delim, gt.n - i));
        const size_t end = e ? static_cast<size_t>(e - gt.p) : gt.n;
        const size_t len = end - i;
        if (!(len == 1 && gt.p[i] == '.')) {
            if (len == 1 && gt.p[i] >= '0' && gt.p[i] <= '9') out.alleles.push_back(gt.p[i] - '0');
            else {
                try { out.alleles.push_back(std::stoi(std::string(gt.p + i, len))); } catch (...) {}
            }
        }
        i = end + 1;
    }
}

// parse_vcf_line :232-326 into the flat store; `fields` is scratch
inline Skip parse_line_flat(const char* line, size_t n, VcfPart& out, std::vector<Span>& fields, bool light = false)
{
    if (n == 0 || line[0] == '#') return Skip::HEADER;
    fields.clear();
    for (size_t i = 0; i < n;) {                             // std::getline(ss, tok, '\t'), empty tokens dropped
        const char* e = static_cast<const char*>(memchr(line + i, '\t', n - i));
        const size_t end = e ? static_cast<size_t>(e - line) : n;
        if (end > i) fields.push_back(Span{line + i, end - i});
        i = end + 1;
    }
    if (fields.size() < 5) {                                 // ws >> tok
        fields.clear();
        size_t i = 0;
        while (i < n) {
            while (i < n && std::isspace((unsigned char)line[i])) i++;
            size_t j = i;
            while (j < n && !std::isspace((unsigned char)line[j])) j++;
            if (j > i) fields.push_back(Span{line + i, j - i});
            i = j;
        }
    }
    if (fields.size() < 5) return Skip::MALFORMED;
    u64 pos;
    try { pos = std::stoull(std::string(fields[1].p, fields[1].n)); } catch (...) { return Skip::MALFORMED; }
    const Span ref = fields[3];
    // parse_alt_field :142-176 — std::getline(ss, a, ','): empty tokens kept, except one behind the last comma
    const Span alt = fields[4];
    for (size_t i = 0; i < alt.n;) {
        const char* e = static_cast<const char*>(memchr(alt.p + i, ',', alt.n - i));
        const size_t end = e ? static_cast<size_t>(e - alt.p) : alt.n;
        const char* a = alt.p + i;
        const size_t len = end - i;
        if (len && a[0] == '<' && a[len - 1] == '>') {
            const size_t tl = len >= 2 ? len - 2 : 0;        // "<" alone: substr(1, npos-ish) is empty in the reference too
            const std::string t = len >= 2 ? std::string(a + 1, tl) : std::string();
            if (t == "DEL") { out.altoff.push_back(out.altchars.size()); }
            else if (t == "INS") { out.altchars.insert(out.altchars.end(), ref.p, ref.p + ref.n); out.altoff.push_back(out.altchars.size()); }
            else {
                out.drop_open_record();
                out.warns.push_back("Warning: Skipping variant at " + std::string(fields[0].p, fields[0].n) + ":" +
                                    std::to_string(pos) + " - Unsupported structural variant type: " + t);
                return Skip::UNSUPPORTED_SV;
            }
        } else { out.altchars.insert(out.altchars.end(), a, a + len); out.altoff.push_back(out.altchars.size()); }
        i = end + 1;
    }
    if (fields.size() >= 10 && !light)
        for (size_t f = 9; f < fields.size(); f++) {
            Span gt = fields[f];
            const char* c = static_cast<const char*>(memchr(gt.p, ':', gt.n));
            if (c) gt.n = static_cast<size_t>(c - gt.p);
            parse_gt_flat(gt, out);
            out.gtoff.push_back(out.alleles.size());
        }
    out.pos.push_back(pos);
    out.reflen.push_back(ref.n);
    out.alt0.push_back(out.altoff.size() - 1);
    out.gt0.push_back(out.gtoff.size() - 1);
    return Skip::NONE;
}

// Lines are independent: large files are cut at line starts and tokenised by several host threads; records,
// counters and the stderr warnings are put together in file order, so the array handed to std::sort is the
// reference's.  light = positions, REF lengths and line spans only (the index pass of a partitioned run).
inline void tokenise(const uint8_t* vcf, size_t vcf_n, std::vector<VcfPart>& parts, std::vector<u64>& part_base,
                     VcfCounters& stats, bool light)
{
    auto parse_range = [&](size_t lo, size_t hi, VcfPart& out) {
        std::vector<Span> fields;
        size_t pos = lo;
        while (pos < hi && pos < vcf_n) {
            const uint8_t* nl = static_cast<const uint8_t*>(memchr(vcf + pos, '\n', vcf_n - pos));
            const size_t end = nl ? static_cast<size_t>(nl - vcf) : vcf_n;
            const Skip skip = parse_line_flat(reinterpret_cast<const char*>(vcf + pos), end - pos, out, fields, light);
            if (skip == Skip::NONE) {
                out.st.total_variants++; out.st.processed_variants++;
                if (light) { out.loff.push_back(pos); out.llen.push_back(end - pos); }
            }
            else if (skip == Skip::MALFORMED) { out.st.total_variants++; out.st.skipped_malformed++; }
            else if (skip == Skip::UNSUPPORTED_SV) { out.st.total_variants++; out.st.skipped_unsupported_sv++; }
            pos = nl ? end + 1 : vcf_n;
        }
    };
    unsigned nt = 1;
    if (vcf_n >= ((size_t)4 << 20)) {
        const unsigned hc = std::thread::hardware_concurrency();
        nt = std::max(1u, std::min(16u, hc ? hc : 4u));
    }
    std::vector<size_t> cut(nt + 1, vcf_n);
    cut[0] = 0;
    for (unsigned t = 1; t < nt; t++) {                        // first line start at or after t*n/nt
        size_t g = (size_t)((unsigned __int128)vcf_n * t / nt);
        if (g < cut[t - 1]) g = cut[t - 1];
        const uint8_t* nl = g < vcf_n ? static_cast<const uint8_t*>(memchr(vcf + g, '\n', vcf_n - g)) : nullptr;
        cut[t] = nl ? static_cast<size_t>(nl - vcf) + 1 : vcf_n;
        if (g == 0) cut[t] = 0;                                // position 0 is a line start itself
    }
    parts.clear();
    parts.resize(nt);
    if (nt == 1) parse_range(0, vcf_n, parts[0]);
    else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; t++) th.emplace_back([&, t] { parse_range(cut[t], cut[t + 1], parts[t]); });
        for (auto& x : th) x.join();
    }
    part_base.assign(nt + 1, 0);
    for (unsigned t = 0; t < nt; t++) {
        const VcfPart& pt = parts[t];
        part_base[t + 1] = part_base[t] + pt.size();
        stats.total_variants += pt.st.total_variants; stats.processed_variants += pt.st.processed_variants;
        stats.skipped_malformed += pt.st.skipped_malformed; stats.skipped_unsupported_sv += pt.st.skipped_unsupported_sv;
        for (const auto& w : pt.warns) fprintf(stderr, "%s\n", w.c_str());   // the reference warns on stderr (:301-302)
    }
    if (part_base[nt] >= 0xffffffffull) throw FormatError("VCF has too many records for this build");
}

// the reference's std::sort call (:715-718) on (pos, file index) pairs
inline void sort_like_reference(std::vector<std::pair<u64, u32>>& order)
{
    std::sort(order.begin(), order.end(),
              [](const std::pair<u64, u32>& a, const std::pair<u64, u32>& b) { return a.first < b.first; });
}

// ---- index pass and sort order of a partitioned run (VCF row) ------------------------------
// positions, REF lengths and line spans of the accepted records, file order
inline void vcf_index(const uint8_t* vcf, size_t vcf_n, std::vector<u64>& pos, std::vector<u64>& reflen, std::vector<u64>& line_off,
                      std::vector<u64>& line_len, VcfCounters& stats)
{
    stats = VcfCounters();
    std::vector<VcfPart> parts;
    std::vector<u64> part_base;
    tokenise(vcf, vcf_n, parts, part_base, stats, true);
    const size_t n = part_base.back();
    pos.clear(); reflen.clear(); line_off.clear(); line_len.clear();
    pos.reserve(n); reflen.reserve(n); line_off.reserve(n); line_len.reserve(n);
    for (const VcfPart& pt : parts) {
        pos.insert(pos.end(), pt.pos.begin(), pt.pos.end());
        reflen.insert(reflen.end(), pt.reflen.begin(), pt.reflen.end());
        line_off.insert(line_off.end(), pt.loff.begin(), pt.loff.end());
        line_len.insert(line_len.end(), pt.llen.begin(), pt.llen.end());
    }
}

// permutation the reference's std::sort (vcf_transforms.cpp:715-718) gives an array with these positions
inline void vcf_sort_order(const u64* pos, size_t n, u32* order_out)
{
    std::vector<std::pair<u64, u32>> order(n);
    for (size_t i = 0; i < n; i++) order[i] = {pos[i], (u32)i};
    sort_like_reference(order);
    for (size_t i = 0; i < n; i++) order_out[i] = order[i].second;
}

// ---- host tokeniser's records -> what the kernels read ----------------------------------------------------------
// (pos, global index in file order) of every record of the parts, sorted by pos.  std::sort's permutation depends only on
// the outcomes of its comparisons, so sorting (pos, index) pairs by pos ends in the order the reference's sort of whole
// records ends in.  A position range of a partitioned run hands its records over in their final order (the order of the
// whole file's sort, edsx_vcf_sort_order): sorting the slice again could permute equal positions differently.
inline std::vector<std::pair<u64, u32>> host_order(const std::vector<VcfPart>& parts, const std::vector<u64>& part_base, bool presorted)
{
    const unsigned nt = (unsigned)parts.size();
    std::vector<std::pair<u64, u32>> order(part_base[nt]);
    for (unsigned t = 0; t < nt; t++)
        for (size_t i = 0; i < parts[t].size(); i++) order[part_base[t] + i] = {parts[t].pos[i], (u32)(part_base[t] + i)};
    if (!presorted) sort_like_reference(order);
    return order;
}

// the record SoA of VcfDev in sorted order: start (POS - 1), reflen, and the two two-level CSRs with their closing offsets
struct VcfSoA {
    std::vector<u64> start, reflen, alt0, altoff, pair0, pa0;
    std::vector<uint8_t> altchars;
    std::vector<int> alleles;
    u64 max_samples = 0;
};
// two passes: sizes -> offsets (serial prefix sums), then the fill by several host threads
inline VcfSoA build_soa(const std::vector<VcfPart>& parts, const std::vector<u64>& part_base, const std::vector<std::pair<u64, u32>>& order)
{
    // record j of the sorted order -> (part, index in part)
    auto locate = [&](u64 j, const VcfPart*& pt) -> size_t {
        const u64 g = order[j].second;
        size_t t = std::upper_bound(part_base.begin(), part_base.end(), g) - part_base.begin() - 1;
        pt = &parts[t];
        return (size_t)(g - part_base[t]);
    };
    const u64 nrec = order.size();
    VcfSoA s;
    s.start.resize(nrec); s.reflen.resize(nrec);
    s.alt0.resize(nrec + 1); s.pair0.resize(nrec + 1);
    std::vector<u64> altc0(nrec + 1), gtc0(nrec + 1);        // first alt char / first allele of record j
    s.alt0[0] = 0; s.pair0[0] = 0; altc0[0] = 0; gtc0[0] = 0;
    for (u64 j = 0; j < nrec; j++) {
        const VcfPart* pt;
        const size_t i = locate(j, pt);
        const u64 na = pt->alt0[i + 1] - pt->alt0[i], ng = pt->gt0[i + 1] - pt->gt0[i];
        s.alt0[j + 1] = s.alt0[j] + na;
        s.pair0[j + 1] = s.pair0[j] + ng;
        altc0[j + 1] = altc0[j] + (pt->altoff[pt->alt0[i + 1]] - pt->altoff[pt->alt0[i]]);
        gtc0[j + 1] = gtc0[j] + (pt->gtoff[pt->gt0[i + 1]] - pt->gtoff[pt->gt0[i]]);
        s.max_samples = std::max<u64>(s.max_samples, ng);
    }
    s.altoff.resize(s.alt0[nrec] + 1); s.pa0.resize(s.pair0[nrec] + 1);
    s.altchars.resize(altc0[nrec]);
    s.alleles.resize(gtc0[nrec]);
    s.altoff[s.alt0[nrec]] = altc0[nrec];
    s.pa0[s.pair0[nrec]] = gtc0[nrec];
    const unsigned hc = std::thread::hardware_concurrency();
    const unsigned ft = nrec >= 65536 ? std::max(1u, std::min(16u, hc ? hc : 4u)) : 1u;
    auto fill = [&](u64 lo, u64 hi) {
        for (u64 j = lo; j < hi; j++) {
            const VcfPart* pt;
            const size_t i = locate(j, pt);
            s.start[j] = pt->pos[i] - 1;                       // wraps for POS 0 like the reference's size_t
            s.reflen[j] = pt->reflen[i];
            const u64 a0 = pt->alt0[i], a1 = pt->alt0[i + 1], cbase = pt->altoff[a0];
            for (u64 a = a0; a < a1; a++) s.altoff[s.alt0[j] + (a - a0)] = altc0[j] + (pt->altoff[a] - cbase);
            if (pt->altoff[a1] > cbase) memcpy(s.altchars.data() + altc0[j], pt->altchars.data() + cbase, pt->altoff[a1] - cbase);
            const u64 g0 = pt->gt0[i], g1 = pt->gt0[i + 1], ebase = pt->gtoff[g0];
            for (u64 g = g0; g < g1; g++) s.pa0[s.pair0[j] + (g - g0)] = gtc0[j] + (pt->gtoff[g] - ebase);
            if (pt->gtoff[g1] > ebase)
                memcpy(s.alleles.data() + gtc0[j], pt->alleles.data() + ebase, sizeof(int) * (pt->gtoff[g1] - ebase));
        }
    };
    if (ft == 1) fill(0, nrec);
    else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < ft; t++) th.emplace_back(fill, nrec * t / ft, nrec * (t + 1) / ft);
        for (auto& x : th) x.join();
    }
    return s;
}

// The parallel rule "a record opens a group iff its start is not below the largest end seen so far" equals the
// reference's sweep (:482-534, group_end restarts with every group) as long as starts ascend with the sort key and no end
// wraps.  POS 0 (start = 2^64 - 1) or POS near 2^64 ("-5" parses!) break that; such files are swept on the host exactly
// as the reference does it (running group end per record): flag[j] = record j opens a group, end[j] = the running end.
inline bool positions_wrap(const std::vector<u64>& start, const std::vector<u64>& reflen)
{
    bool wraps = false;
    for (u64 j = 0; j < start.size() && !wraps; j++) wraps = start[j] == ~0ull || start[j] + reflen[j] < start[j];
    return wraps;
}
inline void sweep_groups(const std::vector<u64>& start, const std::vector<u64>& reflen, std::vector<u64>& flag, std::vector<u64>& end)
{
    const u64 nrec = start.size();
    flag.resize(nrec); end.resize(nrec);
    u64 ge = 0;
    for (u64 j = 0; j < nrec; j++) {
        const u64 e = start[j] + reflen[j];
        if (j == 0 || !(start[j] < ge)) { flag[j] = 1; ge = e; }
        else { flag[j] = 0; ge = std::max(ge, e); }
        end[j] = ge;
    }
}

// ---- the reference stream of a position range ------------------------------------------------------------------
// What of the file goes to the device: all of it, or (a regular file in a partitioned run) the window of this position
// range, [off(cur0), off(end)) with 16 bytes of slack; refc / blkpre begin at file offset cbase.
struct RefWindow { bool window; u64 up0, up1, cbase; };
inline RefWindow reference_window(const VcfRange& range, const FastaMeta* meta, u64 seq_start, u64 lw, u64 fasta_n)
{
    RefWindow w{meta && meta->regular, 0, fasta_n, seq_start};
    if (w.window) {
        auto off = [&](u64 p) { return seq_start + p + p / lw; };
        const u64 p0 = std::min(range.cur0, meta->seq_size);
        const u64 p1 = std::max(p0, std::min(range.next_start, meta->seq_size));
        w.up0 = std::min<u64>(off(p0), fasta_n);
        w.up1 = std::max(w.up0, std::min<u64>(off(p1) + 16, fasta_n));
        w.cbase = w.up0;
    }
    return w;
}

// tail (:658-665): the common text behind the last group, 0: none.  A position range that is not the last one ends with
// what the reference flushes in front of the next range's first group instead (:570-578, `start > cur`); clamped exactly
// like read_fasta_region: by seq_size here and (tail_clamp) by what the file still holds behind c0 = cur's place in refc
inline u64 tail_length(u64 cur, u64 seq_size, u64 next_start)
{
    const bool last_range = next_start == ~0ull;
    if (!(cur < seq_size && (last_range || next_start > cur))) return 0;
    return last_range ? seq_size - cur : std::min<u64>(next_start - cur, seq_size - cur);
}
inline u64 tail_clamp(u64 length, u64 refc_n, u64 c0) { return std::min<u64>(length, refc_n - c0); }

// ---- planning of a partitioned run (vcf_multi.hip; the C++ port of multigpu.py) ------------------------------------
// start of the first line at or after byte n * k / world (the same rule on every rank: vcf_byte_range)
inline u64 vcf_cut(const uint8_t* v, u64 n, int k, int world)
{
    if (k <= 0) return 0;
    if (k >= world) return n;
    const u64 g = (u64)((unsigned __int128)n * (unsigned)k / (unsigned)world);
    if (g == 0) return 0;
    const void* nl = std::memchr(v + g - 1, '\n', n - (g - 1));
    return nl ? (u64)(static_cast<const uint8_t*>(nl) - v) + 1 : n;
}

// seq_size and `regular` from the slices of the FASTA body [seq_start, fasta_n), slice k = [body * k / N, body * (k + 1) / N).
// regular: one record, no '\r', every grid byte a '\n', and no '\n' off the grid but the one that ends a shorter
// (non-empty) last line
inline FastaMeta fasta_meta(const FaSlice* slices, int N, u64 seq_start, u64 lw, u64 fasta_n)
{
    FastaMeta meta;
    const u64 body = fasta_n - seq_start;
    u64 rec_end = fasta_n, flags = 0, offgrid = ~0ull;
    for (int k = 0; k < N; k++) rec_end = std::min(rec_end, slices[k].rec_end);
    for (int k = 0; k < N; k++) {
        const u64 a = seq_start + (u64)((unsigned __int128)body * (unsigned)k / (unsigned)N);
        if (a >= rec_end) continue;                            // slices behind the first record
        meta.seq_size += slices[k].count;
        flags |= slices[k].flags;
        offgrid = std::min(offgrid, slices[k].offgrid);
    }
    meta.regular = lw > 0 && rec_end == fasta_n && flags == 0 &&
                   (offgrid == ~0ull || (offgrid + 1 == rec_end && (offgrid - seq_start) % (lw + 1) != 0));
    return meta;
}

// The same order and cuts on every rank (plan_vcf_cuts): order (strictly ascending: the identity; distinct positions: a
// stable sort; equal positions: vcf_sort_order over the whole array, the reference's std::sort), the sorted record
// starts (POS - 1) and cuts[0..N] at group starts (start[j] >= every earlier end, :510): cut k is the first group start at
// or after n * k / N.  Wrapped positions (POS 0): not partitioned, every cut but the first is n.
struct VcfPlan { std::vector<u32> order; std::vector<u64> start, cuts; bool wraps = false; };
inline VcfPlan plan_vcf_cuts(const std::vector<u64>& gpos, const std::vector<u64>& gref, int N)
{
    const u64 n = gpos.size();
    VcfPlan p;
    p.cuts.assign(N + 1, 0);
    p.order.resize(n);
    std::iota(p.order.begin(), p.order.end(), 0u);
    bool ascending = true;
    for (u64 j = 1; j < n && ascending; j++) ascending = gpos[j - 1] < gpos[j];
    if (!ascending) {
        std::stable_sort(p.order.begin(), p.order.end(), [&](u32 x, u32 y) { return gpos[x] < gpos[y]; });
        bool equal = false;
        for (u64 j = 1; j < n && !equal; j++) equal = gpos[p.order[j - 1]] == gpos[p.order[j]];
        if (equal) vcf_sort_order(gpos.data(), n, p.order.data());      // the reference's std::sort decides
    }
    p.start.resize(n);
    std::vector<u64> end(n);
    for (u64 j = 0; j < n; j++) {
        p.start[j] = gpos[p.order[j]] - 1;                     // wraps for POS 0 like the reference's size_t
        end[j] = p.start[j] + gref[p.order[j]];
        p.wraps |= p.start[j] == ~0ull || end[j] < p.start[j];
    }
    p.cuts[N] = n;
    if (p.wraps) { for (int k = 1; k < N; k++) p.cuts[k] = n; return p; }
    std::vector<u64> gstarts;
    u64 mx = 0;
    for (u64 j = 0; j < n; j++) {
        if (j == 0 || p.start[j] >= mx) gstarts.push_back(j);
        mx = j == 0 ? end[j] : std::max(mx, end[j]);
    }
    for (int k = 1; k < N; k++) {
        const u64 target = (u64)((unsigned __int128)n * (unsigned)k / (unsigned)N);
        auto it = std::lower_bound(gstarts.begin(), gstarts.end(), target);
        p.cuts[k] = std::max(p.cuts[k - 1], it == gstarts.end() ? n : *it);
    }
    return p;
}

// The records of sorted range [k0, k1) that a rank indexed (global file indices [g0, g1); its byte range of the file
// begins at lo, loff / llen are relative to it), as runs of lines adjacent in the file and in the sorted order
// (multigpu.py, _line_runs)
struct Run { u64 k; const uint8_t* p; u64 n; };   // lines of sorted records k, k+1, ... back to back (inner '\n' kept)
inline std::vector<Run> line_runs(const std::vector<u32>& order, u64 k0, u64 k1, u64 g0, u64 g1, const uint8_t* vcf, u64 lo,
                                  const std::vector<u64>& loff, const std::vector<u64>& llen)
{
    std::vector<Run> runs;
    u64 prev_loc = ~0ull, prev_end = 0;
    for (u64 k = k0; k < k1; k++) {
        const u64 g = order[k];
        if (g < g0 || g >= g1) { prev_loc = ~0ull; continue; }
        const u64 loc = g - g0, o = lo + loff[loc], len = llen[loc];
        if (prev_loc != ~0ull && loc == prev_loc + 1 && prev_end + 1 == o) runs.back().n = o + len - (u64)(runs.back().p - vcf);
        else runs.push_back(Run{k, vcf + o, len});
        prev_loc = loc; prev_end = o + len;
    }
    return runs;
}

} // namespace edsx
