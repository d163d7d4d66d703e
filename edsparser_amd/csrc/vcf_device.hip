// vcf_device.hip — VCF (+ reference FASTA) -> EDS / sEDS on gfx950: the variant-overlay walk.
//
// Host (this file, C++): FASTA metadata, std::sort by POS, and the VCF tokeniser for files the device
// tokeniser does not accept — the text-parsing front end of src/cpp/lib/transforms/vcf_transforms.cpp
// (:51-86, :142-326, :715-718).  Plain files are tokenised on the device (k_vt_*).
// Device (HIP kernels): everything from the sorted records on —
//   group_overlapping_variants :482-534   -> max-scan of the record ends + k_mark_groups
//   read_fasta_region :98-129             -> k_fa_count/k_fa_compact (newline-free reference stream)
//   merge_variant_group :396-476          -> k_grp_count / k_grp_haps / k_grp_samples
//   generate_eds_from_variants :554-668   -> k_grp_sizes / k_grp_emit
//
// Data layout in HBM
//   refc            the FASTA bytes from the first sequence line to EOF with '\n' and '\r' removed
//                   (exactly the characters read_fasta_region can return), blkpre[] = kept bytes
//                   before every 256-byte block, so any file offset maps to a position in refc.
//   records (SoA)   start (0-based), reflen, alt range -> alt strings, per (record, sample) allele
//                   lists (two-level CSR), all in sorted order.
//   groups          first record, span [gs, gs+spanlen) in refc, raw haplotypes materialised once in
//                   hapchars, canonical (deduplicated) index per raw haplotype, carried[hap][sample]
//                   bit matrix.
#include "vcf_device.hpp"
#include "vcf_text_kernels.hpp"
#include "vcf_walk.hpp"

#include <algorithm>
#include <cstring>
#include <sstream>
#include <chrono>
#include <thread>

namespace edsx {

// VcfDev, fa_cpos and the bodies of the thread-per-item kernels below: vcf_walk.hpp

struct WalkGrid {                                            // the grid of a thread-per-item kernel, as its body asks for it
    u32 bi, bd, ti, gd;                                      // (read in the kernel itself; the products are taken where the body uses them)
    __device__ __forceinline__ u64 first() const { return bi * (u64)bd + ti; }
    __device__ __forceinline__ u64 stride() const { return (u64)gd * bd; }
    __device__ __forceinline__ bool lead() const { return bi == 0 && ti == 0; }
};
#define WALK_THREAD WalkGrid{blockIdx.x, blockDim.x, threadIdx.x, gridDim.x}      /* last argument of every body */

// ---- reference stream ---------------------------------------------------------------------------
__global__ void k_fa_count(const uint8_t* __restrict__ f, u64 n, u64 seq_start, u64* __restrict__ blkcnt, u64 nblk)
{
    const u32 lane = threadIdx.x & 63;
    const u64 wave = (blockIdx.x * (u64)blockDim.x + threadIdx.x) >> 6, nw = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 b = wave; b < nblk; b += nw) {
        const u64 base = seq_start + b * 256 + lane * 4;
        u32 c = 0;
        for (int i = 0; i < 4; i++) if (base + i < n) { uint8_t ch = f[base + i]; c += (ch != '\n' && ch != '\r'); }
        for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
        if (lane == 0) blkcnt[b] = c;
    }
}
__global__ void k_fa_compact(const uint8_t* __restrict__ f, u64 n, u64 seq_start, const u64* __restrict__ blkpre,
                             u64 nblk, uint8_t* __restrict__ refc)
{
    const u32 lane = threadIdx.x & 63;
    const u64 wave = (blockIdx.x * (u64)blockDim.x + threadIdx.x) >> 6, nw = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 b = wave; b < nblk; b += nw) {
        const u64 base = seq_start + b * 256 + lane * 4;
        uint8_t ch[4];
        u32 c = 0;
        for (int i = 0; i < 4; i++) {
            ch[i] = base + i < n ? f[base + i] : (uint8_t)'\n';
            c += (ch[i] != '\n' && ch[i] != '\r');
        }
        u32 incl = c;
        for (int o = 1; o < 64; o <<= 1) { u32 a = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += a; }
        u64 o = blkpre[b] + incl - c;
        for (int i = 0; i < 4; i++) if (ch[i] != '\n' && ch[i] != '\r') refc[o++] = ch[i];
    }
}

// seq_size of parse_fasta_metadata (:69-84) on the device: the record ends at the first later line that starts with
// '>' (or at EOF); its size is the number of bytes that are not '\n' from the first sequence line on ('\r' counts,
// as in the reference's getline loop).
__global__ void k_fa_record_end(const uint8_t* __restrict__ f, u64 n, u64 from, u64* __restrict__ rec_end)
{
    fa_record_end_body(f, n, from, rec_end, WALK_THREAD);
}
__global__ void k_fa_seq_bytes(const uint8_t* __restrict__ f, u64 from, const u64* __restrict__ rec_end, u64* __restrict__ count)
{
    const u64 hi = *rec_end;
    u64 c = 0;
    for (u64 i = from + blockIdx.x * (u64)blockDim.x + threadIdx.x; i < hi; i += (u64)gridDim.x * blockDim.x) c += f[i] != '\n';
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd((unsigned long long*)count, (unsigned long long)c);
}

// The same two passes over one slice [a, b) of the FASTA body (partitioned runs: every rank scans its slice; the slices'
// results are put together on the host, vcf_multi.hip).  s[i] is file byte s0 + i, s0 = a - 1 (the byte in front of the
// slice decides whether a '>' at a starts a line).  k_fa_slice_end: the first "\n>" with its '>' in [from, b).
__global__ void k_fa_slice_end(const uint8_t* __restrict__ s, u64 s0, u64 from, u64 b, u64* __restrict__ rec_end)
{
    u64 best = ~0ull;
    for (u64 i = from + blockIdx.x * (u64)blockDim.x + threadIdx.x; i < b; i += (u64)gridDim.x * blockDim.x)
        if (s[i - s0] == '>' && s[i - 1 - s0] == '\n') { best = i; break; }
    if (best != ~0ull) atomicMin((unsigned long long*)rec_end, (unsigned long long)best);
}
// [a, min(rec_end, b)): bytes that are not '\n' (k_fa_seq_bytes) and what breaks the line grid of a regular file: the
// byte at (i - seq_start) % (lw + 1) == lw is '\n' and no other is; no '\r'.  A thread takes 16 consecutive bytes.
// out[0] count, out[1] flags (1: '\r', 2: grid byte that is not '\n'), out[2] first '\n' off the grid
__global__ void k_fa_slice_scan(const uint8_t* __restrict__ s, u64 s0, u64 a, u64 b, const u64* __restrict__ rec_end, u64 seq_start,
                                u64 lw, u64* __restrict__ out)
{
    const u64 re = *rec_end, hi = re < b ? re : b, period = lw + 1;
    u64 cnt = 0, flags = 0, off = ~0ull;
    for (u64 c0 = a + 16 * (blockIdx.x * (u64)blockDim.x + threadIdx.x); c0 < hi; c0 += 16 * (u64)gridDim.x * blockDim.x) {
        const u64 c1 = c0 + 16 < hi ? c0 + 16 : hi;
        u64 m = (c0 - seq_start) % period;
        for (u64 i = c0; i < c1; i++) {
            const uint8_t ch = s[i - s0];
            const bool grid = m == lw;
            cnt += ch != '\n';
            if (ch == '\r') flags |= 1;
            if (grid && ch != '\n') flags |= 2;
            if (!grid && ch == '\n' && i < off) off = i;
            if (++m == period) m = 0;
        }
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd((unsigned long long*)&out[0], (unsigned long long)cnt);
    if (flags) atomicOr((unsigned long long*)&out[1], (unsigned long long)flags);
    if (off != ~0ull) atomicMin((unsigned long long*)&out[2], (unsigned long long)off);
}

// ---- grouping -------------------------------------------------------------------------------------
__global__ void k_rec_ends(const u64* __restrict__ start, const u64* __restrict__ reflen, u64 n, u64* __restrict__ ends)
{
    rec_ends_body(start, reflen, n, ends, WALK_THREAD);
}
__global__ void k_mark_groups(const u64* __restrict__ start, const u64* __restrict__ incl_end, u64 n, u64* __restrict__ flag)
{
    mark_groups_body(start, incl_end, n, flag, WALK_THREAD);
}
__global__ void k_group_firsts(const u64* __restrict__ flag, const u64* __restrict__ gidx, u64 n, u64* __restrict__ grp_r0,
                               const u64* __restrict__ ngrp)
{
    group_firsts_body(flag, gidx, n, grp_r0, ngrp, WALK_THREAD);
}

// ---- per group: thread per group (bodies and the arrays' meaning: vcf_walk.hpp) ------------------------------
__global__ void k_grp_count(VcfDev d, GrpArrays a) { grp_count_body(d, a, WALK_THREAD); }
__global__ void k_grp_haps(VcfDev d, GrpArrays a, HapArrays h) { grp_haps_body(d, a, h, WALK_THREAD); }
__global__ void k_grp_samples(VcfDev d, GrpArrays a, HapArrays h) { grp_samples_body(d, a, h, WALK_THREAD); }
__global__ void k_grp_common(VcfDev d, GrpArrays a) { grp_common_body(d, a, WALK_THREAD); }

// common text in front of every group (the bandwidth part of the output).  A wave takes 64 consecutive groups: every
// lane fetches the numbers of one group (length, offsets, position in refc - one round of dependent loads for 64
// groups instead of one per group) and writes its brackets and "{0}"; then the wave copies the texts one group after the
// other, 16 bytes per lane (unaligned loads and stores), the ragged end byte by byte.
__device__ __forceinline__ u64 readlane64(u64 v, int l)
{
    const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)v, l), hi = (u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), l);
    return (u64)lo | ((u64)hi << 32);
}
__global__ void __launch_bounds__(256) k_grp_emit_common(VcfDev d, GrpArrays a, EmitArrays e)
{
    const u32 lane = threadIdx.x & 63;
    const u64 wave = (blockIdx.x * (u64)blockDim.x + threadIdx.x) >> 6, nw = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 gb = wave * 64; gb < d.ngrp; gb += nw * 64) {
        const u64 g = gb + lane;
        u64 clen = 0, eoff = 0, c0 = 0;
        if (g < d.ngrp) clen = a.commonlen[g];
        if (clen) {
            eoff = e.eds_off[g];
            uint8_t* eo = e.eds + eoff;
            uint8_t* so = e.seds + e.seds_off[g];
            const u64 cur = g ? a.cur_after[g - 1] : d.cur0;
            c0 = fa_cpos(d, d.seq_start + cur + cur / d.lw);
            eo[0] = '{'; eo[clen + 1] = '}'; so[0] = '{'; so[1] = '0'; so[2] = '}';
        }
        u64 todo = ballot64(clen != 0);
        while (todo) {
            const int l = __builtin_ctzll(todo);
            todo &= todo - 1;
            const u64 cl = readlane64(clen, l);
            uint8_t* dst = e.eds + readlane64(eoff, l) + 1;
            const uint8_t* src = d.refc + readlane64(c0, l);
            const u64 full = cl & ~15ull;
            for (u64 i = (u64)lane * 16; i < full; i += 1024) {
                const uint4 v = load16u(src + i);
                U128u w{v.x, v.y, v.z, v.w};
                __builtin_memcpy(dst + i, &w, 16);
            }
            if (lane < (u32)(cl - full)) dst[full + lane] = src[full + lane];
        }
    }
}

__global__ void __launch_bounds__(256) k_grp_emit(VcfDev d, GrpArrays a, HapArrays h, EmitArrays e) { grp_emit_body(d, a, h, e, WALK_THREAD); }
__global__ void k_cpos(VcfDev d, u64 file_off, u64* out) { cpos_body(d, file_off, out, WALK_THREAD); }
__global__ void k_tail(VcfDev d, u64 cur, u64 clen, uint8_t* eo, uint8_t* so) { tail_body(d, cur, clen, eo, so, WALK_THREAD); }

// ---- device tokeniser: vt_parse and the bodies are in vcf_walk.hpp ---------------------------------------------
__global__ void k_vt_count(const uint8_t* __restrict__ raw, u64 n, const u64* __restrict__ lstart, u64 nrec, VtRec r, VtCtl* ctl)
{
    vt_count_body(raw, n, lstart, nrec, r, ctl, WALK_THREAD);
}
__global__ void k_vt_ascending(const u64* __restrict__ pos, u64 nrec, VtCtl* ctl) { vt_ascending_body(pos, nrec, ctl, WALK_THREAD); }
__global__ void k_vt_gather(VtRec r, const u32* __restrict__ order, u64 nrec, u64* __restrict__ a, u64* __restrict__ b,
                            u64* __restrict__ c, u64* __restrict__ d)
{
    vt_gather_body(r, order, nrec, a, b, c, d, WALK_THREAD);
}
__global__ void k_vt_fill(const uint8_t* __restrict__ raw, u64 n, const u64* __restrict__ lstart, const u32* __restrict__ order,
                          u64 nrec, VtOut o, VtCtl* ctl)
{
    vt_fill_body(raw, n, lstart, order, nrec, o, ctl, WALK_THREAD);
}
#undef WALK_THREAD

// ---- host ------------------------------------------------------------------------------------------
namespace {

bool next_line(const uint8_t* f, size_t n, size_t& pos, std::string& line, bool* hit_eof = nullptr)
{
    if (pos >= n) return false;
    const uint8_t* nl = static_cast<const uint8_t*>(memchr(f + pos, '\n', n - pos));
    size_t end = nl ? static_cast<size_t>(nl - f) : n;
    line.assign(reinterpret_cast<const char*>(f + pos), end - pos);
    if (hit_eof) *hit_eof = (nl == nullptr);
    pos = nl ? end + 1 : n;
    return true;
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
void parse_gt_flat(Span gt, VcfPart& out)
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
Skip parse_line_flat(const char* line, size_t n, VcfPart& out, std::vector<Span>& fields, bool light = false)
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

template <class T> void upload(DevBuf& b, const std::vector<T>& v, hipStream_t st)
{
    b.ensure(sizeof(T) * (v.size() + 1) + 16);
    if (!v.empty()) EDSX_HIP(hipMemcpyAsync(b.ptr, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, st));
}

// Lines are independent: large files are cut at line starts and tokenised by several host threads; records,
// counters and the stderr warnings are put together in file order, so the array handed to std::sort is the
// reference's.  light = positions, REF lengths and line spans only (the index pass of a partitioned run).
void tokenise(const uint8_t* vcf, size_t vcf_n, std::vector<VcfPart>& parts, std::vector<u64>& part_base,
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
void sort_like_reference(std::vector<std::pair<u64, u32>>& order)
{
    std::sort(order.begin(), order.end(),
              [](const std::pair<u64, u32>& a, const std::pair<u64, u32>& b) { return a.first < b.first; });
}

} // namespace

// ---- index pass and sort order of a partitioned run (VCF row) ------------------------------
void vcf_index(const uint8_t* vcf, size_t vcf_n, std::vector<u64>& pos, std::vector<u64>& reflen, std::vector<u64>& line_off,
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

void vcf_sort_order(const u64* pos, size_t n, u32* order_out)
{
    std::vector<std::pair<u64, u32>> order(n);
    for (size_t i = 0; i < n; i++) order[i] = {pos[i], (u32)i};
    sort_like_reference(order);
    for (size_t i = 0; i < n; i++) order_out[i] = order[i].second;
}

// Tokenise on the device (kernels above).  false: the file is not plain; the caller runs the host tokeniser.  On success
// the record SoA (sorted order) is in place in HBM and the counters are set.
bool VcfPipeline::tokenize_device(const uint8_t* vcf, size_t n, bool presorted, hipStream_t st, u64& nrec, u64& max_samples,
                                  VcfCounters& stats)
{
    { const char* e = getenv("EDSX_HOST_TOKENIZER"); if (e && atoi(e)) return false; }      // A/B switch for the parity tests
    nrec = 0; max_samples = 0;
    if (n == 0 || !device_scratch_fits(6 * n)) return false;   // raw text + the record arrays (a dozen u64 per record line)
    vt_raw_.ensure(vcf_size::text(n));
    const u64 nblk = vcf_size::line_blocks(n);
    vt_idx_.ensure(vcf_size::line_counts(nblk));                            // line starts per 1 KB block of the text
    scan_tmp_.ensure(8 * ((n + 2) / SCAN_TILE + 4));
    ctl_.ensure(vcf_size::ctl());
    VtCtl* ctl = reinterpret_cast<VtCtl*>(ctl_.as<u64>() + 16);
    VtCtl h{};
    h.n = nblk;                                                // element count of the block scan
    EDSX_HIP(hipMemcpyAsync(ctl, &h, sizeof(h), hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemcpyAsync(vt_raw_.ptr, vcf, n, hipMemcpyHostToDevice, st));
    vcf_h2d_ = n;
    const uint8_t* raw = vt_raw_.as<uint8_t>();
    hipLaunchKernelGGL(k_vt_line_count, dim3(2048), dim3(256), 0, st, raw, (u64)n, vt_idx_.as<u64>(), ctl);
    exclusive_scan_u64(vt_idx_.as<u64>(), vt_idx_.as<u64>(), &ctl->n, &ctl->nrec, scan_tmp_.as<u64>(), st);
    EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    if (h.bad || h.nrec >= 0xffffffffull) return false;
    const u64 nr = h.nrec;
    if (nr) {
        vt_lstart_.ensure(vcf_size::line_starts(nr));
        hipLaunchKernelGGL(k_vt_line_fill, dim3(2048), dim3(256), 0, st, raw, (u64)n, vt_idx_.as<u64>(), vt_lstart_.as<u64>());
    }
    return tokenize_lines(raw, n, vt_lstart_.as<u64>(), nr, presorted, st, nrec, max_samples, stats);
}

// The tokeniser proper: text that is in HBM (n bytes, 256-byte aligned, 16 bytes of slack behind them) and the starts of
// the nr record lines to take from it, in file order.  tokenize_device hands over the whole file it has just uploaded, a
// contig session (vcf_contig.hip) one contig's slice of its regrouped line starts.
bool VcfPipeline::tokenize_lines(const uint8_t* raw, u64 n, const u64* lstart, u64 nr, bool presorted, hipStream_t st, u64& nrec,
                                 u64& max_samples, VcfCounters& stats)
{
    nrec = 0; max_samples = 0;
    stats.total_variants = stats.processed_variants = nr;
    if (nr == 0) return true;
    if (nr >= 0xffffffffull) return false;
    scan_tmp_.ensure(8 * ((nr + 2) / SCAN_TILE + 4));
    ctl_.ensure(vcf_size::ctl());
    VtCtl* ctl = reinterpret_cast<VtCtl*>(ctl_.as<u64>() + 16);
    VtCtl h{};
    EDSX_HIP(hipMemcpyAsync(ctl, &h, sizeof(h), hipMemcpyHostToDevice, st));
    for (DevBuf* b : {&vt_pos_, &vt_reflen_, &vt_nalt_, &vt_altc_, &vt_ngt_, &vt_nall_, &vt_s1_, &vt_s2_, &vt_s3_, &vt_s4_}) b->ensure(vcf_size::per_record(nr));
    VtRec rec{vt_pos_.as<u64>(), vt_reflen_.as<u64>(), vt_nalt_.as<u64>(), vt_altc_.as<u64>(), vt_ngt_.as<u64>(), vt_nall_.as<u64>(), nullptr};
    TraceSpan count_span(st, "tokeniser count pass", 0);
    hipLaunchKernelGGL(k_vt_count, dim3(2048), dim3(256), 0, st, raw, (u64)n, lstart, nr, rec, ctl);
    count_span.end();
    hipLaunchKernelGGL(k_vt_ascending, dim3(1024), dim3(256), 0, st, vt_pos_.as<u64>(), nr, ctl);
    EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    if (h.oob) throw DeviceError("VCF tokeniser: byte index " + std::to_string(h.oob & ((1ull << 62) - 1)) + " outside the text of " +
                                 std::to_string(n) + " bytes (flags " + std::to_string(h.oob >> 62) + ")");
    if (h.bad) return false;
    // The reference's unstable std::sort (:715-718) on (pos, file index) pairs, as on the host path — unless the
    // positions already ascend strictly (the usual VCF) or the caller hands the records over in final order.
    const u32* d_order = nullptr;
    std::vector<u32> order;
    bool need_host_sort = !presorted && h.t_alt;
    if (need_host_sort) {
        // Not ascending.  If the positions are pairwise distinct there is exactly one sorted order, so a device radix
        // sort gives the reference's permutation; equal positions (checked on the sorted keys) need the host's
        // std::sort, whose unstable permutation of them is part of the output.
        vt_s2_.ensure(vcf_size::per_record(nr)); vt_order_.ensure(vcf_size::order(nr));
        {   // eight passes: positions -> tmp -> (vt_s2_, vt_order_) -> tmp ... the last pass ends in (vt_s2_, vt_order_)
            const u64 ntiles = (nr + RS_TILE - 1) / RS_TILE, nbins = 256 * ntiles;
            vt_sorttmp_.ensure(12 * (nr + 2) + 8 * (nbins + 2) + 64);
            u64* tkeys = vt_sorttmp_.as<u64>();
            u32* tvals = reinterpret_cast<u32*>(tkeys + nr + 2);
            u64* table = reinterpret_cast<u64*>(vt_sorttmp_.as<uint8_t>() + ((12 * (nr + 2) + 15) & ~(size_t)15));
            scan_tmp_.ensure(8 * (nbins / SCAN_TILE + 4));
            EDSX_HIP(hipMemcpyAsync(&ctl->n, &nbins, 8, hipMemcpyHostToDevice, st));
            const unsigned grid = (unsigned)std::min<u64>(ntiles, 1u << 16);
            for (u32 pass = 0; pass < 8; pass++) {
                const u64* kin = pass == 0 ? vt_pos_.as<u64>() : (pass & 1) ? tkeys : vt_s2_.as<u64>();
                const u32* vin = pass == 0 ? nullptr : (pass & 1) ? tvals : vt_order_.as<u32>();
                u64* kout = (pass & 1) ? vt_s2_.as<u64>() : tkeys;
                u32* vout = (pass & 1) ? vt_order_.as<u32>() : tvals;
                hipLaunchKernelGGL(k_rs_hist, dim3(grid), dim3(64), 0, st, kin, nr, 8 * pass, ntiles, table);
                exclusive_scan_u64(table, table, &ctl->n, &ctl->nrec, scan_tmp_.as<u64>(), st);
                hipLaunchKernelGGL(k_rs_scatter, dim3(grid), dim3(64), 0, st, kin, vin, nr, 8 * pass, ntiles, table, kout, vout);
            }
        }
        VtCtl z{};
        EDSX_HIP(hipMemcpyAsync(&ctl->t_alt, &z.t_alt, 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_vt_ascending, dim3(1024), dim3(256), 0, st, vt_s2_.as<u64>(), nr, ctl);   // sorted keys: strict?
        EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        if (!h.t_alt) { need_host_sort = false; d_order = vt_order_.as<u32>(); }
    }
    if (need_host_sort) {
        std::vector<u64> hpos(nr);
        EDSX_HIP(hipMemcpy(hpos.data(), vt_pos_.ptr, 8 * nr, hipMemcpyDeviceToHost));
        order.resize(nr);
        const auto ts0 = std::chrono::steady_clock::now();
        vcf_sort_order(hpos.data(), nr, order.data());
        { const char* e = getenv("EDSX_TRACE");
          if (e && atoi(e)) fprintf(stderr, "[edsx vcf]   std::sort of %llu positions %8.3f ms\n", (unsigned long long)nr,
                                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ts0).count()); }
        vt_order_.ensure(vcf_size::order(nr));
        EDSX_HIP(hipMemcpyAsync(vt_order_.ptr, order.data(), 4 * nr, hipMemcpyHostToDevice, st));
        d_order = vt_order_.as<u32>();
    }
    h.n = nr;
    EDSX_HIP(hipMemcpyAsync(&ctl->n, &h.n, 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_vt_gather, dim3(2048), dim3(256), 0, st, rec, d_order, nr, vt_s1_.as<u64>(), vt_s2_.as<u64>(),
                       vt_s3_.as<u64>(), vt_s4_.as<u64>());
    for (DevBuf* b : {&alt0_, &pair0_, &start_, &reflen_}) b->ensure(vcf_size::per_record(nr));
    exclusive_scan_u64(vt_s1_.as<u64>(), alt0_.as<u64>(), &ctl->n, &ctl->t_alt, scan_tmp_.as<u64>(), st);
    exclusive_scan_u64(vt_s2_.as<u64>(), vt_s2_.as<u64>(), &ctl->n, &ctl->t_altc, scan_tmp_.as<u64>(), st);
    exclusive_scan_u64(vt_s3_.as<u64>(), pair0_.as<u64>(), &ctl->n, &ctl->t_pair, scan_tmp_.as<u64>(), st);
    exclusive_scan_u64(vt_s4_.as<u64>(), vt_s4_.as<u64>(), &ctl->n, &ctl->t_all, scan_tmp_.as<u64>(), st);
    EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));                          // also: `order` stays alive until its upload is done
    altoff_.ensure(vcf_size::altoff(h.t_alt)); altchars_.ensure(vcf_size::altchars(h.t_altc)); pa0_.ensure(vcf_size::pa0(h.t_pair));
    alleles_.ensure(vcf_size::alleles(h.t_all));
    VtOut o{start_.as<u64>(), reflen_.as<u64>(), alt0_.as<u64>(), altoff_.as<u64>(), altchars_.as<uint8_t>(), pair0_.as<u64>(),
            pa0_.as<u64>(), alleles_.as<int>(), vt_s2_.as<u64>(), vt_s4_.as<u64>()};
    hipLaunchKernelGGL(k_vt_fill, dim3(2048), dim3(256), 0, st, raw, (u64)n, lstart, d_order, nr, o, ctl);
    EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    if (h.oob) throw DeviceError("VCF tokeniser (fill): byte index " + std::to_string(h.oob & ((1ull << 62) - 1)) + " outside the text of " +
                                 std::to_string(n) + " bytes (flags " + std::to_string(h.oob >> 62) + ")");
    nrec = nr;
    max_samples = h.max_samples;
    return true;
}

// Index pass of a partitioned run on the device: the first half of tokenize_device (line starts, count pass) with the
// line lengths kept.  false: not a plain file, the host index pass takes it (wrapped positions are fine here: the
// planner decides what to do with them).
bool VcfPipeline::index_device(const uint8_t* vcf, size_t n, hipStream_t st, std::vector<u64>& pos, std::vector<u64>& reflen,
                               std::vector<u64>& line_off, std::vector<u64>& line_len, VcfCounters& stats)
{
    { const char* e = getenv("EDSX_HOST_TOKENIZER"); if (e && atoi(e)) return false; }
    if (n == 0 || !device_scratch_fits(6 * n)) return false;
    vt_raw_.ensure(vcf_size::text(n));
    const u64 nblk = vcf_size::line_blocks(n);
    vt_idx_.ensure(vcf_size::line_counts(nblk));                            // line starts per 1 KB block of the text
    scan_tmp_.ensure(8 * ((n + 2) / SCAN_TILE + 4));
    ctl_.ensure(vcf_size::ctl());
    VtCtl* ctl = reinterpret_cast<VtCtl*>(ctl_.as<u64>() + 16);
    VtCtl h{};
    h.n = nblk;                                                // element count of the block scan
    EDSX_HIP(hipMemcpyAsync(ctl, &h, sizeof(h), hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemcpyAsync(vt_raw_.ptr, vcf, n, hipMemcpyHostToDevice, st));
    const uint8_t* raw = vt_raw_.as<uint8_t>();
    hipLaunchKernelGGL(k_vt_line_count, dim3(2048), dim3(256), 0, st, raw, (u64)n, vt_idx_.as<u64>(), ctl);
    exclusive_scan_u64(vt_idx_.as<u64>(), vt_idx_.as<u64>(), &ctl->n, &ctl->nrec, scan_tmp_.as<u64>(), st);
    EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    if (h.bad || h.nrec >= 0xffffffffull) return false;
    const u64 nr = h.nrec;
    stats = VcfCounters();
    stats.total_variants = stats.processed_variants = nr;
    pos.assign(nr, 0); reflen.assign(nr, 0); line_off.assign(nr, 0); line_len.assign(nr, 0);
    if (nr == 0) return true;
    vt_lstart_.ensure(vcf_size::line_starts(nr));
    hipLaunchKernelGGL(k_vt_line_fill, dim3(2048), dim3(256), 0, st, raw, (u64)n, vt_idx_.as<u64>(), vt_lstart_.as<u64>());
    for (DevBuf* b : {&vt_pos_, &vt_reflen_, &vt_nalt_, &vt_altc_, &vt_ngt_, &vt_nall_, &vt_s1_}) b->ensure(vcf_size::per_record(nr));
    VtRec rec{vt_pos_.as<u64>(), vt_reflen_.as<u64>(), vt_nalt_.as<u64>(), vt_altc_.as<u64>(), vt_ngt_.as<u64>(), vt_nall_.as<u64>(),
              vt_s1_.as<u64>()};
    hipLaunchKernelGGL(k_vt_count, dim3(2048), dim3(256), 0, st, raw, (u64)n, vt_lstart_.as<u64>(), nr, rec, ctl);
    EDSX_HIP(hipMemcpyAsync(pos.data(), vt_pos_.ptr, 8 * nr, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipMemcpyAsync(reflen.data(), vt_reflen_.ptr, 8 * nr, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipMemcpyAsync(line_off.data(), vt_lstart_.ptr, 8 * nr, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipMemcpyAsync(line_len.data(), vt_s1_.ptr, 8 * nr, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    return !h.bad;
}

void fasta_head(const uint8_t* fasta, size_t fasta_n, u64& seq_start, u64& lw, u64& rest_from)
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

FaSlice VcfPipeline::fasta_slice(const uint8_t* fasta, u64 a, u64 b, u64 seq_start, u64 rest_from, u64 lw, hipStream_t st, u64& h2d)
{
    FaSlice r{~0ull, 0, 0, ~0ull};
    h2d = 0;
    if (a >= b) return r;
    if (a == 0 || a < seq_start) throw ParamError("fasta_slice: the slice must lie behind the header line");
    const u64 s0 = a - 1, n = b - s0;
    d_slice_.ensure(n + 16);
    slice_ctl_.ensure(8 * 8);
    u64* ctl = slice_ctl_.as<u64>();
    EDSX_HIP(hipMemcpyAsync(d_slice_.ptr, fasta + s0, n, hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemcpyAsync(ctl, &r, sizeof(r), hipMemcpyHostToDevice, st));
    h2d = n;
    const uint8_t* sl = d_slice_.as<uint8_t>();
    const u64 from = std::max(a, rest_from);
    if (from < b) hipLaunchKernelGGL(k_fa_slice_end, dim3(1024), dim3(256), 0, st, sl, s0, from, b, ctl + 0);
    hipLaunchKernelGGL(k_fa_slice_scan, dim3(1024), dim3(256), 0, st, sl, s0, a, b, ctl + 0, seq_start, lw, ctl + 1);
    EDSX_HIP(hipMemcpyAsync(&r, ctl, sizeof(r), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    return r;
}

bool VcfPipeline::run(const uint8_t* vcf, size_t vcf_n, const uint8_t* fasta, size_t fasta_n, HostBytes& eds,
                      HostBytes& seds, VcfCounters& stats, hipStream_t st, const VcfRange& range, const VcfResident* res)
{
    // EDSX_TRACE=1: wall-clock of the host-visible stages on stderr (every mark follows a stream synchronisation)
    static const bool trace = [] { const char* e = getenv("EDSX_TRACE"); return e && atoi(e); }();
    auto t_last = std::chrono::steady_clock::now();
    auto mark = [&](const char* what) {
        if (!trace) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[edsx vcf] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    stats = VcfCounters();
    fasta_h2d_ = 0; vcf_h2d_ = 0;
    // ---- FASTA metadata (:51-86)
    u64 seq_start, lw, seq_size, rest_from = 0;
    fasta_head(fasta, fasta_n, seq_start, lw, rest_from);
    seq_size = lw;                                             // + the later lines, counted on the device (below)
    const FastaMeta* meta = range.fasta;
    FastaMeta res_meta;
    const bool fasta_resident = res && res->d_fasta;
    if (fasta_resident) { res_meta.seq_size = res->seq_size; res_meta.regular = false; meta = &res_meta; }   // (the index counted it)
    mark("fasta metadata");
    // ---- VCF records (:690-712) and the unstable sort (:715-718)
    std::vector<VcfPart> parts;
    std::vector<u64> part_base;                              // first global record index of every part
    std::vector<std::pair<u64, u32>> order;                  // (pos, global index in file order), sorted by pos
    u64 dev_nrec = 0, dev_max_samples = 0;
    const bool lines_resident = res && res->d_vcf;
    const bool on_device = lines_resident ? tokenize_lines(res->d_vcf, res->vcf_n, res->d_lstart, res->nrec, range.presorted, st,
                                                           dev_nrec, dev_max_samples, stats)
                                          : tokenize_device(vcf, vcf_n, range.presorted, st, dev_nrec, dev_max_samples, stats);
    tokenised_on_device_ = on_device;
    if (lines_resident && !on_device) { stats = VcfCounters(); return false; }   // the caller builds the text on the host
    mark(on_device ? "device tokenise" : "device tokenise attempt");
    if (!on_device) {
        stats = VcfCounters();
        tokenise(vcf, vcf_n, parts, part_base, stats, false);
        mark("host tokenise");
    }
    if (!on_device) {
        const unsigned nt = (unsigned)parts.size();
        // std::sort's permutation depends only on the outcomes of its comparisons, so sorting (pos, index)
        // pairs by pos ends in the order the reference's sort of whole records ends in
        order.resize(part_base[nt]);
        for (unsigned t = 0; t < nt; t++)
            for (size_t i = 0; i < parts[t].size(); i++) order[part_base[t] + i] = {parts[t].pos[i], (u32)(part_base[t] + i)};
        // a position range of a partitioned run hands its records over in their final order (the order of the
        // whole file's sort, edsx_vcf_sort_order): sorting the slice again could permute equal positions differently
        if (!range.presorted) sort_like_reference(order);
    }
    // record j of the sorted order -> (part, index in part)
    auto locate = [&](u64 j, const VcfPart*& pt) -> size_t {
        const u64 g = order[j].second;
        size_t t = std::upper_bound(part_base.begin(), part_base.end(), g) - part_base.begin() - 1;
        pt = &parts[t];
        return (size_t)(g - part_base[t]);
    };
    const u64 nrec = on_device ? dev_nrec : order.size();

    // a reference with an empty first line has no addressable positions; the reference divides by
    // line_width (UB), refuse instead
    if (lw == 0) throw FormatError("Invalid FASTA format: empty first sequence line");

    // ---- reference stream on the device: the whole file, or (a regular file in a partitioned run) the window of this
    // position range, [off(cur0), off(end)) with 16 bytes of slack
    const bool window = meta && meta->regular;
    u64 up0 = 0, up1 = fasta_n;
    if (window) {
        auto off = [&](u64 p) { return seq_start + p + p / lw; };
        const u64 p0 = std::min(range.cur0, meta->seq_size);
        const u64 p1 = std::max(p0, std::min(range.next_start, meta->seq_size));
        up0 = std::min<u64>(off(p0), fasta_n);
        up1 = std::max(up0, std::min<u64>(off(p1) + 16, fasta_n));
    }
    const u64 up_n = up1 - up0, cbase = window ? up0 : seq_start;
    if (!fasta_resident) {
        d_fasta_.ensure(vcf_size::fasta(up_n));
        if (up_n) EDSX_HIP(hipMemcpyAsync(d_fasta_.ptr, fasta + up0, up_n, hipMemcpyHostToDevice, st));
        fasta_h2d_ = up_n;
    }
    const uint8_t* const dfa = fasta_resident ? res->d_fasta : d_fasta_.as<uint8_t>();
    const u64 body = window ? up_n : fasta_n > seq_start ? fasta_n - seq_start : 0;
    const u64 nblk = vcf_size::ref_blocks(body);
    ctl_.ensure(vcf_size::ctl());
    u64* ctl = ctl_.as<u64>();
    blkpre_.ensure(vcf_size::blkpre(nblk));
    scan_tmp_.ensure(8 * ((std::max<u64>(nblk, nrec) + 2) / SCAN_TILE + 4));
    refc_.ensure(vcf_size::refc(body));
    u64 hctl[32] = {0};
    hctl[0] = nblk; hctl[10] = ~0ull;
    hctl[12] = fasta_n;                                      // record end (atomicMin), [13] bytes of the later lines
    EDSX_HIP(hipMemcpyAsync(ctl, hctl, sizeof(hctl), hipMemcpyHostToDevice, st));
    if (!meta && rest_from < fasta_n) {
        hipLaunchKernelGGL(k_fa_record_end, dim3(1024), dim3(256), 0, st, dfa, (u64)fasta_n, rest_from, ctl + 12);
        hipLaunchKernelGGL(k_fa_seq_bytes, dim3(1024), dim3(256), 0, st, dfa, rest_from, ctl + 12, ctl + 13);
    }
    if (nblk) {
        // (window: the buffer is the window, compacted from its first byte)
        const u64 kn = window ? up_n : fasta_n, ks = window ? 0 : seq_start;
        hipLaunchKernelGGL(k_fa_count, dim3(1024), dim3(256), 0, st, dfa, kn, ks, blkpre_.as<u64>(), nblk);
        exclusive_scan_u64(blkpre_.as<u64>(), blkpre_.as<u64>(), ctl + 0, ctl + 1, scan_tmp_.as<u64>(), st);
        hipLaunchKernelGGL(k_fa_compact, dim3(1024), dim3(256), 0, st, dfa, kn, ks, blkpre_.as<u64>(), nblk,
                           refc_.as<uint8_t>());
    }
    EDSX_HIP(hipMemcpyAsync(hctl, ctl, sizeof(hctl), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    const u64 refc_n = nblk ? hctl[1] : 0;
    seq_size = meta ? meta->seq_size : seq_size + hctl[13];
    mark("fasta upload, metadata, compaction");

    VcfDev d{};
    d.fasta = dfa + (cbase - up0); d.fasta_n = fasta_n; d.seq_start = seq_start; d.seq_size = seq_size; d.lw = lw;
    d.refc = refc_.as<uint8_t>(); d.refc_n = refc_n; d.blkpre = blkpre_.as<u64>();
    d.cbase = cbase; d.wend = up1; d.oob = window ? ctl + 20 : nullptr;          // (ctl[20] is zero from the upload above)
    auto window_check = [&](u64 v) {
        if (v) throw DeviceError("VCF reference window: read at file offset " + std::to_string(v & ((1ull << 62) - 1)) +
                                 " outside the window [" + std::to_string(up0) + ", " + std::to_string(up1) + ") (flags " +
                                 std::to_string(v >> 62) + ")");
    };
    d.nrec = nrec; d.cur0 = range.cur0;

    u64 cur = range.cur0, ngrp = 0, E = 0, Q = 0;
    u64 max_samples = dev_max_samples;
    GrpArrays ga{};
    HapArrays ha{};
    if (nrec) {
        std::vector<u64> hstart, hreflen;                         // host path only (the device tokeniser refuses wrapped positions)
        if (!on_device) {
        // ---- records -> SoA
        // two passes: sizes -> offsets (serial prefix sums), then the fill by several host threads
        hstart.resize(nrec); hreflen.resize(nrec);
        std::vector<u64> halt0(nrec + 1), hpair0(nrec + 1);
        std::vector<u64> altc0(nrec + 1), gtc0(nrec + 1);        // first alt char / first allele of record j
        halt0[0] = 0; hpair0[0] = 0; altc0[0] = 0; gtc0[0] = 0;
        for (u64 j = 0; j < nrec; j++) {
            const VcfPart* pt;
            const size_t i = locate(j, pt);
            const u64 na = pt->alt0[i + 1] - pt->alt0[i], ng = pt->gt0[i + 1] - pt->gt0[i];
            halt0[j + 1] = halt0[j] + na;
            hpair0[j + 1] = hpair0[j] + ng;
            altc0[j + 1] = altc0[j] + (pt->altoff[pt->alt0[i + 1]] - pt->altoff[pt->alt0[i]]);
            gtc0[j + 1] = gtc0[j] + (pt->gtoff[pt->gt0[i + 1]] - pt->gtoff[pt->gt0[i]]);
            max_samples = std::max<u64>(max_samples, ng);
        }
        std::vector<u64> haltoff(halt0[nrec] + 1), hpa0(hpair0[nrec] + 1);
        std::vector<uint8_t> haltchars(altc0[nrec]);
        std::vector<int> halleles(gtc0[nrec]);
        haltoff[halt0[nrec]] = altc0[nrec];
        hpa0[hpair0[nrec]] = gtc0[nrec];
        {
            const unsigned hc = std::thread::hardware_concurrency();
            const unsigned ft = nrec >= 65536 ? std::max(1u, std::min(16u, hc ? hc : 4u)) : 1u;
            auto fill = [&](u64 lo, u64 hi) {
                for (u64 j = lo; j < hi; j++) {
                    const VcfPart* pt;
                    const size_t i = locate(j, pt);
                    hstart[j] = pt->pos[i] - 1;                    // wraps for POS 0 like the reference's size_t
                    hreflen[j] = pt->reflen[i];
                    const u64 a0 = pt->alt0[i], a1 = pt->alt0[i + 1], cbase = pt->altoff[a0];
                    for (u64 a = a0; a < a1; a++) haltoff[halt0[j] + (a - a0)] = altc0[j] + (pt->altoff[a] - cbase);
                    if (pt->altoff[a1] > cbase) memcpy(haltchars.data() + altc0[j], pt->altchars.data() + cbase, pt->altoff[a1] - cbase);
                    const u64 g0 = pt->gt0[i], g1 = pt->gt0[i + 1], ebase = pt->gtoff[g0];
                    for (u64 g = g0; g < g1; g++) hpa0[hpair0[j] + (g - g0)] = gtc0[j] + (pt->gtoff[g] - ebase);
                    if (pt->gtoff[g1] > ebase)
                        memcpy(halleles.data() + gtc0[j], pt->alleles.data() + ebase, sizeof(int) * (pt->gtoff[g1] - ebase));
                }
            };
            if (ft == 1) fill(0, nrec);
            else {
                std::vector<std::thread> th;
                for (unsigned t = 0; t < ft; t++) th.emplace_back(fill, nrec * t / ft, nrec * (t + 1) / ft);
                for (auto& x : th) x.join();
            }
        }
        upload(start_, hstart, st); upload(reflen_, hreflen, st); upload(alt0_, halt0, st); upload(altoff_, haltoff, st);
        upload(altchars_, haltchars, st); upload(pair0_, hpair0, st); upload(pa0_, hpa0, st); upload(alleles_, halleles, st);
        }
        d.start = start_.as<u64>(); d.reflen = reflen_.as<u64>(); d.alt0 = alt0_.as<u64>(); d.altstr_off = altoff_.as<u64>();
        d.altchars = altchars_.as<uint8_t>(); d.pair0 = pair0_.as<u64>(); d.pair_a0 = pa0_.as<u64>(); d.alleles = alleles_.as<int>();

        // ---- groups
        for (DevBuf* b : {&ends_, &flag_, &gidx_, &grp_r0_}) b->ensure(vcf_size::per_record(nrec));
        hctl[0] = nrec;
        EDSX_HIP(hipMemcpyAsync(ctl, hctl, 8, hipMemcpyHostToDevice, st));
        // The parallel rule "a record opens a group iff its start is not below the largest end seen so far" equals
        // the reference's sweep (:482-534, group_end restarts with every group) as long as starts ascend with the
        // sort key and no end wraps.  POS 0 (start = 2^64 - 1) or POS near 2^64 ("-5" parses!) break that; such
        // files are swept on the host exactly as the reference does it (running group end per record).
        bool wraps = false;
        for (u64 j = 0; j < hstart.size() && !wraps; j++) wraps = hstart[j] == ~0ull || hstart[j] + hreflen[j] < hstart[j];
        if (!wraps) {
            hipLaunchKernelGGL(k_rec_ends, dim3(1024), dim3(256), 0, st, d.start, d.reflen, nrec, ends_.as<u64>());
            inclusive_max_scan_u64(ends_.as<u64>(), ends_.as<u64>(), ctl + 0, ctl + 2, scan_tmp_.as<u64>(), st);
            hipLaunchKernelGGL(k_mark_groups, dim3(1024), dim3(256), 0, st, d.start, ends_.as<u64>(), nrec, flag_.as<u64>());
        } else {
            std::vector<u64> hflag(nrec), hend(nrec);
            u64 ge = 0;
            for (u64 j = 0; j < nrec; j++) {
                const u64 e = hstart[j] + hreflen[j];
                if (j == 0 || !(hstart[j] < ge)) { hflag[j] = 1; ge = e; }
                else { hflag[j] = 0; ge = std::max(ge, e); }
                hend[j] = ge;
            }
            EDSX_HIP(hipMemcpyAsync(flag_.ptr, hflag.data(), 8 * nrec, hipMemcpyHostToDevice, st));
            EDSX_HIP(hipMemcpyAsync(ends_.ptr, hend.data(), 8 * nrec, hipMemcpyHostToDevice, st));
            EDSX_HIP(hipStreamSynchronize(st));                    // the vectors go out of scope
        }
        exclusive_scan_u64(flag_.as<u64>(), gidx_.as<u64>(), ctl + 0, ctl + 3, scan_tmp_.as<u64>(), st);
        hipLaunchKernelGGL(k_group_firsts, dim3(1024), dim3(256), 0, st, flag_.as<u64>(), gidx_.as<u64>(), nrec,
                           grp_r0_.as<u64>(), ctl + 3);
        EDSX_HIP(hipMemcpyAsync(hctl, ctl, sizeof(hctl), hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        ngrp = hctl[3];
        d.ngrp = ngrp; d.grp_r0 = grp_r0_.as<u64>(); d.incl_end = ends_.as<u64>();

        // ---- per group
        for (DevBuf* b : {&g_gs_, &g_spanlen_, &g_cs_, &g_nraw_, &g_rawchars_, &g_ndist_, &g_bitwords_, &g_eds_, &g_seds_,
                          &g_common_, &g_cur_, &raw0_, &rawc0_, &bit0_}) b->ensure(vcf_size::per_group(ngrp));
        ga = GrpArrays{g_gs_.as<u64>(), g_spanlen_.as<u64>(), g_cs_.as<u64>(), g_nraw_.as<u64>(), g_rawchars_.as<u64>(),
                     g_ndist_.as<u64>(), g_bitwords_.as<u64>(), g_eds_.as<u64>(), g_seds_.as<u64>(), g_common_.as<u64>(),
                       g_cur_.as<u64>(), ctl + 10};
        scan_tmp_.ensure(8 * ((ngrp + 2) / SCAN_TILE + 4));
        hctl[0] = ngrp;
        EDSX_HIP(hipMemcpyAsync(ctl, hctl, 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_grp_count, dim3(1024), dim3(256), 0, st, d, ga);
        exclusive_scan_u64(ga.nraw, raw0_.as<u64>(), ctl + 0, ctl + 4, scan_tmp_.as<u64>(), st);
        exclusive_scan_u64(ga.rawchars, rawc0_.as<u64>(), ctl + 0, ctl + 5, scan_tmp_.as<u64>(), st);
        EDSX_HIP(hipMemcpyAsync(hctl, ctl, sizeof(hctl), hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        const u64 nraw_total = hctl[4], rawchars_total = hctl[5];
        const u32 sw = (u32)std::max<u64>(1, (max_samples + 63) / 64);
        rawlen_.ensure(vcf_size::per_raw(nraw_total)); rawoff_.ensure(vcf_size::per_raw(nraw_total)); canon_.ensure(vcf_size::canon(nraw_total));
        hapchars_.ensure(vcf_size::hapchars(rawchars_total));
        ha = HapArrays{raw0_.as<u64>(), rawc0_.as<u64>(), rawlen_.as<u64>(), rawoff_.as<u64>(), canon_.as<u32>(),
                       hapchars_.as<uint8_t>(), bit0_.as<u64>(), nullptr, sw};
        hipLaunchKernelGGL(k_grp_haps, dim3(1024), dim3(256), 0, st, d, ga, ha);
        exclusive_scan_u64(ga.bitwords, bit0_.as<u64>(), ctl + 0, ctl + 6, scan_tmp_.as<u64>(), st);
        EDSX_HIP(hipMemcpyAsync(hctl, ctl, sizeof(hctl), hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        carried_.ensure(vcf_size::carried(hctl[6]));
        ha.carried = carried_.as<u64>();
        hipLaunchKernelGGL(k_grp_samples, dim3(1024), dim3(256), 0, st, d, ga, ha);
        hipLaunchKernelGGL(k_grp_common, dim3(1024), dim3(256), 0, st, d, ga);
        exclusive_scan_u64(ga.eds_len, ga.eds_len, ctl + 0, ctl + 7, scan_tmp_.as<u64>(), st);
        exclusive_scan_u64(ga.seds_len, ga.seds_len, ctl + 0, ctl + 8, scan_tmp_.as<u64>(), st);
        EDSX_HIP(hipMemcpyAsync(hctl, ctl, sizeof(hctl), hipMemcpyDeviceToHost, st));
        u64 last_cur = 0;
        EDSX_HIP(hipMemcpyAsync(&last_cur, g_cur_.as<u64>() + (ngrp - 1), 8, hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        E = hctl[7]; Q = hctl[8]; cur = last_cur;
        if (window) window_check(hctl[20]);
        mark("groups, haplotypes, sizes");
    }
    // ---- tail (:658-665)
    // A position range that is not the last one ends with what the reference flushes in front of the next
    // range's first group instead (:570-578, `start > cur`, text clamped by read_fasta_region).
    const bool last_range = range.next_start == ~0ull;
    u64 tail = 0;
    if (cur < seq_size && (last_range || range.next_start > cur)) {
        // clamp exactly like read_fasta_region: by seq_size and by what the file still holds
        u64 length = last_range ? seq_size - cur : std::min<u64>(range.next_start - cur, seq_size - cur);
        // position of `cur` in the newline-free stream: ask the device map (one thread)
        hipLaunchKernelGGL(k_cpos, dim3(1), dim3(1), 0, st, d, seq_start + cur + cur / lw, ctl + 11);
        u64 c0 = 0;
        EDSX_HIP(hipMemcpyAsync(&c0, ctl + 11, 8, hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        tail = std::min<u64>(length, refc_n - c0);
        if (window && tail < length) window_check((seq_start + cur + cur / lw) | (1ull << 62));
    }
    const u64 Etot = E + (tail ? tail + 2 : 0), Qtot = Q + (tail ? 3 : 0);
    d_eds_.ensure(vcf_size::eds(Etot)); d_seds_.ensure(vcf_size::eds(Qtot));
    if (ngrp) {
        EmitArrays ea{g_eds_.as<u64>(), g_seds_.as<u64>(), d_eds_.as<uint8_t>(), d_seds_.as<uint8_t>()};
        hipLaunchKernelGGL(k_grp_emit_common, dim3(2048), dim3(256), 0, st, d, ga, ea);
        hipLaunchKernelGGL(k_grp_emit, dim3(2048), dim3(256), 0, st, d, ga, ha, ea);
    }
    if (tail)
        hipLaunchKernelGGL(k_tail, dim3(1024), dim3(256), 0, st, d, cur, tail, d_eds_.as<uint8_t>() + E, d_seds_.as<uint8_t>() + Q);
    mark("tail");
    // malloc'ed, not value-initialised: the pages are first touched by the copy itself (a zero-filling
    // std::string::resize costs as much as the whole device part for a 134 MB output)
    eds.take(Etot);
    seds.take(Qtot);
    PinnedDownload::copy(eds.data, d_eds_.ptr, Etot, st);
    PinnedDownload::copy(seds.data, d_seds_.ptr, Qtot, st);
    u64 oob = 0;
    if (window) EDSX_HIP(hipMemcpyAsync(&oob, ctl + 20, 8, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    window_check(oob);
    stats.variant_groups = ngrp;                             // :724-726
    mark("emit + download");
    return true;
}

} // namespace edsx
