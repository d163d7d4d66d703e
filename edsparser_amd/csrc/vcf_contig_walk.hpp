// vcf_contig_walk.hpp — the per-thread code of contig selection (vcf_contig.hip) and the host arithmetic of VcfSession, as
// one definition that hipcc compiles for the library and g++ compiles for tests/cpp/test_contig_walk.cpp, which runs the
// FASTA record index and the classification of the record lines on the CPU under the address and undefined-behaviour
// sanitizers, on buffers of exactly the sizes at the end of this file (contig_size::*; DESIGN 5, "the contig twin").
// Bodies take (..., grid) as those of vcf_walk.hpp do.  The two wave-level kernels (k_fi_count, k_fi_fill) stay in the
// .hip: their per-lane work is fi_header_mask, and the host program redoes their in-wave sums with a loop over 64 lanes.
#pragma once

#include "errors.hpp"
#include "vcf_walk.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace edsx {

// one FASTA record (the layout of edsx_contig, include/edsx.h)
struct ContigRec {
    u64 name_off, name_len;        // name bytes inside the FASTA: behind '>' up to the first ' ' or the end of the header line
    u64 rec_start, rec_end;        // the record: from its '>' up to the next '>' at a line start (or the end of the file)
    u64 seq_start, line_width;     // first sequence line (vcf_transforms.cpp:59-67); seq_start == rec_end: no such line
    u64 seq_size;                  // bytes of [seq_start, rec_end) that are not '\n' (:69-84)
    u64 vcf_records;               // record lines of the VCF whose first token is this name
    u64 duplicate;                 // 1: an earlier record has the same name
};

constexpr u64 FNV_OFFSET = 1469598103934665603ull, FNV_PRIME = 1099511628211ull;

// ---- FASTA record index ----------------------------------------------------------------------------------
// bit i: byte i0 + i is a '>' that starts a line; nn: bytes of the chunk that are not '\n'
VCF_HDF u32 fi_header_mask(const uint8_t* __restrict__ f, u64 n, u64 i0, u32& nn)
{
    nn = 0;
    if (i0 >= n) return 0;
    const Chunk16 v = *reinterpret_cast<const Chunk16*>(f + i0);          // (256-byte aligned buffer, 16 bytes of slack)
    const u32 valid = n - i0 >= 16 ? 0xffffu : (1u << (n - i0)) - 1u;
    const u32 nl = chunk_eq16b(v, 0x0a0a0a0au), gt = chunk_eq16b(v, 0x3e3e3e3eu);
    const u32 prev_nl = ((nl << 1) | (i0 == 0 || f[i0 - 1] == '\n' ? 1u : 0u)) & 0xffffu;
    nn = (u32)__builtin_popcount(~nl & valid);
    return gt & prev_nl & valid;
}

// nnpre[b] = bytes that are not '\n' in front of block b (b <= nblk; nnpre[nblk] = all of them)
struct FiBlocks { const uint8_t* f; u64 n; const u64* nnpre; u64 nblk; };
VCF_HDF u64 fi_newlines_before(const FiBlocks& k, u64 b)
{
    const u64 bytes = b * VT_BLOCK < k.n ? b * VT_BLOCK : k.n;
    return bytes - k.nnpre[b];
}
// the first '\n' in [from, limit), or limit (limit <= n): the rest of from's block byte by byte, then a binary search over
// the block counts for the next block that holds a newline, then that block
VCF_HD u64 fi_next_newline(const FiBlocks& k, u64 from, u64 limit)
{
    if (from >= limit) return limit;
    const u64 b = from / VT_BLOCK;
    const u64 e = (b + 1) * VT_BLOCK < limit ? (b + 1) * VT_BLOCK : limit;
    for (u64 i = from; i < e; i++) if (k.f[i] == '\n') return i;
    if (e >= limit) return limit;
    const u64 have = fi_newlines_before(k, b + 1);
    u64 lo = b + 1, hi = (limit + VT_BLOCK - 1) / VT_BLOCK;                 // blocks [lo, hi) overlap [e, limit); hi <= nblk
    const u64 end = hi;
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (fi_newlines_before(k, mid + 1) > have) hi = mid; else lo = mid + 1;
    }
    if (lo >= end) return limit;
    const u64 e2 = (lo + 1) * VT_BLOCK < limit ? (lo + 1) * VT_BLOCK : limit;
    for (u64 i = lo * VT_BLOCK; i < e2; i++) if (k.f[i] == '\n') return i;
    return limit;
}
// bytes of [0, x) that are not '\n' (x <= n)
VCF_HD u64 fi_nonnl_before(const FiBlocks& k, u64 x)
{
    const u64 b = x / VT_BLOCK;
    u64 c = k.nnpre[b];
    for (u64 i = b * VT_BLOCK; i < x; i++) c += k.f[i] != '\n';
    return c;
}
// a thread per record: name span, first sequence line and seq_size from the scanned block counts
template <class G> VCF_HDF void fi_records_body(FiBlocks k, const u64* __restrict__ hstart, u64 nhdr, ContigRec* __restrict__ out, G grid)
{
    for (u64 r = grid.first(); r < nhdr; r += grid.stride()) {
        const u64 rs = hstart[r], re = r + 1 < nhdr ? hstart[r + 1] : k.n;
        const u64 hl = fi_next_newline(k, rs, re);                          // end of the header line
        u64 ne = rs + 1;
        while (ne < hl && k.f[ne] != ' ') ne++;
        const u64 ss = hl < re ? hl + 1 : re;
        ContigRec c;
        c.name_off = rs + 1; c.name_len = ne - (rs + 1);
        c.rec_start = rs; c.rec_end = re;
        c.seq_start = ss; c.line_width = fi_next_newline(k, ss, re) - ss;
        c.seq_size = fi_nonnl_before(k, re) - fi_nonnl_before(k, ss);
        c.vcf_records = 0; c.duplicate = 0;
        out[r] = c;
    }
}

// ---- contig of every record line ---------------------------------------------------------------------------
// names: the records that are not duplicates, sorted by the FNV-1a hash of their name
struct VcTable { const u64* hash; const u32* rec; u32 T; const ContigRec* recs; const uint8_t* fasta; u64 nrecs; };
struct VcCtl { u64 n, total, undecidable, oob; };

// HASH_MASK: all ones in the library (the "&" folds away).  The host program also builds a 4-bit instantiation, whose
// table holds the masked hashes: there the loop behind the binary search runs over real collisions.
template <u64 HASH_MASK, class G>
VCF_HDF void vc_classify_body(const uint8_t* __restrict__ raw, u64 n, const u64* __restrict__ lstart, u64 nrec, VcTable t,
                              u64* __restrict__ keys, VcCtl* ctl, G grid)
{
    bool und = false;
    for (u64 j = grid.first(); j < nrec; j += grid.stride()) {
        ByteWindow win(raw, n);
        const u64 lo = lstart[j];
        u64 i = lo, h = FNV_OFFSET;
        bool ws = false;
        for (; i < n; i++) {
            const uint8_t ch = win[i];
            if (ch == '\t' || ch == '\n') break;
            ws |= ch == ' ' || ch == '\r' || ch == '\v' || ch == '\f';
            h = (h ^ ch) * FNV_PRIME;
        }
        h &= HASH_MASK;
        const u64 len = i - lo;
        u64 key = t.nrecs;                                                  // no such contig
        if (len == 0 || ws) und = true;                                     // tab rule and whitespace rule may differ: host
        else {
            u32 a = 0, b = t.T;
            while (a < b) { const u32 m = a + (b - a) / 2; if (t.hash[m] < h) a = m + 1; else b = m; }
            for (; a < t.T && t.hash[a] == h && key == t.nrecs; a++) {      // the hash finds, the bytes decide
                const ContigRec& c = t.recs[t.rec[a]];
                if (c.name_len != len) continue;
                bool eq = true;
                for (u64 x = 0; x < len && eq; x++) eq = win[lo + x] == t.fasta[c.name_off + x];
                if (eq) key = t.rec[a];
            }
        }
        if (win.oob) ctl->oob = win.oob;
        keys[j] = key;
    }
    if (und) ctl->undecidable = 1;
}
// line starts in regrouped order, and the first line of every contig that has one (first[] is preset to ~0)
template <class G>
VCF_HDF void vc_regroup_body(const u64* __restrict__ keys, const u32* __restrict__ order, const u64* __restrict__ lstart, u64 nrec,
                             u64* __restrict__ lsorted, u64* __restrict__ first, G grid)
{
    for (u64 j = grid.first(); j < nrec; j += grid.stride()) {
        lsorted[j] = lstart[order[j]];
        if (j == 0 || keys[j] != keys[j - 1]) first[keys[j]] = j;
    }
}

// ---- host: the arithmetic of VcfSession over host arrays -------------------------------------------------------
inline bool host_isspace(uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }   // what operator>> skips ("C" locale)

inline u64 fnv1a(const uint8_t* p, size_t n)
{
    u64 h = FNV_OFFSET;
    for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * FNV_PRIME;
    return h;
}

// first token of a record line [p, p + n): the first maximal run of bytes that are not whitespace
inline bool first_token(const uint8_t* p, size_t n, size_t& lo, size_t& len)
{
    size_t i = 0;
    while (i < n && host_isspace(p[i])) i++;
    size_t j = i;
    while (j < n && !host_isspace(p[j])) j++;
    lo = i; len = j - i;
    return j > i;
}

typedef std::unordered_map<std::string, size_t> NameIndex;        // name -> first record

// names[r] is record r's name: by_name gets the first record of every name, the later ones are marked
inline void mark_duplicates(const std::vector<std::string>& names, std::vector<ContigRec>& recs, NameIndex& by_name)
{
    for (size_t r = 0; r < recs.size(); r++) recs[r].duplicate = by_name.emplace(names[r], r).second ? 0 : 1;
}

// name table: one entry per distinct name, sorted by (masked) hash
template <u64 HASH_MASK = ~0ull>
inline void name_table(const std::vector<ContigRec>& recs, const std::vector<std::string>& names, std::vector<u64>& hash, std::vector<u32>& rec)
{
    std::vector<std::pair<u64, u32>> tab;
    for (size_t r = 0; r < recs.size(); r++)
        if (!recs[r].duplicate) tab.push_back({fnv1a(reinterpret_cast<const uint8_t*>(names[r].data()), names[r].size()) & HASH_MASK, (u32)r});
    std::sort(tab.begin(), tab.end());
    hash.resize(tab.size()); rec.resize(tab.size());
    for (size_t i = 0; i < tab.size(); i++) { hash[i] = tab[i].first; rec[i] = tab[i].second; }
}

// stable regrouping by record index (K = no such contig, last): one 8-bit pass per byte of K
inline u32 radix_passes(u64 K)
{
    u32 passes = 1;
    while (passes < 4 && (K >> (8 * passes))) passes++;
    return passes;
}

// counts out of first[0..K] (~0: no line): a contig's lines end where the next contig that has lines begins
inline void contig_counts(const std::vector<u64>& first, u64 nr, std::vector<ContigRec>& recs, u64& records_unknown)
{
    const size_t K = recs.size();
    u64 next = nr;
    for (size_t r = K + 1; r-- > 0;) {
        if (first[r] == ~0ull) continue;
        if (first[r] >= next) throw DeviceError("contig regrouping: first lines out of order");
        const u64 cnt = next - first[r];
        if (r < K) recs[r].vcf_records = cnt; else records_unknown = cnt;
        next = first[r];
    }
    if (next != 0) throw DeviceError("contig regrouping: lines without a contig");
}

// names the FASTA lacks, in order of first appearance, with their record lines: "name\tcount\n" each
struct UnknownNames {
    std::unordered_map<std::string, size_t> at;
    std::vector<std::pair<std::string, u64>> names;
    void add(const std::string& key)
    {
        const auto ins = at.emplace(key, names.size());
        if (ins.second) names.push_back({key, 0});
        names[ins.first->second].second++;
    }
    std::string text() const
    {
        std::string out;
        for (const auto& nm : names) out += nm.first + "\t" + std::to_string(nm.second) + "\n";
        return out;
    }
};

// the classification on the host: every record line's first token against by_name
struct HostClassified { u64 total = 0, without_token = 0, unknown = 0; std::string unknown_text; };
inline HostClassified classify_lines_host(const uint8_t* vcf, size_t vcf_n, const NameIndex& by_name, std::vector<ContigRec>& recs)
{
    HostClassified r;
    for (ContigRec& c : recs) c.vcf_records = 0;
    UnknownNames un;
    std::string key;
    for (size_t pos = 0; pos < vcf_n;) {
        const uint8_t* nl = static_cast<const uint8_t*>(memchr(vcf + pos, '\n', vcf_n - pos));
        const size_t end = nl ? static_cast<size_t>(nl - vcf) : vcf_n;
        if (end > pos && vcf[pos] != '#') {
            r.total++;
            size_t lo, len;
            if (!first_token(vcf + pos, end - pos, lo, len)) r.without_token++;
            else {
                key.assign(reinterpret_cast<const char*>(vcf + pos + lo), len);
                const auto it = by_name.find(key);
                if (it != by_name.end()) recs[it->second].vcf_records++;
                else { r.unknown++; un.add(key); }
            }
        }
        pos = nl ? end + 1 : vcf_n;
    }
    r.unknown_text = un.text();
    return r;
}

// V_c: every line that is empty, starts with '#', or is a record line whose first token is `name`
inline void contig_text_of(const uint8_t* vcf, size_t vcf_n, const uint8_t* name, size_t name_len, std::vector<uint8_t>& out)
{
    out.clear();
    for (size_t pos = 0; pos < vcf_n;) {
        const uint8_t* nl = static_cast<const uint8_t*>(memchr(vcf + pos, '\n', vcf_n - pos));
        const size_t end = nl ? static_cast<size_t>(nl - vcf) : vcf_n;
        bool keep = end == pos || vcf[pos] == '#';
        if (!keep) {
            size_t lo, len;
            keep = first_token(vcf + pos, end - pos, lo, len) && len == name_len && memcmp(vcf + pos + lo, name, len) == 0;
        }
        const size_t upto = nl ? end + 1 : vcf_n;
        if (keep) out.insert(out.end(), vcf + pos, vcf + upto);
        pos = upto;
    }
}

// ---- what VcfSession allocates for the arrays above, in bytes ------------------------------------------------------
// (fi_header_mask's 16-byte load and ByteWindow rest on the slack of the two texts; the second block scan puts its total
// at nnpre[nblk]; first[] has an entry for "no such contig" at K.)
namespace contig_size {
inline u64 fasta(u64 n) { return n + 16; }                         // d_fasta_
inline u64 vcf(u64 n) { return vcf_size::text(n); }                 // d_vcf_
inline u64 blocks(u64 n) { return (n + VT_BLOCK - 1) / VT_BLOCK; }
inline u64 block_counts(u64 nblk) { return 8 * (nblk + 2); }        // header starts and non-newline bytes per block
inline u64 hstart(u64 nhdr) { return 8 * (nhdr + 1); }
inline u64 records(u64 nhdr) { return sizeof(ContigRec) * (nhdr + 1); }
inline u64 keys(u64 nr) { return 8 * (nr + 2); }                    // keys, their double buffer, lsorted_
inline u64 order(u64 nr) { return 4 * (nr + 2); }
inline u64 first(u64 K) { return 8 * (K + 2); }
inline u64 table_hash(u64 tab) { return 8 * (tab + 1); }
inline u64 table_rec(u64 tab) { return 4 * (tab + 1); }
}

} // namespace edsx
