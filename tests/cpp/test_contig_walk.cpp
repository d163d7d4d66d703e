// test_contig_walk.cpp — contig selection on the CPU: the per-thread device code and the session's host arithmetic of
// edsparser_amd/csrc/vcf_contig_walk.hpp, run as VcfSession::open and VcfSession::transform run them, over a case file
// written by tests/contig_walk_cases.py; meant to be built with -fsanitize=address,undefined.  Every buffer is a heap block
// of its own, of exactly the size the session asks for (contig_size::*), filled with a byte the case chooses; the two texts
// are 256-byte aligned as on the device.  What the device does with wave operations or library kernels is a plain loop:
// the in-wave sums of k_fi_count / k_fi_fill (a loop over the 64 lanes of a block), the two block scans (the second one's
// total lands at nnpre[nblk], as in the library), the line starts, and the radix sort - std::stable_sort by the low
// 8 * radix_passes(K) bits of the key, which is what `passes` LSD passes of 8 bits sort by.
//
// Case records (little endian): u32 flags (1: the 4-bit hash instantiation, 2: sweep the two block walks first), u32 nfills, fills, u32 name_len, name, u64 vcf_len,
// vcf, u64 fasta_len, fasta, u32 ncontigs, u32 index[ncontigs] (the records to transform).
// One result per (case, fill): u32 name_len, name, u32 fill, u32 status, then for status 0
//   index           u64 K, ContigRec[K] (vcf_records / duplicate as after the classification that counted)
//   classification  u32 on_device (0: the host's, 1: device), u32 passes, u64 undecidable, u64 oob, u64 nr; on_device: u64 keys[nr] in
//                   file order, u64 lsorted[nr], u64 first[K + 1], u64 counts[K], u64 unknown
//   host            u64 total, without_token, unknown, counts[K], u64 len + the unknown-contig text
//   u32 ncontigs, per contig: u32 index, u32 verdict (0: texts follow, 4: refused, 6: duplicate name), u32 host_tokeniser, u64 len + eds,
//                   u64 len + seds, u64 len + the host text of the contig (contig_text_of)
// status 7 (+ u64 detail): fi_next_newline or fi_nonnl_before differs from a byte-by-byte walk; detail = from << 32 | limit
// status 4: the FASTA is refused   5: a record of the index is out of bounds, or the regrouping is inconsistent
#include "vcf_contig_walk.hpp"
#include "vcf_walk_twin.hpp"

namespace {

struct Out {
    std::ofstream& f;
    void u32v(uint32_t v) { f.write(reinterpret_cast<const char*>(&v), 4); }
    void u64v(uint64_t v) { f.write(reinterpret_cast<const char*>(&v), 8); }
    void raw(const void* p, size_t n) { f.write(static_cast<const char*>(p), n); }
    void blob(const void* p, size_t n) { u64v(n); raw(p, n); }
};

// fi_next_newline(from, limit) and fi_nonnl_before(x) against byte-by-byte walks, for from, limit, x within two bytes of
// every block edge, of every newline and of both ends of the text.  ~0: all equal, else from << 32 | limit
u64 sweep_walks(const FiBlocks& k, const std::vector<uint8_t>& F)
{
    const u64 n = F.size();
    std::vector<u64> pts;
    auto around = [&](u64 x) { for (u64 d = 0; d < 5; d++) if (x + d >= 2 && x + d - 2 <= n) pts.push_back(x + d - 2); };
    around(0); around(n);
    for (u64 b = 0; b <= k.nblk; b++) around(b * VT_BLOCK);
    u64 newlines = 0;
    for (u64 i = 0; i < n; i++) if (F[i] == '\n' && newlines++ < 64) around(i);
    std::sort(pts.begin(), pts.end());
    pts.erase(std::unique(pts.begin(), pts.end()), pts.end());
    std::vector<u64> nonnl(n + 1, 0), next(n + 1, n);                   // bytes != '\n' in [0, x); first '\n' at or behind x (n: none)
    for (u64 i = 0; i < n; i++) nonnl[i + 1] = nonnl[i] + (F[i] != '\n');
    for (u64 i = n; i-- > 0;) next[i] = F[i] == '\n' ? i : next[i + 1];
    for (u64 x : pts) if (fi_nonnl_before(k, x) != nonnl[x]) return x << 32 | x;
    for (u64 from : pts)
        for (u64 limit : pts) {
            if (limit < from) continue;
            if (fi_next_newline(k, from, limit) != std::min(next[from], limit)) return from << 32 | limit;
        }
    return ~0ull;
}

// VcfSession::open + transform for the contigs of `pick`
template <u64 HASH_MASK>
void run_case(uint8_t fill, const std::vector<uint8_t>& V, const std::vector<uint8_t>& F, const std::vector<u32>& pick, bool sweep, Out& out)
{
    Arena A(fill);
    // ---- a) index_fasta
    const u64 n = F.size();
    if (n == 0 || F[0] != '>') { out.u32v(4); return; }
    uint8_t* f = A.get<uint8_t>(contig_size::fasta(n), true);
    std::memcpy(f, F.data(), n);
    const u64 nblk = contig_size::blocks(n);
    u64* hdr = A.get<u64>(contig_size::block_counts(nblk));
    u64* nonnl = A.get<u64>(contig_size::block_counts(nblk));
    for (u64 b = 0; b < nblk; b++) {                                   // k_fi_count
        u64 c = 0, nns = 0;
        for (u64 lane = 0; lane < 64; lane++) { u32 nn; c += (u64)__builtin_popcount(fi_header_mask(f, n, b * VT_BLOCK + lane * 16, nn)); nns += nn; }
        hdr[b] = c; nonnl[b] = nns;
    }
    u64 nhdr = 0;
    exclusive_scan(hdr, hdr, nblk, &nhdr);
    exclusive_scan(nonnl, nonnl, nblk, nonnl + nblk);
    if (nhdr == 0 || nhdr >= 0xffffffffull) { out.u32v(5); return; }
    if (sweep) {
        const u64 bad = sweep_walks(FiBlocks{f, n, nonnl, nblk}, F);
        if (bad != ~0ull) { out.u32v(7); out.u64v(bad); return; }
    }
    u64* hstart = A.get<u64>(contig_size::hstart(nhdr));
    ContigRec* drecs = A.get<ContigRec>(contig_size::records(nhdr));
    for (u64 b = 0; b < nblk; b++) {                                   // k_fi_fill
        u64 at = hdr[b];
        for (u64 lane = 0; lane < 64; lane++) {
            const u64 i0 = b * VT_BLOCK + lane * 16;
            u32 nn;
            u32 m = fi_header_mask(f, n, i0, nn);
            while (m) { if (at < nhdr) hstart[at] = i0 + (u32)__builtin_ctz(m); at++; m &= m - 1; }
        }
    }
    each_thread([&](HostGrid g) { fi_records_body(FiBlocks{f, n, nonnl, nblk}, hstart, nhdr, drecs, g); });
    std::vector<ContigRec> recs(drecs, drecs + nhdr);
    std::vector<std::string> names(nhdr);
    for (size_t r = 0; r < recs.size(); r++) {
        const ContigRec& c = recs[r];
        if (c.rec_start >= c.rec_end || c.rec_end > n || c.name_off + c.name_len > c.rec_end || c.seq_start > c.rec_end) { out.u32v(5); return; }
        names[r].assign(reinterpret_cast<const char*>(F.data() + c.name_off), c.name_len);
    }
    NameIndex by_name;
    mark_duplicates(names, recs, by_name);
    std::memcpy(drecs, recs.data(), sizeof(ContigRec) * nhdr);         // (duplicate flags play no part on the device)
    const u64 K = nhdr;

    // ---- b) classify_device
    const u64 vn = V.size();
    bool on_device = vn != 0;
    const u32 passes = radix_passes(K);
    VcCtl vz{};
    u64 nr = 0, unknown = 0;
    uint8_t* raw = nullptr;
    u64 *lstart = nullptr, *keys = nullptr, *lsorted = nullptr;
    std::vector<u64> first(K + 2, ~0ull);
    if (on_device) {
        raw = A.get<uint8_t>(contig_size::vcf(vn), true);
        std::memcpy(raw, V.data(), vn);
        VtCtl vt;
        on_device = line_starts(A, raw, vn, &vt, lstart);
        nr = on_device ? vt.nrec : 0;
    }
    if (on_device && nr) {
        std::vector<u64> hh;
        std::vector<u32> hr;
        name_table<HASH_MASK>(recs, names, hh, hr);
        u64* thash = A.get<u64>(contig_size::table_hash(hh.size()));
        u32* trec = A.get<u32>(contig_size::table_rec(hr.size()));
        if (!hh.empty()) { std::memcpy(thash, hh.data(), 8 * hh.size()); std::memcpy(trec, hr.data(), 4 * hr.size()); }
        keys = A.get<u64>(contig_size::keys(nr));
        const VcTable t{thash, trec, (u32)hh.size(), drecs, f, K};
        each_thread([&](HostGrid g) { vc_classify_body<HASH_MASK>(raw, vn, lstart, nr, t, keys, &vz, g); });
        if (vz.oob || vz.undecidable) on_device = false;
    }
    if (on_device && nr) {
        u64* keys2 = A.get<u64>(contig_size::keys(nr));
        u32* ord = A.get<u32>(contig_size::order(nr));
        u64* dfirst = A.get<u64>(contig_size::first(K));
        lsorted = A.get<u64>(contig_size::keys(nr));
        std::memset(dfirst, 0xff, contig_size::first(K));
        const u64 low = passes >= 8 ? ~0ull : (1ull << (8 * passes)) - 1ull;
        std::vector<u32> idx(nr);
        for (u64 j = 0; j < nr; j++) idx[j] = (u32)j;
        std::stable_sort(idx.begin(), idx.end(), [&](u32 a, u32 b) { return (keys[a] & low) < (keys[b] & low); });
        for (u64 j = 0; j < nr; j++) { keys2[j] = keys[idx[j]]; ord[j] = idx[j]; }
        each_thread([&](HostGrid g) { vc_regroup_body(keys2, ord, lstart, nr, lsorted, dfirst, g); });
        std::memcpy(first.data(), dfirst, 8 * (K + 1));
        try { contig_counts(first, nr, recs, unknown); } catch (const DeviceError&) { out.u32v(5); return; }
    }
    // ---- c) classify_host, always (on its own copy of the records)
    static const uint8_t none = 0;
    const uint8_t* hv = vn ? V.data() : &none;
    std::vector<ContigRec> hrecs = recs;
    const HostClassified h = classify_lines_host(hv, vn, by_name, hrecs);
    if (!on_device) recs = hrecs;

    out.u32v(0);
    out.u64v(K);
    out.raw(recs.data(), sizeof(ContigRec) * K);
    out.u32v(on_device); out.u32v(passes); out.u64v(vz.undecidable); out.u64v(vz.oob); out.u64v(nr);
    if (on_device) {
        if (nr) { out.raw(keys, 8 * nr); out.raw(lsorted, 8 * nr); }
        out.raw(first.data(), 8 * (K + 1));
        for (const ContigRec& c : recs) out.u64v(c.vcf_records);
        out.u64v(unknown);
    }
    out.u64v(h.total); out.u64v(h.without_token); out.u64v(h.unknown);
    for (const ContigRec& c : hrecs) out.u64v(c.vcf_records);
    out.blob(h.unknown_text.data(), h.unknown_text.size());

    // ---- d) VcfSession::transform
    out.u32v((uint32_t)pick.size());
    for (u32 index : pick) {
        out.u32v(index);
        std::vector<uint8_t> text;
        Result r;
        if (index >= K) r.verdict = 4;
        else if (recs[index].duplicate) r.verdict = 6;
        else {
            const ContigRec& c = recs[index];
            const std::vector<uint8_t> fa(F.begin() + c.rec_start, F.begin() + c.rec_end);    // the record's head is parsed on the host
            Resident res;
            res.d_fasta = f + c.rec_start; res.seq_size = c.seq_size;
            bool done = false;
            if (on_device) {
                res.d_vcf = raw; res.vcf_n = vn; res.nrec = c.vcf_records;
                res.d_lstart = c.vcf_records ? lsorted + first[index] : lsorted;
                r = transform(fill, std::vector<uint8_t>(), fa, false, true, VcfRange(), &res);
                done = !(r.verdict == 1);
                res.d_vcf = nullptr; res.d_lstart = nullptr; res.nrec = 0;
            }
            contig_text_of(hv, vn, reinterpret_cast<const uint8_t*>(names[index].data()), c.name_len, text);
            if (!done) r = transform(fill, text, fa, false, true, VcfRange(), &res);
        }
        out.u32v(r.verdict); out.u32v(r.host_tokeniser);
        out.blob(r.eds.data(), r.eds.size()); out.blob(r.seds.data(), r.seds.size()); out.blob(text.data(), text.size());
    }
}

} // namespace

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: test_contig_walk cases.bin results.bin\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::ofstream of(argv[2], std::ios::binary);
    Out out{of};
    size_t at = 0, runs = 0;
    auto u32at = [&]() { uint32_t v; std::memcpy(&v, file.data() + at, 4); at += 4; return v; };
    auto u64at = [&]() { uint64_t v; std::memcpy(&v, file.data() + at, 8); at += 8; return v; };
    auto bytes = [&](u64 n) { std::vector<uint8_t> v(file.begin() + at, file.begin() + at + n); at += n; return v; };
    while (at < file.size()) {
        const uint32_t flags = u32at(), nfills = u32at();
        const std::vector<uint8_t> fills = bytes(nfills);
        const std::vector<uint8_t> name = bytes(u32at());
        const std::vector<uint8_t> vcf = bytes(u64at());
        const std::vector<uint8_t> fa = bytes(u64at());
        std::vector<u32> pick(u32at());
        for (u32& x : pick) x = u32at();
        for (uint8_t fill : fills) {
            out.u32v((uint32_t)name.size()); out.raw(name.data(), name.size());
            out.u32v(fill);
            if (flags & 1) run_case<0xfull>(fill, vcf, fa, pick, (flags & 2) != 0, out); else run_case<~0ull>(fill, vcf, fa, pick, (flags & 2) != 0, out);
            runs++;
        }
    }
    of.close();
    std::fprintf(stderr, "%zu runs\n", runs);
    return of ? 0 : 1;
}
