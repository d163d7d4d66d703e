// vcf_contig.hip — contig selection in front of the VCF -> EDS pipeline (vcf_device.hip).
//
// "Contig c of (V, F)" is defined by reduction to the transform that exists: F_c is the first FASTA record named c,
// V_c is V without the record lines whose first token is not c, and the result is edsx_vcf_transform(V_c, F_c).
// The reference reads the first FASTA record only and never looks at CHROM (vcf_transforms.cpp:51-86, :232-326), so
// users of multi-contig files had to split both on the host.  Here both texts go to HBM once and two passes run over them:
//
//   FASTA record index   k_fi_count / k_fi_fill: header starts ('>' at byte 0 or behind '\n') with the geometry of the
//                        record-line passes (a wave owns 1 KB, 16-byte lane loads), plus the bytes of every block that
//                        are not '\n'; k_fi_records: a thread per record derives name span, first sequence line and
//                        seq_size from the scanned block counts — no walk longer than a block or a header line.
//   contig of each line  k_vc_classify: a thread per record line hashes its first tab field (FNV-1a, through ByteWindow),
//                        looks the hash up in the sorted name table and compares the bytes; the stable radix sort of
//                        vcf_text_kernels.hpp regroups the line starts by record index, file order kept inside a contig.
//
// A transform then hands the pipeline one slice of the regrouped line starts and one record of the resident FASTA.
// Lines whose first tab field is empty or holds whitespace are where the reference's tab split and its whitespace
// fallback (:262-279) can disagree about the first token: such a file (and any with '\r') is classified on the host.
#include "vcf_contig.hpp"
#include "vcf_text_kernels.hpp"

#include <chrono>

namespace edsx {

// fi_header_mask, FiBlocks and the walks over them, the bodies of the thread-per-item kernels, and the host arithmetic of
// the session (name table, radix passes, counts, host classification): vcf_contig_walk.hpp, which the host twin compiles too

// ---- FASTA record index ----------------------------------------------------------------------------------
static __global__ void __launch_bounds__(256) k_fi_count(const uint8_t* __restrict__ f, u64 n, u64* __restrict__ hdr, u64* __restrict__ nonnl)
{
    const u64 nblk = (n + VT_BLOCK - 1) / VT_BLOCK;
    const u32 lane = threadIdx.x & 63;
    for (u64 b = (blockIdx.x * (u64)blockDim.x + threadIdx.x) >> 6; b < nblk; b += ((u64)gridDim.x * blockDim.x) >> 6) {
        u32 nn;
        u32 c = (u32)__builtin_popcount(fi_header_mask(f, n, b * VT_BLOCK + lane * 16u, nn));
        for (int o = 32; o > 0; o >>= 1) { c += __shfl_xor(c, o, 64); nn += __shfl_xor(nn, o, 64); }
        if (lane == 0) { hdr[b] = c; nonnl[b] = nn; }
    }
}
static __global__ void __launch_bounds__(256) k_fi_fill(const uint8_t* __restrict__ f, u64 n, const u64* __restrict__ base, u64 nhdr,
                                                        u64* __restrict__ hstart)
{
    const u64 nblk = (n + VT_BLOCK - 1) / VT_BLOCK;
    const u32 lane = threadIdx.x & 63;
    for (u64 b = (blockIdx.x * (u64)blockDim.x + threadIdx.x) >> 6; b < nblk; b += ((u64)gridDim.x * blockDim.x) >> 6) {
        const u64 i0 = b * VT_BLOCK + lane * 16u;
        u32 nn;
        u32 m = fi_header_mask(f, n, i0, nn);
        const u32 c = (u32)__builtin_popcount(m);
        u32 incl = c;
        for (int o = 1; o < 64; o <<= 1) { const u32 x = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += x; }
        u64 at = base[b] + (incl - c);
        while (m) { if (at < nhdr) hstart[at] = i0 + (u32)__builtin_ctz(m); at++; m &= m - 1; }
    }
}

static __global__ void k_fi_records(FiBlocks k, const u64* __restrict__ hstart, u64 nhdr, ContigRec* __restrict__ out)
{
    fi_records_body(k, hstart, nhdr, out, WALK_THREAD);
}

// ---- contig of every record line ---------------------------------------------------------------------------
static __global__ void k_vc_classify(const uint8_t* __restrict__ raw, u64 n, const u64* __restrict__ lstart, u64 nrec, VcTable t,
                                     u64* __restrict__ keys, VcCtl* ctl)
{
    vc_classify_body<~0ull>(raw, n, lstart, nrec, t, keys, ctl, WALK_THREAD);
}
static __global__ void k_vc_regroup(const u64* __restrict__ keys, const u32* __restrict__ order, const u64* __restrict__ lstart, u64 nrec,
                                    u64* __restrict__ lsorted, u64* __restrict__ first)
{
    vc_regroup_body(keys, order, lstart, nrec, lsorted, first, WALK_THREAD);
}

// ---- host --------------------------------------------------------------------------------------------------
VcfSession::VcfSession(GzText& vcf, GzText& fasta, bool own, bool ignore_chrom) : vcf_(nullptr), vcf_n_(0), fasta_(nullptr), fasta_n_(0)
{
    static const uint8_t none = 0;
    ignore_chrom_ = ignore_chrom;
    auto take = [&](GzText& t, const uint8_t*& host, size_t& n, std::vector<uint8_t>& own_buf, DevBuf& dev, bool& resident) {
        n = t.n;
        if (t.on_device) { std::swap(dev.ptr, t.dev.ptr); std::swap(dev.cap, t.dev.cap); resident = true; host = nullptr; return; }
        if (t.on_host) { own_buf.swap(t.host); host = own_buf.data(); }
        else if (own) { own_buf.assign(t.plain, t.plain + t.n); host = own_buf.data(); }
        else host = t.plain;
        if (n == 0 || !host) host = &none;
    };
    take(vcf, vcf_, vcf_n_, own_vcf_, d_vcf_, vcf_resident_);
    take(fasta, fasta_, fasta_n_, own_fasta_, d_fasta_, fasta_resident_);
}

const uint8_t* VcfSession::host_vcf()
{
    if (!vcf_) {
        own_vcf_.resize(vcf_n_ + 1);
        if (vcf_n_) PinnedDownload::copy(own_vcf_.data(), d_vcf_.ptr, vcf_n_, nullptr);
        vcf_d2h += vcf_n_;
        vcf_ = own_vcf_.data();
    }
    return vcf_;
}

void VcfSession::fetch_fasta(u64 off, u64 len, void* dst)
{
    if (len == 0) return;
    if (fasta_) { memcpy(dst, fasta_ + off, len); return; }
    EDSX_HIP(hipMemcpy(dst, d_fasta_.as<uint8_t>() + off, len, hipMemcpyDeviceToHost));
    fasta_d2h += len;
}

void VcfSession::index_fasta(hipStream_t st)
{
    const u64 n = fasta_n_;
    uint8_t first = 0;
    if (n) fetch_fasta(0, 1, &first);
    if (n == 0 || first != '>') throw FormatError("Invalid FASTA format: expected header line starting with '>'");
    if (!fasta_resident_) {
        d_fasta_.ensure(contig_size::fasta(n));
        EDSX_HIP(hipMemcpyAsync(d_fasta_.ptr, fasta_, n, hipMemcpyHostToDevice, st));
        fasta_h2d += n;
    }
    const u64 nblk = contig_size::blocks(n);
    DevBuf hdr, nonnl, tmp, ctl, hstart;
    hdr.ensure(contig_size::block_counts(nblk)); nonnl.ensure(contig_size::block_counts(nblk)); tmp.ensure(8 * ((nblk + 2) / SCAN_TILE + 4)); ctl.ensure(8 * 8);
    struct FiCtl { u64 n, nhdr; };                                           // the header scan's element count and total
    FiCtl hctl{nblk, 0};
    FiCtl* dctl = ctl.as<FiCtl>();
    EDSX_HIP(hipMemcpyAsync(dctl, &hctl, sizeof(hctl), hipMemcpyHostToDevice, st));
    const uint8_t* f = d_fasta_.as<uint8_t>();
    TraceSpan span(st, "fasta record index", n);
    hipLaunchKernelGGL(k_fi_count, dim3(2048), dim3(256), 0, st, f, n, hdr.as<u64>(), nonnl.as<u64>());
    exclusive_scan_u64(hdr.as<u64>(), hdr.as<u64>(), &dctl->n, &dctl->nhdr, tmp.as<u64>(), st);
    exclusive_scan_u64(nonnl.as<u64>(), nonnl.as<u64>(), &dctl->n, nonnl.as<u64>() + nblk, tmp.as<u64>(), st);
    EDSX_HIP(hipMemcpyAsync(&hctl, dctl, sizeof(hctl), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    const u64 nhdr = hctl.nhdr;                                             // >= 1: byte 0 is a '>'
    if (nhdr == 0 || nhdr >= 0xffffffffull) throw DeviceError("FASTA record index: " + std::to_string(nhdr) + " records");
    hstart.ensure(contig_size::hstart(nhdr));
    d_recs_.ensure(contig_size::records(nhdr));
    hipLaunchKernelGGL(k_fi_fill, dim3(2048), dim3(256), 0, st, f, n, hdr.as<u64>(), nhdr, hstart.as<u64>());
    hipLaunchKernelGGL(k_fi_records, dim3((unsigned)std::min<u64>((nhdr + 255) / 256, 1024)), dim3(256), 0, st, FiBlocks{f, n, nonnl.as<u64>(), nblk},
                       hstart.as<u64>(), nhdr, d_recs_.as<ContigRec>());
    span.end();
    recs_.resize(nhdr);
    EDSX_HIP(hipMemcpyAsync(recs_.data(), d_recs_.ptr, sizeof(ContigRec) * nhdr, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    names_.resize(recs_.size());
    for (size_t r = 0; r < recs_.size(); r++) {
        ContigRec& c = recs_[r];
        if (c.rec_start >= c.rec_end || c.rec_end > n || c.name_off + c.name_len > c.rec_end || c.seq_start > c.rec_end)
            throw DeviceError("FASTA record index: record " + std::to_string(r) + " out of bounds");
        names_[r].resize(c.name_len);
        if (c.name_len) fetch_fasta(c.name_off, c.name_len, &names_[r][0]);
    }
    mark_duplicates(names_, recs_, by_name_);
}

bool VcfSession::classify_device(hipStream_t st)
{
    { const char* e = getenv("EDSX_HOST_TOKENIZER"); if (e && atoi(e)) return false; }
    const u64 n = vcf_n_;
    if (!device_scratch_fits(6 * n)) return false;
    d_vcf_.ensure(contig_size::vcf(n));
    DevBuf idx, tmp, ctlb, lstart, keys, keys2, ord1, ord2, table, first, thash, trec;
    struct ClassifyCtl { VtCtl vt; VcCtl vc; };                             // the line-start step's and the classification's
    ctlb.ensure(8 * 32);
    VtCtl* ctl = &ctlb.as<ClassifyCtl>()->vt;
    VcCtl* vctl = &ctlb.as<ClassifyCtl>()->vc;
    vt_line_starts_reset(n, ctl, idx, tmp, st);
    if (!vcf_resident_) {
        EDSX_HIP(hipMemcpyAsync(d_vcf_.ptr, vcf_, n, hipMemcpyHostToDevice, st));
        vcf_h2d += n;
    }
    const uint8_t* raw = d_vcf_.as<uint8_t>();
    TraceSpan lines(st, "vcf line starts", 2 * n);     // (count pass + fill pass: the text is read twice)
    const u64 nr = vt_line_starts(raw, n, ctl, idx, lstart, tmp, st);
    if (nr == VT_NOT_PLAIN) return false;                                    // '\r' somewhere, or too many lines
    lines.end();
    const u64 K = recs_.size();
    first_.assign(K + 2, ~0ull);
    if (nr == 0) { records_total = 0; return true; }
    if (ignore_chrom_) {                                                     // every record line belongs to record 0, file order
        EDSX_HIP(hipStreamSynchronize(st));
        std::swap(lsorted_.ptr, lstart.ptr); std::swap(lsorted_.cap, lstart.cap);
        first_[0] = 0;
        recs_[0].vcf_records = nr;
        records_total = nr;
        return true;
    }

    // name table: one entry per distinct name, sorted by hash
    std::vector<u64> hh;
    std::vector<u32> hr;
    name_table(recs_, names_, hh, hr);
    thash.ensure(contig_size::table_hash(hh.size())); trec.ensure(contig_size::table_rec(hr.size()));
    EDSX_HIP(hipMemcpyAsync(thash.ptr, hh.data(), 8 * hh.size(), hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemcpyAsync(trec.ptr, hr.data(), 4 * hr.size(), hipMemcpyHostToDevice, st));
    VcCtl vz{};
    EDSX_HIP(hipMemcpyAsync(vctl, &vz, sizeof(vz), hipMemcpyHostToDevice, st));
    keys.ensure(contig_size::keys(nr));
    const VcTable t{thash.as<u64>(), trec.as<u32>(), (u32)hh.size(), d_recs_.as<ContigRec>(), d_fasta_.as<uint8_t>(), K};
    TraceSpan cls(st, "contig classification", n);
    hipLaunchKernelGGL(k_vc_classify, dim3(2048), dim3(256), 0, st, raw, n, lstart.as<u64>(), nr, t, keys.as<u64>(), vctl);
    cls.end();
    EDSX_HIP(hipMemcpyAsync(&vz, vctl, sizeof(vz), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));                                      // (hh, hr are uploaded)
    if (vz.oob) throw DeviceError("contig classification: byte index " + std::to_string(vz.oob & ((1ull << 62) - 1)) +
                                  " outside the text of " + std::to_string(n) + " bytes");
    if (vz.undecidable) return false;

    // stable regrouping by record index (K = no such contig, last): one 8-bit pass per byte of K
    const u32 passes = radix_passes(K);
    const u64 ntiles = (nr + RS_TILE - 1) / RS_TILE, nbins = 256 * ntiles;
    keys2.ensure(contig_size::keys(nr)); ord1.ensure(contig_size::order(nr)); ord2.ensure(contig_size::order(nr)); table.ensure(8 * (nbins + 2));
    tmp.ensure(8 * (nbins / SCAN_TILE + 4));
    first.ensure(contig_size::first(K));
    lsorted_.ensure(contig_size::keys(nr));
    EDSX_HIP(hipMemcpyAsync(&vctl->n, &nbins, 8, hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemsetAsync(first.ptr, 0xff, contig_size::first(K), st));
    const unsigned grid = (unsigned)std::min<u64>(ntiles, 1u << 16);
    TraceSpan srt(st, "regrouping (radix sort)", 0);
    // keys -> (keys2, ord1) -> (keys, ord2) -> (keys2, ord1) ...
    const u64* kin = keys.as<u64>();
    const u32* vin = nullptr;
    for (u32 p = 0; p < passes; p++) {
        u64* kout = (p & 1) ? keys.as<u64>() : keys2.as<u64>();
        u32* vout = (p & 1) ? ord2.as<u32>() : ord1.as<u32>();
        hipLaunchKernelGGL(k_rs_hist, dim3(grid), dim3(64), 0, st, kin, nr, 8 * p, ntiles, table.as<u64>());
        exclusive_scan_u64(table.as<u64>(), table.as<u64>(), &vctl->n, &vctl->total, tmp.as<u64>(), st);
        hipLaunchKernelGGL(k_rs_scatter, dim3(grid), dim3(64), 0, st, kin, vin, nr, 8 * p, ntiles, table.as<u64>(), kout, vout);
        kin = kout; vin = vout;
    }
    hipLaunchKernelGGL(k_vc_regroup, dim3(2048), dim3(256), 0, st, kin, vin, lstart.as<u64>(), nr, lsorted_.as<u64>(), first.as<u64>());
    srt.end();
    EDSX_HIP(hipMemcpyAsync(first_.data(), first.ptr, 8 * (K + 1), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    // counts: a contig's lines end where the next contig that has lines begins
    contig_counts(first_, nr, recs_, records_unknown);
    records_total = nr;
    if (records_unknown) {                                                   // their names, for the caller's warnings
        std::vector<u64> ls(records_unknown);
        EDSX_HIP(hipMemcpy(ls.data(), lsorted_.as<u64>() + first_[K], 8 * records_unknown, hipMemcpyDeviceToHost));
        UnknownNames un;
        const uint8_t* hv = host_vcf();
        for (u64 lo : ls) {
            size_t e = lo;
            while (e < n && hv[e] != '\t' && hv[e] != '\n') e++;
            un.add(std::string(reinterpret_cast<const char*>(hv + lo), e - lo));
        }
        unknown_text_ = un.text();
    }
    return true;
}

void VcfSession::classify_host()
{
    host_vcf();
    if (ignore_chrom_) return;                                               // (the whole text is record 0's)
    const HostClassified h = classify_lines_host(vcf_, vcf_n_, by_name_, recs_);
    records_total = h.total; records_without_token = h.without_token; records_unknown = h.unknown;
    unknown_text_ = h.unknown_text;
}

void VcfSession::open(hipStream_t st)
{
    index_fasta(st);
    classified_on_device = false;
    if (vcf_n_ == 0) return;
    classified_on_device = classify_device(st);
    if (!classified_on_device) {
        host_vcf();                                                          // (before the resident text goes)
        vcf_resident_ = false;
        d_vcf_.release(); lsorted_.release();
        classify_host();
    }
}

bool VcfSession::find(const std::string& name, size_t& index) const
{
    const auto it = by_name_.find(name);
    if (it == by_name_.end()) return false;
    index = it->second;
    return true;
}

// V_c: every line that is empty, starts with '#', or is a record line whose first token is the record's name
void VcfSession::host_text_of(size_t index, std::vector<uint8_t>& out)
{
    host_vcf();
    contig_text_of(vcf_, vcf_n_, reinterpret_cast<const uint8_t*>(names_[index].data()), recs_[index].name_len, out);
}

void VcfSession::transform(VcfPipeline& pipe, size_t index, HostBytes& eds, HostBytes& seds, VcfCounters& stats, hipStream_t st)
{
    if (index >= recs_.size()) throw ParamError("contig index " + std::to_string(index) + " out of range");
    const ContigRec& c = recs_[index];
    if (c.duplicate)
        throw ParamError("Contig '" + names_[index] +
                         "': record " + std::to_string(index) + " repeats the name of an earlier FASTA record");
    VcfResident res;
    res.d_fasta = d_fasta_.as<uint8_t>() + c.rec_start;
    res.seq_size = c.seq_size;
    const size_t fa_n = c.rec_end - c.rec_start;
    static const uint8_t none = 0;
    // the pipeline parses the record's header line and first sequence line on the host: of a FASTA that lives in HBM
    // only, a window that holds both comes down (64 KiB, larger while the two lines do not end inside it)
    std::vector<uint8_t> head;
    const uint8_t* fa = fasta_ ? fasta_ + c.rec_start : nullptr;
    if (!fa) {
        for (u64 w = std::min<u64>(fa_n, 1u << 16);; w = std::min<u64>(fa_n, w * 4)) {
            head.resize(w + 1);
            fetch_fasta(c.rec_start, w, head.data());
            if (w == fa_n) break;
            bool inside = false;
            try { u64 ss, lw, rf; fasta_head(head.data(), w, ss, lw, rf); inside = rf < w; } catch (const FormatError&) {}
            if (inside) break;
        }
        fa = head.data();
    }
    if (classified_on_device) {
        res.d_vcf = d_vcf_.as<uint8_t>(); res.vcf_n = vcf_n_;
        res.nrec = c.vcf_records;
        res.d_lstart = c.vcf_records ? lsorted_.as<u64>() + first_[index] : lsorted_.as<u64>();
        if (pipe.run(&none, 0, fa, fa_n, eds, seds, stats, st, VcfRange(), &res)) return;
        res.d_vcf = nullptr; res.d_lstart = nullptr; res.nrec = 0;           // the tokeniser refuses these lines: host text
    }
    std::vector<uint8_t> text;
    const uint8_t* tp = &none;
    size_t tn = 0;
    if (ignore_chrom_) { tp = host_vcf(); tn = vcf_n_; }
    else { host_text_of(index, text); if (!text.empty()) { tp = text.data(); tn = text.size(); } }
    try {
        pipe.run(tp, tn, fa, fa_n, eds, seds, stats, st, VcfRange(), &res);
    } catch (...) { vcf_h2d += pipe.vcf_h2d_bytes(); throw; }
    vcf_h2d += pipe.vcf_h2d_bytes();
}

} // namespace edsx
