// vcf_contig.hpp — contig selection for vcf2eds: a multi-record FASTA and a multi-contig VCF stay in HBM, a FASTA record
// index and a per-line contig classification are built in front of the pipeline that exists (see vcf_contig.hip).
#pragma once

#include "bgzf_device.hpp"
#include "vcf_contig_walk.hpp"
#include "vcf_device.hpp"

#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace edsx {

// ContigRec, one FASTA record: vcf_contig_walk.hpp

class VcfSession {
public:
    // both buffers stay the caller's and outlive the session
    VcfSession(const uint8_t* vcf, size_t vcf_n, const uint8_t* fasta, size_t fasta_n)
        : vcf_(vcf), vcf_n_(vcf_n), fasta_(fasta), fasta_n_(fasta_n) {}
    // Compressed-input sessions (edsx_vcf_session_open_z): the texts are inflate(vcf) and inflate(fasta) as gz_open left
    // them.  A text that was inflated on the device stays there: the session reads the few bytes the host-side parsing
    // needs (first byte, record names, the head of a record) through small downloads and brings the whole VCF back only
    // when a host path is taken; vcf_d2h / fasta_d2h count those bytes.  own: plain inputs are copied (the caller may
    // release its buffers).  ignore_chrom: the session serves edsx_vcf_transform's meaning - record 0 gets every
    // record line of the VCF, CHROM is not read.
    VcfSession(GzText& vcf, GzText& fasta, bool own, bool ignore_chrom);
    void open(hipStream_t st);

    const std::vector<ContigRec>& contigs() const { return recs_; }
    const std::string& name(size_t index) const { return names_[index]; }
    bool find(const std::string& name, size_t& index) const;       // first record of that name
    // edsx_vcf_transform(V_c, F_c, 0) for record `index`, from the resident inputs where the device accepts them
    void transform(VcfPipeline& pipe, size_t index, HostBytes& eds, HostBytes& seds, VcfCounters& stats, hipStream_t st);
    // contigs the VCF names and the FASTA lacks, with their record lines, in order of first appearance per path:
    // "name\tcount\n" each
    const std::string& unknown_contigs() const { return unknown_text_; }

    u64 records_total = 0, records_without_token = 0, records_unknown = 0, vcf_h2d = 0, fasta_h2d = 0;
    u64 vcf_d2h = 0, fasta_d2h = 0;                                // inflated text copied back to the host
    bool classified_on_device = false;

private:
    void index_fasta(hipStream_t st);
    bool classify_device(hipStream_t st);
    void classify_host();
    void host_text_of(size_t index, std::vector<uint8_t>& out);
    const uint8_t* host_vcf();                                     // the whole VCF text on the host (downloaded once if need be)
    void fetch_fasta(u64 off, u64 len, void* dst);                 // FASTA bytes [off, off + len) from wherever they are

    const uint8_t* vcf_; size_t vcf_n_;
    const uint8_t* fasta_; size_t fasta_n_;
    bool vcf_resident_ = false, fasta_resident_ = false, ignore_chrom_ = false;
    std::vector<uint8_t> own_vcf_, own_fasta_;
    std::vector<ContigRec> recs_;
    std::vector<std::string> names_;                               // per record
    std::unordered_map<std::string, size_t> by_name_;              // name -> first record
    std::vector<u64> first_;                                       // per record: its first line in lsorted_ (device path)
    std::string unknown_text_;
    DevBuf d_fasta_, d_vcf_, lsorted_, d_recs_;
};

} // namespace edsx
