// vcf_device.hpp — host driver of the VCF -> EDS overlay pipeline (see vcf_device.hip).
#pragma once

#include "msa_device.hpp"
#include "vcf_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

namespace edsx {

// VcfCounters, FastaMeta, FaSlice, VcfRange, fasta_head, vcf_index, vcf_sort_order and the rest of the host code of this
// path: vcf_host.hpp, which has no HIP include

// Inputs that are already in HBM (a contig session, vcf_contig.hpp): nothing of them is uploaded again.
struct VcfResident {
    // the whole VCF text (256-byte aligned, 16 bytes of slack behind its vcf_n bytes) and the record lines to transform, in
    // file order; d_vcf == nullptr: the text comes from the host buffer as in a call without resident inputs
    const uint8_t* d_vcf = nullptr; u64 vcf_n = 0;
    const u64* d_lstart = nullptr; u64 nrec = 0;
    // first byte of the FASTA record inside the resident file (which has 16 bytes of slack behind its end); the host
    // pointer handed to run() is the same record, [rec_start, rec_end).  seq_size as parse_fasta_metadata counts it.
    const uint8_t* d_fasta = nullptr; u64 seq_size = 0;
};

inline bool vcf_trace_on() { static const bool t = [] { const char* e = getenv("EDSX_TRACE"); return e && atoi(e); }(); return t; }

// EDSX_TRACE=1: device time of a stretch of stream work (events around it), with the text bytes it read
struct TraceSpan {
    hipStream_t st; const char* what; u64 bytes; hipEvent_t a = nullptr, b = nullptr;
    TraceSpan(hipStream_t s, const char* w, u64 by) : st(s), what(w), bytes(by)
    {
        if (!vcf_trace_on()) return;
        EDSX_HIP(hipEventCreate(&a)); EDSX_HIP(hipEventCreate(&b)); EDSX_HIP(hipEventRecord(a, st));
    }
    void end()
    {
        if (!a) return;
        EDSX_HIP(hipEventRecord(b, st)); EDSX_HIP(hipEventSynchronize(b));
        float ms = 0;
        EDSX_HIP(hipEventElapsedTime(&ms, a, b));
        if (bytes) fprintf(stderr, "[edsx pass] %-28s %8.3f ms  %7.1f GB/s of text\n", what, ms, ms > 0 ? bytes / (ms * 1e6) : 0.0);
        else fprintf(stderr, "[edsx pass] %-28s %8.3f ms\n", what, ms);
        (void)hipEventDestroy(a); (void)hipEventDestroy(b); a = b = nullptr;
    }
    ~TraceSpan() { if (a) { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } }
};

// the state of one VcfPipeline::run, handed from stage to stage
struct VcfWalk {
    VcfDev d{}; GrpArrays ga{}; HapArrays ha{};
    RefWindow w{};                 // what of the FASTA the device holds
    u64 max_samples = 0;
    u64 ngrp = 0, E = 0, Q = 0;    // groups and the bytes of their symbols (EDS, sEDS; common text in front included)
    u64 cur = 0, tail = 0;         // reference position behind the last group; bases of the closing common text
    u64 Etot() const { return E + (tail ? tail + 2 : 0); }
    u64 Qtot() const { return Q + (tail ? 3 : 0); }
};

class VcfPipeline {
public:
    // host buffers in; eds/seds text out (FULL brackets, no trailing newline, like the reference)
    // res: inputs that are resident already.  false (only with res->d_vcf): the device tokeniser does not accept these
    // lines, nothing was produced and the caller hands the text over from the host instead.
    bool run(const uint8_t* vcf, size_t vcf_n, const uint8_t* fasta, size_t fasta_n, HostBytes& eds, HostBytes& seds,
             VcfCounters& stats, hipStream_t st, const VcfRange& range = VcfRange(), const VcfResident* res = nullptr);

    bool tokenised_on_device() const { return tokenised_on_device_; }
    u64 fasta_h2d_bytes() const { return fasta_h2d_; }          // FASTA bytes the last run copied to the device
    u64 vcf_h2d_bytes() const { return vcf_h2d_; }              // VCF text bytes the last run copied to the device
    // metadata pass of a partitioned run over the slice [a, b) of the FASTA body (a > seq_start - 1); h2d: bytes copied
    FaSlice fasta_slice(const uint8_t* fasta, u64 a, u64 b, u64 seq_start, u64 rest_from, u64 lw, hipStream_t st, u64& h2d);
    bool index_device(const uint8_t* vcf, size_t n, hipStream_t st, std::vector<u64>& pos, std::vector<u64>& reflen,
                      std::vector<u64>& line_off, std::vector<u64>& line_len, VcfCounters& stats);

private:
    bool tokenised_on_device_ = false;
    u64 fasta_h2d_ = 0, vcf_h2d_ = 0;
    bool tokenize_device(const uint8_t* vcf, size_t n, bool presorted, hipStream_t st, u64& nrec, u64& max_samples,
                         VcfCounters& stats);
    bool tokenize_lines(const uint8_t* raw, u64 n, const u64* lstart, u64 nr, bool presorted, hipStream_t st, u64& nrec,
                        u64& max_samples, VcfCounters& stats);
    // the stages of run(), in its order (vcf_device.hip)
    void reference_stream(VcfWalk& k, const uint8_t* fasta, u64 rest_from, const FastaMeta* meta, const VcfRange& range,
                          const uint8_t* d_resident, hipStream_t st);
    void host_records(VcfWalk& k, const VcfSoA& s, hipStream_t st);
    void grouping(VcfWalk& k, const VcfSoA* host, hipStream_t st);
    void haplotypes_and_sizes(VcfWalk& k, hipStream_t st);
    void tail(VcfWalk& k, u64 next_start, hipStream_t st);
    void emit(const VcfWalk& k, hipStream_t st);
    void download(const VcfWalk& k, HostBytes& eds, HostBytes& seds, hipStream_t st);
    void window_check(const VcfWalk& k, u64 v) const;
    // ctl_ holds one VcfCtl (vcf_walk.hpp); hctl_ is the host's image of it
    VtCtl* vt_ctl() { ctl_.ensure(vcf_size::ctl()); return &ctl_.as<VcfCtl>()->vt; }
    void read_ctl(hipStream_t st);
    void set_scan_count(u64 n, hipStream_t st);
    VcfCtl hctl_{};
    DevBuf vt_raw_, vt_idx_, vt_lstart_, vt_pos_, vt_reflen_, vt_nalt_, vt_altc_, vt_ngt_, vt_nall_, vt_s1_, vt_s2_, vt_s3_,
           vt_s4_, vt_order_, vt_sorttmp_;
    DevBuf d_fasta_, refc_, blkpre_, scan_tmp_, ctl_, start_, reflen_, alt0_, altoff_, altchars_, pair0_, pa0_, alleles_,
           ends_, flag_, gidx_, grp_r0_, g_gs_, g_spanlen_, g_cs_, g_nraw_, g_rawchars_, g_ndist_, g_bitwords_, g_eds_,
           g_seds_, g_common_, g_cur_, raw0_, rawc0_, bit0_, rawlen_, rawoff_, canon_, hapchars_, carried_, d_eds_, d_seds_,
           d_one_, d_slice_, slice_ctl_;
};

} // namespace edsx
