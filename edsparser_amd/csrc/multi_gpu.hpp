// multi_gpu.hpp — MSA -> EDS over several GPUs of one node from C++: column slabs + boundary stitch over RCCL.
//
// One host thread per GPU.  Every rank cuts its column slab [L*r/N, L*(r+1)/N) out of every row of the host FASTA image
// (column c of row s is byte start[s] + c + c / line_width, msa_transforms.cpp:268-269), uploads it as a
// one-line-per-row image (2D copies: a row's slab is one contiguous piece), transforms it with its own MsaPipeline as
// if it were a whole alignment, and the runs that cross a slab boundary are repaired with KB-sized exchanges
// (SURVEY §8(e)): an all-gather of twelve numbers per rank (the edge descriptors), and - only when a VARIANT run
// crosses a boundary - an all-gather of the raw boundary columns, from which the left-most rank recomputes that
// segment.  With a context length l > 0 every boundary is recomputed between the nearest standalone common runs of at
// least l columns on either side (the anchors).  What is decided on the host - the geometry of the image, the cuts, the
// descriptors and which bytes and boundaries follow from them (SlabStitch) - is msa_slabs.hpp, without a HIP include
// and tested on the CPU; MultiMsa::run_rank (one rank, either context length) and msa_transform_batched (the same slabs
// one after the other on one GPU) in multi_gpu.hip run on it.  The exchanges are ncclAllGather calls on one
// communicator per rank (RcclExchange); LocalExchange moves the same bytes between the rank threads directly and exists
// so that the whole path can be tested with several contexts sharing ONE GPU (RCCL does not run two ranks on one device).
#pragma once

#include "msa_device.hpp"
#include "msa_slabs.hpp"
#include "rank_barrier.hpp"
#include "merge_device.hpp"
#include "merge_scan.hpp"
#include "vcf_device.hpp"

#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace edsx {

// columns [c0, c1) of every row as a one-line-per-row image in HBM, every row on a multiple of 128 bytes (see multi_gpu.hip)
struct RowImage { u64 rows = 0, cols = 0, hdr0 = 0, hdr = 0, bytes = 0; };
RowImage upload_row_image(const uint8_t* fasta, const MsaLayout& lay, u64 c0, u64 c1, DevBuf& d_img, std::vector<uint8_t>& host_tmp,
                          hipStream_t st);
// one alignment image on the current device: the n bytes in d_img -> plan, emit, download; _plain uploads the file as it is first
void msa_image_to_text(MsaPipeline& p, const DevBuf& d_img, size_t n, uint32_t l, DevBuf& d_eds, DevBuf& d_seds, HostBytes& eds,
                       HostBytes& seds, hipStream_t st);
void msa_transform_plain(MsaPipeline& p, const uint8_t* msa, size_t n, uint32_t l, DevBuf& d_img, DevBuf& d_eds, DevBuf& d_seds,
                         HostBytes& eds, HostBytes& seds, hipStream_t st);

// What transforms slabs on one device, the owner's members: the slab's pipeline and a second one through which boundary
// segments are recomputed (the slab's plan stays), the slab image, its text, the mini alignment, and host scratch
struct SlabWorker { MsaPipeline* slab; MsaPipeline* mini; DevBuf* d_img; DevBuf* d_eds; DevBuf* d_seds; DevBuf* d_mini; std::vector<uint8_t>* host; };

// msa2eds in K column batches on one GPU (working set of one slab; see multi_gpu.hip).  false: not batched - the image is
// not a plain uniform alignment, the batches would be too narrow, or (l > 0) a slab has no standalone common runs to
// anchor the stitch on; nothing has been written to eds / seds then.
bool msa_transform_batched(const SlabWorker& w, const uint8_t* fasta, const MsaLayout& lay, uint32_t l, int K,
                           HostBytes& eds, HostBytes& seds, hipStream_t st);

// all ranks call with `bytes` bytes each; `all` receives world * bytes bytes in rank order
class Exchange {
public:
    virtual ~Exchange() = default;
    virtual void all_gather(int rank, const void* mine, size_t bytes, void* all) = 0;
    virtual const char* name() const = 0;
    // variable sizes: a gather of the sizes, then one all_gather padded to the largest; piece r of `all` is
    // [r * cap, r * cap + sizes[r]) with cap = all.size() / world
    void all_gather_v(int rank, int world, const void* mine, size_t bytes, std::vector<uint8_t>& all, std::vector<u64>& sizes);
};

// of the last MultiMsa::vcf_transform (edsx_vcf_multi_info)
struct VcfMultiInfo {
    bool partitioned = false, fasta_windowed = false;
    u64 records_min = 0, records_max = 0, moved_line_bytes = 0, fasta_h2d_bytes_max = 0;
};

// of the last MultiMsa::leds_merge_multi (edsx_merge_multi_info)
struct MergeMultiInfo {
    bool partitioned = false;
    int ranges = 0;
    int fallback = 0;           // 0 partitioned; 1 one rank / l = 0; 2 text not plain; 3 no sentinel; 4 source sets; 5 merged / failed
    u64 range_bytes_min = 0, range_bytes_max = 0, eds_h2d_bytes_max = 0, seds_h2d_bytes_max = 0;
};

class MultiMsa {
public:
    MultiMsa(const std::vector<int>& devices, bool use_rccl);
    ~MultiMsa();
    // msa2eds: column slabs (context length > 0: stitched between standalone common runs); an odd file, or an l-EDS
    // without such runs near the slab ends: rank 0 transforms the whole image
    void transform(const uint8_t* fasta, size_t n, uint32_t context_len, HostBytes& eds, HostBytes& seds);
    int world() const { return (int)devices_.size(); }
    bool partitioned() const { return partitioned_; }
    int chains() const { return chains_; }
    const char* exchange_name() const { return xch_ ? xch_->name() : "none"; }
    // vcf2eds by position ranges (vcf_multi.hip): the outputs, counters and errors of VcfPipeline::run on the whole file
    // (counters: as far as known when it throws)
    void vcf_transform(const uint8_t* vcf, size_t vcf_n, const uint8_t* fasta, size_t fasta_n, HostBytes& eds, HostBytes& seds,
                       VcfCounters& stats);
    // EDS text -> l-EDS: the LINEAR merge with defaults (compact) on the first device (vcf_transforms.cpp:735-755)
    void leds_merge(HostBytes& eds, HostBytes& seds, uint32_t context_len);
    const VcfMultiInfo& last_vcf() const { return vcf_info_; }
    // EDS text -> l-EDS by symbol ranges (merge_multi.hip): the outputs and errors of MergePipeline::run on the whole text;
    // seds == nullptr: CARTESIAN
    void leds_merge_multi(const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, uint32_t context_len, bool compact,
                          HostBytes& leds, HostBytes& seds_out);
    const MergeMultiInfo& last_merge() const { return merge_info_; }
private:
    struct Rank;
    struct VcfShared;
    struct MergeShared;
    void run_rank(int r, const uint8_t* fasta, const MsaLayout& lay, uint32_t l, HostBytes& eds, HostBytes& seds);
    void run_rank_vcf(int r, VcfShared& sh);
    void run_rank_merge(int r, MergeShared& sh);
    // one_rank(r) on a thread per rank (multi_gpu.hip); throws what the failed rank threw (errors[rank]) or a DeviceError
    void run_ranks(const std::function<void(int)>& one_rank, const std::vector<std::exception_ptr>* errors);
    std::vector<int> devices_;
    std::vector<std::unique_ptr<Rank>> ranks_;
    std::unique_ptr<Exchange> xch_;
    std::unique_ptr<RankBarrier> bar_;
    bool partitioned_ = false;
    bool no_anchor_ = false;             // l > 0: some slab has no standalone common runs to anchor the stitch on
    int chains_ = 0;
    VcfMultiInfo vcf_info_;
    MergeMultiInfo merge_info_;
};

struct MultiMsa::Rank {
    int device = 0;
    MsaPipeline slab, mini;              // the slab's pipeline; boundary segments are recomputed through a second one
    DevBuf d_img, d_eds, d_seds, d_mini;
    std::vector<uint8_t> host_img;       // wrapped rows: the slab image is put together on the host; mini alignments
    SlabWorker worker() { return SlabWorker{&slab, &mini, &d_img, &d_eds, &d_seds, &d_mini, &host_img}; }
    std::string error;
    std::unique_ptr<VcfPipeline> vcf;    // vcf_transform: created on first use
    std::unique_ptr<MergePipeline> merge;   // (rank 0, context length > 0; every rank in leds_merge_multi)
    DeviceEds merge_eds;                    // the text that merge works on
    std::unique_ptr<RangeScanner> scan;     // leds_merge_multi: the device scans of this rank's slices
};

} // namespace edsx
