// vcf_export_device.hpp — host driver of the VCF export kernels (see vcf_export_device.hip): an EDS and its sources as
// VCF 4.2 text, one record per symbol with two strings or more and one genotype column per path, plus the reference FASTA
// the records refer to.  Semantics: include/edsx.h, "eds2vcf"; where the bytes lie: vcf_text.hpp.
#pragma once

#include "eds_device.hpp"
#include "kernel_times.hpp"
#include "vcf_text.hpp"

#include <string>
#include <vector>

namespace edsx {

// edsx_vcf_export_info (include/edsx.h) without its last member
struct VcfExportInfo {
    u64 symbols = 0, strings = 0, paths = 0, records = 0, anchored = 0, overlapping = 0, ref_length = 0, header_bytes = 0,
        body_bytes = 0;
};

struct VcfExportOpts {
    std::string chrom = "eds", prefix = "path";
    u64 ref_path = 0, line_width = 60, max_bytes = 0;
    const char* const* names = nullptr;
    size_t n_names = 0;
};

class VcfExportPipeline {
public:
    // Loads eds (+ seds) into de as edsx_eds_gfa does, reads it through de.view() and leaves the VCF in `vcf` and, when
    // fasta is not null, the reference FASTA there.  info is filled in as far as the counts were known when an error is
    // thrown (all of it for the max_bytes LimitError, which is raised before the body is allocated).
    void run(DeviceEds& de, const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, const VcfExportOpts& opts,
             HostBytes& vcf, HostBytes* fasta, VcfExportInfo& info, hipStream_t st);

    // device time per kernel, accumulated while on (edsx_set_timing / edsx_get_timing)
    void set_timing(bool on) { times_.set(on); }
    int get_timing(const char** names, float* ms, int* counts, int cap) const { return times_.get(names, ms, counts, cap); }

private:
    KernelTimes times_;
    DevBuf ctl_, scan_tmp_, orb_, chrom_;
    DevBuf refidx_, refpos_, rank_, anchor_, recsym_;            // per symbol (n + 1)
    DevBuf table_;                                               // per record: fixed part, tile 0, tile 1, ... (+ 1)
    DevBuf out_, fa_;
};

} // namespace edsx
