// gfa_device.hpp — host driver of the GFA graph kernels (see gfa_device.hip): an EDS as GFA 1.0 text, header, S lines and
// L lines.  The P lines come from a path session (path_device.hip), which shares segment_ranks and gfa_text.hpp.
#pragma once

#include "eds_device.hpp"
#include "kernel_times.hpp"
#include "gfa_text.hpp"

#include <vector>

namespace edsx {

// edsx_gfa_info (include/edsx.h) without its last member
struct GfaInfo {
    u64 n_symbols = 0, n_strings = 0, n_segments = 0, n_empty_strings = 0, n_open_symbols = 0, n_links = 0, header_bytes = 0,
        segment_bytes = 0, link_bytes = 0;
};

constexpr u64 GFA_MAX_STRINGS = 1ull << 32;    // segment ids are handled as 32-bit numbers of at most ten digits

// seg_rank[j] (0 <= j <= m): the non-empty strings before j, so that string j, when it is not empty, is segment
// seg_rank[j] + 1 and seg_rank[m] is the number of segments.  d_m1: m + 1 in device memory; d_total: receives seg_rank[m];
// tmp: m / SCAN_TILE + 4 u64.  LimitError for GFA_MAX_STRINGS strings and more.
void segment_ranks(const EdsView& v, u64* seg_rank, const u64* d_m1, u64* d_total, u64* tmp, hipStream_t st);

class GfaPipeline {
public:
    // Loads eds (+ seds when given: it is parsed and must match, but the graph does not depend on it) into de as
    // edsx_leds_merge does, reads it through de.view() and leaves the text in `out`.  max_links: 0 = 2^32; more links is a
    // ParamError raised from the counts, before the text is allocated.
    void run(DeviceEds& de, const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, u64 max_links, HostBytes& out,
             GfaInfo& info, hipStream_t st);

    // device time per kernel, accumulated while on (edsx_set_timing / edsx_get_timing)
    void set_timing(bool on) { times_.set(on); }
    int get_timing(const char** names, float* ms, int* counts, int cap) const { return times_.get(names, ms, counts, cap); }

private:
    KernelTimes times_;
    DevBuf ctl_, scan_tmp_;
    DevBuf seg_rank_;                                            // per string (m + 1)
    DevBuf cscan_, closed_, vend_, lcount_, loff_;               // per symbol (n + 1)
    DevBuf out_;
};

} // namespace edsx
