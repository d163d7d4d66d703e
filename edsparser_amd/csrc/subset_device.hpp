// subset_device.hpp — host driver of the path subsetting kernels (see subset_device.hip): an EDS with sources restricted
// to a chosen set of paths, again as .eds + .seds text.
#pragma once

#include "eds_device.hpp"
#include "kernel_times.hpp"

#include <vector>

namespace edsx {

// edsx_subset_info (include/edsx.h)
struct SubsetInfo {
    u64 symbols_in = 0, symbols_out = 0, strings_in = 0, strings_out = 0, chars_in = 0, chars_out = 0, paths_in = 0, paths_out = 0,
        symbols_removed = 0, common_runs_merged = 0;
};

class SubsetPipeline {
public:
    static constexpr u32 MAX_GROUP = 64;       // lanes that share one string's bitset in the filter and .seds kernels

    // Loads eds / seds into de as edsx_paths_open does (same statuses and texts; seds == nullptr: ParamError), reads it
    // through de.view() and leaves the two texts in eds_out / seds_out.  ids: the keep set (ParamError when it is empty,
    // holds an id outside 1..P or holds an id twice).
    void run(DeviceEds& de, const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, const u64* ids, size_t n,
             bool keep_ids, HostBytes& eds_out, HostBytes& seds_out, SubsetInfo& info, hipStream_t st);

    // device time per kernel, accumulated while on (edsx_set_timing / edsx_get_timing)
    void set_timing(bool on) { times_.set(on); }
    int get_timing(const char** names, float* ms, int* counts, int cap) const { return times_.get(names, ms, counts, cap); }

    // lanes per string for bitsets of W words: the power of two that covers W, at most a wave
    static u32 group_for(u32 W)
    {
        u32 g = 1;
        while (g < W && g < MAX_GROUP) g <<= 1;
        return g;
    }

private:
    KernelTimes times_;
    DevBuf ctl_, scan_tmp_, orbits_, mask_, below_, dig_;
    DevBuf kscan_, lscan_, bscan_, sflag_;                       // per string (m + 1)
    DevBuf sscan_, scls_, kj_;                                   // per symbol (n + 1)
    DevBuf sidx_, rcls_, hscan_, cscan_;                         // per surviving symbol (<= n, + 1)
    DevBuf headpos_, eoff_, soff_, aoff_;                        // per run (<= n, + 1)
    DevBuf dst_, sdst_;                                          // per string: where its text / its set goes
    DevBuf out_eds_, out_seds_;
};

} // namespace edsx
