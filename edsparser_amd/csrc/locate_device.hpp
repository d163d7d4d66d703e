// locate_device.hpp — host driver of the EDS pattern search (see locate_device.hip): every occurrence of every pattern,
// in EDS::check_position's coordinates, over the tables QueryPipeline builds.
#pragma once

#include "query_device.hpp"

#include <vector>

namespace edsx {

// edsx_locate_hit (include/edsx.h)
struct LocateHit { u64 common_pos, symbol, string, offset; };

struct LocateOut {
    std::vector<u64> hit_off;                // n + 1
    std::vector<LocateHit> hits;             // hit_off[n]
    std::vector<u64> choice_off;             // hit_off[n] + 1
    std::vector<int32_t> choices;
    std::vector<u64> totals;                 // n
    std::vector<uint8_t> flags;              // n: bit 0 hits left out, bit 1 a walk was cut at its 65th choice
};

class LocatePipeline {
public:
    static constexpr u32 MAX_CHOICES = 64;                   // EDSX_LOCATE_MAX_CHOICES
    static constexpr u64 MAX_HITS_CEILING = 1ull << 32;      // a larger max_hits acts as this one
    static constexpr u64 COUNT_ENTRIES = 32ull << 20;        // (pattern, tile) counters per launch: 256 MB

    // n patterns as CSR.  Counts and times of the call go to qp's QueryInfo (edsx_query_last_info).
    void run(QueryPipeline& qp, DeviceEds& de, const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n,
             size_t n, const u64* pattern_off, const uint8_t* patterns, u64 max_hits, bool common_only, LocateOut& out,
             hipStream_t st);

private:
    DevBuf str_sym_, pat_, poff_, seed_, pmask_, counts_, flags_, kept_, totals_, hoff_, hits_, hit_k_, coff_, choices_, ctl_,
           scan_tmp_;
};

} // namespace edsx
