// query_device.hpp — host driver of the EDS query kernels (see query_device.hip): pattern sampling
// (EDS::generate_patterns) and position checks (EDS::check_position) over a DeviceEds and two scans of its own.
#pragma once

#include "eds_device.hpp"

#include <vector>

namespace edsx {

// What the last call learnt about its EDS, and where its time went (device events for the tables and the kernels).
struct QueryInfo {
    u64 n_symbols = 0, n_strings = 0, n_chars = 0, num_common_chars = 0, num_degenerate_strings = 0;
    double tokenise_ms = 0, tables_ms = 0, kernel_ms = 0, download_ms = 0;
};

// The source rule of EDS::check_position (calculate_path_intersection, eds.cpp:1300-1418) over the strings of T walk
// steps: the first step after which their path sets (W words per string, bit 0 = universal) have an empty intersection,
// Q_NONE when they keep a path.  sid_at(t, d) names the string of step t; d counts the choices it has consumed and starts
// at 0 for every word: the steps are re-walked once per 64-bit word, so no W-word accumulator is kept.  A universal set
// drops out: the intersection of a prefix is that of its other sets, or non-empty when it has none, and it is empty from
// step max over words of (first step whose running AND of that word is 0).  Shared by k_pat_check and the locate kernels.
constexpr u64 Q_NONE = ~0ull;
template <class SidAt>
__device__ __forceinline__ u64 first_empty_step(const u64* __restrict__ bits, u32 W, u64 T, SidAt sid_at)
{
    u64 E = Q_NONE;
    for (u32 w = 0; w < W; w++) {
        u64 acc = ~0ull, z = Q_NONE, d = 0;
        bool seen = false;
        for (u64 t = 0; t < T; t++) {
            const u64* b = bits + sid_at(t, d) * W;
            if (b[0] & 1) continue;                            // universal
            seen = true;
            acc &= b[w];
            if (acc == 0) { z = t; break; }
        }
        if (!seen || z == Q_NONE) return Q_NONE;               // this word keeps a path: never empty
        E = (w == 0 || z > E) ? z : E;
    }
    return E;
}

class QueryPipeline {
public:
    // count patterns of pattern_length characters, each followed by '\n' (count * (pattern_length + 1) bytes).
    // wpos (nullable): start common position per pattern, UINT64_MAX for a wrapped pattern or an EDS without common
    // characters; woff / wdeg (with wpos): the degenerate string numbers each pattern chose, as CSR (empty when wpos is).
    void genpatterns(DeviceEds& de, const uint8_t* eds, size_t eds_n, u64 count, u32 pattern_length, u64 seed,
                     HostBytes& out, std::vector<u64>* wpos, std::vector<u64>* woff, std::vector<int32_t>* wdeg, hipStream_t st);
    // status[q] of query q: 1 match, 0 no match, -1 out_of_range, -2 invalid_argument (EDS::check_position's answer).
    void check(DeviceEds& de, const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, size_t nq,
               const u64* pos, const u64* choice_off, const int32_t* choices, const u64* pattern_off, const uint8_t* patterns,
               int8_t* status, hipStream_t st);
    const QueryInfo& info() const { return info_; }

    // For a consumer that searches over the same tables (LocatePipeline): load eds (+ seds) into de and scan
    // cum_common / cum_deg (n + 1 entries each, see query_device.hip); returns n.  The consumer adds its times to info().
    u64 tables(DeviceEds& de, const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, hipStream_t st);
    const u64* cum_common() const { return cum_common_.as<u64>(); }
    const u64* cum_deg() const { return cum_deg_.as<u64>(); }
    QueryInfo& info() { return info_; }

    static constexpr u64 CHUNK_PATTERNS = 1ull << 20;        // patterns per sampling launch
    static constexpr u64 CHUNK_BYTES = 256ull << 20;         // ... and at most this much text per launch

private:
    u64 n_ = 0, C_ = 0, D_ = 0;
    QueryInfo info_;
    DevBuf cum_common_, cum_deg_, ctl_, scan_tmp_, out_, wpos_, wcnt_, woff_, wdeg_;
    DevBuf q_pos_, q_coff_, q_ch_, q_poff_, q_pat_, q_status_;
};

} // namespace edsx
