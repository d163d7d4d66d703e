// query_device.hpp — host driver of the EDS query kernels (see query_device.hip): pattern sampling
// (EDS::generate_patterns) and position checks (EDS::check_position) over the tables MergePipeline::prepare builds.
#pragma once

#include "merge_device.hpp"

#include <vector>

namespace edsx {

// What the last call learnt about its EDS, and where its time went (device events for the tables and the kernels).
struct QueryInfo {
    u64 n_symbols = 0, n_strings = 0, n_chars = 0, num_common_chars = 0, num_degenerate_strings = 0;
    double tokenise_ms = 0, tables_ms = 0, kernel_ms = 0, download_ms = 0;
};

class QueryPipeline {
public:
    // count patterns of pattern_length characters, each followed by '\n' (count * (pattern_length + 1) bytes).
    // wpos (nullable): start common position per pattern, UINT64_MAX for a wrapped pattern or an EDS without common
    // characters; woff / wdeg (with wpos): the degenerate string numbers each pattern chose, as CSR (empty when wpos is).
    void genpatterns(MergePipeline& mp, const uint8_t* eds, size_t eds_n, u64 count, u32 pattern_length, u64 seed,
                     HostBytes& out, std::vector<u64>* wpos, std::vector<u64>* woff, std::vector<int32_t>* wdeg, hipStream_t st);
    // status[q] of query q: 1 match, 0 no match, -1 out_of_range, -2 invalid_argument (EDS::check_position's answer).
    void check(MergePipeline& mp, const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, size_t nq,
               const u64* pos, const u64* choice_off, const int32_t* choices, const u64* pattern_off, const uint8_t* patterns,
               int8_t* status, hipStream_t st);
    const QueryInfo& info() const { return info_; }

    static constexpr u64 CHUNK_PATTERNS = 1ull << 20;        // patterns per sampling launch
    static constexpr u64 CHUNK_BYTES = 256ull << 20;         // ... and at most this much text per launch

private:
    u64 tables(MergePipeline& mp, const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, hipStream_t st);
    u64 n_ = 0, m_ = 0, C_ = 0, D_ = 0;
    u32 W_ = 0;
    QueryInfo info_;
    DevBuf cum_common_, cum_deg_, ctl_, scan_tmp_, out_, wpos_, wcnt_, woff_, wdeg_;
    DevBuf q_pos_, q_coff_, q_ch_, q_poff_, q_pat_, q_status_;
};

} // namespace edsx
