// eds_device.hpp — an .eds (+ .seds) text tokenised into HBM (see eds_device.hip): the one form that the l-EDS merge,
// the statistics, pattern sampling and position checks, the pattern search and path spelling all read.
#pragma once

#include "msa_device.hpp"

#include <chrono>

namespace edsx {

// per symbol of the current round: number of strings, first string / pool entry, length of the only string when size == 1
struct SymArrays { u64* size; u64* ent_off; u64* len1; };
struct SymView { const u64* size; const u64* ent_off; const u64* len1; };

// What a reader gets, and all it gets.  chars ends in 16 bytes of slack; str_off has m + 1 entries; elen is the length
// of every string; bits (W words per string, bit 0 = the universal path "0") is null when the text was loaded without
// sources, and W is 0 then.
struct EdsView {
    SymView sym;
    const u64* str_off; const uint8_t* chars; const u32* elen; const u64* bits;
    u64 n, m, n_chars; u32 W;
};

// EDS::calculate_statistics / calculate_source_statistics (eds.cpp:361-470, :472-505) and is_leds
// (eds_transforms.cpp:439-468) of an .eds (+ .seds) text, as reductions over the tokenised arrays in HBM.
struct EdsStats {
    u64 n_symbols, n_chars, n_strings;                 // n, N, m
    u64 num_degenerate, total_change_size, num_common_chars, num_context_blocks, min_context, max_context, num_empty_strings;
    u64 has_sources, num_paths, max_paths_per_string, total_paths;
    u64 is_leds;                                       // for the given context length
};

// EDSX_TRACE=1: wall-clock of the host-visible stages on stderr (every mark follows a stream synchronisation)
class StageTrace {
public:
    void restart() { last_ = std::chrono::steady_clock::now(); }
    void mark(const char* what);
private:
    std::chrono::steady_clock::time_point last_ = std::chrono::steady_clock::now();
};

class DeviceEds {
public:
    // Tokenise eds / seds (host buffers; linear: with sources) on the device when the text is plain, else on the host
    // (same error texts as the reference), and leave the arrays of EdsView in HBM.  merge_headroom: elen / bits get room
    // for the entries the merge appends (max(2m + 1024, 4096)) instead of m.
    void load(const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, bool linear, hipStream_t st,
              bool merge_headroom = false);

    // of the last load
    u64 n() const { return n_; }
    u64 m() const { return m_; }
    u32 W() const { return W_; }                         // 0 without sources
    u64 n_chars() const { return n_chars_; }
    u64 head_len() const { return head_len_; }           // length of the first string
    bool head_single() const { return head_single_; }    // the first / last symbol has one string
    bool tail_single() const { return tail_single_; }
    bool with_sources() const { return with_sources_; }
    bool tokenised_on_device() const { return tokenised_on_device_; }

    EdsView view() const;                                // DeviceError once consumed
    void drop_scratch();                                 // what only tokenising needs goes back to the allocator

    // The merge is the one consumer that writes: it appends product entries behind the m strings in elen / bits (growing
    // them) and uses the symbol arrays as one half of its double buffer.  The object is consumed until the next load.
    struct Pool { DevBuf& elen; DevBuf& bits; SymArrays sym; const u64* str_off; const uint8_t* chars; };
    Pool consume();

private:
    bool load_device(const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, bool linear, bool merge_headroom, hipStream_t st);
    void load_host(const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, bool linear, bool merge_headroom, hipStream_t st);
    void ensure_strings(bool merge_headroom, bool linear);
    SymArrays sym() const { return SymArrays{size_.as<u64>(), ent_off_.as<u64>(), len1_.as<u64>()}; }

    u64 n_ = 0, m_ = 0, n_chars_ = 0, head_len_ = 0;
    u32 W_ = 0;
    bool head_single_ = false, tail_single_ = false, with_sources_ = false, tokenised_on_device_ = false, consumed_ = false;
    DevBuf raw_, tk_a_, tk_b_, tk_c_, sym_first_, scan_tmp_;          // scratch of the tokenisers
    DevBuf ctl_, chars_, str_off_, size_, ent_off_, len1_, elen_, bits_;
};

// Statistics and l-EDS validity (context length l; 0: not asked) of a loaded DeviceEds; acc: scratch of the caller's.
void eds_stats(const DeviceEds& de, uint32_t l, DevBuf& acc, EdsStats& out, hipStream_t st);

} // namespace edsx
