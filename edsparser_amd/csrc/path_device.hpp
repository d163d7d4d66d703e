// path_device.hpp — host driver of the path spelling kernels (see path_device.hip): the sequence of every path of an
// EDS with sources, as FASTA.  The inverse of the transforms: path s + 1 of msa2eds(A) is row s of A without its gaps.
#pragma once

#include "eds_device.hpp"

#include <vector>

namespace edsx {

struct PathInfo {
    u64 n_symbols = 0, n_strings = 0, n_chars = 0, num_paths = 0, n_choice_symbols = 0;
    bool tokenised_on_device = false;
};

// of the last lengths() / spell(): device events around the kernels, a host clock around the downloads
struct PathTiming {
    double tokenise_ms = 0, choose_ms = 0, scan_ms = 0, copy_ms = 0, download_ms = 0;
    u64 bytes_written = 0;
};

// one requested path of an output batch: where its record and its body start in the batch's buffer, where its header
// text lies in the header blob, its length, the line width in force (>= 1), the body bytes (characters + newlines) and
// its row of the choice tables
struct PathRec { u64 rec_off, body_off, hdr_src, L, lw, body, row; };

// One EDS + sEDS kept tokenised in HBM in a DeviceEds of its own (other calls on the context do not touch it).
class PathPipeline {
public:
    // Tokenises as edsx_leds_merge does in LINEAR mode (same statuses and texts); seds == nullptr: ParamError.
    void open(const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, hipStream_t st);
    const PathInfo& info() const { return info_; }
    const PathTiming& timing() const { return timing_; }

    // length[k] / missing[k] of path ids[k] (1 <= id <= P, else ParamError); duplicates allowed
    void lengths(const u64* ids, size_t n, u64* length, u64* missing, hipStream_t st);
    // FASTA of the paths in request order: '>' name '\n', then the sequence in lines of line_width characters (0: one
    // line; an empty sequence has no line).  names (nullable): n C strings; else prefix (nullable: "path") + id.
    void spell(const u64* ids, size_t n, const char* const* names, const char* prefix, u64 line_width, HostBytes& out,
               u64* missing, hipStream_t st);

private:
    void check_ids(const u64* ids, size_t n) const;
    u64 table_batch(size_t n) const;
    static u64 budget_override();
    // choose + scan for ids[0..K): device tables for the copy kernel, host lengths and missing counts
    void tables(const u64* ids, u64 K, std::vector<u64>& len, std::vector<u64>& miss, hipStream_t st);

    DeviceEds eds_;
    PathInfo info_;
    PathTiming timing_;
    u64 n_ = 0, nc_ = 0, F_ = 0;
    DevBuf cum_fixed_, rank_, cidx_, ctl_, scan_tmp_, ids_, csid_, clen_, tot_, miss_, rec_, hdr_, hoff_, out_;
};

} // namespace edsx
