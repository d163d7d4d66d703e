// path_device.hpp — host driver of the path spelling kernels (see path_device.hip): the sequence of every path of an
// EDS with sources, as FASTA.  The inverse of the transforms: path s + 1 of msa2eds(A) is row s of A without its gaps.
#pragma once

#include "eds_device.hpp"
#include "gfa_device.hpp"
#include "lift_core.hpp"
#include "slice_core.hpp"

#include <vector>

namespace edsx {

struct PathInfo {
    u64 n_symbols = 0, n_strings = 0, n_chars = 0, num_paths = 0, n_choice_symbols = 0;
    bool tokenised_on_device = false;
};

// of the last lengths() / spell() / walks() / align() / lift(): device events around the kernels, a host clock around the downloads
// (walks: scan_ms holds both scans of a batch, copy_ms is k_path_walk; align: copy_ms is k_path_align; lift: copy_ms is
// k_lift_find + k_lift_place, bytes_written the result bytes; slice: scan_ms is resolve + count + scan, copy_ms the fill
// kernels, bytes_written both texts)
struct PathTiming {
    double tokenise_ms = 0, choose_ms = 0, scan_ms = 0, copy_ms = 0, download_ms = 0;
    u64 bytes_written = 0;
};

// one requested path of an output batch: where its record and its body start in the batch's buffer, where its header
// text lies in the header blob, its length, the line width in force (>= 1), the body bytes (characters + newlines) and
// its row of the choice tables
struct PathRec { u64 rec_off, body_off, hdr_src, L, lw, body, row; };

// the column layout of the session's alignment view (align): W = n_columns
struct AlignInfo { u64 n_symbols = 0, n_columns = 0, n_zero_width_symbols = 0, widest_symbol = 0, num_paths = 0; };

typedef lift::Site LiftSite;
// sites given by the host as three columns of n entries each (the columns of a locate hit)
struct LiftColumns { const u64* symbol; const u64* string; const u64* offset; };

// edsx_slice_region (include/edsx.h)
struct SliceRegion { u64 symbol_first, symbol_last, cut_first, cut_end, column_first, column_end, strings, chars, eds_off, eds_len, seds_off, seds_len; };

// device time per kernel, accumulated while on (edsx_set_timing / edsx_get_timing), as SubsetPipeline keeps it
class KernelTimes {
public:
    void set(bool on) { on_ = on; acc_.clear(); }
    bool on() const { return on_; }
    void add(const char* name, float ms);
    int get(const char** names, float* ms, int* counts, int cap) const;
private:
    struct Acc { const char* name; float total_ms; int count; };
    bool on_ = false;
    std::vector<Acc> acc_;
};

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

    // GFA P lines of the paths in request order: "P\t<name>\t<id>+,<id>+,...\t*\n" over the segment ids (segment_ranks) of
    // the non-empty chosen strings.  steps[k] (nullable): the ids listed; a path with none gets no line.  names as in spell;
    // a name that is empty or holds a tab, line feed or blank is a ParamError.
    void walks(const u64* ids, size_t n, const char* const* names, const char* prefix, HostBytes& out, u64* missing, u64* steps,
               hipStream_t st);

    // The paths as rows of one alignment: symbol i owns w[i] columns, the length of its longest string, and
    // holds the chosen string of the path left-justified and filled up with `gap`; every row has W = sum w[i] characters,
    // whatever paths are asked for.  FASTA as spell() writes it.  max_bytes (0: none): ParamError, from the counts and
    // before any table or text is made, when the text is larger.
    const AlignInfo& align_info(hipStream_t st) { align_open(st); return ainfo_; }
    void align(const u64* ids, size_t n, const char* const* names, const char* prefix, u64 line_width, uint8_t gap, u64 max_bytes,
               HostBytes& out, u64* missing, hipStream_t st);

    // Positions between the paths of the EDS (lift_core.hpp), n queries, duplicates allowed, any order.
    //   src_path + src_pos: the site of character src_pos[q] of path src_path[q] (status 0, or RANGE with every field ~0)
    //   site_in instead:    given sites, as three columns that are uploaded as they are
    //   dst_path:           the place of each site on path dst_path[q]: dst_pos and SAME / ALIGNED / GAP / MISSING / RANGE
    // With src and dst the sites stay on the device in between.  site_out / dst_pos may be null; status has n bytes.
    void lift(size_t n, const u64* src_path, const u64* src_pos, const LiftColumns* site_in, const u64* dst_path, LiftSite* site_out,
              u64* dst_pos, uint8_t* status, hipStream_t st);

    // Regions of the EDS as FULL-form .eds + .seds texts laid end to end (slice_core.hpp, slice_device.hip), n
    // regions (path, start, end), half open; path 0: columns of the alignment view.  A region that is empty or leaves its
    // path gets status RANGE and no bytes; a path id above P is a ParamError, and so is a summed size above max_bytes (0:
    // none), found before the texts are allocated.  region (nullable) has n entries, status n bytes.
    void slice(size_t n, const u64* path, const u64* start, const u64* end, u64 max_bytes, HostBytes& eds_out, HostBytes& seds_out,
               SliceRegion* region, uint8_t* status, KernelTimes* times, hipStream_t st);

private:
    void check_ids(const u64* ids, size_t n) const;
    u64 table_batch(size_t n, u64 cell_bytes = 16) const;
    // seg_rank and the token bytes of the fixed symbols: made by the first walks() of a session, kept until it closes
    void walk_open(hipStream_t st);
    // tables(), then the token bytes of every (path, choice symbol) and their scan; tok / cnt: token bytes and ids per path
    void walk_tables(const u64* ids, u64 K, std::vector<u64>& tok, std::vector<u64>& miss, std::vector<u64>& cnt, hipStream_t st);
    // col (the exclusive scan of the symbol widths, n + 1 entries): made by the first align() or align_info() of a
    // session, kept until it closes
    void align_open(hipStream_t st);
    static u64 budget_override();
    // choose + scan for ids[0..K): device tables for the copy kernel, host lengths and missing counts
    void tables(const u64* ids, u64 K, std::vector<u64>& len, std::vector<u64>& miss, hipStream_t st);

    DeviceEds eds_;
    PathInfo info_;
    PathTiming timing_;
    u64 n_ = 0, nc_ = 0, F_ = 0;
    DevBuf cum_fixed_, rank_, cidx_, ctl_, scan_tmp_, ids_, csid_, clen_, tot_, miss_, rec_, hdr_, hoff_, out_;
    bool walk_ready_ = false;
    u64 Ftok_ = 0, Fcnt_ = 0;                                    // token bytes / ids of the fixed symbols
    DevBuf seg_rank_, cum_tok_, tlen_, cnt_;
    bool align_ready_ = false;
    AlignInfo ainfo_;
    DevBuf col_;
    // cum_common (n + 1 entries) next to col: made by the first lift() of a session, kept until it closes
    void lift_open(hipStream_t st);
    void lift_group(u64 m, u64 D, std::vector<u64>& start, hipStream_t st);
    void lift_run(size_t n, const u64* src_path, const u64* src_pos, const LiftColumns* site_in, const u64* dst_path, LiftSite* site_out,
                  u64* dst_pos, uint8_t* status, LiftSite* dev_site, uint8_t* dev_status, hipStream_t st);
    bool lift_ready_ = false;
    DevBuf cum_common_, lmap_, lcnt_, lcur_, lq_path_, lq_pos_, lq_aux_, lperm_, lsite_, lst_, lst2_, litems_;
    // the scanned .seds bytes per string (m + 1 entries) and the symbol of every string (m): made by the first slice() of a
    // session, kept until it closes
    void slice_open(hipStream_t st);
    bool slice_ready_ = false;
    DevBuf sb_, symof_, s_in_, s_site_, s_sst_, s_reg_, s_st_, s_sum_, s_scan_, s_edst_, s_eds_, s_seds_;
};

} // namespace edsx
