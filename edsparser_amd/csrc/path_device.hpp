// path_device.hpp — host driver of the path spelling kernels (see path_device.hip): the sequence of every path of an
// EDS with sources, as FASTA.  The inverse of the transforms: path s + 1 of msa2eds(A) is row s of A without its gaps.
// The session's coordinate lift, region slice, path distances and linkage disequilibrium: lift_device.hip,
// slice_device.hip, dist_device.hip, ld_device.hip; the segments two paths share: ibs_device.hip; a path as a mosaic of
// other paths: mosaic_device.hip; windowed diversity between groups of paths: div_device.hip (where an operation
// goes).
#pragma once

#include "dist_core.hpp"
#include "div_core.hpp"
#include "eds_device.hpp"
#include "ibs_core.hpp"
#include "kernel_times.hpp"
#include "ld_core.hpp"
#include "lift_core.hpp"
#include "mosaic_core.hpp"
#include "path_records.hpp"

#include <functional>
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

// the column layout of the session's alignment view (align): W = n_columns
struct AlignInfo { u64 n_symbols = 0, n_columns = 0, n_zero_width_symbols = 0, widest_symbol = 0, num_paths = 0; };

typedef lift::Site LiftSite;
// sites given by the host as three columns of n entries each (the columns of a locate hit)
struct LiftColumns { const u64* symbol; const u64* string; const u64* offset; };

// edsx_slice_region (include/edsx.h)
struct SliceRegion { u64 symbol_first, symbol_last, cut_first, cut_end, column_first, column_end, strings, chars, eds_off, eds_len, seds_off, seds_len; };

// edsx_dist_info (include/edsx.h)
struct DistInfo { u64 units = 0, variable_units = 0, class_columns = 0, chunk_columns = 0, chunks = 0; };

// edsx_ld_opts, edsx_ld_info, edsx_ld_pair, edsx_ld_allele (include/edsx.h)
struct LdOpts { u64 window; double min_r2; u64 min_count; int all_strings; u64 max_pairs; };
struct LdInfo { u64 paths = 0, choice_symbols = 0, alleles = 0, candidate_pairs = 0, undefined_pairs = 0, pairs = 0, row_words = 0, tiles = 0; };
struct LdPair { u64 symbol_a, string_a, symbol_b, string_b, n_ab, n_a, n_b, n; double r2; };
struct LdAllele { u64 symbol, string, count, present; };

// edsx_ibs_info, edsx_ibs_segment (include/edsx.h)
struct IbsInfo { u64 paths = 0, choice_symbols = 0, class_columns = 0, chunk_columns = 0, chunks = 0, pairs = 0, candidate_segments = 0, segments = 0; };
typedef ibs::Segment IbsSegment;

// edsx_mosaic_info, edsx_mosaic_segment (include/edsx.h)
struct MosaicInfo { u64 targets = 0, donors = 0, choice_symbols = 0, class_columns = 0, segments = 0, private_segments = 0, private_symbols = 0, switches = 0; };
typedef mosaic::Segment MosaicSegment;

// edsx_div_opts, edsx_div_info, edsx_div_window, edsx_div_group, edsx_div_pair (include/edsx.h)
struct DivOpts { int unit; u64 size, step, max_windows; };
struct DivInfo { u64 groups = 0, paths = 0, choice_symbols = 0, windows = 0, pairs = 0, row_words = 0, extent = 0; };
struct DivWindow { u64 start, end, rank_first, rank_end; };
struct DivGroup { u64 segregating, present; };
struct DivPair { u64 diff, comp; };

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
    const AlignInfo& align_info(hipStream_t st) { align_open(st); return align_.info; }
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

    // Pairwise distances between n paths in request order, duplicates allowed (dist_core.hpp, dist_device.hip):
    // matrix has n x n entries, row-major; missing (nullable) n.  metric: dist::COLUMNS - the columns of the alignment of
    // align() at which two rows differ - or dist::STRINGS - the symbols at which two paths take different strings; anything
    // else is a ParamError, and so is a matrix above max_bytes (0: none), found before anything is allocated.  The bit
    // rows and the matrix have to fit budget(2): LimitError.
    void distances(const u64* ids, size_t n, int metric, u64 max_bytes, u64* matrix, u64* missing, DistInfo& info, KernelTimes* times,
                   hipStream_t st);

    // Linkage disequilibrium between the alleles of the EDS over the paths ids[0..n) (n == 0: all paths; duplicates count
    // once) (ld_core.hpp, ld_device.hip): the reported pairs as LdPair in (x, y) order, the listed alleles as
    // LdAllele (nullable).  window == 0 or min_r2 outside [0, 1]: ParamError, and so are more pairs than max_pairs (0:
    // none), found from the counts before the pairs are allocated.  The allele and presence rows have to fit budget(2):
    // LimitError.  info is filled in as far as the call got.
    void ld(const u64* ids, size_t n, const LdOpts& opts, HostBytes& pairs, HostBytes* alleles, LdInfo& info, KernelTimes* times,
            hipStream_t st);

    // The segments every two of the paths ids[0..n) share (n == 0: all paths; duplicates allowed), pairs are request
    // positions x < y (ibs_core.hpp, ibs_device.hip): the maximal intervals of symbols at all of which the two
    // paths take the same string, those with sites >= min_sites and columns >= min_columns, as IbsSegment in (x, y,
    // symbol_first) order; pair_off: K (K - 1) / 2 + 1 u64, the CSR over the pairs.  More segments than max_segments
    // (0: none): ParamError, from the counts and before the records are allocated.  The bit rows, the per-(pair, chunk)
    // scratch and the records have to fit budget(2): LimitError.  info is filled in as far as the call got.
    void ibs(const u64* ids, size_t n, u64 min_sites, u64 min_columns, u64 max_segments, HostBytes& segments, HostBytes& pair_off,
             IbsInfo& info, KernelTimes* times, hipStream_t st);

    // Every target path as a minimal mosaic of the donor paths (mosaic_core.hpp, mosaic_device.hip): targets
    // [0..nt) and donors[0..nd) in request order, duplicates allowed, a count of 0: all paths; a donor position is eligible
    // for a target unless it names the target's own path.  The fewest segments that tile [0, n - 1], each a copy from one
    // donor (the furthest-reaching one, then the smallest request position) or private (donor NONE), as MosaicSegment in
    // (target, symbol_first) order; target_off: nt + 1 u64, the CSR over the targets.  More segments than max_segments
    // (0: none): ParamError, from the counts and before the records are allocated.  The bit rows of the distinct paths, the
    // donor scratch and the records have to fit budget(2): LimitError.  info is filled in as far as the call got.
    void mosaic(const u64* targets, size_t nt, const u64* donors, size_t nd, u64 max_segments, HostBytes& segments,
                HostBytes& target_off, MosaicInfo& info, KernelTimes* times, hipStream_t st);

    // Windowed diversity within and between groups of paths (div_core.hpp, div_device.hip).  The groups as a CSR
    // over path ids (group_off: n_groups + 1 entries); n_groups == 0: one group of all paths; a duplicate inside a group counts
    // once.  More than diversity::MAX_GROUPS groups, an id outside 1..P, an empty group, an id in two groups, a unit that is
    // neither SYMBOLS nor COLUMNS, or more windows than opts.max_windows (0: none; from the counts, before anything is
    // allocated): ParamError.  windows: NW DivWindow; groups: NW x G DivGroup; pairs: NW x G (G + 1) / 2 DivPair, (g, h) with
    // g <= h row-major; sfs (nullable): sum (K_g + 1) u64, the unfolded spectrum of every group over all choice symbols.  The
    // per-symbol sums and the records have to fit budget(2), and nc max K_g^2 has to stay below 2^63: LimitError.  info is
    // filled in as far as the call got.
    void diversity(const u64* group_off, const u64* group_ids, size_t n_groups, const DivOpts& opts, HostBytes& windows, HostBytes& groups,
                   HostBytes& pairs, HostBytes* sfs, DivInfo& info, KernelTimes* times, hipStream_t st);

private:
    // what a feature keeps with the session from its first call until the session closes (`ready`), and its buffers
    // walks: seg_rank (segment_ranks, m + 1); the token bytes of the fixed symbols, scanned (cum_tok, n + 1), their sum and
    // the number of such symbols; per table batch the token bytes of the choice cells, scanned (tlen), and the steps per row
    struct WalkState { bool ready = false; u64 Ftok = 0, Fcnt = 0; DevBuf seg_rank, cum_tok, tlen, cnt; };
    // align: col, the exclusive scan of the symbol widths (n + 1 entries)
    struct AlignState { bool ready = false; AlignInfo info; DevBuf col; };
    // lift: cum_common next to col (n + 1); the row of every path of the call (map), the queries of a chunk (q_*), grouped
    // by row (cnt, cur, perm, items), their sites and the statuses of both steps
    struct LiftState { bool ready = false; DevBuf cum_common, map, cnt, cur, q_path, q_pos, q_aux, perm, site, st, st2, items; };
    // slice: the scanned .seds bytes per string (sb, m + 1) and the symbol of every string (symof, m); per call the regions
    // as given (in), the sites of their ends, the regions resolved (reg, st), A per region (sum), the five scanned counts
    // (scan), the destinations of the edge strings (edst) and both texts
    struct SliceState { bool ready = false; DevBuf sb, symof, in, site, sst, reg, st, sum, scan, edst, eds, seds; };

    // distances: per choice symbol whether it may leave a path without a string (may_miss, nc bytes) and its first column
    // among the columns of the choice symbols (ccol, nc + 1; CW of them); per metric, from its first call, the class list
    // (desc: one descriptor per class column, C of them, over V listed units); per call the classes per unit while they
    // are counted (cnt), the bit rows of all requested paths (rows) and the K x K sums that become the matrix (sums)
    struct DistClasses { bool ready = false; u64 V = 0, C = 0; DevBuf desc; };
    struct DistState { bool ready = false; u64 CW = 0; DevBuf may_miss, ccol, cnt, rows, sums; DistClasses cls[2]; };

    // ld: the strings of the choice symbols in front of every choice symbol (soff, nc + 1; S of them), session state; per
    // call the row of the requested paths (mask), per string its carriers (cnt, S), per choice symbol the paths present
    // (pres), its listed alleles and whether it needs a presence row, both scanned (afirst, uidx: nc + 1), the allele rows
    // (trows, A x WP) and presence rows (urows), the alleles as they are returned (al) and their choice symbols (ar), the
    // column tiles per row tile, scanned (tstart), the reported pairs per (allele, column tile), scanned (cntx), the pairs
    struct LdState { bool ready = false; u64 S = 0; DevBuf soff, mask, cnt, pres, afirst, uidx, trows, urows, al, ar, tstart, cntx, pairs; };

    // ibs: ready - the first ibs() of the session has made the columns (align_.col) its records name; the bit rows are
    // dist_.rows under the STRINGS class list.  Per call and (pair, chunk) the reported interior segments (icnt) and the
    // first and last differing rank (first, last); per (pair, chunk + 1) the segments of the slot, scanned (tot); pair_off
    // and the records
    struct IbsState { bool ready = false; DevBuf icnt, first, last, tot, pair_off, seg; };

    // mosaic: ready - as ibs, the columns its records name; the bit rows are dist_.rows.  Per call the row of every target
    // and donor (rowof), the donor rows word-major in request order (rt), the alive bits per (target, lane) (alive), the
    // segments per target, scanned: target_off (cnt), and the records
    struct MosaicState { bool ready = false; DevBuf rowof, rt, alive, cnt, seg; };

    // diversity: per call the rows of the groups (masks, G x WP), per choice symbol the NA sums, array-major and scanned
    // (arr), the walk rows of the lane groups when a row does not fit the registers (seen), the spectrum and the records
    struct DivState { DevBuf masks, arr, seen, sfs, win, grp, pr; };

    // ---- session and choice tables
    void check_ids(const u64* ids, size_t n) const;
    void begin_call();                                            // a fresh PathTiming that keeps tokenise_ms
    u64 table_batch(size_t n, u64 cell_bytes = 16) const;
    static u64 budget(u64 part);                                  // bytes a batch may take: 1 / part of the free HBM
    // choose + scan for ids[0..K): device tables for the copy kernel, host lengths and missing counts
    void tables(const u64* ids, u64 K, std::vector<u64>& len, std::vector<u64>& miss, hipStream_t st);
    // The records of spell / align / walks (path_records.hpp) into `out`, batch by batch within the budgets.
    //   make_tables(i0, K, len, miss)             the tables of ids [i0, i0 + K) and the lengths that size their records
    //   launch_body(rec, nrec, max_tiles, dst)    the body kernel over the nrec records of an output batch
    template <class Tables, class Body>
    void emit_records(records::Rule rule, size_t n, const records::Headers& hdr, u64 line_width, u64 cell_bytes, HostBytes& out,
                      u64* missing, Tables&& make_tables, Body&& launch_body, hipStream_t st);
    // ---- walks: made by the first walks() of a session
    void walk_open(hipStream_t st);
    // tables(), then the token bytes of every (path, choice symbol) and their scan; tok / cnt: token bytes and ids per path
    void walk_tables(const u64* ids, u64 K, std::vector<u64>& tok, std::vector<u64>& miss, std::vector<u64>& cnt, hipStream_t st);
    // ---- align: made by the first align() or align_info() of a session
    void align_open(hipStream_t st);
    // ---- lift (lift_device.hip): made by the first lift() of a session
    void lift_open(hipStream_t st);
    void lift_group(u64 m, u64 D, std::vector<u64>& start, hipStream_t st);
    void lift_run(size_t n, const u64* src_path, const u64* src_pos, const LiftColumns* site_in, const u64* dst_path, LiftSite* site_out,
                  u64* dst_pos, uint8_t* status, LiftSite* dev_site, uint8_t* dev_status, hipStream_t st);
    // ---- slice (slice_device.hip): made by the first slice() of a session
    void slice_open(hipStream_t st);
    // ---- distances (dist_device.hip): the symbol tables by the first distances() of a session, a class list by the first
    // of its metric
    void dist_open(hipStream_t st);
    void dist_classes(dist::Metric metric, TimedRuns& timed, hipStream_t st);
    // both, then the bit rows of ids[0..n) in dist_.rows; fits: the caller's budget check, run once the class list is known
    dist::Plan dist_rows(const u64* ids, size_t n, dist::Metric m, u64* missing, TimedRuns& timed,
                         const std::function<void(const DistClasses&, const dist::Plan&)>& fits, hipStream_t st);
    // ---- linkage disequilibrium (ld_device.hip): made by the first ld() of a session
    void ld_open(hipStream_t st);

    DeviceEds eds_;
    PathInfo info_;
    PathTiming timing_;
    u64 n_ = 0, nc_ = 0, F_ = 0;
    DevBuf cum_fixed_, rank_, cidx_, ctl_, scan_tmp_, ids_, csid_, clen_, tot_, miss_, rec_, hdr_, out_;
    WalkState walk_;
    AlignState align_;
    LiftState lift_;
    SliceState slice_;
    DistState dist_;
    LdState ld_;
    IbsState ibs_;
    MosaicState mosaic_;
    DivState div_;
};

} // namespace edsx
