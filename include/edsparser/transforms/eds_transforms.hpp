// edsparser/transforms/eds_transforms.hpp — EDS -> l-EDS (LINEAR with sources / CARTESIAN).
// API of the reference's src/cpp/lib/transforms/eds_transforms.hpp (:29-37, :45-51, :57),
// implemented over edsx_leds_merge (include/edsx.h).
#ifndef EDSPARSER_TRANSFORMS_EDS_TRANSFORMS_HPP
#define EDSPARSER_TRANSFORMS_EDS_TRANSFORMS_HPP

#include "../common.hpp"
#include "../formats/eds.hpp"
#include <iostream>
#include <string>
#include <vector>

namespace edsparser {

// num_threads is accepted for compatibility; the merge runs on the GPU and its result does not
// depend on it (as in the reference).  context_length == 0 throws std::invalid_argument.
void eds_to_leds_linear(std::istream& input, std::ostream& output, Length context_length,
                        std::istream* phasing_input = nullptr, std::ostream* phasing_output = nullptr,
                        size_t num_threads = 1, bool compact = true);

void eds_to_leds_cartesian(std::istream& input, std::ostream& output, Length context_length,
                           size_t num_threads = 1, bool compact = true);

// true iff no internal common block is shorter than context_length and no two degenerate
// symbols are adjacent (host-side check on the container's metadata).
bool is_leds(const EDS& eds, Length context_length);

// eds2fasta: the sequence of the given paths (empty: all paths 1..P, P the largest id in the sources) of an EDS with
// sources as FASTA, one record per requested path in request order, lines of line_width characters (0: one line).
// Record k is named (*names)[k] when names is given, else "path<id>".  A path takes, per symbol, the first string whose
// source set holds it or 0 (EDS::path_sequence); the spelling runs on the GPU (edsx_eds_spell_paths).  Returns the
// number of symbols without a string per record when missing is given.  std::invalid_argument for a path outside 1..P.
void eds_to_fasta(std::istream& eds, std::istream& seds, std::ostream& out, const std::vector<int>& paths = {},
                  size_t line_width = 60, const std::vector<std::string>* names = nullptr,
                  std::vector<size_t>* missing = nullptr);

// eds2msa: the given paths (empty: all paths 1..P) as rows of one alignment, FASTA in request order.  Symbol i owns as
// many columns as its longest string has characters; a row holds the string the path takes there (as eds_to_fasta
// chooses it) left-justified and `gap` in the other columns, so every row has info->n_columns characters whatever paths
// are asked for, and rows of separate calls stack into one alignment (edsx_paths_align states the rules in full).
// line_width 0: one line per row.  max_bytes 0: no limit.  std::invalid_argument for a path outside 1..P, a gap that is
// '>', a line feed, a carriage return, a blank, a brace or a comma, and a text above max_bytes.
struct AlignInfo {
    size_t n_symbols = 0, n_columns = 0, n_zero_width_symbols = 0, widest_symbol = 0, num_paths = 0;
    std::vector<size_t> missing;               // per requested path
};
void eds_to_msa(std::istream& eds, std::istream& seds, std::ostream& out, const std::vector<int>& paths = {},
                size_t line_width = 0, const std::vector<std::string>* names = nullptr, const std::string& prefix = "path",
                char gap = '-', size_t max_bytes = 0, AlignInfo* info = nullptr);

// edsparser-lift: positions between the paths of an EDS with sources.  Query q asks where character src_pos of path
// src_path lies on path dst_path: its site in the EDS (symbol, string = index within the symbol, offset; the alignment
// column of eds_to_msa; common_pos, the pattern search's coordinate, or ~0 inside a degenerate symbol) and dst_pos with
// the status SAME (the very character), ALIGNED (another one in the same column), GAP (dst_pos is the next character to
// the right, possibly the length of the path) or MISSING (the path has no string in the symbol).  A src_pos at or above
// the length of the path gives RANGE and ~0 in every field; it does not fail the call (edsx_paths_lift states the rules
// in full).  Any order, duplicates allowed.  std::invalid_argument for a path outside 1..P.
enum class LiftStatus : unsigned char { SAME = 0, ALIGNED = 1, GAP = 2, MISSING = 3, RANGE = 4 };
struct LiftQuery { size_t src_path = 0, src_pos = 0, dst_path = 0; };
struct LiftResult {
    size_t dst_pos = 0, symbol = 0, string = 0, offset = 0, column = 0, common_pos = 0;
    LiftStatus status = LiftStatus::RANGE;
};
std::vector<LiftResult> lift_positions(std::istream& eds, std::istream& seds, const std::vector<LiftQuery>& queries);

// edsparser-dist: the pairwise distances of the given paths (empty: all paths 1..P; duplicates allowed), K x K row-major in
// request order, symmetric with a zero diagonal.  COLUMNS: the columns of the alignment of eds_to_msa at which two rows
// differ, where "no character" is a value of its own (there is no gap parameter); STRINGS: the symbols at which two paths
// take different strings, compared as string indices (edsx_paths_distances states the rules in full).  `units` is the
// denominator of a normalised distance: the columns of the alignment, or the number of symbols.
// std::invalid_argument for a path outside 1..P.
enum class DistanceMetric : int { COLUMNS = 0, STRINGS = 1 };
struct PathDistances {
    size_t K = 0, units = 0, variable_units = 0, class_columns = 0;
    std::vector<uint64_t> matrix;              // K * K
    std::vector<size_t> missing;               // per requested path
    uint64_t at(size_t a, size_t b) const { return matrix[a * K + b]; }
};
PathDistances path_distances(std::istream& eds, std::istream& seds, const std::vector<int>& paths = {},
                             DistanceMetric metric = DistanceMetric::COLUMNS);

// edsparser-ld: r² between the alleles of the EDS over the given paths (empty: all paths 1..P; duplicates count once), for
// every two listed alleles whose choice symbols lie at most `window` choice symbols apart, the pairs with r2 >= min_r2 in
// (symbol_a, string_a, symbol_b, string_b) order, and the listed alleles with their counts (edsx_paths_ld states the rules
// in full).  std::invalid_argument for a path outside 1..P, window == 0 or min_r2 outside [0, 1].
struct LdOptions {
    uint64_t window = 100;
    double min_r2 = 0.2;
    uint64_t min_count = 1;
    bool all_strings = false;
    uint64_t max_pairs = 0;                    // 0: no limit
};
struct LdPair { uint64_t symbol_a, string_a, symbol_b, string_b, n_ab, n_a, n_b, n; double r2; };
struct LdAllele { uint64_t symbol, string, count, present; };
struct PathLd {
    std::vector<LdPair> pairs;
    std::vector<LdAllele> alleles;
    size_t paths = 0, choice_symbols = 0, candidate_pairs = 0, undefined_pairs = 0;
};
PathLd path_ld(std::istream& eds, std::istream& seds, const std::vector<int>& paths = {}, const LdOptions& options = LdOptions());

// edsparser-ibs: the segments every two of the given paths share (empty: all paths 1..P; duplicates allowed; pairs are
// request positions x < y): the maximal intervals of symbols at all of which the two paths take the same string, those
// with at least min_sites choice symbols and min_columns alignment columns, in (x, y, symbol_first) order (edsx_paths_ibs
// states the rules in full).  pair_off: K (K - 1) / 2 + 1 offsets into segments, pairs in row-major upper-triangle order.
// std::invalid_argument for a path outside 1..P and for more segments than max_segments.
struct IbsOptions {
    uint64_t min_sites = 1;
    uint64_t min_columns = 0;
    uint64_t max_segments = 0;                 // 0: no limit
};
struct IbsSegment { uint64_t x, y, symbol_first, symbol_last, sites, column_first, column_end; };
struct PathIbs {
    std::vector<IbsSegment> segments;
    std::vector<uint64_t> pair_off;
    size_t paths = 0, choice_symbols = 0, candidate_segments = 0;
};
PathIbs path_ibs(std::istream& eds, std::istream& seds, const std::vector<int>& paths = {}, const IbsOptions& options = IbsOptions());

// edsparser-mosaic: every target path written as the fewest copies from the donor paths (each list empty: all paths 1..P;
// duplicates allowed; both are named by request position; a donor that names the target's own path is skipped for it).
// A copied segment reaches as far as any donor does, of equals the smallest position; a private segment (donor
// MOSAIC_PRIVATE) holds the symbols no donor shares; the segments of a target tile [0, n - 1], in (target, symbol_first)
// order (edsx_paths_mosaic states the rules in full).  target_off: T + 1 offsets into segments.  std::invalid_argument for
// a path outside 1..P and for more segments than max_segments.
constexpr uint64_t MOSAIC_PRIVATE = ~0ull;
struct MosaicOptions {
    uint64_t max_segments = 0;                 // 0: no limit
};
struct MosaicSegment { uint64_t target, donor, symbol_first, symbol_last, sites, column_first, column_end; };
struct PathMosaic {
    std::vector<MosaicSegment> segments;
    std::vector<uint64_t> target_off;
    size_t targets = 0, donors = 0, choice_symbols = 0, private_segments = 0, private_symbols = 0, switches = 0;
};
PathMosaic path_mosaic(std::istream& eds, std::istream& seds, const std::vector<int>& targets = {}, const std::vector<int>& donors = {},
                       const MosaicOptions& options = MosaicOptions());

// edsparser-diversity: per window along the EDS the diversity within and between groups of paths (no group: one group of
// all paths 1..P; a duplicate inside a group counts once; at most 16 disjoint groups).  Windows of `size` coordinates every
// `step` (0: size; size 0: one window), coordinates being choice symbols or columns of the alignment view.  Per (window,
// group): the segregating choice symbols and the paths present, summed; per (window, g <= h), row-major: the path pairs that
// both have a string (comp) and those whose strings differ (diff), summed - pi = diff / comp on the diagonal, d_xy off it
// (edsx_paths_diversity states the rules in full; edsparser_amd/host/div_stats.hpp derives pi, d_xy, F_ST, theta_W and
// Tajima's D from the integers).  sfs: per group K_g + 1 bins of the unfolded spectrum over all complete choice symbols.
// std::invalid_argument for a path outside 1..P, an empty group, a path in two groups, more than 16 groups and more
// windows than max_windows.
enum class DiversityUnit { SYMBOLS = 0, COLUMNS = 1 };
struct DiversityOptions {
    DiversityUnit unit = DiversityUnit::SYMBOLS;
    uint64_t size = 0, step = 0;
    uint64_t max_windows = 0;                  // 0: no limit
    bool sfs = false;
};
struct DiversityWindow { uint64_t start, end, rank_first, rank_end; };
struct DiversityGroup { uint64_t segregating, present; };
struct DiversityPair { uint64_t diff, comp; };
struct PathDiversity {
    std::vector<DiversityWindow> windows;      // NW
    std::vector<DiversityGroup> groups;        // NW x G
    std::vector<DiversityPair> pairs;          // NW x G (G + 1) / 2
    std::vector<std::vector<uint64_t>> sfs;    // G spectra, with options.sfs
    std::vector<uint64_t> group_paths;         // K_g
    size_t n_groups = 0, paths = 0, choice_symbols = 0, n_pairs = 0, extent = 0;
    static size_t pair_index(size_t G, size_t g, size_t h) { return g * G - g * (g + 1) / 2 + h; }     // g <= h
};
PathDiversity path_diversity(std::istream& eds, std::istream& seds, const std::vector<std::vector<int>>& groups = {},
                             const DiversityOptions& options = DiversityOptions());

// edsparser-subset: the EDS with sources restricted to the given paths (ids of 1..P, each once), as FULL .eds text and
// .seds text, each with a trailing line feed.  A string is kept when its set holds 0 or one of the paths; symbols without
// a kept string go, a symbol whose only kept string is universal or holds every kept path becomes common, and runs of
// adjacent common symbols are joined (edsx_eds_subset states the rules in full).  Kept paths are renumbered 1..|paths| in
// ascending order of their ids unless keep_ids.  Every kept path spells the sequence it spelled before.
// std::invalid_argument for an empty list, a path outside 1..P or a path listed twice.
struct SubsetInfo {
    size_t symbols_in = 0, symbols_out = 0, strings_in = 0, strings_out = 0, chars_in = 0, chars_out = 0, paths_in = 0,
           paths_out = 0, symbols_removed = 0, common_runs_merged = 0;
};
void eds_subset(std::istream& eds, std::istream& seds, std::ostream& eds_out, std::ostream& seds_out,
                const std::vector<int>& paths, bool keep_ids = false, SubsetInfo* info = nullptr);

// eds2gfa: the EDS as GFA 1.0 text - header, one S line per non-empty string (ids from 1 in file order), the L lines of
// adjacent symbols (across symbols that hold an empty string), and, when seds is given, one P line per path of `paths`
// (empty: all paths 1..P) named (*names)[k], else prefix + id (edsx_eds_gfa_graph / edsx_paths_gfa_walks state the rules
// in full).  max_links: 0 = 2^32.  std::invalid_argument for a graph of more links, a path outside 1..P, paths or names
// without sources, or a name that is empty or holds a tab, line feed or blank.
struct GfaInfo {
    size_t n_symbols = 0, n_strings = 0, n_segments = 0, n_empty_strings = 0, n_open_symbols = 0, n_links = 0, header_bytes = 0,
           segment_bytes = 0, link_bytes = 0;
    std::vector<size_t> missing, steps;        // per requested path (with sources)
};
void eds_to_gfa(std::istream& eds, std::istream* seds, std::ostream& gfa, const std::vector<int>& paths = {},
                const std::vector<std::string>* names = nullptr, const std::string& prefix = "path", size_t max_links = 0,
                GfaInfo* info = nullptr);

} // namespace edsparser

#endif
