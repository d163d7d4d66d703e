/*
 * edsx.h — C ABI of the MI355X-native EDS transformation engine (libedsx.so).
 *
 * This is the drop-in boundary for EDSParser's transform hot path.  Every entry point is
 * `extern "C"`, takes plain pointers and sizes, returns an int status and never throws.
 * The host-buffer calls are exactly what the reference's Transforms layer would bind (one call
 * per public function of src/cpp/lib/transforms/): the `edsparser::` C++ shims in
 * edsparser_amd/host/ slurp the std::istream into a byte buffer and call these.
 *
 *   edsx_msa_transform   replaces parse_msa_to_eds_streaming  (msa_transforms.hpp:27,  .cpp:334-345)
 *                        and      parse_msa_to_leds_streaming (msa_transforms.hpp:37-39, .cpp:351-365)
 *   edsx_leds_merge      replaces eds_to_leds_linear          (eds_transforms.hpp:29-37, .cpp:313-373)
 *                        and      eds_to_leds_cartesian       (eds_transforms.hpp:45-51, .cpp:381-426)
 *   edsx_vcf_transform   replaces parse_vcf_to_eds_streaming  (vcf_transforms.hpp:59-62, .cpp:677-729)
 *                        and      parse_vcf_to_leds_streaming (vcf_transforms.hpp:75-79, .cpp:735-755)
 *
 * The same transforms spread over the GPUs of one node from one process (edsx_multi): edsx_msa_transform_multi
 * (column slabs), edsx_vcf_transform_multi (reference-position ranges) and edsx_leds_merge_multi (symbol ranges).
 *
 * Status codes mirror the reference's (unused) ErrorCode enum, src/cpp/lib/common.hpp:37-45.
 * The *_device calls take HBM pointers on the context's GPU and a hipStream_t (passed as void*),
 * so pipelines and the benchmark can keep data resident; they are what the host-buffer calls
 * are built from.  There is NO CPU fallback: every call fails with EDSX_ERR_BUILD_FAILED when no
 * gfx950 device is usable.
 */
#ifndef EDSX_H
#define EDSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum edsx_status {
    EDSX_OK = 0,
    EDSX_ERR_FILE_NOT_FOUND = 1,
    EDSX_ERR_INVALID_FORMAT = 2,     /* std::runtime_error in the reference (format errors)   */
    EDSX_ERR_INVALID_PARAMETER = 3,  /* std::invalid_argument / std::out_of_range             */
    EDSX_ERR_BUILD_FAILED = 4,       /* device / HIP runtime failure, no GPU, out of memory   */
    EDSX_ERR_QUERY_FAILED = 5,
    EDSX_ERR_UNKNOWN = 99
};

typedef struct edsx_ctx edsx_ctx;

/* Host byte buffer allocated by the library; release with edsx_buf_free. */
typedef struct { uint8_t* data; size_t size; } edsx_buf;

/* Counters of vcf_transforms.hpp:24-35 (VCFStats). */
typedef struct {
    uint64_t total_variants, processed_variants, skipped_malformed,
             skipped_unsupported_sv, variant_groups;
} edsx_vcf_stats;

/* ---- context: one per (host thread, GPU) ---- */
int  edsx_ctx_create(int device, edsx_ctx** out);
void edsx_ctx_destroy(edsx_ctx* ctx);
/* Message of the last failing call on this context (valid until the next call). */
const char* edsx_last_error(const edsx_ctx* ctx);
void edsx_buf_free(edsx_buf* buf);
const char* edsx_version(void);

/* ---- host-buffer entry points (the drop-in boundary) ---- */

/* MSA (FASTA with '-' gaps) -> EDS (context_len == 0) or l-EDS (context_len > 0) + sEDS.
 * Output bytes are identical to the std::string pair the reference returns. */
int edsx_msa_transform(edsx_ctx* ctx, const uint8_t* msa, size_t msa_size, uint32_t context_len,
                       edsx_buf* eds, edsx_buf* seds);
/* The same in `batches` column batches, one after the other on the context's GPU: the device holds one batch (its
 * image, variant columns, records and tables) at a time, every batch's text goes to the host as it is written, and the
 * segments that cross a batch boundary are stitched as between the GPUs of edsx_msa_transform_multi.  Output is
 * byte-identical to edsx_msa_transform, which falls back to this (2, 4, 8 ... batches) when an alignment and its tables
 * do not fit the device in one piece.  An input that cannot be cut (not a plain uniform alignment, batches narrower than
 * 4 * context_len columns, or - context_len > 0 - a batch without a common run of context_len columns near both ends)
 * is transformed in one piece.  *batches_used (may be NULL) receives the number of batches taken (1: one piece). */
int edsx_msa_transform_batched(edsx_ctx* ctx, const uint8_t* msa, size_t msa_size, uint32_t context_len, int batches,
                               edsx_buf* eds, edsx_buf* seds, int* batches_used);
/* column batches the last successful edsx_msa_transform / _batched of this context took (1: one piece; 0: none yet) */
int edsx_msa_last_batches(const edsx_ctx* ctx);

/* EDS (+ optional sEDS) -> l-EDS.  seds == NULL => CARTESIAN, else LINEAR.
 * compact != 0 => COMPACT brackets (the CLI default), else FULL.  Outputs end in '\n' like
 * EDS::save / save_sources; seds_out->size == 0 when no sources were given. */
int edsx_leds_merge(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size,
                    const uint8_t* seds, size_t seds_size, uint32_t context_len, int compact,
                    edsx_buf* leds, edsx_buf* seds_out);

/* 1 when the last edsx_leds_merge / _range call on this context tokenised its .eds/.seds text on the GPU (plain text:
 * no inner whitespace, no comma outside braces, well-formed), 0 when the host tokenisers took it (anything else,
 * and every input that ends in one of the reference's format errors). */
int edsx_leds_tokenised_on_device(const edsx_ctx* ctx);

/* VCF + FASTA -> EDS (context_len == 0) or l-EDS (> 0) + sEDS; stats may be NULL. */
int edsx_vcf_transform(edsx_ctx* ctx, const uint8_t* vcf, size_t vcf_size,
                       const uint8_t* fasta, size_t fasta_size, uint32_t context_len,
                       edsx_buf* eds, edsx_buf* seds, edsx_vcf_stats* stats);

/* 1 when the last edsx_vcf_transform / _range / session transform call on this context tokenised the VCF text on the GPU (plain files:
 * tab-separated lines without empty fields, POS all digits, no symbolic ALT other than <DEL>/<INS>, alleles "." or
 * digits, no '\r', no POS 0), 0 when the host tokeniser took the file (everything else). */
int edsx_vcf_tokenised_on_device(const edsx_ctx* ctx);

/* ---- contig selection: multi-contig VCF + multi-record FASTA ----
 * The reference reads the first FASTA record only and never compares its name with CHROM (vcf_transforms.cpp:51-86),
 * and edsx_vcf_transform reproduces that.  A session keeps both texts in HBM and transforms one contig at a time.
 * "Contig c of (V, F)" is defined by reduction to edsx_vcf_transform:
 *   F_c = the bytes of the first FASTA record named c.  A record starts at a '>' that is byte 0 of the file or follows
 *         '\n' and ends in front of the next such '>' (or at the end of the file); its name is the header line behind
 *         '>' up to the first ' ' (or the whole line).
 *   V_c = V without the record lines (lines that are neither empty nor start with '#') whose first token - the first
 *         maximal run of non-whitespace bytes - is not c.  A record line without a token belongs to no contig.
 *   result = what edsx_vcf_transform(V_c, F_c, context_len) returns: texts, counters, status code and error text.
 * Plain inputs are indexed, classified and tokenised on the device from the resident texts; a VCF with '\r', or with a
 * record line whose first tab field is empty or holds whitespace, is classified on the host, and a contig whose lines the
 * device tokeniser refuses is handed over as host text (outputs equal either way; EDSX_HOST_TOKENIZER=1 forces it). */
typedef struct { uint64_t name_off, name_len,      /* name bytes inside the FASTA */
                 rec_start, rec_end,               /* the record's bytes */
                 seq_start, line_width, seq_size,  /* first sequence line and size as parse_fasta_metadata finds them */
                 vcf_records,                      /* record lines of the VCF whose first token is this name */
                 duplicate; } edsx_contig;         /* 1: an earlier record has the same name (never selected) */
typedef struct { uint64_t records_total, records_without_token, records_unknown_contig,
                 vcf_h2d_bytes, fasta_h2d_bytes;   /* raw input bytes copied to the device since open */
                 int classified_on_device; } edsx_vcf_session_stats;
typedef struct edsx_vcf_session edsx_vcf_session;

/* Both buffers stay the caller's and must outlive the session.  vcf_size == 0: the session is the FASTA index alone.
 * A FASTA that does not begin with '>' fails as edsx_vcf_transform does.  Errors of every session call are read with
 * edsx_last_error(ctx); the context must outlive the session. */
int  edsx_vcf_session_open(edsx_ctx* ctx, const uint8_t* vcf, size_t vcf_size, const uint8_t* fasta, size_t fasta_size,
                           edsx_vcf_session** out);
/* the FASTA records in file order; the array lives as long as the session */
int  edsx_vcf_session_contigs(const edsx_vcf_session* s, const edsx_contig** records, size_t* n);
/* index of the first record of that name; none: EDSX_ERR_INVALID_PARAMETER,
 * "Contig '<name>' not found in reference FASTA" */
int  edsx_vcf_session_find(const edsx_vcf_session* s, const char* name, size_t* index);
int  edsx_vcf_session_transform(edsx_vcf_session* s, size_t index, uint32_t context_len,
                                edsx_buf* eds, edsx_buf* seds, edsx_vcf_stats* stats);
int  edsx_vcf_session_info(const edsx_vcf_session* s, edsx_vcf_session_stats* out);
/* contigs the VCF names and the FASTA lacks: "<name>\t<record lines>\n" each, in order of first appearance */
int  edsx_vcf_session_unknown_contigs(const edsx_vcf_session* s, edsx_buf* text);
void edsx_vcf_session_close(edsx_vcf_session* s);
/* open + find + transform + close */
int  edsx_vcf_transform_contig(edsx_ctx* ctx, const uint8_t* vcf, size_t vcf_size, const uint8_t* fasta, size_t fasta_size,
                               const char* contig, uint32_t context_len, edsx_buf* eds, edsx_buf* seds,
                               edsx_vcf_stats* stats);

/* ---- compressed input: gzip and BGZF (bgzip) files, DEFLATE decoded on the device ----
 * inflate(x) is x itself when x does not begin with the bytes 1f 8b; otherwise the concatenated payloads of all gzip
 * members of x (RFC 1952 / 1951: what Python's gzip.decompress returns); bytes behind the last member that are not a
 * member are an error.  A file is BGZF when every member has CM 8, FLG 4, an extra subfield 'B' 'C' of length 2, its
 * block inside the file and ISIZE <= 65536; every block is then one wave's work on the device (inflate + CRC-32).
 * Any other gzip file is inflated on the host, on the calling thread.  No compression library is involved.
 * Errors of the compressed layer are EDSX_ERR_INVALID_FORMAT, "Compressed <VCF|FASTA|input>: block <k> at byte <off>:
 * <reason>" for the lowest failing member k (from 0) at byte offset off; reason: truncated | not a gzip member |
 * block size beyond the end of the file | invalid DEFLATE stream | length mismatch | CRC mismatch.
 * The existing entry points do not look for gzip magic; only the calls below do. */
/* host only: *kind = 0 plain, 1 BGZF, 2 gzip; never fails on garbage */
int edsx_gz_probe(const uint8_t* data, size_t size, int* kind);
typedef struct { uint64_t comp_off, out_off; uint32_t comp_len, isize; } edsx_bgzf_block;
/* host only, no context: the block table of a BGZF file (an array of edsx_bgzf_block in blocks, EOF block included)
 * and the size of its text; EDSX_ERR_INVALID_FORMAT when the file is not BGZF.  Reads headers and trailers only. */
int edsx_bgzf_index(const uint8_t* data, size_t size, edsx_buf* blocks, uint64_t* text_size);
/* text = inflate(data).  BGZF: on the device; gzip: on the host; plain: a copy. */
int edsx_gz_inflate(edsx_ctx* ctx, const uint8_t* data, size_t size, edsx_buf* text);
/* edsx_vcf_transform (contig == NULL: first FASTA record, CHROM ignored) or edsx_vcf_transform_contig on
 * (inflate(vcf), inflate(fasta)): same texts, counters, status and error text.  Either input may be compressed or
 * plain.  Text inflated on the device stays in HBM, where the tokeniser, the FASTA index and the contig classifier read it. */
int edsx_vcf_transform_z(edsx_ctx* ctx, const uint8_t* vcf, size_t vcf_size, const uint8_t* fasta, size_t fasta_size,
                         const char* contig, uint32_t context_len, edsx_buf* eds, edsx_buf* seds, edsx_vcf_stats* stats);
/* edsx_vcf_session_open on (inflate(vcf), inflate(fasta)); the session works with every edsx_vcf_session_* call and
 * owns what it needs: the caller's buffers may be released after the call. */
int edsx_vcf_session_open_z(edsx_ctx* ctx, const uint8_t* vcf, size_t vcf_size, const uint8_t* fasta, size_t fasta_size,
                            edsx_vcf_session** out);
/* The name of FASTA record `index` (not zero-terminated; valid until close): edsx_contig's name_off points into the
 * inflated FASTA, which a caller of edsx_vcf_session_open_z does not hold.  Works for every session. */
int edsx_vcf_session_contig_name(const edsx_vcf_session* s, size_t index, const char** name, size_t* len);
/* A session opened with _open_z keeps the info of its two inputs; every edsx_vcf_session_transform on it publishes them
 * again (with its downloads so far) as the context's last info, whatever other call ran in between.
 * The compressed layer of the last call above, per input: which = 0 the VCF (or the input of edsx_gz_inflate), 1 the
 * FASTA.  h2d_bytes: compressed bytes + block table copied to the device (BGZF); text_d2h_bytes: bytes of inflated
 * text copied back to the host (windows for the host-side header parse, or the whole text when a host path was taken). */
typedef struct { int kind; int inflated_on_device; uint64_t blocks, comp_bytes, text_bytes, h2d_bytes, text_d2h_bytes;
                 double index_ms, inflate_ms, crc_ms; } edsx_gz_info;
int edsx_gz_last_info(const edsx_ctx* ctx, int which, edsx_gz_info* out);

/* ---- multi-GPU VCF: partition by reference position ----
 * Groups of overlapping records (vcf_transforms.cpp:482-534) never span a cut placed at a group start, so
 * every GPU walks its own position range and the pieces concatenate to the reference's text with no repair.
 * What has to be global is the order of the records: the reference sorts the whole array with an unstable
 * std::sort (:715-718), so every rank indexes its byte range of the file, the (POS, REF length) arrays are
 * all-gathered, every rank derives the same order and cuts, and record lines that fall into another rank's
 * position range are exchanged (edsparser_amd/multigpu.py, VcfSharder). */

/* Index pass over VCF text: POS and REF length (uint64 each) and the line span (offset, length; uint64 each)
 * of every record the transform would accept, in file order; counters as edsx_vcf_transform (variant_groups
 * stays 0).  Genotypes are not parsed. */
int edsx_vcf_index(edsx_ctx* ctx, const uint8_t* vcf, size_t vcf_size, edsx_buf* pos, edsx_buf* reflen,
                   edsx_buf* line_off, edsx_buf* line_len, edsx_vcf_stats* stats);
/* order_out[k] = index (into pos) of the k-th record after the reference's std::sort of n records. */
int edsx_vcf_sort_order(const uint64_t* pos, size_t n, uint32_t* order_out);
/* edsx_vcf_transform (context_len 0) of one position range: `vcf` holds the range's record lines already in
 * their final order; the walk starts at reference position cur0 (pass the start of the range's first group
 * for every range but the first, 0 for the first) and the closing common text stops at next_start (0-based
 * start of the next range's first group; UINT64_MAX for the last range: flush to the end of the reference). */
int edsx_vcf_transform_range(edsx_ctx* ctx, const uint8_t* vcf, size_t vcf_size, const uint8_t* fasta,
                             size_t fasta_size, uint64_t cur0, uint64_t next_start, edsx_buf* eds,
                             edsx_buf* seds, edsx_vcf_stats* stats);

/* ---- multi-GPU merge: partition by symbol range ----
 * edsx_leds_merge of one symbol range of a larger EDS.  Neighbouring ranges overlap in one sentinel symbol (a single
 * string of at least context_len characters between two degenerate symbols; edsparser_amd/multigpu.py, MergeSharder,
 * finds them): head_sentinel / tail_sentinel say that the first / last symbol of this text is such a shared symbol.
 * The range that has it as its tail prints it, the one that has it as its head drops it; only a range without a tail
 * sentinel ends its outputs in '\n'.  *head_intact / *tail_intact come back 0 when the sentinel was drawn into a merge
 * (possible only when a LINEAR product collapses its neighbour to a single short string): the partition is then
 * invalid for this input and the caller must run edsx_leds_merge on the whole text. */
int edsx_leds_merge_range(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                          uint32_t context_len, int compact, int head_sentinel, int tail_sentinel,
                          edsx_buf* leds, edsx_buf* seds_out, int* head_intact, int* tail_intact);

/* Device scans of one byte range of an .eds / .seds text: what the symbol-range partition learns about a rank's slice
 * (edsparser_amd/multigpu.py, eds_scan_range / seds_scan_range, are the spec).  Each call copies only its window of the
 * text to the device.
 * .eds bytes [lo, hi) (hi <= eds_size; hi <= lo: an empty slice): ok = no whitespace, braces alternate from the state at
 * lo, no comma outside braces, no '{' inside braces; strings = string starts in the slice ('{', ',' and the first byte
 * of a bare run; 0 when not ok).  For lo > 0 only, has_cut: the first sentinel whose preceding '}' lies in [lo, hi),
 * spelled COMPACT `}p{x,y}` or FULL `}{p}{x,y}` with p of at least max(context_len, 1) characters, searched in a window
 * from the last '{' in front of lo up to min(end, hi + 65536 + 4 context_len) (end: the text without trailing
 * whitespace); [sym_start, sym_end) are its bytes and strings_before the string starts in [lo, sym_start). */
typedef struct { int ok; uint64_t strings; int has_cut; uint64_t sym_start, sym_end, strings_before; } edsx_eds_range_scan;
int edsx_eds_scan_range(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, uint64_t lo, uint64_t hi, uint32_t context_len,
                        edsx_eds_range_scan* out);
/* .seds bytes [lo, hi): *ok = no whitespace, *braces = the number of '{' (0 when not ok).  When ok, for every i <
 * n_ordinals: [set_start[i], set_end[i]) = the bytes from the ordinals[i]-th '{' of the slice (counted from 0) to one
 * past the first '}' behind it anywhere in the buffer (set_end 0: there is none).  An ordinal >= *braces is
 * EDSX_ERR_INVALID_PARAMETER. */
int edsx_seds_scan_range(edsx_ctx* ctx, const uint8_t* seds, size_t seds_size, uint64_t lo, uint64_t hi,
                         const uint64_t* ordinals, size_t n_ordinals, int* ok, uint64_t* braces,
                         uint64_t* set_start, uint64_t* set_end);

/* ---- statistics and validation of an EDS / l-EDS (what edsparser-stats prints) ----
 * Replaces EDS::calculate_statistics / calculate_source_statistics (src/cpp/lib/formats/eds.cpp:361-470, :472-505,
 * struct EDS::Statistics eds.hpp:107-120) and is_leds (src/cpp/lib/transforms/eds_transforms.cpp:439-468): the text is
 * tokenised as for edsx_leds_merge and the numbers are device reductions over the per-symbol / per-string arrays.
 * seds == NULL: no sources (the three path fields stay 0).  Parse errors: as edsx_leds_merge. */
typedef struct {
    uint64_t n_symbols, n_chars, n_strings;            /* EDS::length(), size(), cardinality() */
    uint64_t num_degenerate_symbols, total_change_size, num_common_chars, num_empty_strings;
    uint64_t min_context_length, max_context_length, num_context_blocks;
    double   avg_context_length;                       /* num_common_chars / num_context_blocks (0 when there are none) */
    uint64_t has_sources, num_paths, max_paths_per_string, total_paths;
    double   avg_paths_per_string;                     /* total_paths / n_strings */
    int      is_leds;                                  /* is_leds(eds, context_len) */
} edsx_eds_statistics;
int edsx_eds_stats(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                   uint32_t context_len, edsx_eds_statistics* out);

/* ---- queries: pattern sampling and position checks (EDS::generate_patterns / EDS::check_position) ----
 * The text is tokenised as for edsx_leds_merge; parse errors as there.
 * edsx_eds_genpatterns: count patterns of pattern_length characters, each followed by '\n' (count * (pattern_length + 1)
 * bytes), the bytes of EDS::generate_patterns(os, count, pattern_length, seed).  Draw k of pattern i is
 * hash3(seed, i, k) (k = 0 the start among the common characters, k = 1, 2, ... the strings in walk order, then the
 * wrap), bounded by the high 64 bits of r * bound.  An empty EDS, pattern_length 0, and a wrap-around that reaches a
 * symbol without a non-empty string are EDSX_ERR_INVALID_PARAMETER; count 0 gives an empty buffer.  Witnesses (all three
 * NULL, or all three set): witness_pos = the start common position of every pattern (uint64; UINT64_MAX when the pattern
 * wrapped or the EDS has no common character), witness_off (uint64, count + 1) / witness_deg (int32) = the degenerate
 * string numbers each pattern chose, as CSR (none for a UINT64_MAX pattern).  EDS::check_position(pos, choices, pattern)
 * holds for every other pattern when no sources are given. */
int edsx_eds_genpatterns(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, uint64_t count, uint32_t pattern_length,
                         uint64_t seed, edsx_buf* patterns, edsx_buf* witness_pos, edsx_buf* witness_off, edsx_buf* witness_deg);
/* n queries as CSR: query q asks EDS::check_position(common_pos[q], choices[choice_off[q] .. choice_off[q+1]),
 * patterns[pattern_off[q] .. pattern_off[q+1])) of the .eds (+ .seds: the chosen strings must share a path; seds NULL:
 * no sources).  status_out[q]: 1 true, 0 false, -1 std::out_of_range, -2 std::invalid_argument (also for offsets that
 * decrease or pass choice_off[n] / pattern_off[n]). */
int edsx_eds_check_positions(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                             size_t n, const uint64_t* common_pos, const uint64_t* choice_off, const int32_t* choices,
                             const uint64_t* pattern_off, const uint8_t* patterns, int8_t* status_out);
/* ---- pattern search: every occurrence of every pattern ----
 * n patterns as CSR (pattern_off[n + 1], patterns); the .eds (+ .seds) as for edsx_eds_check_positions.  An occurrence of
 * a pattern P of L >= 1 bytes is (string g, offset o, choices d_1..d_k): g is a string of symbol `symbol` (its index
 * there is `string`, in file order, the order the .seds uses) and o < |g|, so an occurrence begins on a character.  The
 * walk takes g[o:], then, while fewer than L characters are taken and symbols remain, the only string of a common symbol
 * or the string the next choice names of a degenerate one (a degenerate string number, cum_deg[symbol] + index, as in
 * check_position), each cut to what is still needed.  It spells P with exactly L characters; k is exactly the number of
 * degenerate symbols visited after g's, and a symbol after the last character is not visited.  With sources the strings
 * used, g included, must share a path by check_position's rule (bit 0 / {0} is universal).  So for a start in a common
 * symbol, (common_pos, choices) is an occurrence exactly when check_position(common_pos, choices, P) is true and no
 * choice is left over.  Bytes are compared raw: a pattern with '{', '}', ',' or white space never matches.
 * Order: by pattern; within a pattern ascending by (symbol, string, offset), then by choices in lexicographic order
 * (depth-first over the alternatives in file order).
 * Caps, reported in pattern_flags[q]:
 *   bit 0  hits were left out: the first min(found, max_hits) in the order above are returned; a single start stops
 *          enumerating at max_hits of its own.  totals[q] sums min(occurrences of the start, max_hits) over the starts:
 *          the exact number of occurrences when the flags are 0, a lower bound otherwise.  max_hits above 2^32 acts as 2^32.
 *   bit 1  a walk was cut where it needed choice number EDSX_LOCATE_MAX_CHOICES + 1: whatever lies beyond is neither
 *          reported nor counted.
 * n = 0: empty buffers, hit_off = [0].  An empty EDS has no hits.  An empty pattern, a pattern_off that decreases and
 * max_hits = 0 are EDSX_ERR_INVALID_PARAMETER (the text names the pattern); parse errors as for edsx_leds_merge. */
typedef struct { uint64_t common_pos;   /* UINT64_MAX: the start is inside a degenerate symbol */
                 uint64_t symbol, string, offset; } edsx_locate_hit;
#define EDSX_LOCATE_COMMON_ONLY 1u      /* report only starts in common symbols (check_position's domain) */
#define EDSX_LOCATE_MAX_CHOICES 64
int edsx_eds_locate(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                    size_t n, const uint64_t* pattern_off, const uint8_t* patterns, uint64_t max_hits, uint32_t flags,
                    edsx_buf* hit_off,      /* uint64, n + 1 */
                    edsx_buf* hits,         /* edsx_locate_hit, hit_off[n] */
                    edsx_buf* choice_off,   /* uint64, hit_off[n] + 1 */
                    edsx_buf* choices,      /* int32 */
                    edsx_buf* totals,       /* uint64, n */
                    edsx_buf* pattern_flags /* uint8, n */);
/* Of the last edsx_eds_genpatterns / edsx_eds_check_positions / edsx_eds_locate on this context: the EDS's counts and where the time
 * went (tokenise: host clock around the upload and tokeniser; tables / kernels: device events; download: host clock). */
typedef struct {
    uint64_t n_symbols, n_strings, n_chars, num_common_chars, num_degenerate_strings;
    double tokenise_ms, tables_ms, kernel_ms, download_ms;
} edsx_query_info;
int edsx_query_last_info(const edsx_ctx* ctx, edsx_query_info* out);

/* ---- synthetic inputs: genrandomeds-shaped .eds + .seds generated in HBM ----
 * Flags and shape of src/cpp/tools/genrandomeds.cpp:383-405 / :221-352 (reference uniform over `alphabet`, single-position
 * variant sites with min_alt..max_alt alternatives, snp_ratio SNPs, else insertions of 1..var_len_max characters /
 * deletions, max(max_alt, 3) paths, {0} for common blocks, FULL brackets, no trailing newline).  Counter-based, not the
 * reference's mt19937 stream: the same (seed, flags) always give the same text, but not the reference's bytes; with
 * min_context == 0 the number of sites is binomial around total_bp * variability instead of exactly its floor. */
int edsx_genrandomeds(edsx_ctx* ctx, uint64_t total_bp, double variability, uint32_t min_alt, uint32_t max_alt,
                      uint32_t var_len_max, double snp_ratio, const char* alphabet, uint64_t min_context, uint64_t seed,
                      edsx_buf* eds, edsx_buf* seds, uint64_t* n_sites);

/* ---- device-resident MSA path (inputs/outputs stay in HBM) ----
 * The two calls below read and write memory the caller owns, on a stream the caller chooses (a hipStream_t; null: the
 * default stream).  What they promise (pinned by tests/test_msa_resident_gpu.py on buffers between guard zones, except
 * that a test cannot see a load whose value is discarded: that no byte outside the input is even loaded was established
 * by reading the kernels):
 *   - Pointers: any byte address.  No alignment is assumed for d_msa, d_eds or d_seds.
 *   - Input: exactly the bytes [d_msa, d_msa + msa_size) are read.  Nothing in front of or behind them needs to be
 *     readable, and no result or error text depends on what lies there.
 *   - Outputs: exactly eds_bytes and seds_bytes bytes are written, every one of them, and none outside: buffers of
 *     exactly the planned sizes are enough (no slack).
 *   - Stream order: all work is ordered on `stream`.  emit also runs kernels on streams of its own, which it forks from
 *     and joins back into `stream`: whatever the caller enqueues on `stream` after emit, or a wait for `stream` alone,
 *     sees the complete outputs.  Work the caller has on OTHER streams is not waited for.
 *   - The plan lives in the context until the next plan: emit may be called any number of times after one successful
 *     plan (into the same or other buffers, on the same stream), without waiting in between.  A plan that fails leaves
 *     the context without a plan: emit then returns EDSX_ERR_INVALID_PARAMETER. */

/* Phase 1: index rows, scan columns, build the segment table and size the outputs.
 * d_msa must stay valid and unchanged until the last edsx_msa_emit_device of this plan has completed.  Synchronises
 * `stream` (and only it) to hand the sizes back: once for the row index and once for the sizes, once more when the
 * variant-column store had to grow.  Format errors are EDSX_ERR_INVALID_FORMAT with their text in edsx_last_error. */
int edsx_msa_plan_device(edsx_ctx* ctx, const uint8_t* d_msa, size_t msa_size, uint32_t context_len,
                         void* stream, uint64_t* eds_bytes, uint64_t* seds_bytes);
/* Phase 2: write the .eds / .seds text into caller-provided HBM buffers of the planned sizes (d_eds and d_seds must not
 * overlap).  Asynchronous: returns once the work is enqueued; complete in `stream` order. */
int edsx_msa_emit_device(edsx_ctx* ctx, uint8_t* d_eds, uint8_t* d_seds, void* stream);

/* Geometry of the last planned alignment (for reporting). */
typedef struct {
    uint64_t n_rows, n_cols, line_width, n_variant_cols, n_segments, msa_bytes,
             n_slow_segments;   /* variant segments handled by the generic (slow) kernels */
} edsx_msa_info;
/* (EDSX_ERR_INVALID_PARAMETER when there is no plan, or the last transform ran in column batches: the numbers would be
 * those of its last batch) */
int edsx_msa_last_info(const edsx_ctx* ctx, edsx_msa_info* info);

/* ---- multi-GPU column slabs: what the boundary stitch needs from a planned+emitted slab ----
 * A run that crosses a slab boundary is stitched by the caller (edsparser_amd/multigpu.py): common
 * runs are joined textually, variant runs are recomputed from the raw columns of both sides. */
typedef struct {
    uint64_t n_segments;
    uint64_t first_is_variant, first_cols, first_eds_bytes, first_seds_bytes;
    uint64_t last_is_variant, last_cols, last_eds_bytes, last_seds_bytes;
} edsx_msa_edges;
int edsx_msa_edge_info(edsx_ctx* ctx, edsx_msa_edges* out);
/* l-EDS slabs (context length l > 0): the first and the last common segment of at least min_cols columns of the planned
 * alignment - the anchors between which a slab's text does not depend on its neighbours (msa_transforms.cpp:153).
 * found = 0: there is none.  last_*: the last anchor's first column and the text offsets in front of it; first_*: the
 * column behind the first anchor and the text offsets behind it. */
typedef struct {
    uint64_t n_segments, found, first_seg, last_seg;
    uint64_t last_col, last_eds_bytes, last_seds_bytes;
    uint64_t first_end, first_eds_end, first_seds_end;
} edsx_msa_anchors;
int edsx_msa_anchor_info(edsx_ctx* ctx, uint64_t min_cols, edsx_msa_anchors* out);
/* Alignment columns [col0, col0+ncols) of every row of the planned alignment, row-major
 * (n_rows * ncols bytes) into a host buffer. */
int edsx_msa_copy_columns(edsx_ctx* ctx, uint64_t col0, uint64_t ncols, uint8_t* host_out);
/* First segment of the planned alignment that starts at or after alignment column `col`: its index, start
 * column and the byte offsets of its text in the .eds / .seds outputs (index n_segments, column n_cols and
 * the output sizes when no segment starts there).  Lets a caller cut the device-resident outputs at segment
 * boundaries, e.g. to check sampled column windows of a 100 GB alignment against the CPU path. */
int edsx_msa_locate_segment(edsx_ctx* ctx, uint64_t col, uint64_t* seg, uint64_t* seg_col, uint64_t* eds_off,
                            uint64_t* seds_off);

/* ---- MSA -> EDS over several GPUs of one node, from C/C++ (replaces the single call of msa2eds.cpp:123-132 when the
 * alignment should be spread over N GPUs) ----
 * One host thread per GPU inside the call.  The alignment columns are range-partitioned into n column slabs; every
 * GPU transforms its slab, and the segments that cross a slab boundary are stitched with KB-sized all-gathers:
 * ncclAllGather over RCCL (use_rccl = 1: one distinct device per rank), or an in-process exchange between the rank
 * threads (use_rccl = 0: ranks may share a device - rehearsals and tests on a one-GPU box).  Output is byte-identical
 * to edsx_msa_transform.  With context_len > 0 every boundary is recomputed between the nearest common runs of at
 * least context_len columns on either side; files that are not plain uniform alignments, and l-EDS slabs without such
 * runs near their ends, are transformed by rank 0 alone. */
typedef struct edsx_multi edsx_multi;
int  edsx_multi_create(const int* device_ids, int n, int use_rccl, edsx_multi** out);
void edsx_multi_destroy(edsx_multi* m);
const char* edsx_multi_last_error(const edsx_multi* m);
int  edsx_msa_transform_multi(edsx_multi* m, const uint8_t* msa, size_t msa_size, uint32_t context_len,
                              edsx_buf* eds, edsx_buf* seds);
/* of the last edsx_msa_transform_multi: 1 if the columns were partitioned, the number of boundary chains stitched */
int  edsx_multi_last_partition(const edsx_multi* m, int* partitioned, int* chains);

/* vcf2eds over the handle's GPUs: the records are partitioned by reference position (cuts at group starts, record lines
 * moved between ranks as runs of lines), every rank transforms its range with only its window of a regular FASTA on
 * its device, and the pieces are put together in rank order.  Outputs, stats, return codes and error texts (read
 * through edsx_multi_last_error) equal those of edsx_vcf_transform on the same input, for any number of ranks.
 * context_len > 0: the first device runs the LINEAR merge on the assembled text, as edsx_vcf_transform does. */
int  edsx_vcf_transform_multi(edsx_multi* m, const uint8_t* vcf, size_t vcf_size, const uint8_t* fasta, size_t fasta_size,
                              uint32_t context_len, edsx_buf* eds, edsx_buf* seds, edsx_vcf_stats* stats);
typedef struct {
    int partitioned;            /* 0: rank 0 transformed the whole file (wrapped positions, < 2 ranks with records) */
    int fasta_windowed;         /* 1: every rank uploaded only its window of the FASTA (a regular FASTA) */
    uint64_t records_min, records_max;      /* sorted records per rank, over ranks that own records */
    uint64_t moved_line_bytes;              /* record-line text that changed rank, all ranks together */
    uint64_t fasta_h2d_bytes_max;           /* most FASTA bytes one rank copied to its device (metadata slice + window) */
} edsx_vcf_multi_info;
/* of the last edsx_vcf_transform_multi */
int  edsx_multi_last_vcf(const edsx_multi* m, edsx_vcf_multi_info* out);

/* eds2leds over the handle's GPUs: the symbol-range partition of edsx_leds_merge_range, run on the rank threads.  Every
 * rank scans its slice of the .eds (and .seds) on its device with the kernels of edsx_eds_scan_range /
 * edsx_seds_scan_range, the ranks exchange fixed-size records, cut the text at sentinels (the rule of
 * edsparser_amd/multigpu.py, MergeSharder: the same input and number of ranks give the same ranges), locate the
 * sentinels' source sets, and every range's owner merges eds[e0, e1) / seds[s0, s1) on its device; the pieces are put
 * together in rank order.  A rank copies its scan window and its range to its device, never the whole text.  Rank 0
 * merges the whole text instead with one rank or context_len 0, a slice that is not plain text, no sentinel, source sets
 * that do not match, or a sentinel drawn into a merge / a failed range.  Outputs, return codes and error texts (read
 * through edsx_multi_last_error) equal those of edsx_leds_merge on the same input, for any number of ranks. */
int  edsx_leds_merge_multi(edsx_multi* m, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                           uint32_t context_len, int compact, edsx_buf* leds, edsx_buf* seds_out);
typedef struct {
    int partitioned, ranges;    /* ranges: symbol ranges merged (1 when not partitioned) */
    int fallback;   /* 0 partitioned; 1 one rank / context_len 0; 2 text not plain; 3 no sentinel;
                       4 source sets do not match; 5 a sentinel was merged or a range failed */
    uint64_t range_bytes_min, range_bytes_max;          /* .eds bytes of the ranges (the whole text when not partitioned) */
    uint64_t eds_h2d_bytes_max, seds_h2d_bytes_max;     /* most .eds / .seds bytes one rank copied to its device */
} edsx_merge_multi_info;
/* of the last edsx_leds_merge_multi */
int  edsx_multi_last_merge(const edsx_multi* m, edsx_merge_multi_info* out);

/* ---- eds2fasta: the sequence of every path of an EDS with sources (path_device.hip) ----
 * The texts are parsed exactly as edsx_leds_merge parses them in LINEAR mode (same tokenisers, statuses and error
 * texts).  P is the largest path id in the .seds (0 for an empty EDS).  The chosen string of path p (1 <= p <= P) at a
 * symbol is the first string of the symbol, in file order, whose source set holds p or 0; the sequence of p is the
 * concatenation over all symbols; a symbol without such a string contributes nothing and adds one to missing[p].
 * A session keeps the tokenised EDS in HBM in tables of its own: other calls on the context do not invalidate it, and
 * the input buffers may be released after edsx_paths_open.  seds == NULL: EDSX_ERR_INVALID_PARAMETER, "Path spelling
 * needs sources (.seds)".  A path id of 0 or above P: EDSX_ERR_INVALID_PARAMETER, "Path id <p> out of range (1..<P>)".
 * Errors are read through edsx_last_error of the context.
 * (A .leds written with compact = 1 prints nothing for a single-string symbol whose string is empty; it then no longer
 * matches its .seds in cardinality and is refused here as by edsx_leds_merge.  Write such files with compact = 0.) */
typedef struct edsx_paths_session edsx_paths_session;
typedef struct {
    uint64_t n_symbols, n_strings, n_chars, num_paths /* P */, n_choice_symbols;
    int tokenised_on_device;
} edsx_paths_info_t;
typedef struct {
    double tokenise_ms, choose_ms, scan_ms, copy_ms, download_ms;   /* device events; download: host clock */
    uint64_t bytes_written;                                         /* FASTA bytes of the last edsx_paths_spell */
} edsx_paths_timing;
int  edsx_paths_open(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                     edsx_paths_session** out);
int  edsx_paths_info(const edsx_paths_session* s, edsx_paths_info_t* out);
/* length[k] and missing[k] (may be NULL) of path ids[k]; duplicates allowed. */
int  edsx_paths_lengths(edsx_paths_session* s, const uint64_t* ids, size_t n, uint64_t* length, uint64_t* missing);
/* FASTA, one record per requested path in request order (n == 0: all paths 1..P): '>' name '\n', then the sequence in
 * lines of line_width characters, each ended by '\n' (line_width == 0: one line; an empty sequence has no line).  The
 * name is names[k] when names is given (n of them, n > 0), else prefix (NULL: "path") followed by the decimal id.
 * missing (may be NULL): one count per record. */
int  edsx_paths_spell(edsx_paths_session* s, const uint64_t* ids, size_t n, const char* const* names, const char* prefix,
                      uint64_t line_width, edsx_buf* fasta, uint64_t* missing);
/* of the last edsx_paths_lengths / edsx_paths_spell / edsx_paths_gfa_walks / edsx_paths_align / edsx_paths_lift* (tokenise_ms: of
 * edsx_paths_open; walks: scan_ms holds both scans of a batch, copy_ms the walk kernel, bytes_written the P lines; align:
 * copy_ms the alignment kernel, bytes_written the alignment; the lift calls: copy_ms the search and place kernels,
 * bytes_written the result bytes) */
int  edsx_paths_last_timing(const edsx_paths_session* s, edsx_paths_timing* out);
void edsx_paths_close(edsx_paths_session* s);
/* open + spell + close */
int  edsx_eds_spell_paths(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                          const uint64_t* ids, size_t n, const char* const* names, const char* prefix, uint64_t line_width,
                          edsx_buf* fasta, uint64_t* missing);

/* ---- edsparser-lift: positions between the paths of an EDS with sources (path_device.hip, lift_core.hpp) ----
 * chosen(p, i) is the string edsx_paths_spell chooses for path p in symbol i (none: "missing"); sym_pos_p(i) is the
 * number of characters of p in front of symbol i; col[i] is the first alignment column of symbol i (edsx_paths_align).
 *   Site of (p, x), 0 <= x < length of p: symbol i is the LARGEST with sym_pos_p(i) <= x (runs of symbols that add nothing
 *      to p share one offset), string j = the index of chosen(p, i) within the symbol, offset o = x - sym_pos_p(i), so
 *      that character x of p is character o of that string; column = col[i] + o; common_pos = edsx_eds_locate's
 *      coordinate when symbol i has one string, else UINT64_MAX.
 *   Place of (i, j, o) on path t, with start = sym_pos_t(i) and c = chosen(t, i):
 *      MISSING  c is none                  pos = start
 *      GAP      o >= length of c           pos = start + length of c: the next character to the right, or the length of t
 *      SAME     c is string j              pos = start + o, the very same character
 *      ALIGNED  otherwise                  pos = start + o, a character in the same alignment column
 *   Lift of (a, x) to b: the place of the site of (a, x) on b; the sites stay on the device in between.
 * Per-query errors do not fail the call: x at or above the length of the path, i at or above the number of symbols, j at
 * or above the size of the symbol and o at or above the length of string j give status RANGE and UINT64_MAX in every
 * output field of the query.  Queries may come in any order and repeat.  Path ids outside 1..P and a missing .seds give
 * the statuses and texts of edsx_paths_spell.  edsx_paths_last_timing: choose_ms / scan_ms of the tables, copy_ms the
 * search and place kernels, bytes_written the result bytes. */
typedef struct { uint64_t symbol, string, offset, column, common_pos; } edsx_lift_site;
#define EDSX_LIFT_SAME 0
#define EDSX_LIFT_ALIGNED 1
#define EDSX_LIFT_GAP 2
#define EDSX_LIFT_MISSING 3
#define EDSX_LIFT_RANGE 4
/* status[q]: 0 or EDSX_LIFT_RANGE */
int edsx_paths_lift_sites(edsx_paths_session* s, size_t n, const uint64_t* path, const uint64_t* pos, edsx_lift_site* site,
                          uint8_t* status);
int edsx_paths_lift_place(edsx_paths_session* s, size_t n, const uint64_t* symbol, const uint64_t* string, const uint64_t* offset,
                          const uint64_t* dst_path, uint64_t* dst_pos, uint8_t* status);
/* site (may be NULL): the site of every (src_path, src_pos) */
int edsx_paths_lift(edsx_paths_session* s, size_t n, const uint64_t* src_path, const uint64_t* src_pos, const uint64_t* dst_path,
                    uint64_t* dst_pos, uint8_t* status, edsx_lift_site* site);
/* open + lift + close */
int edsx_eds_lift(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size, size_t n,
                  const uint64_t* src_path, const uint64_t* src_pos, const uint64_t* dst_path, uint64_t* dst_pos, uint8_t* status,
                  edsx_lift_site* site);

/* ---- edsparser-slice: regions of an EDS with sources as EDSs of their own (slice_device.hip, slice_core.hpp) ----
 * Input: a path session and n regions (path, start, end), 0-based and half open.  path >= 1: characters [start, end) of
 * that path.  path == 0: columns [start, end) of the alignment of edsx_paths_align, within [0, W).
 *   Ends.  Path region: (i0, j0, o0, c0) is the site of (path, start) and (i1, j1, o1, c1) the site of (path, end - 1), by
 *      the rule of the lift above (the LARGEST symbol with sym_pos <= x).  Column region: i0 is the largest symbol with
 *      col[i0] <= start, o0 = start - col[i0], c0 = start; i1, o1 and c1 likewise from end - 1.  The cut offsets are o0
 *      and o1e = o1 + 1, the column window is [c0, c1 + 1).
 *   Symbols.  The slice holds the symbols i0 .. i1 in order, each with all its strings in order, empty ones too.  Every
 *      symbol strictly between the ends is copied as it is, whether the anchor path adds to it or not.  EVERY string t of
 *      symbol i0 becomes t[o0:], every string of symbol i1 becomes t[:o1e] (t[o0:o1e] when i0 == i1): the edge symbols
 *      are cut at the alignment column, in all strings, not only in the anchor's.  A string shorter than the cut becomes
 *      empty and stays.  Nothing is dropped, merged or reordered.
 *   Sources.  Every string keeps its source set, one set per string, ids unchanged.
 *   Texts.  Each region is a FULL-form text: the .eds has braces around every symbol ("{}" is one empty string, "{,}" are
 *      two) and ends with a line feed; the .seds has one "{ids}" per string, ids ascending, a set that holds 0 written
 *      "{0}", and ends with a line feed.  The regions lie one behind the other in eds_out and in seds_out, in request order.
 *   It follows that row p of the alignment of a slice is columns [c0, c1 + 1) of row p of the alignment of the input, for
 *      every path p, and that the slice spells characters [start, end) of its anchor path.
 * region (may be NULL), per region: the symbol range (symbol_last inclusive), the cut offsets o0 and o1e, the column
 * window, the number of strings and characters of the slice, and where its two texts lie (lengths with the line feed).
 * Per-region errors do not fail the call: start >= end, or end above the length of the path (above W for columns), gives
 * status EDSX_SLICE_RANGE, eds_len = seds_len = 0 and UINT64_MAX in every other field.  Regions may overlap, repeat and
 * come in any order.  A path id above P fails with the status and text of edsx_paths_spell.  max_bytes (0: none) is held
 * against the summed size of both buffers before they are allocated: EDSX_ERR_INVALID_PARAMETER, "Slices have <n> bytes,
 * above the limit of <max>".  n == 0 gives two empty buffers.  edsx_paths_last_timing: scan_ms the resolve, count and scan
 * steps (choose_ms the lift's tables), copy_ms the fill kernels, bytes_written both buffers; under edsx_set_timing the
 * kernels come back by name from edsx_get_timing. */
typedef struct { uint64_t symbol_first, symbol_last, cut_first, cut_end, column_first, column_end,
                 strings, chars, eds_off, eds_len, seds_off, seds_len; } edsx_slice_region;
#define EDSX_SLICE_RANGE 4
int edsx_paths_slice(edsx_paths_session* s, size_t n, const uint64_t* path, const uint64_t* start, const uint64_t* end,
                     uint64_t max_bytes, edsx_buf* eds_out, edsx_buf* seds_out, edsx_slice_region* region, uint8_t* status);
/* open + slice + close */
int edsx_eds_slice(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size, size_t n,
                   const uint64_t* path, const uint64_t* start, const uint64_t* end, uint64_t max_bytes, edsx_buf* eds_out,
                   edsx_buf* seds_out, edsx_slice_region* region, uint8_t* status);

/* ---- edsparser-dist: pairwise distances between the paths of an EDS with sources (dist_device.hip, dist_core.hpp) ----
 * Input: a path session and K path ids in request order; duplicates are allowed; n == 0 means all paths 1..P.  An id of 0
 * or above P is EDSX_ERR_INVALID_PARAMETER, "Path id <p> out of range (1..<P>)".
 *   Chosen string.  chosen(p, i) is the session's rule: the first string of symbol i, in file order, whose source set holds
 *      p or 0.  Otherwise it is none, and missing[p] counts those symbols.
 *   Metric EDSX_DIST_COLUMNS.  D[a][b] is the number of columns of the edsx_paths_align alignment at which the rows of the
 *      two paths differ.  Symbol i owns w[i] columns, where w[i] is the length of its longest string over all strings.  A
 *      path shows its chosen string left-justified and no character elsewhere - everywhere in the symbol when it has none.
 *      "No character" is a value of its own: it equals itself and differs from every byte; a '-' inside a string is an
 *      ordinary byte, and the metric has no gap parameter.
 *   Metric EDSX_DIST_STRINGS.  D[a][b] is the number of symbols i with chosen(a, i) != chosen(b, i), compared as string
 *      indices.  Two none are equal.  Equal texts are not merged, the convention of eds2gfa and eds2vcf.
 *   Any other metric is EDSX_ERR_INVALID_PARAMETER.
 *   Output.  matrix: K x K uint64, row-major, in request order, allocated by the caller (for n == 0, K = P from
 *      edsx_paths_info); it is symmetric and has a zero diagonal.  missing (may be NULL): K counts.  info (may be NULL):
 *      units            W for COLUMNS, the number of symbols for STRINGS: the denominator of a normalised distance
 *      variable_units   the units that got class columns (the others cannot tell two paths apart)
 *      class_columns    the bits of a path's row: one per class of every variable unit
 *      chunk_columns    class columns per chunk of the pair kernel
 *      chunks           the number of chunks
 *   Limits.  max_bytes (0: none) is held against 8 * K * K before anything is allocated: EDSX_ERR_INVALID_PARAMETER,
 *      "Distance matrix has <n> bytes, above the limit of <max>".  The bit rows (K * ceil(class_columns / 64) * 8 bytes)
 *      and the matrix must fit the session's budget: otherwise EDSX_ERR_BUILD_FAILED, with both sizes in the text and info
 *      filled in.  An EDS without choice symbols gives a zero matrix, P = 0 an empty one.
 * edsx_paths_last_timing: choose_ms the choice tables, scan_ms the class list (made by the first call per metric and kept
 * with the session) and the tables' scan, copy_ms the bit rows, the pair kernel and the finish, bytes_written the matrix;
 * under edsx_set_timing the kernels come back by name from edsx_get_timing. */
#define EDSX_DIST_COLUMNS 0
#define EDSX_DIST_STRINGS 1
typedef struct { uint64_t units, variable_units, class_columns, chunk_columns, chunks; } edsx_dist_info;
int edsx_paths_distances(edsx_paths_session* s, const uint64_t* ids, size_t n, int metric, uint64_t max_bytes, uint64_t* matrix,
                         uint64_t* missing, edsx_dist_info* info);
/* open + distances + close (n == 0: the caller learns P, and so the size of matrix, from the .seds or a session) */
int edsx_eds_distances(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                       const uint64_t* ids, size_t n, int metric, uint64_t max_bytes, uint64_t* matrix, uint64_t* missing,
                       edsx_dist_info* info);

/* ---- edsparser-ld: linkage disequilibrium between the alleles of an EDS with sources (ld_device.hip, ld_core.hpp) ----
 * Input: a path session and a set M of path ids; n == 0 means all paths 1..P; duplicates count once; K = |M|.  An id of 0
 * or above P is EDSX_ERR_INVALID_PARAMETER, "Path id <p> out of range (1..<P>)".
 *   Choice symbols.  The symbols that are not a single universal string, numbered r = 0..nc-1 in file order
 *      (n_choice_symbols of edsx_paths_info); every symbol with two strings or more is one.
 *   Carrier rule.  chosen(p, i) is the session's rule: the first string of symbol i, in file order, whose source set holds
 *      p or 0.  Overlapping sets therefore do not count a path twice: the alleles of a symbol partition the paths that
 *      have a string there.  T(r, j) = { p in M : chosen(p, symbol r) = string j }, U(r) = the union over j of T(r, j),
 *      the paths present at r; count(r, j) = |T(r, j)|, present(r) = |U(r)|.
 *   Listed alleles.  By default j >= 1: string 0 is REF in eds2vcf's convention, and for a biallelic site its r2 equals
 *      that of string 1; all_strings != 0 lists j = 0 too.  An allele is listed iff min_count <= count <= present -
 *      min_count; min_count = 0 lists everything, zero counts included.  Listed alleles are numbered 0..A-1 in (r, j)
 *      order.  Equal texts are not merged, the convention of eds2gfa, eds2vcf and the distances.
 *   Candidate pairs.  Listed alleles x = (r, j) and y = (r', j') with r < r' <= r + window.  window counts choice symbols
 *      and must be >= 1: window == 0 is EDSX_ERR_INVALID_PARAMETER.  Two alleles of one symbol are never a pair.
 *   Counts of a pair, over the paths present at both symbols: n = |U(r) & U(r')|, n_a = |T(x) & U(r')|, n_b = |T(y) & U(r)|,
 *      n_ab = |T(x) & T(y)|.  Where neither symbol leaves a path of M without a string these are K, count(x), count(y).
 *   r2.  With da = n_a (n - n_a), db = n_b (n - n_b) and D = n n_ab - n_a n_b (signed 64-bit): a pair with da db == 0 is
 *      undefined; it is never reported and is counted in info.undefined_pairs.  Otherwise
 *      r2 = ((double)D / (double)da) * ((double)D / (double)db), computed in exactly this form: with P <= 9 999 999 all
 *      three integers are below 2^53, so the value is two correctly rounded divisions and one multiplication.
 *   Filter and order.  A pair is reported iff r2 >= min_r2; min_r2 must lie in [0, 1], NaN or a value outside is
 *      EDSX_ERR_INVALID_PARAMETER.  Pairs come back in (x, y) order: ascending symbol_a, string_a, symbol_b, string_b.
 *   Output.  pairs: edsx_ld_pair records; alleles (may be NULL): the A listed alleles as edsx_ld_allele; both are
 *      edsx_buf, freed by edsx_buf_free.  symbol is the index among all symbols, as in locate and lift, string the index
 *      within the symbol.  info (may be NULL), filled in as far as the call got, on errors too:
 *      paths K, choice_symbols nc, alleles A, candidate_pairs the sum over x of its partners in the band (a closed form),
 *      undefined_pairs, pairs the reported ones, row_words ceil(P / 64), tiles the 64 x 64 allele tiles of the band.
 *   Limits.  max_pairs (0: none) is held against the counted number of reported pairs before the pair buffer is
 *      allocated: EDSX_ERR_INVALID_PARAMETER, "LD has <n> pairs, above the limit of <max>".  The allele rows (A * row_words
 *      * 8 bytes) and the presence rows must fit the session's budget: otherwise EDSX_ERR_BUILD_FAILED, with the sizes
 *      and the budget in the text.  An EDS without choice symbols, A = 0 or K = 0 gives empty buffers and status 0.  Every
 *      error leaves the session usable.
 * edsx_paths_last_timing: scan_ms the allele list and the tile list (and the scan between the pair passes), copy_ms the
 * rows and both pair passes, bytes_written the pairs and the alleles; under edsx_set_timing the kernels come back by name
 * from edsx_get_timing. */
typedef struct { uint64_t symbol_a, string_a, symbol_b, string_b, n_ab, n_a, n_b, n; double r2; } edsx_ld_pair;
typedef struct { uint64_t symbol, string, count, present; } edsx_ld_allele;
typedef struct { uint64_t window; double min_r2; uint64_t min_count; int all_strings; uint64_t max_pairs; } edsx_ld_opts;
typedef struct { uint64_t paths, choice_symbols, alleles, candidate_pairs, undefined_pairs, pairs, row_words, tiles; } edsx_ld_info;
int edsx_paths_ld(edsx_paths_session* s, const uint64_t* ids, size_t n, const edsx_ld_opts* opts, edsx_buf* pairs,
                  edsx_buf* alleles, edsx_ld_info* info);
/* open + ld + close */
int edsx_eds_ld(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size, const uint64_t* ids,
                size_t n, const edsx_ld_opts* opts, edsx_buf* pairs, edsx_buf* alleles, edsx_ld_info* info);

/* ---- edsparser-ibs: the segments two paths of an EDS with sources share (ibs_device.hip, ibs_core.hpp) ----
 * Input: a path session and n path ids in request order; n == 0 means all paths 1..P; duplicates are allowed, as in
 * edsx_paths_distances; K is the number of requested paths.  An id of 0 or above P is EDSX_ERR_INVALID_PARAMETER, "Path id
 * <p> out of range (1..<P>)".  Pairs are the request positions x < y, K (K - 1) / 2 of them.
 *   Agreement.  chosen(p, i) is the session's rule: the first string of symbol i, in file order, whose source set holds p
 *      or 0.  Two paths agree at symbol i iff they take the same string index there; two paths without a string agree.
 *      Equal texts are not merged, the convention of the `strings` distances, eds2gfa and eds2vcf.  A symbol that is a
 *      single universal string is fixed: all paths agree there.
 *   Segment.  A segment of a pair is a maximal non-empty interval of symbols [symbol_first, symbol_last] at all of which
 *      the two paths agree: it is bounded on each side by a symbol where they differ or by an end of the EDS.  Two
 *      adjacent differing symbols have no segment between them.  A pair that never differs, and every pair of an EDS
 *      without choice symbols, has the one segment [0, n - 1].
 *   Record (edsx_ibs_segment).  x, y: the request positions; symbol_first, symbol_last; sites: the choice symbols
 *      (n_choice_symbols of edsx_paths_info counts them) inside the interval, may be 0; column_first, column_end: the
 *      interval's columns in the view of edsx_paths_align, col[symbol_first] and col[symbol_last + 1], may be equal.
 *   Reporting rule.  A segment is reported iff sites >= min_sites and column_end - column_first >= min_columns; with
 *      0, 0 every segment is reported (the tools and the Python call default to 1, 0).
 *   Order.  By (x, y), then symbol_first.
 *   Output.  segments: an edsx_buf of records, freed by edsx_buf_free.  pair_off: an edsx_buf of K (K - 1) / 2 + 1
 *      uint64_t, a CSR over the pairs in row-major upper-triangle order ((0,1), (0,2), .., (1,2), ..): the records of pair
 *      q are [pair_off[q], pair_off[q + 1]).  info (may be NULL), filled in as far as the call got, on errors too: paths
 *      K, choice_symbols, class_columns and chunk_columns and chunks of the `strings` class list as edsx_dist_info names
 *      them, pairs, candidate_segments (the segments before the thresholds), segments (the reported ones).
 *   Limits.  max_segments (0: none) is held against the counted number of reported segments before the records are
 *      allocated: EDSX_ERR_INVALID_PARAMETER, "IBS has <n> segments, above the limit of <max>".  The bit rows, the
 *      per-(pair, chunk) scratch and the records must fit the session's budget: otherwise EDSX_ERR_BUILD_FAILED, with the
 *      sizes and the budget in the text and "request fewer paths at a time".  K < 2 gives no record and pair_off = {0}.
 *      Every error leaves the session usable.
 * edsx_paths_last_timing: choose_ms the choice tables, scan_ms the class list, the stitch passes and the scan between
 * them, copy_ms the bit rows and both scan passes, bytes_written the records and pair_off; under edsx_set_timing the
 * kernels come back by name from edsx_get_timing. */
typedef struct { uint64_t x, y, symbol_first, symbol_last, sites, column_first, column_end; } edsx_ibs_segment;
typedef struct { uint64_t paths, choice_symbols, class_columns, chunk_columns, chunks, pairs, candidate_segments, segments; } edsx_ibs_info;
int edsx_paths_ibs(edsx_paths_session* s, const uint64_t* ids, size_t n, uint64_t min_sites, uint64_t min_columns,
                   uint64_t max_segments, edsx_buf* segments, edsx_buf* pair_off, edsx_ibs_info* info);
/* open + ibs + close */
int edsx_eds_ibs(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size, const uint64_t* ids,
                 size_t n, uint64_t min_sites, uint64_t min_columns, uint64_t max_segments, edsx_buf* segments, edsx_buf* pair_off,
                 edsx_ibs_info* info);

/* ---- edsparser-mosaic: a path of an EDS with sources as a minimal mosaic of other paths (mosaic_device.hip, mosaic_core.hpp) ----
 * Input: a path session and two id lists.  targets: nt path ids in request order, duplicates allowed; nt == 0 means all
 * paths 1..P; T is the number of requested targets.  donors: nd ids likewise, nd == 0 means all paths 1..P; D is the number
 * of requested donors.  An id of 0 or above P in either list is EDSX_ERR_INVALID_PARAMETER, "Path id <p> out of range
 * (1..<P>)".  Targets and donors are named by their request positions x and y.
 *   Agreement.  chosen(p, i) and "agree at symbol i" are those of edsx_paths_ibs: two paths agree iff they take the same
 *      string index; two paths without a string agree; equal texts are not merged; at a fixed symbol all paths agree.
 *   Eligibility.  For the target position x with path id t a donor position y is eligible iff donors[y] != t (leave one
 *      out: with both lists empty every path is written in terms of all the others).
 *   Mosaic of a target, n the number of symbols.  Start at s = 0 and repeat while s < n.  For every eligible y let e(y) be
 *      the first symbol i >= s at which t and donors[y] differ, n without one, and best = max e(y).  If an eligible donor
 *      exists and best > s: a copied segment [s, best - 1] whose donor is the smallest eligible y with e(y) = best; s =
 *      best.  Otherwise a private segment [s, j - 1], j the first symbol > s at which some eligible donor agrees with t,
 *      or n; its donor is UINT64_MAX; s = j.  Without an eligible donor the whole EDS is one private segment; n = 0 gives
 *      no record.  The segments of a target tile [0, n - 1] without gaps or overlaps, and no way of writing t as copies
 *      from single donors plus the symbols no donor shares has fewer pieces: reaching furthest is optimal.
 *   Record (edsx_mosaic_segment).  target: x; donor: y or UINT64_MAX; symbol_first, symbol_last; sites, column_first,
 *      column_end as in edsx_ibs_segment: the choice symbols inside, col[symbol_first] and col[symbol_last + 1].
 *   Order.  By target, then symbol_first.
 *   Output.  segments: an edsx_buf of records, freed by edsx_buf_free.  target_off: an edsx_buf of T + 1 uint64_t, the CSR
 *      over the targets.  info (may be NULL), filled in as far as the call got, on errors too: targets T, donors D,
 *      choice_symbols, class_columns of the `strings` class list, segments, private_segments, private_symbols (the
 *      symbols inside private segments), switches (the sum over the targets of segments - 1).
 *   Limits.  max_segments (0: none) is held against the counted number of segments before the records are allocated:
 *      EDSX_ERR_INVALID_PARAMETER, "Mosaic has <n> segments, above the limit of <max>".  The bit rows of the distinct
 *      requested paths, the donor scratch and the records must fit the session's budget: otherwise EDSX_ERR_BUILD_FAILED,
 *      with the sizes and the budget in the text and "request fewer paths at a time".  Every error leaves the session
 *      usable.
 * edsx_paths_last_timing: choose_ms the choice tables, scan_ms the class list and the scan of the counts, copy_ms the bit
 * rows, the donor transpose and both passes of the march, bytes_written the records and target_off; under edsx_set_timing
 * the kernels come back by name from edsx_get_timing. */
typedef struct { uint64_t target, donor, symbol_first, symbol_last, sites, column_first, column_end; } edsx_mosaic_segment;
typedef struct { uint64_t targets, donors, choice_symbols, class_columns, segments, private_segments, private_symbols, switches; } edsx_mosaic_info;
int edsx_paths_mosaic(edsx_paths_session* s, const uint64_t* targets, size_t nt, const uint64_t* donors, size_t nd,
                      uint64_t max_segments, edsx_buf* segments, edsx_buf* target_off, edsx_mosaic_info* info);
/* open + mosaic + close */
int edsx_eds_mosaic(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size, const uint64_t* targets,
                    size_t nt, const uint64_t* donors, size_t nd, uint64_t max_segments, edsx_buf* segments, edsx_buf* target_off,
                    edsx_mosaic_info* info);

/* ---- edsparser-diversity: windowed diversity within and between groups of paths (div_device.hip, div_core.hpp) ----
 * Input: a path session and G >= 1 groups of path ids as a CSR: group g holds group_ids[group_off[g] .. group_off[g + 1]);
 * n_groups == 0 means one group of all paths 1..P.  A duplicate id inside a group counts once; M_g is the set of group g and
 * K_g = |M_g|.  All of the following are EDSX_ERR_INVALID_PARAMETER: an id of 0 or above P, "Path id <p> out of range
 * (1..<P>)"; an empty group, "Group <g> is empty"; an id in two groups, "Path id <p> is in groups <a> and <b>", for the
 * lowest such p and its two lowest groups; more than EDSX_DIV_MAX_GROUPS groups.  Group pairs are (g, h) with g <= h in
 * row-major order, NP = G (G + 1) / 2 of them.
 *   Per choice symbol.  The choice symbols r = 0..nc-1 and the carrier rule are those of edsx_paths_ld: T(r, j) is the set
 *      of paths that take string j of r, the first string in file order whose source set holds the path or 0; equal texts
 *      are not merged.  c_g(r, j) = |T(r, j) & M_g| and n_g(r) = sum_j c_g(r, j).
 *      comp_gh(r): the pairs (p in M_g, q in M_h) that both take a string at r; unordered with p != q when g == h.
 *      diff_gh(r): those of them whose string indices differ.
 *      seg_g(r) = 1 iff at least two strings of r have a carrier in M_g.  present_g(r) = n_g(r).
 *      (Closed forms: between groups comp = n_g n_h and diff = n_g n_h - sum_j c_gj c_hj; within a group comp =
 *      n_g (n_g - 1) / 2 and diff = (n_g^2 - sum_j c_gj^2) / 2.)
 *   Windows.  unit EDSX_DIV_SYMBOLS: the coordinate of r is r and the extent E = nc.  EDSX_DIV_COLUMNS: the coordinate is
 *      min(col[i], E - 1), i the symbol index of r, col the first column of a symbol in the view of edsx_paths_align, W its
 *      number of columns and E = max(W, 1).  Window k covers the coordinates [k step, min(k step + size, E)) for every k
 *      with k step < E; step == 0 means step = size; size == 0 means the one window [0, E).  A window without a choice
 *      symbol is still a record, with zero sums.  nc = 0 gives empty buffers and status 0.  max_windows (0: none) is held
 *      against the window count before anything is allocated: "Diversity has <n> windows, above the limit of <max>".
 *   Output, all edsx_buf, sized exactly, freed by edsx_buf_free.  windows: NW edsx_div_window, rank_first and rank_end the
 *      choice symbols [rank_first, rank_end) of the window.  groups: NW x G edsx_div_group.  pairs: NW x NP edsx_div_pair.
 *      Every field is the sum over the window's choice symbols.  sfs (may be NULL): sum over g of (K_g + 1) uint64_t, group
 *      after group; sfs[g][c] is the number of (r, j >= 1) over ALL choice symbols with n_g(r) = K_g and c_g(r, j) = c: the
 *      unfolded spectrum against string 0 on complete sites, bin 0 kept.  info (may be NULL), filled in as far as the call
 *      got, on errors too: groups G, paths sum K_g, choice_symbols nc, windows NW, pairs NP, row_words ceil(P / 64), extent E.
 *   Limits.  The NA = 2 G + 2 NP sums the device keeps per choice symbol (8 NA (nc + 1) bytes), the records and, above
 *      8192 paths, the walk rows must fit the session's budget: otherwise EDSX_ERR_BUILD_FAILED, with the sizes and the
 *      budget in the text; slabs of the symbol range are not built.  nc max_g K_g^2 >= 2^63 is refused the same way: the
 *      sums are 64-bit.  Every error leaves the session usable.
 *   Derived statistics (pi, d_xy, F_ST, Watterson's theta, Tajima's D) are host arithmetic over these integers:
 *      edsparser_amd/host/div_stats.hpp.
 * edsx_paths_last_timing: copy_ms the k_div_sites launches, scan_ms the scans and the window kernel, bytes_written the
 * records and the spectrum; under edsx_set_timing the kernels come back by name from edsx_get_timing. */
#define EDSX_DIV_SYMBOLS 0
#define EDSX_DIV_COLUMNS 1
#define EDSX_DIV_MAX_GROUPS 16
typedef struct { int unit; uint64_t size, step, max_windows; } edsx_div_opts;
typedef struct { uint64_t groups, paths, choice_symbols, windows, pairs, row_words, extent; } edsx_div_info;
typedef struct { uint64_t start, end, rank_first, rank_end; } edsx_div_window;
typedef struct { uint64_t segregating, present; } edsx_div_group;
typedef struct { uint64_t diff, comp; } edsx_div_pair;
int edsx_paths_diversity(edsx_paths_session* s, const uint64_t* group_off, const uint64_t* group_ids, size_t n_groups,
                         const edsx_div_opts* opts, edsx_buf* windows, edsx_buf* groups, edsx_buf* pairs, edsx_buf* sfs,
                         edsx_div_info* info);
/* open + diversity + close */
int edsx_eds_diversity(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                       const uint64_t* group_off, const uint64_t* group_ids, size_t n_groups, const edsx_div_opts* opts,
                       edsx_buf* windows, edsx_buf* groups, edsx_buf* pairs, edsx_buf* sfs, edsx_div_info* info);

/* ---- edsparser-subset: an EDS with sources restricted to a keep set K of its paths (subset_device.hip) ----
 * Input: an .eds + .seds, parsed exactly as edsx_paths_open parses them (same tokenisers, statuses and error texts), and
 * n path ids, the keep set K.  P is the largest path id in the .seds.
 *   1. Strings.  String j has the source set S_j.  If S_j holds 0 the string is kept and stays universal.  Otherwise
 *      S'_j = S_j & K, and the string is kept iff S'_j is not empty.  File order is kept; equal texts are not merged.
 *   2. Symbols.  A symbol without a kept string is removed (no kept path took a string there).  A symbol with exactly
 *      one kept string whose set is universal or holds all of K is COMMON: its set becomes {0}.  A symbol with one kept
 *      string whose set does not hold all of K stays a one-string symbol with its explicit set ({0} would hand the string
 *      to paths that had none there).  Sets inside symbols with several kept strings are never rewritten to {0}, not
 *      even when they equal K.
 *   3. Runs.  After the removals, every maximal run of adjacent common symbols is concatenated into one symbol with the
 *      set {0}; removed symbols between two commons do not break a run.  A run whose concatenation is empty is dropped.
 *   Ids.  Path p of K becomes its 1-based rank in ascending K (ids stay dense), or stays p with keep_ids != 0.
 *   Output.  The .eds is always in FULL form - braces around every symbol - followed by '\n', as EDS::save writes it;
 *      the .seds has one "{ids}" per kept string, ids ascending, followed by '\n'.  There is no compact form: a
 *      one-string symbol with an explicit set, printed without braces, would fuse with its neighbours when read back and
 *      no longer match its .seds in cardinality.  When every symbol is dropped both texts are "\n".
 *   Invariant.  For every p of K, the sequence edsx_paths_spell spells for p's new id in the output equals the sequence
 *      it spells for p in the input; missing[p] can only decrease (removed symbols no longer count).
 * info (may be NULL): symbols_removed counts the symbols of step 2; common_runs_merged the runs of step 3 that were
 * formed from two or more symbols (dropped ones included).
 * Errors, all EDSX_ERR_INVALID_PARAMETER: seds == NULL "Path subsetting needs sources (.seds)"; n == 0 "No paths
 * selected"; an id of 0 or above P "Path id <p> out of range (1..<P>)"; an id listed twice "Path id <p> given twice".
 * The call tokenises into the context's own tables, like edsx_eds_stats: path sessions are not touched. */
typedef struct { uint64_t symbols_in, symbols_out, strings_in, strings_out, chars_in, chars_out,
                 paths_in /* P */, paths_out /* |K| */, symbols_removed, common_runs_merged; } edsx_subset_info;
int edsx_eds_subset(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                    const uint64_t* ids, size_t n, int keep_ids, edsx_buf* eds_out, edsx_buf* seds_out,
                    edsx_subset_info* info);

/* ---- eds2gfa: an EDS and its paths as a GFA 1.0 graph (gfa_device.hip, path_device.hip) ----
 * The text is, in this order: the header line "H\tVN:Z:1.0", all S lines, all L lines, all P lines; fields are separated
 * by a tab and every line ends with '\n'.  The .eds (+ .seds) is parsed exactly as edsx_leds_merge / edsx_paths_open
 * parse it (same tokenisers, statuses and error texts).
 *   Segments.  "S\t<id>\t<sequence>": every non-empty string of the EDS is one segment, in file order; its id is its
 *      1-based rank among the non-empty strings, in decimal.  Equal texts are not merged, the bytes are copied verbatim,
 *      and an empty string is no segment (GFA has no sequence of length 0).
 *   Links.  "L\t<u>\t+\t<v>\t+\t0M": a symbol is OPEN when it has an empty string.  For i < j every segment of symbol i is
 *      linked to every segment of symbol j iff every symbol k with i < k < j is open: the links of symbol i reach
 *      i + 1, i + 2, ... up to and including the first symbol that is not open, or the last symbol.  Lines are ordered
 *      by (u, v) ascending.  The links follow the language of the EDS, with or without sources: they are not restricted to
 *      the pairs some path uses.  The sequences spelled by the walks that start at a segment with only open symbols in
 *      front of it and end at one with only open symbols behind it are the language of the EDS (less the empty word).
 *   Paths.  "P\t<name>\t<id>+,<id>+,...\t*": the segment ids of the non-empty chosen strings of path p (chosen as
 *      edsx_paths_spell chooses them) in symbol order.  steps[k] is the number of ids and missing[k] is as in
 *      edsx_paths_spell; a path with steps == 0 gets no line (GFA has no empty path).  With missing[k] == 0 every
 *      consecutive pair of the line is a link; with missing[k] > 0 a pair may not be one - the line is written all the
 *      same.  Names as in edsx_paths_spell: names[k], else prefix (NULL: "path") + id.  A name that is empty or holds a
 *      tab, line feed or blank: EDSX_ERR_INVALID_PARAMETER, "Path name <k> is not a GFA name" (k: its place in the
 *      request, from 0).
 *   Limits.  max_links (0: 2^32) caps the number of links; more is EDSX_ERR_INVALID_PARAMETER, "Graph has <n> links,
 *      above the limit of <cap>", raised from the counts before the text is allocated (info is filled in): a long run of
 *      open symbols with many strings each is quadratic by nature.  All offsets and counts are 64-bit; 2^32 strings or
 *      more are EDSX_ERR_BUILD_FAILED.  An EDS without a non-empty string gives the header line alone.
 * edsx_eds_gfa_graph tokenises into the context's own tables, like edsx_eds_stats: path sessions are not touched. */
typedef struct { uint64_t n_symbols, n_strings, n_segments, n_empty_strings, n_open_symbols, n_links,
                 header_bytes, segment_bytes, link_bytes; int tokenised_on_device; } edsx_gfa_info;
/* H + S + L; sources are not needed */
int edsx_eds_gfa_graph(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, uint64_t max_links, edsx_buf* gfa,
                       edsx_gfa_info* info);
/* P lines of the requested paths in request order (n == 0: all paths 1..P); missing, steps: may be NULL, one per id */
int edsx_paths_gfa_walks(edsx_paths_session* s, const uint64_t* ids, size_t n, const char* const* names, const char* prefix,
                         edsx_buf* lines, uint64_t* missing, uint64_t* steps);
/* graph + walks of all paths when seds != NULL, the graph alone otherwise */
int edsx_eds_gfa(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                 uint64_t max_links, const char* prefix, edsx_buf* gfa, edsx_gfa_info* info);

/* ---- eds2vcf: an EDS and its sources as VCF 4.2 text plus the reference FASTA (vcf_export_device.hip) ----
 * The .eds (+ .seds) is parsed exactly as edsx_eds_gfa / edsx_paths_open parse it (same tokenisers, statuses and error
 * texts).  n symbols, numbered from 0; P is the largest path id in the .seds.
 *   Reference allele of symbol i.  ref_path == 0: the first string in file order (where vcf2eds puts REF).  ref_path ==
 *      p >= 1: the string path p takes under the rule of edsx_paths_spell, the first string whose set holds p or 0; a
 *      symbol where p takes none is EDSX_ERR_INVALID_PARAMETER, "Path <p> takes no string of symbol <i>" (the first such
 *      i).  p > P: EDSX_ERR_INVALID_PARAMETER, "Path id <p> out of range (1..<P>)"; p without a .seds:
 *      EDSX_ERR_INVALID_PARAMETER, "A reference path needs sources (.seds)".
 *   Reference sequence.  The reference strings end to end, length L; refpos[i] is the sum of their lengths before i.
 *   Records.  One per symbol with two strings or more, in symbol order; a one-string symbol gives none.  Allele 0 is the
 *      reference string, the other strings follow in file order as alleles 1..k-1.  Equal texts are not merged and
 *      nothing is trimmed, as in eds2gfa.
 *   Anchor.  A record with an empty string is anchored.  If refpos[i] > 0 every allele gets the reference base at 0-based
 *      refpos[i] - 1 in front, and POS = refpos[i].  Otherwise every allele gets, behind it, the reference base that follows
 *      the symbol's reference string, and POS = 1; when there is no such base (the reference ends with this symbol's
 *      reference string) the call is EDSX_ERR_INVALID_FORMAT, "Symbol <i> has an empty string and no reference base to
 *      anchor it".  A record without an empty string: POS = refpos[i] + 1, alleles verbatim.
 *   Line.  CHROM \t POS \t . \t REF \t ALT1,ALT2,... \t . \t . \t .   and, with sources, \t GT and one cell per path 1..P,
 *      each behind a tab.  The cell of path p holds the numbers of the alleles whose set holds p or 0, ascending, joined
 *      by '/' (an .seds has no phase); no allele at all gives ".".
 *   Header.  "##fileformat=VCFv4.2", "##source=eds2vcf", "##contig=<ID=<chrom>,length=<L>>", with sources
 *      "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">", then the tab-separated "#CHROM POS ID REF ALT QUAL
 *      FILTER INFO" line, with sources followed by FORMAT and the sample names: names[k] for path k + 1 when names is
 *      given (n_names must be P: "Expected <P> sample names, got <n>"), else prefix (NULL: "path") + id, as
 *      edsx_paths_spell names its records.  A name that is empty or holds a tab or line feed: "Sample name <k> is not a
 *      VCF sample name".  chrom NULL: "eds"; empty or holding whitespace: "Chromosome name is empty or holds whitespace".
 *      All three are EDSX_ERR_INVALID_PARAMETER.
 *   Reference FASTA (ref_fasta may be NULL).  ">" chrom "\n", then the reference sequence in lines of line_width
 *      characters, each ended by '\n' (0: one line; an empty sequence has no line): for ref_path = p the body edsx_paths_spell
 *      gives for p.
 *   info (may be NULL).  anchored: records with an anchor base.  overlapping: records whose POS is not behind the last
 *      reference base of the record before them, which anchoring next to another degenerate symbol can cause.
 *   max_bytes.  0: no limit beyond what can be allocated.  The body (all record lines) is sized exactly from scanned counts
 *      before it is allocated; a body above the limit is EDSX_ERR_BUILD_FAILED, "VCF body of <n> bytes is above the limit
 *      of <max>", with info filled in.  There is no path selection: edsx_eds_subset does that and renumbers densely.
 * opts == NULL: all defaults (line_width 60).  A zeroed opts differs from that only in line_width 0.
 * The call tokenises into the context's own tables, like edsx_eds_stats: path sessions are not touched. */
typedef struct {
    const char* chrom;              /* NULL: "eds" */
    uint64_t ref_path;              /* 0: the first string of every symbol */
    const char* const* names;       /* NULL, or n_names sample names */
    size_t n_names;
    const char* prefix;             /* NULL: "path" */
    uint64_t line_width;            /* of the reference FASTA; 0: one line */
    uint64_t max_bytes;             /* 0: no limit */
} edsx_vcf_export_opts;
typedef struct { uint64_t symbols, strings, paths, records, anchored, overlapping, ref_length, header_bytes, body_bytes;
                 int tokenised_on_device; } edsx_vcf_export_info;
int edsx_eds_vcf(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size,
                 const edsx_vcf_export_opts* opts, edsx_buf* vcf, edsx_buf* ref_fasta, edsx_vcf_export_info* info);

/* ---- eds2msa: the paths of an EDS with sources as the rows of one alignment (path_device.hip) ----
 * Input: an .eds + .seds, parsed exactly as edsx_paths_open parses them; n symbols, P the largest path id.
 *   Width.  w[i] is the length of the longest string of symbol i - over all its strings, not over those the requested
 *      paths take - col[i] the exclusive prefix sum of w, W = sum w[i].  Widths do not depend on the request, so rows
 *      written by separate calls stack into one alignment.
 *   Row of path p.  Symbol i occupies columns col[i] .. col[i] + w[i] - 1 and holds the string edsx_paths_spell chooses
 *      for p there, left-justified and filled up with the gap byte; a symbol at which p has no string is w[i] gap bytes
 *      and counts in missing.  Every row has exactly W characters; a symbol of width 0 occupies no column.
 *   Text.  FASTA, one record per requested path in request order (n == 0: all paths 1..P); headers, names and prefix as
 *      in edsx_paths_spell; the row in lines of line_width characters, each ended by '\n' (0: one line; W == 0: no line).
 *   Gap byte.  gap == 0 means '-'; otherwise any byte value except '>', '\n', '\r', blank, '{', '}' and ',' - anything
 *      else is EDSX_ERR_INVALID_PARAMETER, "Gap character is not usable in an alignment".  Strings are copied verbatim: a
 *      string that itself holds the gap byte is the caller's business.
 *   Limit.  max_bytes == 0: none; a larger text is EDSX_ERR_INVALID_PARAMETER, "Alignment has <n> bytes, above the limit
 *      of <cap>", raised from the counts before anything is allocated for the text (an alignment is P x W bytes however
 *      small the EDS is).
 *   Errors.  Path ids, a missing .seds and names give the statuses and texts of edsx_paths_spell.
 * The column table (8 bytes per symbol) is made by the first of these calls on a session and kept until it closes. */
typedef struct { uint64_t n_symbols, n_columns /* W */, n_zero_width_symbols, widest_symbol, num_paths; } edsx_align_info;
int edsx_paths_align_info(edsx_paths_session* s, edsx_align_info* out);
/* missing (may be NULL): one count per record */
int edsx_paths_align(edsx_paths_session* s, const uint64_t* ids, size_t n, const char* const* names, const char* prefix,
                     uint64_t line_width, int gap, uint64_t max_bytes, edsx_buf* fasta, uint64_t* missing);
/* open + align + close; info (may be NULL) is filled as soon as the column table is known, so also when the limit refuses */
int edsx_eds_msa(edsx_ctx* ctx, const uint8_t* eds, size_t eds_size, const uint8_t* seds, size_t seds_size, const uint64_t* ids,
                 size_t n, const char* const* names, const char* prefix, uint64_t line_width, int gap, uint64_t max_bytes,
                 edsx_buf* fasta, uint64_t* missing, edsx_align_info* info);

/* Per-kernel device time, measured with HIP events on the stream each kernel is launched on and
 * accumulated over all plan/emit calls (and edsx_eds_subset / edsx_eds_gfa_graph / edsx_eds_vcf calls) since edsx_set_timing(ctx, 1).  Arrays of capacity cap;
 * total_ms[i] / launches[i] is the average duration of kernel names[i].  Returns the entry count. */
void edsx_set_timing(edsx_ctx* ctx, int enabled);
int  edsx_get_timing(edsx_ctx* ctx, const char** names, float* total_ms, int* launches, int cap);

/* ---- synthetic VCF + FASTA of BASELINE configs[3]'s shape, generated in HBM ----
 * One FASTA record of ref_len uniform ACGT bases in 60-column lines; n_records record lines with strictly ascending
 * POS, 70 % SNP / 15 % insertion of 1..10 bases / 15 % deletion of 1..10 bases (REF spans them: a few per cent of the
 * records overlap the next one), n_samples diploid phased samples, each allele ALT with p = 0.3.  Counter-based: the
 * text depends on the parameters only.  Needs ref_len >= 64 and n_records <= ref_len / 16. */
int edsx_genvcf(edsx_ctx* ctx, uint64_t ref_len, uint64_t n_records, uint32_t n_samples, uint64_t seed,
                edsx_buf* vcf, edsx_buf* fasta);

/* ---- synthetic genrandomeds-shaped alignment, generated in HBM (bench / tests) ----
 * Rows 0..n_rows-1 of alignment columns [col0, col0+n_cols) of a virtual alignment, one line per
 * row, headers ">s<row>", trailing newline.  Bytes depend only on (seed, global column, row), so a
 * column slab generated on another GPU is bit-identical to the same columns of the whole.
 * Both generators write exactly the bytes [d_out, d_out + size) - every one of them, none outside, d_out at any byte
 * address - asynchronously on `stream`; a capacity below the size is EDSX_ERR_INVALID_PARAMETER and writes nothing. */
size_t edsx_msa_synth_size(uint32_t n_rows, uint64_t n_cols);
int edsx_msa_synth_device(edsx_ctx* ctx, uint8_t* d_out, size_t capacity, uint32_t n_rows,
                          uint64_t col0, uint64_t n_cols, double variant_fraction, uint64_t seed,
                          void* stream, size_t* written);
/* The same alignment with every header padded with blanks (">s<row>    ...") so that each row's first column lies a
 * multiple of row_align bytes (a power of two, e.g. 128) from the start of the image: the layout an upload that places
 * the rows for the column scan produces.  row_align <= 1: the plain image above.  Same cells, same outputs. */
size_t edsx_msa_synth_size_aligned(uint32_t n_rows, uint64_t n_cols, uint32_t row_align);
int edsx_msa_synth_device_aligned(edsx_ctx* ctx, uint8_t* d_out, size_t capacity, uint32_t n_rows, uint64_t col0, uint64_t n_cols,
                                  double variant_fraction, uint64_t seed, uint32_t row_align, void* stream, size_t* written);

#ifdef __cplusplus
}
#endif
#endif /* EDSX_H */
