"""ctypes bindings of include/edsx.h."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

STATUS = {0: "OK", 1: "FILE_NOT_FOUND", 2: "INVALID_FORMAT", 3: "INVALID_PARAMETER",
          4: "BUILD_FAILED", 5: "QUERY_FAILED", 99: "UNKNOWN_ERROR"}


class EdsxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (STATUS.get(code, code), msg))
        self.code = code
        self.message = msg


class _Buf(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("size", ctypes.c_size_t)]


class VcfStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in
                ("total_variants", "processed_variants", "skipped_malformed",
                 "skipped_unsupported_sv", "variant_groups")]


class Contig(ctypes.Structure):
    """One FASTA record of a VcfSession (edsx_contig)."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("name_off", "name_len", "rec_start", "rec_end", "seq_start", "line_width",
                                                "seq_size", "vcf_records", "duplicate")]


class BgzfBlock(ctypes.Structure):
    _fields_ = [("comp_off", ctypes.c_uint64), ("out_off", ctypes.c_uint64), ("comp_len", ctypes.c_uint32), ("isize", ctypes.c_uint32)]


class GzInfo(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("inflated_on_device", ctypes.c_int)] + \
               [(n, ctypes.c_uint64) for n in ("blocks", "comp_bytes", "text_bytes", "h2d_bytes", "text_d2h_bytes")] + \
               [(n, ctypes.c_double) for n in ("index_ms", "inflate_ms", "crc_ms")]


class VcfSessionStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("records_total", "records_without_token", "records_unknown_contig",
                                                "vcf_h2d_bytes", "fasta_h2d_bytes")] + [("classified_on_device", ctypes.c_int)]


class VcfMultiInfo(ctypes.Structure):
    _fields_ = [("partitioned", ctypes.c_int), ("fasta_windowed", ctypes.c_int)] + \
               [(n, ctypes.c_uint64) for n in ("records_min", "records_max", "moved_line_bytes", "fasta_h2d_bytes_max")]


class MergeMultiInfo(ctypes.Structure):
    _fields_ = [("partitioned", ctypes.c_int), ("ranges", ctypes.c_int), ("fallback", ctypes.c_int)] + \
               [(n, ctypes.c_uint64) for n in ("range_bytes_min", "range_bytes_max", "eds_h2d_bytes_max", "seds_h2d_bytes_max")]


class EdsRangeScan(ctypes.Structure):
    _fields_ = [("ok", ctypes.c_int), ("strings", ctypes.c_uint64), ("has_cut", ctypes.c_int),
                ("sym_start", ctypes.c_uint64), ("sym_end", ctypes.c_uint64), ("strings_before", ctypes.c_uint64)]


class EdsStatistics(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("n_symbols", "n_chars", "n_strings", "num_degenerate_symbols",
                                                "total_change_size", "num_common_chars", "num_empty_strings",
                                                "min_context_length", "max_context_length", "num_context_blocks")] +
                [("avg_context_length", ctypes.c_double)] +
                [(n, ctypes.c_uint64) for n in ("has_sources", "num_paths", "max_paths_per_string", "total_paths")] +
                [("avg_paths_per_string", ctypes.c_double), ("is_leds", ctypes.c_int)])


class QueryInfo(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("n_symbols", "n_strings", "n_chars", "num_common_chars", "num_degenerate_strings")] +
                [(n, ctypes.c_double) for n in ("tokenise_ms", "tables_ms", "kernel_ms", "download_ms")])


class PathsInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("n_symbols", "n_strings", "n_chars", "num_paths", "n_choice_symbols")] + \
               [("tokenised_on_device", ctypes.c_int)]


class PathsTiming(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ("tokenise_ms", "choose_ms", "scan_ms", "copy_ms", "download_ms")] + \
               [("bytes_written", ctypes.c_uint64)]


class AlignInfo(ctypes.Structure):
    """edsx_align_info"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("n_symbols", "n_columns", "n_zero_width_symbols", "widest_symbol", "num_paths")]


class DistInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("units", "variable_units", "class_columns", "chunk_columns", "chunks")]


class LdInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("paths", "choice_symbols", "alleles", "candidate_pairs", "undefined_pairs", "pairs",
                                                "row_words", "tiles")]


class LdOpts(ctypes.Structure):
    _fields_ = [("window", ctypes.c_uint64), ("min_r2", ctypes.c_double), ("min_count", ctypes.c_uint64), ("all_strings", ctypes.c_int),
                ("max_pairs", ctypes.c_uint64)]


class IbsInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("paths", "choice_symbols", "class_columns", "chunk_columns", "chunks", "pairs",
                                                "candidate_segments", "segments")]


class MosaicInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("targets", "donors", "choice_symbols", "class_columns", "segments", "private_segments",
                                                "private_symbols", "switches")]


class DivInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("groups", "paths", "choice_symbols", "windows", "pairs", "row_words", "extent")]


class DivOpts(ctypes.Structure):
    _fields_ = [("unit", ctypes.c_int), ("size", ctypes.c_uint64), ("step", ctypes.c_uint64), ("max_windows", ctypes.c_uint64)]


class SubsetInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("symbols_in", "symbols_out", "strings_in", "strings_out", "chars_in", "chars_out",
                                                "paths_in", "paths_out", "symbols_removed", "common_runs_merged")]


class GfaInfo(ctypes.Structure):
    """edsx_gfa_info"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("n_symbols", "n_strings", "n_segments", "n_empty_strings", "n_open_symbols",
                                                "n_links", "header_bytes", "segment_bytes", "link_bytes")] + \
               [("tokenised_on_device", ctypes.c_int)]


class VcfExportOpts(ctypes.Structure):
    """edsx_vcf_export_opts"""
    _fields_ = [("chrom", ctypes.c_char_p), ("ref_path", ctypes.c_uint64), ("names", ctypes.POINTER(ctypes.c_char_p)),
                ("n_names", ctypes.c_size_t), ("prefix", ctypes.c_char_p), ("line_width", ctypes.c_uint64),
                ("max_bytes", ctypes.c_uint64)]


class VcfExportInfo(ctypes.Structure):
    """edsx_vcf_export_info"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("symbols", "strings", "paths", "records", "anchored", "overlapping", "ref_length",
                                                "header_bytes", "body_bytes")] + [("tokenised_on_device", ctypes.c_int)]


class MsaInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in
                ("n_rows", "n_cols", "line_width", "n_variant_cols", "n_segments", "msa_bytes",
                 "n_slow_segments")]


class MsaAnchors(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("n_segments", "found", "first_seg", "last_seg", "last_col", "last_eds_bytes",
                                               "last_seds_bytes", "first_end", "first_eds_end", "first_seds_end")]


class MsaEdges(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in
                ("n_segments", "first_is_variant", "first_cols", "first_eds_bytes", "first_seds_bytes",
                 "last_is_variant", "last_cols", "last_eds_bytes", "last_seds_bytes")]


def lib_path():
    return os.environ.get("EDSX_LIB") or os.path.join(_HERE, "libedsx.so")


def load_library():
    """Load libedsx.so; fails loudly when the HIP extension has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # torch bundles its own HIP runtime (same SONAME libamdhip64.so.7): it must be the first one
    # mapped, so that libedsx.so binds to it instead of bringing a second runtime into the process
    import torch  # noqa: F401
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError("libedsx.so is missing: build it with `python -m edsparser_amd.build` "
                          "(there is no CPU fallback)")
    lib = ctypes.CDLL(path)
    P = ctypes.POINTER
    lib.edsx_version.restype = ctypes.c_char_p
    lib.edsx_ctx_create.argtypes = [ctypes.c_int, P(ctypes.c_void_p)]
    lib.edsx_ctx_destroy.argtypes = [ctypes.c_void_p]
    lib.edsx_ctx_destroy.restype = None
    lib.edsx_last_error.argtypes = [ctypes.c_void_p]
    lib.edsx_last_error.restype = ctypes.c_char_p
    lib.edsx_buf_free.argtypes = [P(_Buf)]
    lib.edsx_buf_free.restype = None
    lib.edsx_msa_transform.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32,
                                       P(_Buf), P(_Buf)]
    lib.edsx_msa_last_batches.argtypes = [ctypes.c_void_p]
    lib.edsx_msa_transform_batched.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int,
                                               P(_Buf), P(_Buf), P(ctypes.c_int)]
    lib.edsx_leds_merge.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                    ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int, P(_Buf), P(_Buf)]
    lib.edsx_vcf_transform.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                       ctypes.c_size_t, ctypes.c_uint32, P(_Buf), P(_Buf), P(VcfStats)]
    lib.edsx_eds_stats.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                   ctypes.c_uint32, P(EdsStatistics)]
    lib.edsx_genrandomeds.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32,
                                      ctypes.c_uint32, ctypes.c_double, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64,
                                      P(_Buf), P(_Buf), P(ctypes.c_uint64)]
    lib.edsx_leds_tokenised_on_device.argtypes = [ctypes.c_void_p]
    lib.edsx_vcf_tokenised_on_device.argtypes = [ctypes.c_void_p]
    lib.edsx_vcf_session_open.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                          P(ctypes.c_void_p)]
    lib.edsx_vcf_session_contigs.argtypes = [ctypes.c_void_p, P(P(Contig)), P(ctypes.c_size_t)]
    lib.edsx_vcf_session_find.argtypes = [ctypes.c_void_p, ctypes.c_char_p, P(ctypes.c_size_t)]
    lib.edsx_vcf_session_transform.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, P(_Buf), P(_Buf), P(VcfStats)]
    lib.edsx_vcf_session_info.argtypes = [ctypes.c_void_p, P(VcfSessionStats)]
    lib.edsx_vcf_session_unknown_contigs.argtypes = [ctypes.c_void_p, P(_Buf)]
    lib.edsx_vcf_session_close.argtypes = [ctypes.c_void_p]
    lib.edsx_vcf_session_close.restype = None
    lib.edsx_vcf_transform_contig.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                              ctypes.c_char_p, ctypes.c_uint32, P(_Buf), P(_Buf), P(VcfStats)]
    lib.edsx_gz_probe.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P(ctypes.c_int)]
    lib.edsx_bgzf_index.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P(_Buf), P(ctypes.c_uint64)]
    lib.edsx_gz_inflate.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, P(_Buf)]
    lib.edsx_gz_last_info.argtypes = [ctypes.c_void_p, ctypes.c_int, P(GzInfo)]
    lib.edsx_vcf_transform_z.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                         ctypes.c_char_p, ctypes.c_uint32, P(_Buf), P(_Buf), P(VcfStats)]
    lib.edsx_vcf_session_open_z.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                            P(ctypes.c_void_p)]
    lib.edsx_vcf_session_contig_name.argtypes = [ctypes.c_void_p, ctypes.c_size_t, P(ctypes.c_char_p), P(ctypes.c_size_t)]
    lib.edsx_leds_merge_range.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                          ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          P(_Buf), P(_Buf), P(ctypes.c_int), P(ctypes.c_int)]
    lib.edsx_vcf_index.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, P(_Buf), P(_Buf), P(_Buf), P(_Buf),
                                   P(VcfStats)]
    lib.edsx_vcf_sort_order.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.edsx_vcf_transform_range.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                             ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint64, P(_Buf), P(_Buf),
                                             P(VcfStats)]
    lib.edsx_msa_plan_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32,
                                         ctypes.c_void_p, P(ctypes.c_uint64), P(ctypes.c_uint64)]
    lib.edsx_msa_emit_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.edsx_msa_last_info.argtypes = [ctypes.c_void_p, P(MsaInfo)]
    lib.edsx_msa_edge_info.argtypes = [ctypes.c_void_p, P(MsaEdges)]
    lib.edsx_msa_anchor_info.argtypes = [ctypes.c_void_p, ctypes.c_uint64, P(MsaAnchors)]
    lib.edsx_msa_copy_columns.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
    lib.edsx_msa_locate_segment.argtypes = [ctypes.c_void_p, ctypes.c_uint64] + [P(ctypes.c_uint64)] * 4
    lib.edsx_set_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.edsx_set_timing.restype = None
    lib.edsx_get_timing.argtypes = [ctypes.c_void_p, P(ctypes.c_char_p), P(ctypes.c_float), P(ctypes.c_int),
                                    ctypes.c_int]
    lib.edsx_msa_synth_size.argtypes = [ctypes.c_uint32, ctypes.c_uint64]
    lib.edsx_msa_synth_size.restype = ctypes.c_size_t
    lib.edsx_msa_synth_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32,
                                          ctypes.c_uint64, ctypes.c_uint64, ctypes.c_double, ctypes.c_uint64,
                                          ctypes.c_void_p, P(ctypes.c_size_t)]
    lib.edsx_multi_create.argtypes = [P(ctypes.c_int), ctypes.c_int, ctypes.c_int, P(ctypes.c_void_p)]
    lib.edsx_multi_destroy.argtypes = [ctypes.c_void_p]
    lib.edsx_multi_destroy.restype = None
    lib.edsx_multi_last_error.argtypes = [ctypes.c_void_p]
    lib.edsx_multi_last_error.restype = ctypes.c_char_p
    lib.edsx_msa_transform_multi.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, P(_Buf), P(_Buf)]
    lib.edsx_multi_last_partition.argtypes = [ctypes.c_void_p, P(ctypes.c_int), P(ctypes.c_int)]
    lib.edsx_vcf_transform_multi.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                             ctypes.c_size_t, ctypes.c_uint32, P(_Buf), P(_Buf), P(VcfStats)]
    lib.edsx_multi_last_vcf.argtypes = [ctypes.c_void_p, P(VcfMultiInfo)]
    lib.edsx_leds_merge_multi.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                          ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int, P(_Buf), P(_Buf)]
    lib.edsx_multi_last_merge.argtypes = [ctypes.c_void_p, P(MergeMultiInfo)]
    lib.edsx_eds_scan_range.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint64,
                                        ctypes.c_uint32, P(EdsRangeScan)]
    lib.edsx_seds_scan_range.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint64,
                                         ctypes.c_void_p, ctypes.c_size_t, P(ctypes.c_int), P(ctypes.c_uint64),
                                         ctypes.c_void_p, ctypes.c_void_p]
    lib.edsx_genvcf.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, P(_Buf), P(_Buf)]
    lib.edsx_msa_synth_size_aligned.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32]
    lib.edsx_msa_synth_size_aligned.restype = ctypes.c_size_t
    lib.edsx_msa_synth_device_aligned.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32,
                                                  ctypes.c_uint64, ctypes.c_uint64, ctypes.c_double, ctypes.c_uint64,
                                                  ctypes.c_uint32, ctypes.c_void_p, P(ctypes.c_size_t)]
    lib.edsx_eds_genpatterns.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32,
                                         ctypes.c_uint64, P(_Buf), P(_Buf), P(_Buf), P(_Buf)]
    lib.edsx_eds_check_positions.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                             ctypes.c_size_t] + [ctypes.c_void_p] * 6
    lib.edsx_query_last_info.argtypes = [ctypes.c_void_p, P(QueryInfo)]
    lib.edsx_eds_locate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                    ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32] + [P(_Buf)] * 6
    lib.edsx_paths_open.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                    P(ctypes.c_void_p)]
    lib.edsx_paths_info.argtypes = [ctypes.c_void_p, P(PathsInfo)]
    lib.edsx_paths_lengths.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    lib.edsx_paths_spell.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, P(ctypes.c_char_p), ctypes.c_char_p,
                                     ctypes.c_uint64, P(_Buf), ctypes.c_void_p]
    lib.edsx_paths_last_timing.argtypes = [ctypes.c_void_p, P(PathsTiming)]
    lib.edsx_paths_close.argtypes = [ctypes.c_void_p]
    lib.edsx_paths_close.restype = None
    lib.edsx_eds_spell_paths.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                         ctypes.c_void_p, ctypes.c_size_t, P(ctypes.c_char_p), ctypes.c_char_p, ctypes.c_uint64,
                                         P(_Buf), ctypes.c_void_p]
    lib.edsx_eds_subset.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                    ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, P(_Buf), P(_Buf), P(SubsetInfo)]
    lib.edsx_eds_gfa_graph.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, P(_Buf), P(GfaInfo)]
    lib.edsx_paths_gfa_walks.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, P(ctypes.c_char_p), ctypes.c_char_p,
                                         P(_Buf), ctypes.c_void_p, ctypes.c_void_p]
    lib.edsx_eds_gfa.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64,
                                 ctypes.c_char_p, P(_Buf), P(GfaInfo)]
    lib.edsx_eds_vcf.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                 P(VcfExportOpts), P(_Buf), P(_Buf), P(VcfExportInfo)]
    lib.edsx_paths_align_info.argtypes = [ctypes.c_void_p, P(AlignInfo)]
    lib.edsx_paths_align.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, P(ctypes.c_char_p), ctypes.c_char_p,
                                     ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, P(_Buf), ctypes.c_void_p]
    lib.edsx_eds_msa.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                 ctypes.c_void_p, ctypes.c_size_t, P(ctypes.c_char_p), ctypes.c_char_p, ctypes.c_uint64,
                                 ctypes.c_int, ctypes.c_uint64, P(_Buf), ctypes.c_void_p, P(AlignInfo)]
    V = ctypes.c_void_p
    lib.edsx_paths_lift_sites.argtypes = [V, ctypes.c_size_t, V, V, V, V]
    lib.edsx_paths_lift_place.argtypes = [V, ctypes.c_size_t, V, V, V, V, V, V]
    lib.edsx_paths_lift.argtypes = [V, ctypes.c_size_t, V, V, V, V, V, V]
    lib.edsx_eds_lift.argtypes = [V, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, V, V, V, V, V, V]
    lib.edsx_paths_slice.argtypes = [V, ctypes.c_size_t, V, V, V, ctypes.c_uint64, P(_Buf), P(_Buf), V, V]
    lib.edsx_eds_slice.argtypes = [V, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, V, V, V,
                                   ctypes.c_uint64, P(_Buf), P(_Buf), V, V]
    lib.edsx_paths_distances.argtypes = [V, V, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64, V, V, P(DistInfo)]
    lib.edsx_eds_distances.argtypes = [V, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, V, ctypes.c_size_t,
                                       ctypes.c_int, ctypes.c_uint64, V, V, P(DistInfo)]
    lib.edsx_paths_ld.argtypes = [V, V, ctypes.c_size_t, P(LdOpts), P(_Buf), P(_Buf), P(LdInfo)]
    lib.edsx_eds_ld.argtypes = [V, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, V, ctypes.c_size_t, P(LdOpts),
                                P(_Buf), P(_Buf), P(LdInfo)]
    U64 = ctypes.c_uint64
    lib.edsx_paths_ibs.argtypes = [V, V, ctypes.c_size_t, U64, U64, U64, P(_Buf), P(_Buf), P(IbsInfo)]
    lib.edsx_eds_ibs.argtypes = [V, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, V, ctypes.c_size_t, U64, U64, U64,
                                 P(_Buf), P(_Buf), P(IbsInfo)]
    lib.edsx_paths_mosaic.argtypes = [V, V, ctypes.c_size_t, V, ctypes.c_size_t, U64, P(_Buf), P(_Buf), P(MosaicInfo)]
    lib.edsx_eds_mosaic.argtypes = [V, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, V, ctypes.c_size_t, V, ctypes.c_size_t,
                                    U64, P(_Buf), P(_Buf), P(MosaicInfo)]
    lib.edsx_paths_diversity.argtypes = [V, V, V, ctypes.c_size_t, P(DivOpts), P(_Buf), P(_Buf), P(_Buf), P(_Buf), P(DivInfo)]
    lib.edsx_eds_diversity.argtypes = [V, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, V, V, ctypes.c_size_t, P(DivOpts),
                                       P(_Buf), P(_Buf), P(_Buf), P(_Buf), P(DivInfo)]
    _LIB = lib
    return lib


# edsx_locate_hit as a numpy structured dtype
LOCATE_HIT = [("common_pos", "<u8"), ("symbol", "<u8"), ("string", "<u8"), ("offset", "<u8")]
# edsx_lift_site likewise, and the statuses of a lift
LIFT_SITE = [("symbol", "<u8"), ("string", "<u8"), ("offset", "<u8"), ("column", "<u8"), ("common_pos", "<u8")]
LIFT_SAME, LIFT_ALIGNED, LIFT_GAP, LIFT_MISSING, LIFT_RANGE = 0, 1, 2, 3, 4
# edsx_slice_region likewise, and the status of a region that is empty or leaves its path
SLICE_REGION = [(f, "<u8") for f in ("symbol_first", "symbol_last", "cut_first", "cut_end", "column_first", "column_end", "strings",
                                     "chars", "eds_off", "eds_len", "seds_off", "seds_len")]
SLICE_RANGE = 4


# edsx_ld_pair and edsx_ld_allele as numpy structured types
LD_PAIR = [(f, "<u8") for f in ("symbol_a", "string_a", "symbol_b", "string_b", "n_ab", "n_a", "n_b", "n")] + [("r2", "<f8")]
LD_ALLELE = [(f, "<u8") for f in ("symbol", "string", "count", "present")]


def _ld_call(ctx, fn, head, paths, window, min_r2, min_count, all_strings, max_pairs):
    """edsx_paths_ld / edsx_eds_ld behind their leading arguments -> (pairs, alleles, info); an EdsxError carries the info
    dict, filled in as far as the call got, as its `info`"""
    import numpy as np
    ids = np.ascontiguousarray([] if paths is None else list(paths), dtype=np.uint64)
    opts = LdOpts(int(window), float(min_r2), int(min_count), 1 if all_strings else 0, int(max_pairs))
    p, a, info = _Buf(), _Buf(), LdInfo()
    rc = fn(*head, ids.ctypes.data if len(ids) else None, len(ids), ctypes.byref(opts), ctypes.byref(p), ctypes.byref(a), ctypes.byref(info))
    try:
        ctx._check(rc)
    except EdsxError as ex:
        ex.info = _fields(info)
        raise
    return (np.frombuffer(ctx._take(p), dtype=LD_PAIR), np.frombuffer(ctx._take(a), dtype=LD_ALLELE), _fields(info))


# edsx_ibs_segment as a numpy structured type
IBS_SEGMENT = [(f, "<u8") for f in ("x", "y", "symbol_first", "symbol_last", "sites", "column_first", "column_end")]


def _ibs_call(ctx, fn, head, paths, min_sites, min_columns, max_segments):
    """edsx_paths_ibs / edsx_eds_ibs behind their leading arguments -> (segments, pair_off, info); an EdsxError carries the
    info dict, filled in as far as the call got, as its `info`"""
    import numpy as np
    ids = np.ascontiguousarray([] if paths is None else list(paths), dtype=np.uint64)
    sg, po, info = _Buf(), _Buf(), IbsInfo()
    rc = fn(*head, ids.ctypes.data if len(ids) else None, len(ids), int(min_sites), int(min_columns), int(max_segments),
            ctypes.byref(sg), ctypes.byref(po), ctypes.byref(info))
    try:
        ctx._check(rc)
    except EdsxError as ex:
        ex.info = _fields(info)
        raise
    return (np.frombuffer(ctx._take(sg), dtype=IBS_SEGMENT), np.frombuffer(ctx._take(po), dtype=np.uint64), _fields(info))


# edsx_mosaic_segment as a numpy structured type; donor MOSAIC_PRIVATE: a private segment
MOSAIC_SEGMENT = [(f, "<u8") for f in ("target", "donor", "symbol_first", "symbol_last", "sites", "column_first", "column_end")]
MOSAIC_PRIVATE = 2 ** 64 - 1


def _mosaic_call(ctx, fn, head, targets, donors, max_segments):
    """edsx_paths_mosaic / edsx_eds_mosaic behind their leading arguments -> (segments, target_off, info); an EdsxError
    carries the info dict, filled in as far as the call got, as its `info`"""
    import numpy as np
    t = np.ascontiguousarray([] if targets is None else list(targets), dtype=np.uint64)
    d = np.ascontiguousarray([] if donors is None else list(donors), dtype=np.uint64)
    sg, to, info = _Buf(), _Buf(), MosaicInfo()
    rc = fn(*head, t.ctypes.data if len(t) else None, len(t), d.ctypes.data if len(d) else None, len(d), int(max_segments),
            ctypes.byref(sg), ctypes.byref(to), ctypes.byref(info))
    try:
        ctx._check(rc)
    except EdsxError as ex:
        ex.info = _fields(info)
        raise
    return (np.frombuffer(ctx._take(sg), dtype=MOSAIC_SEGMENT), np.frombuffer(ctx._take(to), dtype=np.uint64), _fields(info))


# edsx_div_window, edsx_div_group and edsx_div_pair as numpy structured types; the window units (EDSX_DIV_*)
DIV_WINDOW = [(f, "<u8") for f in ("start", "end", "rank_first", "rank_end")]
DIV_GROUP = [(f, "<u8") for f in ("segregating", "present")]
DIV_PAIR = [(f, "<u8") for f in ("diff", "comp")]
DIV_UNITS = {"symbols": 0, "columns": 1}
DIV_MAX_GROUPS = 16


def _div_call(ctx, fn, head, groups, unit, size, step, max_windows, sfs):
    """edsx_paths_diversity / edsx_eds_diversity behind their leading arguments -> (windows, groups, pairs, sfs, info):
    windows (NW,) DIV_WINDOW, groups (NW, G) DIV_GROUP, pairs (NW, G (G + 1) / 2) DIV_PAIR with (g, h), g <= h, row-major,
    sfs a list of G uint64 arrays of K_g + 1 bins (None unless asked for); an EdsxError carries the info dict, filled in as
    far as the call got, as its `info`"""
    import numpy as np
    if isinstance(unit, str):
        if unit not in DIV_UNITS:
            raise ValueError("the unit is one of %s" % ", ".join(sorted(DIV_UNITS)))
        unit = DIV_UNITS[unit]
    groups = [list(g) for g in groups] if groups is not None else []
    off = np.zeros(len(groups) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(g) for g in groups], dtype=np.uint64) if groups else []
    ids = np.ascontiguousarray([p for g in groups for p in g], dtype=np.uint64)
    opts = DivOpts(int(unit), int(size), int(step), int(max_windows))
    w, g, p, f, info = _Buf(), _Buf(), _Buf(), _Buf(), DivInfo()
    rc = fn(*head, off.ctypes.data if groups else None, ids.ctypes.data if len(ids) else None, len(groups), ctypes.byref(opts),
            ctypes.byref(w), ctypes.byref(g), ctypes.byref(p), ctypes.byref(f) if sfs else None, ctypes.byref(info))
    try:
        ctx._check(rc)
    except EdsxError as ex:
        ex.info = _fields(info)
        raise
    info = _fields(info)
    G, NP = max(info["groups"], 1), max(info["pairs"], 1)
    spectra = None
    if sfs:
        flat = np.frombuffer(ctx._take(f), dtype=np.uint64)
        sizes = [len(set(x)) + 1 for x in groups] if groups else [info["paths"] + 1]
        spectra, at = [], 0
        for n in sizes:
            spectra.append(flat[at:at + n])
            at += n
    return (np.frombuffer(ctx._take(w), dtype=DIV_WINDOW), np.frombuffer(ctx._take(g), dtype=DIV_GROUP).reshape(-1, G),
            np.frombuffer(ctx._take(p), dtype=DIV_PAIR).reshape(-1, NP), spectra, info)


# the metrics of the path distances (EDSX_DIST_*)
DIST_METRICS = {"columns": 0, "strings": 1}


def _metric(metric):
    """The metric parameter of the distance calls as the C int: a name of DIST_METRICS, or the number itself."""
    if isinstance(metric, str):
        if metric not in DIST_METRICS:
            raise ValueError("the metric is one of %s" % ", ".join(sorted(DIST_METRICS)))
        return DIST_METRICS[metric]
    return int(metric)


def _slice_regions(reg, st):
    """The edsx_slice_region array as a dict of uint64 columns, plus `status`."""
    import numpy as np
    out = {f: np.ascontiguousarray(reg[f]) for f, _ in SLICE_REGION}
    out["status"] = st
    return out


def _u64s(*cols):
    """Contiguous uint64 arrays of one length."""
    import numpy as np
    out = [np.ascontiguousarray(c, dtype=np.uint64).reshape(-1) for c in cols]
    if any(len(c) != len(out[0]) for c in out):
        raise ValueError("the query columns differ in length")
    return out


def _take(lib, b):
    """The bytes of an edsx_buf, which is freed."""
    if b.size < (1 << 31):
        data = ctypes.string_at(b.data, b.size) if b.size else b""
    else:                                                          # (string_at takes its size as a C int)
        data = bytes((ctypes.c_char * b.size).from_address(b.data))
    lib.edsx_buf_free(ctypes.byref(b))
    return data


def _input(obj):
    """(pointer, length, keep-alive) of bytes, or of any object with the buffer protocol (handed over in place)."""
    if isinstance(obj, bytes):
        return obj, len(obj), obj
    import numpy as np
    keep = np.frombuffer(obj, dtype=np.uint8)
    return ctypes.c_void_p(keep.ctypes.data), int(keep.size), keep


def _opt(b):
    """(bytes or None, length) of an optional text."""
    if b is None:
        return None, 0
    b = bytes(b)
    return b, len(b)


def _raw(x):
    return x


def _fields(st, conv=int, flags=()):
    """A ctypes struct as a dict: conv(value) per field (_raw: as ctypes gives it), bool for the fields in `flags`."""
    return {n: (bool if n in flags else conv)(getattr(st, n)) for n, _ in st._fields_}


def _name(contig):
    return contig.encode() if isinstance(contig, str) else bytes(contig)


class _Handle:
    """A library handle in self._h, destroyed once by the function named _destroy: close(), `with`, or collection."""
    _destroy = None

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._lib, self._destroy)(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gz_probe(data):
    """0 plain, 1 BGZF, 2 gzip (edsx_gz_probe: host only, never fails on garbage)."""
    data = bytes(data)
    kind = ctypes.c_int()
    rc = load_library().edsx_gz_probe(data, len(data), ctypes.byref(kind))
    if rc != 0:
        raise EdsxError(rc, "edsx_gz_probe")
    return kind.value


def bgzf_index(data):
    """([(comp_off, out_off, comp_len, isize)], text size) of a BGZF file (edsx_bgzf_index: host only)."""
    data = bytes(data)
    lib = load_library()
    b, n = _Buf(), ctypes.c_uint64()
    rc = lib.edsx_bgzf_index(data, len(data), ctypes.byref(b), ctypes.byref(n))
    if rc != 0:
        raise EdsxError(rc, "not a BGZF file")
    raw = _take(lib, b)
    blocks = (BgzfBlock * (len(raw) // ctypes.sizeof(BgzfBlock))).from_buffer_copy(raw)
    return [(int(x.comp_off), int(x.out_off), int(x.comp_len), int(x.isize)) for x in blocks], int(n.value)


class MultiGpu(_Handle):
    """edsx_multi: MSA -> EDS over several GPUs from one process (C++ rank threads, RCCL or in-process exchange)."""
    _destroy = "edsx_multi_destroy"

    def __init__(self, devices, use_rccl=True):
        self._lib = load_library()
        arr = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p()
        rc = self._lib.edsx_multi_create(arr, len(devices), 1 if use_rccl else 0, ctypes.byref(h))
        if rc != 0:
            raise EdsxError(rc, "edsx_multi_create failed for devices %r (rccl=%r)" % (list(devices), use_rccl))
        self._h = h

    def _check(self, rc):
        if rc != 0:
            raise EdsxError(rc, self._lib.edsx_multi_last_error(self._h).decode(errors="replace"))

    def msa_transform(self, msa, context_len=0):
        e, s = _Buf(), _Buf()
        ptr, n, keep = _input(msa)
        self._check(self._lib.edsx_msa_transform_multi(self._h, ptr, n, context_len, ctypes.byref(e), ctypes.byref(s)))
        del keep
        return _take(self._lib, e), _take(self._lib, s)

    def last_partition(self):
        p, c = ctypes.c_int(), ctypes.c_int()
        self._lib.edsx_multi_last_partition(self._h, ctypes.byref(p), ctypes.byref(c))
        return bool(p.value), int(c.value)

    def vcf_transform(self, vcf, fasta, context_len=0):
        """VCF + reference FASTA -> (eds, seds, stats) by reference-position ranges over the handle's GPUs; the same
        outputs, stats and errors as Context.vcf_transform."""
        e, s, st = _Buf(), _Buf(), VcfStats()
        vcf, fasta = bytes(vcf), bytes(fasta)
        self._check(self._lib.edsx_vcf_transform_multi(self._h, vcf, len(vcf), fasta, len(fasta), context_len,
                                                       ctypes.byref(e), ctypes.byref(s), ctypes.byref(st)))
        return _take(self._lib, e), _take(self._lib, s), _fields(st)

    def last_vcf(self):
        """Of the last vcf_transform: partitioned, fasta_windowed, records_min / _max, moved_line_bytes,
        fasta_h2d_bytes_max."""
        info = VcfMultiInfo()
        self._lib.edsx_multi_last_vcf(self._h, ctypes.byref(info))
        return _fields(info, flags=("partitioned", "fasta_windowed"))

    def leds_merge(self, eds, seds=None, context_len=1, compact=True):
        """EDS (+ sEDS: LINEAR, else CARTESIAN) -> (leds, seds_out) by symbol ranges over the handle's GPUs; the same
        outputs and errors as Context.leds_merge."""
        o, so = _Buf(), _Buf()
        eds = bytes(eds)
        self._check(self._lib.edsx_leds_merge_multi(self._h, eds, len(eds), *_opt(seds), context_len, 1 if compact else 0,
                                                    ctypes.byref(o), ctypes.byref(so)))
        return _take(self._lib, o), _take(self._lib, so)

    def last_merge(self):
        """Of the last leds_merge: partitioned, ranges, fallback (0 partitioned; 1 one rank / l = 0; 2 text not plain;
        3 no sentinel; 4 source sets do not match; 5 a sentinel was merged or a range failed), range_bytes_min / _max,
        eds_h2d_bytes_max, seds_h2d_bytes_max."""
        info = MergeMultiInfo()
        self._lib.edsx_multi_last_merge(self._h, ctypes.byref(info))
        return _fields(info, flags=("partitioned",))


def synth_size(n_rows, n_cols, row_align=0):
    if row_align > 1:
        return int(load_library().edsx_msa_synth_size_aligned(n_rows, n_cols, row_align))
    return int(load_library().edsx_msa_synth_size(n_rows, n_cols))


class Context(_Handle):
    """One context per (thread, GPU); mirrors edsx_ctx_create/destroy."""
    _destroy = "edsx_ctx_destroy"

    def __init__(self, device=0):
        self._lib = load_library()
        h = ctypes.c_void_p()
        rc = self._lib.edsx_ctx_create(device, ctypes.byref(h))
        if rc != 0:
            raise EdsxError(rc, "no usable gfx950 device %d (the engine has no CPU fallback)" % device)
        self._h = h
        self.device = device

    def _check(self, rc):
        if rc != 0:
            raise EdsxError(rc, self._lib.edsx_last_error(self._h).decode(errors="replace"))

    def _take(self, b):
        return _take(self._lib, b)

    # ---- host-buffer entry points
    def msa_transform(self, msa, context_len=0):
        """msa: bytes, or any object with the buffer protocol (a mapped file is handed over in place, not copied)."""
        e, s = _Buf(), _Buf()
        ptr, n, keep = _input(msa)
        self._check(self._lib.edsx_msa_transform(self._h, ptr, n, context_len, ctypes.byref(e), ctypes.byref(s)))
        del keep
        return self._take(e), self._take(s)

    def msa_last_batches(self):
        return int(self._lib.edsx_msa_last_batches(self._h))

    def msa_transform_batched(self, msa, context_len=0, batches=2):
        """The same in `batches` column batches, one after the other on this GPU (bounded working set).  Returns
        (eds, seds, batches taken) - 1 when the input is not cut."""
        e, s = _Buf(), _Buf()
        used = ctypes.c_int(0)
        ptr, n, keep = _input(msa)
        self._check(self._lib.edsx_msa_transform_batched(self._h, ptr, n, context_len, batches, ctypes.byref(e), ctypes.byref(s),
                                                         ctypes.byref(used)))
        del keep
        return self._take(e), self._take(s), used.value

    def leds_merge(self, eds, seds=None, context_len=1, compact=True):
        o, so = _Buf(), _Buf()
        eds = bytes(eds)
        self._check(self._lib.edsx_leds_merge(self._h, eds, len(eds), *_opt(seds),
                                              context_len, 1 if compact else 0, ctypes.byref(o), ctypes.byref(so)))
        return self._take(o), self._take(so)

    def eds_stats(self, eds, seds=None, context_len=0):
        """Statistics (EDS::Statistics) and is_leds(context_len) of an .eds (+ .seds) text as a dict."""
        st = EdsStatistics()
        self._check(self._lib.edsx_eds_stats(self._h, eds, len(eds), seds, len(seds) if seds is not None else 0,
                                             context_len, ctypes.byref(st)))
        return _fields(st, _raw)

    # ---- queries (EDS::generate_patterns / EDS::check_position on the GPU)
    def eds_genpatterns(self, eds, count, length, seed, witness=False):
        """count patterns of `length` characters, one per line (bytes).  witness=True: (patterns, pos, off, deg) with the
        start common position per pattern (numpy uint64, 2**64-1 for a wrapped pattern) and the chosen degenerate string
        numbers as CSR (off uint64 count+1, deg int32)."""
        import numpy as np
        p, wp, wo, wd = _Buf(), _Buf(), _Buf(), _Buf()
        eds = bytes(eds)
        w = [ctypes.byref(b) for b in (wp, wo, wd)] if witness else [None, None, None]
        self._check(self._lib.edsx_eds_genpatterns(self._h, eds, len(eds), int(count), int(length), int(seed) & (2**64 - 1),
                                                   ctypes.byref(p), *w))
        pats = self._take(p)
        if not witness:
            return pats
        pos = np.frombuffer(self._take(wp), dtype=np.uint64)
        off = np.frombuffer(self._take(wo), dtype=np.uint64)
        deg = np.frombuffer(self._take(wd), dtype=np.int32)
        return pats, pos, off, deg

    def eds_check_positions(self, eds, positions, choice_off, choices, pattern_off, patterns, seds=None):
        """EDS::check_position per query (CSR inputs, numpy-convertible) -> numpy int8: 1 true, 0 false,
        -1 out_of_range, -2 invalid_argument."""
        import numpy as np
        eds = bytes(eds)
        pos = np.ascontiguousarray(positions, dtype=np.uint64)
        coff = np.ascontiguousarray(choice_off, dtype=np.uint64)
        ch = np.ascontiguousarray(choices, dtype=np.int32)
        poff = np.ascontiguousarray(pattern_off, dtype=np.uint64)
        pat = np.frombuffer(bytes(patterns), dtype=np.uint8) if not isinstance(patterns, np.ndarray) else \
            np.ascontiguousarray(patterns, dtype=np.uint8)
        n = len(pos)
        if len(coff) != n + 1 or len(poff) != n + 1:
            raise ValueError("choice_off and pattern_off need len(positions) + 1 entries")
        out = np.empty(n, dtype=np.int8)
        self._check(self._lib.edsx_eds_check_positions(self._h, eds, len(eds), *_opt(seds), n,
                                                       pos.ctypes.data, coff.ctypes.data, ch.ctypes.data, poff.ctypes.data,
                                                       pat.ctypes.data, out.ctypes.data))
        return out

    def eds_locate(self, eds, patterns, seds=None, max_hits=1024, common_only=False):
        """Every occurrence of every pattern (a list of bytes) in the .eds (+ .seds), in check_position's coordinates.
        Returns numpy arrays (hit_off, hits, choice_off, choices, totals, flags): the hits of pattern q are
        hits[hit_off[q]:hit_off[q + 1]] (LOCATE_HIT: common_pos, 2**64-1 for a start inside a degenerate symbol; symbol;
        string, its index in the symbol; offset), ascending by (symbol, string, offset), then by choices; hit h chose the
        degenerate string numbers choices[choice_off[h]:choice_off[h + 1]].  At most max_hits hits come back per pattern:
        flags[q] bit 0 says some were left out (totals[q] is then a lower bound), bit 1 that a walk was cut at its 65th
        choice.  common_only: only starts in common symbols."""
        import numpy as np
        patterns = [bytes(p) for p in patterns]
        poff = np.zeros(len(patterns) + 1, dtype=np.uint64)
        poff[1:] = np.cumsum([len(p) for p in patterns], dtype=np.uint64)
        text = np.frombuffer(b"".join(patterns), dtype=np.uint8)
        bufs = [_Buf() for _ in range(6)]
        ptr, n, keep = _input(eds)
        self._check(self._lib.edsx_eds_locate(self._h, ptr, n, *_opt(seds), len(patterns), poff.ctypes.data, text.ctypes.data,
                                              int(max_hits), 1 if common_only else 0, *[ctypes.byref(b) for b in bufs]))
        del keep
        dtypes = (np.uint64, LOCATE_HIT, np.uint64, np.int32, np.uint64, np.uint8)
        return tuple(np.frombuffer(self._take(b), dtype=d) for b, d in zip(bufs, dtypes))

    def query_last_info(self):
        """Counts and timing of the last eds_genpatterns / eds_check_positions / eds_locate call."""
        q = QueryInfo()
        self._check(self._lib.edsx_query_last_info(self._h, ctypes.byref(q)))
        return _fields(q, _raw)

    def genrandomeds(self, total_bp, variability=0.10, min_alt=2, max_alt=4, var_len_max=10, snp_ratio=0.7,
                     alphabet="ACGT", min_context=0, seed=42):
        """genrandomeds-shaped (.eds, .seds, number of variant sites), generated on the GPU."""
        e, s = _Buf(), _Buf()
        n = ctypes.c_uint64(0)
        self._check(self._lib.edsx_genrandomeds(self._h, total_bp, variability, min_alt, max_alt, var_len_max, snp_ratio,
                                                alphabet.encode(), min_context, seed, ctypes.byref(e), ctypes.byref(s),
                                                ctypes.byref(n)))
        return self._take(e), self._take(s), n.value

    def gz_inflate(self, data):
        """inflate(data): BGZF on the device, any other gzip file on the host, plain bytes copied (edsx_gz_inflate)."""
        data = bytes(data)
        t = _Buf()
        self._check(self._lib.edsx_gz_inflate(self._h, data, len(data), ctypes.byref(t)))
        return self._take(t)

    def gz_last_info(self, which=0):
        """The compressed layer of the last gz_inflate / compressed=True call: which=0 the VCF (or the input), 1 the FASTA."""
        info = GzInfo()
        self._check(self._lib.edsx_gz_last_info(self._h, which, ctypes.byref(info)))
        return _fields(info, _raw)

    def vcf_transform(self, vcf, fasta, context_len=0, contig=None, compressed=False):
        """contig=None: the first FASTA record, CHROM ignored (the reference's rule).  contig=name: the record lines whose
        first token is `name` over the first FASTA record of that name (edsx_vcf_transform_contig).
        compressed=True: either input may be gzip or BGZF (edsx_vcf_transform_z); the result is that of the plain texts."""
        e, s, st = _Buf(), _Buf(), VcfStats()
        vcf, fasta = bytes(vcf), bytes(fasta)
        if compressed:
            name = None if contig is None else _name(contig)
            rc = self._lib.edsx_vcf_transform_z(self._h, vcf, len(vcf), fasta, len(fasta), name, context_len,
                                                ctypes.byref(e), ctypes.byref(s), ctypes.byref(st))
        elif contig is None:
            rc = self._lib.edsx_vcf_transform(self._h, vcf, len(vcf), fasta, len(fasta), context_len,
                                              ctypes.byref(e), ctypes.byref(s), ctypes.byref(st))
        else:
            name = _name(contig)
            rc = self._lib.edsx_vcf_transform_contig(self._h, vcf, len(vcf), fasta, len(fasta), name, context_len,
                                                     ctypes.byref(e), ctypes.byref(s), ctypes.byref(st))
        self._check(rc)
        return self._take(e), self._take(s), _fields(st)

    def vcf_session(self, vcf, fasta, compressed=False):
        return VcfSession(self, vcf, fasta, compressed)

    # ---- path spelling (eds2fasta)
    def paths_open(self, eds, seds):
        """A PathSession: the EDS + sEDS tokenised in HBM, for .info / .lengths / .spell."""
        return PathSession(self, eds, seds)

    def eds_spell_paths(self, eds, seds, paths=None, line_width=60, names=None, prefix=None):
        """One-shot edsx_eds_spell_paths -> (fasta bytes, missing counts as numpy uint64)."""
        import numpy as np
        eds = bytes(eds)
        sb, sn = _opt(seds)
        ids, nm, n_out = _path_args(paths, names)
        if paths is None or len(ids) == 0:                       # all paths: P records, learnt from the text
            n_out = max([int(x) for x in _re_ids(sb)] + [0]) if sb else 0
        miss = np.zeros(max(n_out, 1), dtype=np.uint64)
        f = _Buf()
        self._check(self._lib.edsx_eds_spell_paths(self._h, eds, len(eds), sb, sn,
                                                   ids.ctypes.data if len(ids) else None, len(ids), nm,
                                                   prefix.encode() if prefix is not None else None, int(line_width),
                                                   ctypes.byref(f), miss.ctypes.data))
        return self._take(f), miss[:n_out]

    # ---- alignment export (eds2msa)
    def eds_msa(self, eds, seds, paths=None, line_width=60, names=None, prefix=None, gap="-", max_bytes=0):
        """One-shot edsx_eds_msa: the requested paths (None or empty: all paths 1..P) as rows of one alignment, FASTA ->
        (fasta bytes, missing counts as numpy uint64, info dict of the column layout)."""
        import numpy as np
        eds = bytes(eds)
        sb, sn = _opt(seds)
        ids, nm, n_out = _path_args(paths, names)
        if paths is None or len(ids) == 0:                       # all paths: P records, learnt from the text
            n_out = max([int(x) for x in _re_ids(sb)] + [0]) if sb else 0
        miss = np.zeros(max(n_out, 1), dtype=np.uint64)
        f, info = _Buf(), AlignInfo()
        self._check(self._lib.edsx_eds_msa(self._h, eds, len(eds), sb, sn, ids.ctypes.data if len(ids) else None, len(ids), nm,
                                           prefix.encode() if prefix is not None else None, int(line_width), _gap(gap),
                                           int(max_bytes), ctypes.byref(f), miss.ctypes.data, ctypes.byref(info)))
        return self._take(f), miss[:n_out], _fields(info)

    # ---- coordinate lift (edsparser-lift)
    def eds_lift(self, eds, seds, src, pos, dst, with_sites=False):
        """One-shot edsx_eds_lift: PathSession.lift on a session opened and closed for this call."""
        import numpy as np
        eds = bytes(eds)
        src, pos, dst = _u64s(src, pos, dst)
        n = len(src)
        out, st = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint8)
        sites = np.zeros(n, dtype=LIFT_SITE) if with_sites else None
        self._check(self._lib.edsx_eds_lift(self._h, eds, len(eds), *_opt(seds), n, src.ctypes.data, pos.ctypes.data, dst.ctypes.data,
                                            out.ctypes.data, st.ctypes.data, sites.ctypes.data if with_sites else None))
        return (out, st, sites) if with_sites else (out, st)

    # ---- region slices (edsparser-slice)
    def eds_slice(self, eds, seds, path, start, end, max_bytes=0):
        """One-shot edsx_eds_slice: PathSession.slice on a session opened and closed for this call."""
        import numpy as np
        eds = bytes(eds)
        path, start, end = _u64s(path, start, end)
        n = len(path)
        reg, st = np.zeros(n, dtype=SLICE_REGION), np.zeros(n, dtype=np.uint8)
        e, q = _Buf(), _Buf()
        self._check(self._lib.edsx_eds_slice(self._h, eds, len(eds), *_opt(seds), n, path.ctypes.data, start.ctypes.data, end.ctypes.data,
                                             int(max_bytes), ctypes.byref(e), ctypes.byref(q), reg.ctypes.data, st.ctypes.data))
        return self._take(e), self._take(q), _slice_regions(reg, st)

    # ---- path distances (edsparser-dist)
    def eds_distances(self, eds, seds, paths=None, metric="columns", max_bytes=0):
        """One-shot edsx_eds_distances: PathSession.distances on a session opened and closed for this call."""
        import numpy as np
        eds = bytes(eds)
        sb, sn = _opt(seds)
        ids = np.ascontiguousarray([] if paths is None else list(paths), dtype=np.uint64)
        K = len(ids)
        if K == 0:                                                # all paths: P x P, learnt from the text
            K = max([int(x) for x in _re_ids(sb)] + [0]) if sb else 0
        if max_bytes and 8 * K * K > max_bytes:                   # refused by the library before it writes: no matrix needed
            mat = np.zeros((0, 0), dtype=np.uint64)
        else:
            mat = np.zeros((K, K), dtype=np.uint64)
        miss, info = np.zeros(max(K, 1), dtype=np.uint64), DistInfo()
        self._check(self._lib.edsx_eds_distances(self._h, eds, len(eds), sb, sn, ids.ctypes.data if len(ids) else None, len(ids),
                                                 _metric(metric), int(max_bytes), mat.ctypes.data if mat.size else None,
                                                 miss.ctypes.data, ctypes.byref(info)))
        return mat, miss[:K], _fields(info)

    # ---- linkage disequilibrium (edsparser-ld)
    def eds_ld(self, eds, seds, paths=None, window=100, min_r2=0.0, min_count=1, all_strings=False, max_pairs=0):
        """One-shot edsx_eds_ld: PathSession.ld on a session opened and closed for this call."""
        eds = bytes(eds)
        sb, sn = _opt(seds)
        return _ld_call(self, self._lib.edsx_eds_ld, (self._h, eds, len(eds), sb, sn), paths, window, min_r2, min_count, all_strings,
                        max_pairs)

    # ---- shared segments (edsparser-ibs)
    def eds_ibs(self, eds, seds, paths=None, min_sites=1, min_columns=0, max_segments=0):
        """One-shot edsx_eds_ibs: PathSession.ibs on a session opened and closed for this call."""
        eds = bytes(eds)
        sb, sn = _opt(seds)
        return _ibs_call(self, self._lib.edsx_eds_ibs, (self._h, eds, len(eds), sb, sn), paths, min_sites, min_columns, max_segments)

    # ---- mosaics (edsparser-mosaic)
    def eds_mosaic(self, eds, seds, targets=None, donors=None, max_segments=0):
        """One-shot edsx_eds_mosaic: PathSession.mosaic on a session opened and closed for this call."""
        eds = bytes(eds)
        sb, sn = _opt(seds)
        return _mosaic_call(self, self._lib.edsx_eds_mosaic, (self._h, eds, len(eds), sb, sn), targets, donors, max_segments)

    # ---- diversity (edsparser-diversity)
    def eds_diversity(self, eds, seds, groups=None, unit="symbols", size=0, step=0, max_windows=0, sfs=False):
        """One-shot edsx_eds_diversity: PathSession.diversity on a session opened and closed for this call."""
        eds = bytes(eds)
        sb, sn = _opt(seds)
        return _div_call(self, self._lib.edsx_eds_diversity, (self._h, eds, len(eds), sb, sn), groups, unit, size, step, max_windows, sfs)

    # ---- path subsetting (edsparser-subset)
    def eds_subset(self, eds, seds, paths, keep_ids=False):
        """The .eds + .seds restricted to the paths `paths` (ids of 1..P, each once) -> (eds bytes, seds bytes, info dict):
        FULL .eds text and .seds, each with a trailing line feed; kept paths are renumbered 1..len(paths) in ascending
        order of their ids unless keep_ids (edsx_eds_subset)."""
        import numpy as np
        ids = np.ascontiguousarray(list(paths), dtype=np.uint64)
        e, s, info = _Buf(), _Buf(), SubsetInfo()
        ptr, n, keep = _input(eds)
        self._check(self._lib.edsx_eds_subset(self._h, ptr, n, *_opt(seds), ids.ctypes.data if len(ids) else None, len(ids),
                                              1 if keep_ids else 0, ctypes.byref(e), ctypes.byref(s), ctypes.byref(info)))
        del keep
        return self._take(e), self._take(s), _fields(info)

    # ---- GFA export (eds2gfa)
    def eds_gfa_graph(self, eds, max_links=0):
        """The EDS as GFA 1.0 text without paths - header, S lines, L lines - and an info dict (edsx_eds_gfa_graph).
        max_links: 0 = 2**32."""
        g, info = _Buf(), GfaInfo()
        ptr, n, keep = _input(eds)
        self._check(self._lib.edsx_eds_gfa_graph(self._h, ptr, n, int(max_links), ctypes.byref(g), ctypes.byref(info)))
        del keep
        return self._take(g), _fields(info, flags=("tokenised_on_device",))

    def eds_gfa(self, eds, seds=None, max_links=0, prefix=None):
        """The graph, followed by one P line per path when seds is given (edsx_eds_gfa) -> (gfa bytes, info dict)."""
        g, info = _Buf(), GfaInfo()
        ptr, n, keep = _input(eds)
        self._check(self._lib.edsx_eds_gfa(self._h, ptr, n, *_opt(seds), int(max_links),
                                           prefix.encode() if prefix is not None else None, ctypes.byref(g), ctypes.byref(info)))
        del keep
        return self._take(g), _fields(info, flags=("tokenised_on_device",))

    # ---- VCF export (eds2vcf)
    def eds_vcf(self, eds, seds=None, chrom=None, ref_path=0, names=None, prefix=None, line_width=60, max_bytes=0):
        """The EDS as VCF 4.2 text - one record per symbol with two strings or more, with seds one genotype column per
        path - and the reference FASTA its positions refer to (edsx_eds_vcf) -> (vcf bytes, fasta bytes, info dict).
        ref_path: 0 = the first string of every symbol is REF, p = the string path p takes; names: one per path 1..P."""
        enc = lambda x: None if x is None else (x.encode() if isinstance(x, str) else bytes(x))
        opts = VcfExportOpts(enc(chrom), int(ref_path), None, 0, enc(prefix), int(line_width), int(max_bytes))
        if names is not None:
            arr = (ctypes.c_char_p * max(len(names), 1))(*[enc(x) for x in names])
            opts.names, opts.n_names = arr, len(names)
        v, f, info = _Buf(), _Buf(), VcfExportInfo()
        ptr, n, keep = _input(eds)
        self._check(self._lib.edsx_eds_vcf(self._h, ptr, n, *_opt(seds), ctypes.byref(opts), ctypes.byref(v), ctypes.byref(f),
                                           ctypes.byref(info)))
        del keep
        return self._take(v), self._take(f), _fields(info, flags=("tokenised_on_device",))

    def vcf_tokenised_on_device(self):
        return bool(self._lib.edsx_vcf_tokenised_on_device(self._h))

    def leds_tokenised_on_device(self):
        return bool(self._lib.edsx_leds_tokenised_on_device(self._h))

    # ---- symbol-range partition of the merge (multi-GPU, see multigpu.MergeSharder)
    def leds_merge_range(self, eds, seds=None, context_len=1, compact=True, head_sentinel=False, tail_sentinel=False):
        """-> (leds, seds_out, head_intact, tail_intact)"""
        o, so = _Buf(), _Buf()
        hi, ti = ctypes.c_int(), ctypes.c_int()
        eds = bytes(eds)
        self._check(self._lib.edsx_leds_merge_range(self._h, eds, len(eds), *_opt(seds),
                                                    context_len, 1 if compact else 0, 1 if head_sentinel else 0,
                                                    1 if tail_sentinel else 0, ctypes.byref(o), ctypes.byref(so),
                                                    ctypes.byref(hi), ctypes.byref(ti)))
        return self._take(o), self._take(so), bool(hi.value), bool(ti.value)

    def eds_scan_range(self, eds, lo, hi, context_len):
        """Device scan of .eds bytes [lo, hi): dict(ok, strings, cut) as multigpu.eds_scan_range, cut = None or
        (sym_start, sym_end, strings in [lo, sym_start))."""
        out = EdsRangeScan()
        eds = bytes(eds)
        self._check(self._lib.edsx_eds_scan_range(self._h, eds, len(eds), int(lo), int(hi), int(context_len), ctypes.byref(out)))
        cut = (int(out.sym_start), int(out.sym_end), int(out.strings_before)) if out.has_cut else None
        return {"ok": bool(out.ok), "strings": int(out.strings), "cut": cut}

    def seds_scan_range(self, seds, lo, hi, ordinals=()):
        """Device scan of .seds bytes [lo, hi) -> (ok, number of '{', [(start, end) of the k-th '{' ... '}' for k in
        ordinals]); end = find('}', start) + 1 over the whole buffer."""
        import numpy as np
        seds = bytes(seds)
        ords = np.ascontiguousarray(list(ordinals), dtype=np.uint64)
        p0 = np.zeros(len(ords), dtype=np.uint64)
        p1 = np.zeros(len(ords), dtype=np.uint64)
        ok, braces = ctypes.c_int(), ctypes.c_uint64()
        self._check(self._lib.edsx_seds_scan_range(self._h, seds, len(seds), int(lo), int(hi), ords.ctypes.data, len(ords),
                                                   ctypes.byref(ok), ctypes.byref(braces), p0.ctypes.data, p1.ctypes.data))
        return bool(ok.value), int(braces.value), [(int(a), int(b)) for a, b in zip(p0, p1)]

    # ---- position-range partition of the VCF path (multi-GPU, see multigpu.VcfSharder)
    def vcf_index(self, vcf):
        """(pos, reflen, line_off, line_len) as numpy uint64 arrays, file order, + counters."""
        import numpy as np
        bufs = [_Buf() for _ in range(4)]
        st = VcfStats()
        vcf = bytes(vcf)
        self._check(self._lib.edsx_vcf_index(self._h, vcf, len(vcf), *[ctypes.byref(b) for b in bufs], ctypes.byref(st)))
        arrs = [np.frombuffer(self._take(b), dtype=np.uint64) for b in bufs]
        return (*arrs, _fields(st))

    def vcf_sort_order(self, pos):
        """Permutation of the reference's std::sort for these positions (numpy uint64 -> uint32)."""
        import numpy as np
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        out = np.empty(len(pos), dtype=np.uint32)
        rc = self._lib.edsx_vcf_sort_order(pos.ctypes.data, len(pos), out.ctypes.data)
        if rc != 0:
            raise EdsxError(rc, "edsx_vcf_sort_order failed")
        return out

    def vcf_transform_range(self, vcf_lines, fasta, cur0=0, next_start=None):
        e, s, st = _Buf(), _Buf(), VcfStats()
        vcf_lines, fasta = bytes(vcf_lines), bytes(fasta)
        nxt = 0xFFFFFFFFFFFFFFFF if next_start is None else int(next_start)
        self._check(self._lib.edsx_vcf_transform_range(self._h, vcf_lines, len(vcf_lines), fasta, len(fasta), int(cur0),
                                                       nxt, ctypes.byref(e), ctypes.byref(s), ctypes.byref(st)))
        return self._take(e), self._take(s), _fields(st)

    # ---- device-resident entry points (pointers are ints: tensor.data_ptr())
    def msa_plan_device(self, d_msa, n, context_len=0, stream=0):
        """Plan the alignment in the n device bytes at d_msa -> (eds_bytes, seds_bytes).  d_msa may be any byte address;
        only [d_msa, d_msa + n) is read, and nothing around it needs to be readable.  stream: a hipStream_t as an int
        (torch: stream.cuda_stream; 0: the default stream); the call waits for that stream (and only it) to hand the
        sizes back.  The plan stays in the context until the next plan; the input must stay unchanged until the last
        emit of it has completed."""
        E, Q = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.edsx_msa_plan_device(self._h, d_msa, n, context_len, stream,
                                                   ctypes.byref(E), ctypes.byref(Q)))
        return int(E.value), int(Q.value)

    def msa_emit_device(self, d_eds, d_seds, stream=0):
        """Write the planned .eds / .seds text to device buffers of exactly the planned sizes (any byte address, no
        slack: every byte of them is written and none outside).  Asynchronous; complete in `stream` order although
        internal streams take part - a wait for `stream` alone, or later work on it, sees the whole text.  May be
        repeated after one plan, without waiting in between; after a failed plan it raises (code 3)."""
        self._check(self._lib.edsx_msa_emit_device(self._h, d_eds, d_seds, stream))

    def msa_info(self):
        info = MsaInfo()
        rc = self._lib.edsx_msa_last_info(self._h, ctypes.byref(info))
        if rc != 0:
            raise EdsxError(rc, "no planned alignment")
        return _fields(info)

    def msa_edge_info(self):
        e = MsaEdges()
        self._check(self._lib.edsx_msa_edge_info(self._h, ctypes.byref(e)))
        return _fields(e)

    def msa_anchor_info(self, min_cols):
        """First / last common segment of at least min_cols columns of the planned alignment (see edsx.h)."""
        a = MsaAnchors()
        self._check(self._lib.edsx_msa_anchor_info(self._h, min_cols, ctypes.byref(a)))
        return _fields(a)

    def msa_copy_columns(self, col0, ncols, n_rows):
        buf = ctypes.create_string_buffer(n_rows * ncols)
        self._check(self._lib.edsx_msa_copy_columns(self._h, col0, ncols, buf))
        return buf.raw

    def msa_locate_segment(self, col):
        """-> (segment index, start column, .eds offset, .seds offset) of the first segment starting at or after col"""
        v = [ctypes.c_uint64() for _ in range(4)]
        self._check(self._lib.edsx_msa_locate_segment(self._h, int(col), *[ctypes.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def set_timing(self, on):
        self._lib.edsx_set_timing(self._h, 1 if on else 0)

    def get_timing(self):
        cap = 64
        names = (ctypes.c_char_p * cap)()
        ms = (ctypes.c_float * cap)()
        cnt = (ctypes.c_int * cap)()
        n = self._lib.edsx_get_timing(self._h, names, ms, cnt, cap)
        return [(names[i].decode(), float(ms[i]), int(cnt[i])) for i in range(n)]

    def genvcf(self, ref_len, n_records, n_samples=8, seed=42):
        """Synthetic (vcf, fasta) bytes of BASELINE configs[3]'s shape, generated on the device."""
        v, f = _Buf(), _Buf()
        self._check(self._lib.edsx_genvcf(self._h, ref_len, n_records, n_samples, seed, ctypes.byref(v), ctypes.byref(f)))
        return self._take(v), self._take(f)

    def msa_synth_device(self, d_out, capacity, n_rows, n_cols, col0=0, variant_fraction=0.05, seed=42,
                         stream=0, row_align=0):
        w = ctypes.c_size_t()
        if row_align > 1:
            self._check(self._lib.edsx_msa_synth_device_aligned(self._h, d_out, capacity, n_rows, col0, n_cols,
                                                                variant_fraction, seed, row_align, stream, ctypes.byref(w)))
        else:
            self._check(self._lib.edsx_msa_synth_device(self._h, d_out, capacity, n_rows, col0, n_cols,
                                                        variant_fraction, seed, stream, ctypes.byref(w)))
        return int(w.value)


def _re_ids(seds):
    import re
    return re.findall(rb"\d+", seds)


def _path_args(paths, names):
    """(ids as numpy uint64, names as a char* array or None, number of records; 0 ids = all paths)"""
    import numpy as np
    ids = np.ascontiguousarray([] if paths is None else list(paths), dtype=np.uint64)
    nm = None
    if names is not None:
        if len(names) != len(ids) or len(ids) == 0:
            raise ValueError("names need one entry per explicitly requested path")
        nm = (ctypes.c_char_p * len(ids))(*[_name(x) for x in names])
    return ids, nm, len(ids)


def _gap(gap):
    """The gap parameter of the align calls as the C int: one character or byte, or its value (0: the default '-')."""
    if isinstance(gap, int):
        return gap
    g = gap.encode("latin-1") if isinstance(gap, str) else bytes(gap)
    if len(g) != 1:
        raise ValueError("the gap is one byte")
    return g[0]


class PathSession(_Handle):
    """An EDS with sources kept tokenised in HBM (edsx_paths_*): the sequence of every path as FASTA.  The session owns its
    device tables: other calls on the context do not invalidate it."""
    _destroy = "edsx_paths_close"

    def __init__(self, ctx, eds, seds):
        self._ctx, self._lib = ctx, ctx._lib
        eds = bytes(eds)
        h = ctypes.c_void_p()
        ctx._check(self._lib.edsx_paths_open(ctx._h, eds, len(eds), *_opt(seds), ctypes.byref(h)))
        self._h = h

    @property
    def info(self):
        i = PathsInfo()
        self._ctx._check(self._lib.edsx_paths_info(self._h, ctypes.byref(i)))
        return _fields(i)

    @property
    def timing(self):
        """Of the last lengths / spell / gfa_walks / align / lift* / slice: tokenise_ms (of the open), choose_ms, scan_ms, copy_ms, download_ms, bytes_written."""
        t = PathsTiming()
        self._ctx._check(self._lib.edsx_paths_last_timing(self._h, ctypes.byref(t)))
        return _fields(t, _raw)

    def _ids(self, paths):
        import numpy as np
        if paths is None:
            return np.arange(1, self.info["num_paths"] + 1, dtype=np.uint64)
        return np.ascontiguousarray(list(paths), dtype=np.uint64)

    def lengths(self, paths=None):
        """(length, missing) as numpy uint64, one entry per requested path (None: all paths 1..P)."""
        import numpy as np
        ids = self._ids(paths)
        ln, ms = np.zeros(len(ids), dtype=np.uint64), np.zeros(len(ids), dtype=np.uint64)
        if len(ids):
            self._ctx._check(self._lib.edsx_paths_lengths(self._h, ids.ctypes.data, len(ids), ln.ctypes.data, ms.ctypes.data))
        return ln, ms

    def spell(self, paths=None, line_width=60, names=None, prefix=None, as_numpy=False):
        """(fasta, missing): FASTA of the requested paths in request order (None or empty: all paths 1..P), bytes - or,
        as_numpy=True, a numpy uint8 array (texts above 2 GiB without another copy) - and the missing counts (numpy
        uint64)."""
        import numpy as np
        ids, nm, n_out = _path_args(paths, names)
        if len(ids) == 0:
            n_out = self.info["num_paths"]
        miss = np.zeros(max(n_out, 1), dtype=np.uint64)
        f = _Buf()
        self._ctx._check(self._lib.edsx_paths_spell(self._h, ids.ctypes.data if len(ids) else None, len(ids), nm,
                                                    prefix.encode() if prefix is not None else None, int(line_width),
                                                    ctypes.byref(f), miss.ctypes.data))
        if as_numpy:
            out = np.empty(f.size, dtype=np.uint8)
            if f.size:
                ctypes.memmove(out.ctypes.data, f.data, f.size)
            self._lib.edsx_buf_free(ctypes.byref(f))
            return out, miss[:n_out]
        return self._ctx._take(f), miss[:n_out]

    def align_info(self):
        """The column layout of align(): n_symbols, n_columns (W), n_zero_width_symbols, widest_symbol, num_paths."""
        i = AlignInfo()
        self._ctx._check(self._lib.edsx_paths_align_info(self._h, ctypes.byref(i)))
        return _fields(i)

    def align(self, paths=None, line_width=60, names=None, prefix=None, gap="-", max_bytes=0, as_numpy=False):
        """(fasta, missing): the requested paths (None or empty: all paths 1..P) as rows of one alignment, FASTA in request
        order.  Every symbol owns as many columns as its longest string has characters; a row holds the path's strings
        left-justified there and `gap` elsewhere, so all rows have align_info()["n_columns"] characters whatever paths
        are asked for (edsx_paths_align).  max_bytes: 0 = no limit.  as_numpy as in spell()."""
        import numpy as np
        ids, nm, n_out = _path_args(paths, names)
        if len(ids) == 0:
            n_out = self.info["num_paths"]
        miss = np.zeros(max(n_out, 1), dtype=np.uint64)
        f = _Buf()
        self._ctx._check(self._lib.edsx_paths_align(self._h, ids.ctypes.data if len(ids) else None, len(ids), nm,
                                                    prefix.encode() if prefix is not None else None, int(line_width),
                                                    _gap(gap), int(max_bytes), ctypes.byref(f), miss.ctypes.data))
        if as_numpy:
            out = np.empty(f.size, dtype=np.uint8)
            if f.size:
                ctypes.memmove(out.ctypes.data, f.data, f.size)
            self._lib.edsx_buf_free(ctypes.byref(f))
            return out, miss[:n_out]
        return self._ctx._take(f), miss[:n_out]

    def lift_sites(self, paths, pos):
        """(sites, status): where character pos[q] of path paths[q] lies in the EDS (LIFT_SITE: symbol, string = index within
        the symbol, offset, alignment column, common_pos or 2**64-1), status 0, or LIFT_RANGE with every field 2**64-1 when
        the path has no such character (edsx_paths_lift_sites).  Any order, duplicates allowed."""
        import numpy as np
        paths, pos = _u64s(paths, pos)
        n = len(paths)
        sites, st = np.zeros(n, dtype=LIFT_SITE), np.zeros(n, dtype=np.uint8)
        self._ctx._check(self._lib.edsx_paths_lift_sites(self._h, n, paths.ctypes.data, pos.ctypes.data, sites.ctypes.data, st.ctypes.data))
        return sites, st

    def lift_place(self, symbol, string, offset, dst):
        """(pos, status): where character `offset` of string `string` of symbol `symbol` lies on path dst[q] - LIFT_SAME: the
        very character; LIFT_ALIGNED: another in the same alignment column; LIFT_GAP: the next character to the right;
        LIFT_MISSING: the path has no string there; LIFT_RANGE (pos 2**64-1): no such character (edsx_paths_lift_place).
        Takes the symbol / string / offset columns of an eds_locate hit array as they are."""
        import numpy as np
        symbol, string, offset, dst = _u64s(symbol, string, offset, dst)
        n = len(dst)
        out, st = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint8)
        self._ctx._check(self._lib.edsx_paths_lift_place(self._h, n, symbol.ctypes.data, string.ctypes.data, offset.ctypes.data,
                                                         dst.ctypes.data, out.ctypes.data, st.ctypes.data))
        return out, st

    def lift(self, src, pos, dst, with_sites=False):
        """(dst_pos, status[, sites]): the place on path dst[q] of character pos[q] of path src[q]; the sites stay on the
        device in between (edsx_paths_lift)."""
        import numpy as np
        src, pos, dst = _u64s(src, pos, dst)
        n = len(src)
        out, st = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint8)
        sites = np.zeros(n, dtype=LIFT_SITE) if with_sites else None
        self._ctx._check(self._lib.edsx_paths_lift(self._h, n, src.ctypes.data, pos.ctypes.data, dst.ctypes.data, out.ctypes.data,
                                                   st.ctypes.data, sites.ctypes.data if with_sites else None))
        return (out, st, sites) if with_sites else (out, st)

    def slice(self, path, start, end, max_bytes=0):
        """(eds bytes, seds bytes, regions): the regions [start[r], end[r]) of path path[r] - path 0: of the columns of
        align() - as FULL-form .eds + .seds texts laid end to end (edsx_paths_slice).  regions: a dict of uint64 arrays
        named as the fields of edsx_slice_region, plus `status` (0, or SLICE_RANGE with no bytes for a region that is empty
        or leaves its path).  max_bytes (0: none): EdsxError when both buffers together are larger."""
        import numpy as np
        path, start, end = _u64s(path, start, end)
        n = len(path)
        reg, st = np.zeros(n, dtype=SLICE_REGION), np.zeros(n, dtype=np.uint8)
        e, q = _Buf(), _Buf()
        self._ctx._check(self._lib.edsx_paths_slice(self._h, n, path.ctypes.data, start.ctypes.data, end.ctypes.data, int(max_bytes),
                                                    ctypes.byref(e), ctypes.byref(q), reg.ctypes.data, st.ctypes.data))
        return self._ctx._take(e), self._ctx._take(q), _slice_regions(reg, st)

    def distances(self, paths=None, metric="columns", max_bytes=0):
        """(matrix, missing, info): the pairwise distances of the requested paths in request order (None or empty: all paths
        1..P; duplicates allowed) as a numpy uint64 (K, K) array, symmetric with a zero diagonal, the missing counts and
        the info dict of edsx_dist_info (edsx_paths_distances).  metric "columns": the columns of the alignment of align()
        at which two rows differ, "no character" being a value of its own; "strings": the symbols at which two paths
        take different strings.  info["units"] is the denominator of a normalised distance.  max_bytes (0: none):
        EdsxError when the matrix is larger."""
        import numpy as np
        ids = np.ascontiguousarray([] if paths is None else list(paths), dtype=np.uint64)
        K = len(ids) if len(ids) else self.info["num_paths"]
        if max_bytes and 8 * K * K > max_bytes:                   # refused by the library before it writes: no matrix needed
            mat = np.zeros((0, 0), dtype=np.uint64)
        else:
            mat = np.zeros((K, K), dtype=np.uint64)
        miss, info = np.zeros(max(K, 1), dtype=np.uint64), DistInfo()
        self._ctx._check(self._lib.edsx_paths_distances(self._h, ids.ctypes.data if len(ids) else None, len(ids), _metric(metric),
                                                        int(max_bytes), mat.ctypes.data if mat.size else None, miss.ctypes.data,
                                                        ctypes.byref(info)))
        return mat, miss[:K], _fields(info)

    def ld(self, paths=None, window=100, min_r2=0.0, min_count=1, all_strings=False, max_pairs=0):
        """(pairs, alleles, info): r² between the alleles of the EDS over the paths `paths` (None or empty: all paths 1..P;
        duplicates count once), for every pair of listed alleles whose choice symbols lie at most `window` choice symbols
        apart (edsx_paths_ld).  An allele is a string of a choice symbol - string 0 only with all_strings - that between
        min_count and present - min_count of the paths take.  pairs: numpy structured array (LD_PAIR) of the pairs with
        r2 >= min_r2 in (symbol_a, string_a, symbol_b, string_b) order; alleles: the listed alleles with their counts
        (LD_ALLELE), the allele frequency table of the panel; info: the dict of edsx_ld_info.  max_pairs (0: none):
        EdsxError when more pairs would be reported."""
        return _ld_call(self._ctx, self._lib.edsx_paths_ld, (self._h,), paths, window, min_r2, min_count, all_strings, max_pairs)

    def ibs(self, paths=None, min_sites=1, min_columns=0, max_segments=0):
        """(segments, pair_off, info): the segments every two of the paths `paths` share (None or empty: all paths 1..P;
        duplicates allowed), pairs being request positions x < y (edsx_paths_ibs).  A segment is a maximal interval of
        symbols at all of which the two paths take the same string; it is reported when it holds at least min_sites choice
        symbols and min_columns alignment columns (0, 0: every segment).  segments: numpy structured array (IBS_SEGMENT) in
        (x, y, symbol_first) order; pair_off: K (K - 1) / 2 + 1 offsets, the records of pair q = (x, y) in row-major
        upper-triangle order are segments[pair_off[q]:pair_off[q + 1]]; info: the dict of edsx_ibs_info.  max_segments
        (0: none): EdsxError when more segments would be reported."""
        return _ibs_call(self._ctx, self._lib.edsx_paths_ibs, (self._h,), paths, min_sites, min_columns, max_segments)

    def diversity(self, groups=None, unit="symbols", size=0, step=0, max_windows=0, sfs=False):
        """-> (windows, groups, pairs, sfs, info): per window along the EDS the diversity within and between groups of paths
        (edsx_paths_diversity).  groups: lists of path ids, at most DIV_MAX_GROUPS, disjoint (None: one group of all paths).
        unit "symbols": windows of `size` choice symbols every `step` (0: size; size 0: one window); "columns": of columns of
        the alignment view.  windows: (NW,) DIV_WINDOW; groups: (NW, G) DIV_GROUP - segregating sites and present paths summed
        over the window; pairs: (NW, G (G + 1) / 2) DIV_PAIR for (g, h), g <= h, row-major - the path pairs that both have a
        string (comp) and those that differ (diff), summed: pi = diff / comp on the diagonal, d_xy off it.  sfs=True: per
        group the unfolded site frequency spectrum over all complete choice symbols, K_g + 1 bins.  info: the dict of
        edsx_div_info.  max_windows (0: none): EdsxError when there are more windows."""
        return _div_call(self._ctx, self._lib.edsx_paths_diversity, (self._h,), groups, unit, size, step, max_windows, sfs)

    def mosaic(self, targets=None, donors=None, max_segments=0):
        """(segments, target_off, info): every path of `targets` written as the fewest copies from the paths of `donors`
        (each None or empty: all paths 1..P; duplicates allowed; a donor naming the target's own path is skipped), both
        named by request position (edsx_paths_mosaic).  A copied segment is an interval of symbols over which the target
        and its donor take the same strings, chosen to reach as far as any donor does (then the smallest position); a
        private segment (donor MOSAIC_PRIVATE) holds symbols no eligible donor shares.  segments: numpy structured array
        (MOSAIC_SEGMENT) in (target, symbol_first) order, the segments of a target tile [0, n - 1]; target_off: T + 1
        offsets, the records of target x are segments[target_off[x]:target_off[x + 1]]; info: the dict of
        edsx_mosaic_info.  max_segments (0: none): EdsxError when there are more segments."""
        return _mosaic_call(self._ctx, self._lib.edsx_paths_mosaic, (self._h,), targets, donors, max_segments)

    def gfa_walks(self, paths=None, names=None, prefix=None):
        """(lines, missing, steps): the GFA P lines of the requested paths in request order (None or empty: all paths
        1..P) over the segment ids of Context.eds_gfa_graph, and per path the missing count and the number of ids (numpy
        uint64); a path without a step has no line (edsx_paths_gfa_walks)."""
        import numpy as np
        ids, nm, n_out = _path_args(paths, names)
        if len(ids) == 0:
            n_out = self.info["num_paths"]
        miss, steps = np.zeros(max(n_out, 1), dtype=np.uint64), np.zeros(max(n_out, 1), dtype=np.uint64)
        f = _Buf()
        self._ctx._check(self._lib.edsx_paths_gfa_walks(self._h, ids.ctypes.data if len(ids) else None, len(ids), nm,
                                                        prefix.encode() if prefix is not None else None, ctypes.byref(f),
                                                        miss.ctypes.data, steps.ctypes.data))
        return self._ctx._take(f), miss[:n_out], steps[:n_out]


class VcfSession(_Handle):
    """A multi-contig VCF and a multi-record FASTA kept in HBM (edsx_vcf_session_*): the FASTA record index, the contig of
    every record line, and one transform per contig without another upload.  vcf=b"": the FASTA index alone."""
    _destroy = "edsx_vcf_session_close"

    def __init__(self, ctx, vcf, fasta, compressed=False):
        self._ctx, self._lib = ctx, ctx._lib
        self._compressed = compressed
        h = ctypes.c_void_p()
        if compressed:                                             # gzip / BGZF inputs: the session owns what it needs
            vcf, fasta = bytes(vcf), bytes(fasta)
            ctx._check(self._lib.edsx_vcf_session_open_z(ctx._h, vcf, len(vcf), fasta, len(fasta), ctypes.byref(h)))
            self._h = h
            return
        self._vcf, self._fasta = bytes(vcf), bytes(fasta)          # the library reads them until close()
        ctx._check(self._lib.edsx_vcf_session_open(ctx._h, self._vcf, len(self._vcf), self._fasta, len(self._fasta),
                                                   ctypes.byref(h)))
        self._h = h

    def contigs(self):
        """FASTA records in file order: dicts of the edsx_contig fields plus "name" (bytes)."""
        p, n = ctypes.POINTER(Contig)(), ctypes.c_size_t()
        self._ctx._check(self._lib.edsx_vcf_session_contigs(self._h, ctypes.byref(p), ctypes.byref(n)))
        out = []
        for i in range(n.value):
            d = _fields(p[i])
            if self._compressed:                                   # (name_off points into the inflated FASTA)
                q, ln = ctypes.c_char_p(), ctypes.c_size_t()
                self._ctx._check(self._lib.edsx_vcf_session_contig_name(self._h, i, ctypes.byref(q), ctypes.byref(ln)))
                d["name"] = ctypes.string_at(q, ln.value)
            else:
                d["name"] = self._fasta[d["name_off"]:d["name_off"] + d["name_len"]]
            out.append(d)
        return out

    def find(self, name):
        i = ctypes.c_size_t()
        self._ctx._check(self._lib.edsx_vcf_session_find(self._h, _name(name), ctypes.byref(i)))
        return i.value

    def transform(self, contig, context_len=0):
        """contig: a record index, or a name (its first record).  (eds, seds, stats) as Context.vcf_transform."""
        index = contig if isinstance(contig, int) else self.find(contig)
        e, s, st = _Buf(), _Buf(), VcfStats()
        self._ctx._check(self._lib.edsx_vcf_session_transform(self._h, index, context_len, ctypes.byref(e), ctypes.byref(s),
                                                              ctypes.byref(st)))
        return self._ctx._take(e), self._ctx._take(s), _fields(st)

    def info(self):
        st = VcfSessionStats()
        self._ctx._check(self._lib.edsx_vcf_session_info(self._h, ctypes.byref(st)))
        return _fields(st)

    def unknown_contigs(self):
        """[(name, record lines)] of the contigs the VCF names and the FASTA lacks."""
        b = _Buf()
        self._ctx._check(self._lib.edsx_vcf_session_unknown_contigs(self._h, ctypes.byref(b)))
        return [(ln.rsplit(b"\t", 1)[0], int(ln.rsplit(b"\t", 1)[1])) for ln in self._ctx._take(b).split(b"\n") if ln]
