"""ctypes binding of libblu_consensus.so (include/blu_consensus.h)."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# BLU_CONSENSUS_LIB: load an experimental build of the same ABI (kernel A/B experiments under scripts/)
LIB_PATH = os.environ.get("BLU_CONSENSUS_LIB") or os.path.join(_HERE, "lib", "libblu_consensus.so")

# every symbol include/blu_consensus.h declares
EXPORTS = (
    "blu_abi_version", "blu_last_error", "blu_consensus_run_multi", "blu_shard_ranges", "blu_taxonomy_create", "blu_taxonomy_destroy", "blu_taxonomy_n_tax",
    "blu_taxonomy_n_shapes", "blu_taxonomy_n_rank_codes", "blu_taxonomy_max_depth", "blu_taxonomy_device_bytes",
    "blu_taxonomy_rank_name", "blu_taxonomy_row_cutoffs", "blu_taxonomy_lookup", "blu_taxonomy_row_map", "blu_consensus_run",
    "blu_consensus_last_launch", "blu_hits_pack", "blu_hits_pack64", "blu_taxonomy_shared_levels", "blu_taxonomy_trim",
    "blu_consensus_report", "blu_report_free", "blu_dev_exclusive_scan", "blu_dev_radix_sort_pairs", "blu_dev_line_index",
    "blu_consensus_sample_table", "blu_sample_table_free", "blu_consensus_support", "blu_hits_score_band",
    "blu_hits_subject_keep", "blu_hits_subject_best", "blu_hits_cover_keep", "blu_hits_cover_apply",
    "blu_consensus_sample_table_counts", "blu_sample_distances", "blu_sample_distance_free",
    "blu_rarefy_stream", "blu_sample_rarefy", "blu_rarefied_free", "blu_alpha_log2", "blu_sample_alpha", "blu_alpha_free",
)
# include/blu_pipeline.h
PIPELINE_EXPORTS = ("blu_build_consensus", "blu_build_consensus_with", "blu_build_consensus_identities", "blu_build_consensus_identities_cfg",
                    "blu_build_consensus_identities_to_file", "blu_free_text", "blu_custom_taxon_from_file", "blu_ingest_only",
                    "blu_ingest_only_on", "blu_ingest_columns_on", "blu_ingest_columns_selected", "blu_ingest_columns_free",
                    "blu_last_ingest_path", "blu_last_min_cover_stats", "blu_db_cache_build", "blu_taxdb_build", "blu_seqdb_export", "blu_qiime_taxonomy_tsv",
                    "blu_seqdb_export_labelled", "blu_seqdb_render_labels", "blu_table_layout_parse", "blu_build_consensus_laid_out",
                    "blu_ingest_columns_laid_out", "blu_query_cover_parse", "blu_build_consensus_covered", "blu_ingest_columns_covered",
                    "blu_lineage_db_build", "blu_distance_features_from_table", "blu_distance_features_free", "blu_distance_render",
                    "blu_distance_matrix_file", "blu_distance_matrix_file_with", "blu_alpha_render", "blu_alpha_table_file")

BLU_UNMATCHED_TAXID = 0xFFFFFFFF
BLU_NONE_U8, BLU_NONE_U16, BLU_MAR_NEVER_EQUAL = 0xFF, 0xFFFF, 0xFFFE
BLU_OK, BLU_ERR_INVALID_ARG, BLU_ERR_NO_DEVICE, BLU_ERR_HIP, BLU_ERR_DEPTH, BLU_ERR_CUSTOM_MISSING = 0, 1, 2, 3, 4, 5
BLU_ERR_INTERNAL = 10
ST_MULTI, ST_SINGLE, ST_NO_HITS = 0, 1, 2
ST_ERR_UNMATCHED, ST_ERR_BAD_LINEAGE, ST_ERR_ROOT, ST_ERR_SINGLE_BELOW, ST_ERR_BAD_PIDENT = 16, 17, 18, 19, 20
FLAG_MUTATED, FLAG_AGREE = 1, 2
TAXON = {"fungi": 0, "bacteria": 1, "eukaryotes": 2, "custom": 3}
STRATEGY = {"cautious": 0, "relaxed": 1}
CUSTOM_FIELDS = ("domain", "kingdom", "phylum", "class", "order", "family", "genus", "species")


class CutoffConfig(C.Structure):
    _fields_ = [("taxon", C.c_int32), ("has_custom", C.c_int32), ("custom", C.c_int16 * 8),
                ("custom_has", C.c_uint8 * 8)]


class TaxonomyDesc(C.Structure):
    _fields_ = [("n_tax", C.c_uint64), ("taxid", C.c_void_p), ("lin_off", C.c_void_p), ("lin_node", C.c_void_p),
                ("lin_rank", C.c_void_p), ("n_ranks", C.c_uint32), ("rank_names", C.c_void_p), ("bad", C.c_void_p)]


class Hits(C.Structure):
    _fields_ = [("bitscore", C.c_void_p), ("tax_row", C.c_void_p), ("pident", C.c_void_p), ("align_len", C.c_void_p),
                ("acc_rank", C.c_void_p), ("seg_off", C.c_void_p), ("n_hits", C.c_uint64), ("n_queries", C.c_uint64),
                ("on_device", C.c_int32), ("reserved", C.c_int32), ("pident_milli", C.c_void_p), ("packed", C.c_void_p),
                ("packed64", C.c_void_p)]


class RunParams(C.Structure):
    _fields_ = [("strategy", C.c_int32), ("flags", C.c_int32), ("stream", C.c_void_p)]


BAND_TOP_PERCENT, BAND_TOP_BITS = 1, 2


class ScoreBandC(C.Structure):
    """include/blu_consensus.h: blu_score_band"""
    _fields_ = [("top_percent_milli", C.c_uint32), ("mask", C.c_uint32), ("top_bits", C.c_uint64)]


class ScoreBandStats(C.Structure):
    """include/blu_consensus.h: blu_score_band_stats"""
    _fields_ = [("n_hits", C.c_uint64), ("n_raised", C.c_uint64), ("n_queries", C.c_uint64), ("n_widened", C.c_uint64)]


def band_counts(st: ScoreBandStats) -> dict:
    return {f: int(getattr(st, f)) for f, _ in ScoreBandStats._fields_}


SUBJECT_BEST_PER_QUERY = 1


class SubjectBestC(C.Structure):
    """include/blu_consensus.h: blu_subject_best"""
    _fields_ = [("mask", C.c_uint32), ("reserved", C.c_uint32)]


class SubjectBestStats(C.Structure):
    """include/blu_consensus.h: blu_subject_best_stats"""
    _fields_ = [("n_hits", C.c_uint64), ("n_kept", C.c_uint64), ("n_queries", C.c_uint64), ("n_thinned", C.c_uint64)]


def subject_counts(st: SubjectBestStats) -> dict:
    return {f: int(getattr(st, f)) for f, _ in SubjectBestStats._fields_}


MIN_COVER_MILLI_LOW, MIN_COVER_MILLI_HIGH = 50001, 100000


class MinCoverStats(C.Structure):
    """include/blu_consensus.h: blu_min_cover_stats"""
    _fields_ = [("n_hits", C.c_uint64), ("n_kept", C.c_uint64), ("n_queries", C.c_uint64), ("n_narrowed", C.c_uint64),
                ("n_unresolved", C.c_uint64)]


def cover_counts(st: MinCoverStats) -> dict:
    return {f: int(getattr(st, f)) for f, _ in MinCoverStats._fields_}


DISTANCE_MAX_SAMPLES, DISTANCE_CHUNK, DISTANCE_PARTNERS = 4096, 8192, 64


class DistanceDesc(C.Structure):
    """include/blu_consensus.h: blu_distance_desc"""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("n_features", C.c_uint64), ("n_samples", C.c_uint32),
                ("reserved", C.c_uint32), ("row_ptr", C.c_void_p), ("sample", C.c_void_p), ("count", C.c_void_p), ("stream", C.c_void_p)]


class SampleDistance(C.Structure):
    """include/blu_consensus.h: blu_sample_distance"""
    _fields_ = [("n_samples", C.c_uint32), ("reserved", C.c_uint32), ("total", C.POINTER(C.c_uint64)),
                ("richness", C.POINTER(C.c_uint32)), ("min_sum", C.POINTER(C.c_uint64)), ("shared", C.POINTER(C.c_uint32)),
                ("t_device_ms", C.c_double)]


RAREFY_TILE, RAREFY_MAX_READS = 65536, 1 << 36


class RarefyDesc(C.Structure):
    """include/blu_consensus.h: blu_rarefy_desc"""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("n_features", C.c_uint64), ("n_samples", C.c_uint32),
                ("reserved", C.c_uint32), ("row_ptr", C.c_void_p), ("sample", C.c_void_p), ("count", C.c_void_p),
                ("sample_stream", C.c_void_p), ("depth", C.c_uint64), ("stream", C.c_void_p)]


class Rarefied(C.Structure):
    """include/blu_consensus.h: blu_rarefied"""
    _fields_ = [("n_features", C.c_uint64), ("n_kept", C.c_uint32), ("reserved", C.c_uint32), ("kept_sample", C.POINTER(C.c_uint32)),
                ("row_ptr", C.POINTER(C.c_uint64)), ("sample", C.POINTER(C.c_uint32)), ("count", C.POINTER(C.c_uint64)),
                ("t_device_ms", C.c_double)]


ALPHA_MAX_DEPTHS, ALPHA_TILE = 32, 8192


class AlphaDesc(C.Structure):
    """include/blu_consensus.h: blu_alpha_desc"""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("n_features", C.c_uint64), ("n_samples", C.c_uint32),
                ("n_depths", C.c_uint32), ("row_ptr", C.c_void_p), ("sample", C.c_void_p), ("count", C.c_void_p),
                ("sample_stream", C.c_void_p), ("depths", C.c_void_p), ("stream", C.c_void_p)]


class Alpha(C.Structure):
    """include/blu_consensus.h: blu_alpha"""
    _fields_ = [("n_samples", C.c_uint32), ("n_slots", C.c_uint32), ("present", C.POINTER(C.c_uint8)), ("n", C.POINTER(C.c_uint64)),
                ("observed", C.POINTER(C.c_uint32)), ("singletons", C.POINTER(C.c_uint32)), ("doubletons", C.POINTER(C.c_uint32)),
                ("sum_sq", C.POINTER(C.c_uint64)), ("sum_xlog", C.POINTER(C.c_uint64)), ("t_device_ms", C.c_double)]


class NativeLibraryMissing(RuntimeError):
    pass


_lib = None


def lib() -> C.CDLL:
    """Loads the HIP library; raises loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryMissing(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C blutils_amd/csrc).  blutils_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    L.blu_abi_version.restype = C.c_uint32
    L.blu_last_error.restype = C.c_size_t
    L.blu_last_error.argtypes = [C.c_char_p, C.c_size_t]
    L.blu_taxonomy_create.restype = C.c_int
    L.blu_taxonomy_create.argtypes = [C.POINTER(TaxonomyDesc), C.POINTER(CutoffConfig), C.c_int, C.POINTER(C.c_void_p)]
    L.blu_taxonomy_destroy.argtypes = [C.c_void_p]
    for name, rt in (("blu_taxonomy_n_tax", C.c_uint64), ("blu_taxonomy_n_shapes", C.c_uint32),
                     ("blu_taxonomy_n_rank_codes", C.c_uint32), ("blu_taxonomy_max_depth", C.c_uint32),
                     ("blu_taxonomy_device_bytes", C.c_uint64)):
        getattr(L, name).restype = rt
        getattr(L, name).argtypes = [C.c_void_p]
    L.blu_taxonomy_rank_name.restype = C.c_char_p
    L.blu_taxonomy_rank_name.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
    L.blu_taxonomy_row_cutoffs.restype = C.c_int32
    L.blu_taxonomy_row_cutoffs.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.blu_taxonomy_lookup.restype = C.c_int
    L.blu_taxonomy_lookup.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.blu_taxonomy_row_map.restype = C.c_int
    L.blu_taxonomy_row_map.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.blu_consensus_run.restype = C.c_int
    L.blu_consensus_run.argtypes = [C.c_void_p, C.POINTER(Hits), C.POINTER(RunParams), C.c_void_p]
    for name in ("blu_hits_pack", "blu_hits_pack64"):
        if not hasattr(L, name):                 # (an A/B library of an older ABI: BLU_CONSENSUS_LIB, scripts/ab.sh)
            continue
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [C.c_void_p, C.POINTER(Hits), C.c_void_p, C.c_void_p]
    if hasattr(L, "blu_taxonomy_shared_levels"):
        L.blu_taxonomy_shared_levels.restype = C.c_int
        L.blu_taxonomy_shared_levels.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
        L.blu_taxonomy_trim.restype = C.c_int
        L.blu_taxonomy_trim.argtypes = [C.c_void_p]
    if hasattr(L, "blu_dev_exclusive_scan"):
        L.blu_dev_exclusive_scan.restype = C.c_int
        L.blu_dev_exclusive_scan.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
        L.blu_dev_radix_sort_pairs.restype = C.c_int
        L.blu_dev_radix_sort_pairs.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int]
        L.blu_dev_line_index.restype = C.c_int
        L.blu_dev_line_index.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    if hasattr(L, "blu_hits_score_band"):        # (an A/B library of an older build: BLU_CONSENSUS_LIB)
        L.blu_hits_score_band.restype = C.c_int
        L.blu_hits_score_band.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(ScoreBandC),
                                          C.c_void_p, C.c_void_p, C.POINTER(ScoreBandStats)]
    if hasattr(L, "blu_hits_subject_keep"):      # (an A/B library of an older build: BLU_CONSENSUS_LIB)
        L.blu_hits_subject_keep.restype = C.c_int
        L.blu_hits_subject_keep.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p,
                                            C.c_void_p, C.POINTER(SubjectBestStats)]
        L.blu_hits_subject_best.restype = C.c_int
        L.blu_hits_subject_best.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                            C.c_uint64, C.c_int, C.POINTER(SubjectBestC), C.c_void_p, C.c_uint32,
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(SubjectBestStats)]
    if hasattr(L, "blu_hits_cover_keep"):        # (an A/B library of an older build: BLU_CONSENSUS_LIB)
        L.blu_hits_cover_keep.restype = C.c_int
        L.blu_hits_cover_keep.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int,
                                          C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MinCoverStats)]
        L.blu_hits_cover_apply.restype = C.c_int
        L.blu_hits_cover_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.c_void_p, C.c_uint32,
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(MinCoverStats)]
        L.blu_last_min_cover_stats.restype = C.c_int
        L.blu_last_min_cover_stats.argtypes = [C.POINTER(MinCoverStats)]
    if hasattr(L, "blu_sample_distances"):       # (an A/B library of an older build: BLU_CONSENSUS_LIB)
        L.blu_sample_distances.restype = C.c_int
        L.blu_sample_distances.argtypes = [C.POINTER(DistanceDesc), C.POINTER(SampleDistance)]
        L.blu_sample_distance_free.argtypes = [C.POINTER(SampleDistance)]
    if hasattr(L, "blu_sample_rarefy"):          # (an A/B library of an older build: BLU_CONSENSUS_LIB)
        L.blu_rarefy_stream.restype = C.c_uint64
        L.blu_rarefy_stream.argtypes = [C.c_uint64, C.c_char_p, C.c_uint64]
        L.blu_sample_rarefy.restype = C.c_int
        L.blu_sample_rarefy.argtypes = [C.POINTER(RarefyDesc), C.POINTER(Rarefied)]
        L.blu_rarefied_free.argtypes = [C.POINTER(Rarefied)]
    if hasattr(L, "blu_sample_alpha"):           # (an A/B library of an older build: BLU_CONSENSUS_LIB)
        L.blu_alpha_log2.restype = C.c_uint64
        L.blu_alpha_log2.argtypes = [C.c_uint64]
        L.blu_sample_alpha.restype = C.c_int
        L.blu_sample_alpha.argtypes = [C.POINTER(AlphaDesc), C.POINTER(Alpha)]
        L.blu_alpha_free.argtypes = [C.POINTER(Alpha)]
    L.blu_consensus_last_launch.restype = C.c_int
    L.blu_consensus_last_launch.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    _lib = L
    return L


def last_error() -> str:
    buf = C.create_string_buffer(1024)
    lib().blu_last_error(buf, 1024)
    return buf.value.decode("utf-8", "replace")


class BluError(RuntimeError):
    def __init__(self, code: int, where: str):
        self.code = code
        super().__init__(f"{where} failed with blu_error {code}: {last_error()}")
