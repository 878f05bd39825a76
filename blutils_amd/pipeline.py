"""ctypes front end of the host pipeline (include/blu_pipeline.h): the drop-in for the reference use-case

    build_consensus_identities(blast_output, taxonomies_file, taxon, strategy, use_taxid, custom_taxon_values)
    (core/src/use_cases/build_consensus_identities/mod.rs:40-47)  +  write_blutils_output (write_blutils_output.rs:33)

Same argument names and meaning; the consensus itself runs on the GPU (no CPU fallback).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import decimal
import json
from typing import Optional, Sequence, Union

from . import _native as N

OUT_FORMAT = {"json": 0, "jsonl": 1, "yaml": 2, "json-compact": 3}
BLU_ERR_REFERENCE_PANIC = 9


class PipelineParams(C.Structure):
    _fields_ = [("cutoffs", N.CutoffConfig), ("strategy", C.c_int32), ("use_taxid", C.c_int32), ("device", C.c_int32),
                ("out_format", C.c_int32), ("lenient", C.c_int32), ("reserved", C.c_int32)]


class PipelineStats(C.Structure):
    _fields_ = [("n_hits", C.c_uint64), ("n_queries", C.c_uint64), ("n_taxids", C.c_uint64),
                ("n_unmatched_rows", C.c_uint64), ("t_load_db_s", C.c_double), ("t_load_hits_s", C.c_double),
                ("t_engine_s", C.c_double), ("t_render_s", C.c_double)]


@dataclasses.dataclass(frozen=True)
class HitFilter:
    """Thresholds on the table's lines (include/blu_pipeline.h: blu_hit_filter; not in the reference).  A line
    is kept when every threshold that is not None holds; the run then gives what it gives on a copy of the table without
    the other lines.  min_bit_score compares the score as written, before its truncation."""
    min_perc_identity: Optional[float] = None
    min_align_length: Optional[int] = None
    max_e_value: Optional[float] = None
    min_bit_score: Optional[float] = None

    def active(self) -> bool:
        return any(v is not None for v in dataclasses.astuple(self))


class HitFilterC(C.Structure):
    _fields_ = [("min_perc_identity", C.c_double), ("min_align_length", C.c_int64), ("max_e_value", C.c_double),
                ("min_bit_score", C.c_double), ("mask", C.c_uint32), ("reserved", C.c_uint32)]


class HitFilterStats(C.Structure):
    _fields_ = [("n_lines", C.c_uint64), ("n_kept", C.c_uint64)]


FILTER_BITS = {"min_perc_identity": 1, "min_align_length": 2, "max_e_value": 4, "min_bit_score": 8}


def _hit_filter(hit_filter: Union[None, dict, HitFilter]) -> Optional[HitFilterC]:
    """None -> None (today's calls); a dict or HitFilter -> the C struct (an empty one has an empty mask)."""
    if hit_filter is None:
        return None
    if isinstance(hit_filter, HitFilter):
        hit_filter = dataclasses.asdict(hit_filter)
    unknown = set(hit_filter) - set(FILTER_BITS)
    if unknown:
        raise ValueError(f"hit_filter: unknown keys {sorted(unknown)}")
    f = HitFilterC()
    for key, bit in FILTER_BITS.items():
        v = hit_filter.get(key)
        if v is None:
            continue
        if key == "min_align_length":
            if int(v) != v or not -(1 << 63) <= int(v) < (1 << 63):
                raise ValueError(f"hit_filter: min_align_length must be an integer, got {v!r}")
            v = int(v)
        else:
            v = float(v)
        setattr(f, key, v)
        f.mask |= bit
    return f


@dataclasses.dataclass(frozen=True)
class TaxonFilter:
    """Lines dropped by the lineage of their subject (include/blu_pipeline.h: blu_taxon_filter; not in the
    reference).  Elements are spelled `RANK__IDENTIFIER` as in the lineage flavour of the run (`s__1423` under use_taxid); an
    identifier ending in `*` is a prefix pattern.  A line passes when none of its lineage's elements is in `exclude` and, if
    `only` is not empty, at least one is in `only`; an element that names no taxon of the taxonomies file is an error."""
    exclude: Sequence[str] = ()
    only: Sequence[str] = ()

    def active(self) -> bool:
        return bool(self.exclude) or bool(self.only)


class TaxonFilterC(C.Structure):
    _fields_ = [("exclude", C.POINTER(C.c_char_p)), ("n_exclude", C.c_uint64), ("only", C.POINTER(C.c_char_p)),
                ("n_only", C.c_uint64)]


class TaxonFilterStats(C.Structure):
    _fields_ = [("n_lines", C.c_uint64), ("n_excluded", C.c_uint64), ("n_not_only", C.c_uint64),
                ("excluded_by", C.POINTER(C.c_uint64))]


class _TaxonArgs:
    """The C filter of one call and the arrays it points into."""

    def __init__(self, exclude, only):
        self.exclude, self.only = [str(e) for e in exclude], [str(e) for e in only]
        self._ex = (C.c_char_p * max(1, len(self.exclude)))(*[e.encode() for e in self.exclude])
        self._on = (C.c_char_p * max(1, len(self.only)))(*[e.encode() for e in self.only])
        self.by = (C.c_uint64 * max(1, len(self.exclude)))()      # (the caller's excluded_by array)
        self.filter = TaxonFilterC(self._ex, len(self.exclude), self._on, len(self.only))

    def counts(self, st: TaxonFilterStats) -> dict:
        return {"n_lines": int(st.n_lines), "n_excluded": int(st.n_excluded), "n_not_only": int(st.n_not_only),
                "exclude": list(self.exclude), "excluded_by": [int(self.by[k]) for k in range(len(self.exclude))]}


def _taxon_filter(taxon_filter: Union[None, dict, TaxonFilter]) -> Optional[_TaxonArgs]:
    """None or two empty lists -> None (the calls without it); a dict or TaxonFilter -> the C structs."""
    if taxon_filter is None:
        return None
    if isinstance(taxon_filter, TaxonFilter):
        taxon_filter = {"exclude": taxon_filter.exclude, "only": taxon_filter.only}
    unknown = set(taxon_filter) - {"exclude", "only"}
    if unknown:
        raise ValueError(f"taxon_filter: unknown keys {sorted(unknown)}")
    exclude, only = taxon_filter.get("exclude") or (), taxon_filter.get("only") or ()
    if isinstance(exclude, str) or isinstance(only, str):
        raise ValueError("taxon_filter: exclude and only are lists of elements")
    if not exclude and not only:
        return None
    return _TaxonArgs(exclude, only)


def top_percent_milli(value) -> int:
    """A --top-percent value -> thousandths of a percent (0 .. 100000), exactly: a decimal with at most three decimals in
    0 .. 100.  Read with decimal.Decimal (never through a float); anything else — NaN, infinities, a fourth decimal, an
    exponent form that is no whole number of thousandths — is a ValueError."""
    if isinstance(value, (float, bool)):
        raise ValueError(f"top_percent: pass a decimal string or decimal.Decimal, not {value!r}")
    try:
        d = value if isinstance(value, decimal.Decimal) else decimal.Decimal(str(value).strip())
    except decimal.InvalidOperation:
        raise ValueError(f"top_percent: not a decimal number: {value!r}")
    if not d.is_finite():
        raise ValueError(f"top_percent: not a finite number: {value!r}")
    if not 0 <= d <= 100:
        raise ValueError(f"top_percent: must be between 0 and 100, got {value!r}")
    m = d * 1000
    if m != m.to_integral_value():
        raise ValueError(f"top_percent: at most three decimals, got {value!r}")
    return int(m)


def min_cover_milli(value) -> int:
    """A --min-cover value -> thousandths of a percent (50001 .. 100000), exactly: a decimal with at most three decimals, above
    50 and at most 100.  Read with decimal.Decimal (never through a float); anything else — NaN, infinities, a fourth decimal,
    50 itself — is a ValueError."""
    if isinstance(value, (float, bool)):
        raise ValueError(f"min_cover: pass a decimal string or decimal.Decimal, not {value!r}")
    try:
        d = value if isinstance(value, decimal.Decimal) else decimal.Decimal(str(value).strip())
    except decimal.InvalidOperation:
        raise ValueError(f"min_cover: not a decimal number: {value!r}")
    if not d.is_finite():
        raise ValueError(f"min_cover: not a finite number: {value!r}")
    m = d * 1000
    if m != m.to_integral_value():
        raise ValueError(f"min_cover: at most three decimals, got {value!r}")
    if not 50 < d <= 100:
        raise ValueError(f"min_cover: must be above 50 and at most 100, got {value!r}")
    return int(m)


def top_bits_value(value) -> int:
    """A --top-bits value: an integer in 0 .. 2^32 - 1."""
    if isinstance(value, (float, bool)) or (not isinstance(value, int) and not str(value).strip().lstrip("+-").isdigit()):
        raise ValueError(f"top_bits: not an integer: {value!r}")
    v = int(value)
    if not 0 <= v < (1 << 32):
        raise ValueError(f"top_bits: must be between 0 and 2^32 - 1, got {value!r}")
    return v


@dataclasses.dataclass(frozen=True)
class ScoreBand:
    """A band under each query's top bit-score inside which hits count as tied (include/blu_consensus.h: blu_score_band;
    DESIGN.md §17; not in the reference).  top_percent: a decimal string or Decimal with at most three decimals, 0 .. 100 —
    a hit with truncated score b is in the band under the top t when b * 100000 >= t * (100000 - 1000 * top_percent);
    top_bits: an integer — when b >= t - top_bits.  Both given: both must hold.  In-band hits get the score t before the
    engine runs; the run then gives what it gives on a copy of the table with column 12 of those lines rewritten."""
    top_percent: Union[None, str, decimal.Decimal] = None
    top_bits: Optional[int] = None

    def active(self) -> bool:
        return self.top_percent is not None or self.top_bits is not None


def _score_band(score_band: Union[None, dict, ScoreBand]) -> Optional[N.ScoreBandC]:
    """None or no criterion -> None (the calls without it); a dict or ScoreBand -> the C struct."""
    if score_band is None:
        return None
    if isinstance(score_band, ScoreBand):
        score_band = {"top_percent": score_band.top_percent, "top_bits": score_band.top_bits}
    unknown = set(score_band) - {"top_percent", "top_bits"}
    if unknown:
        raise ValueError(f"score_band: unknown keys {sorted(unknown)}")
    b = N.ScoreBandC(0, 0, 0)
    if score_band.get("top_percent") is not None:
        b.top_percent_milli = top_percent_milli(score_band["top_percent"])
        b.mask |= N.BAND_TOP_PERCENT
    if score_band.get("top_bits") is not None:
        b.top_bits = top_bits_value(score_band["top_bits"])
        b.mask |= N.BAND_TOP_BITS
    return b if b.mask else None


class HitSelection(C.Structure):
    """include/blu_pipeline.h: blu_hit_selection (NULL members: not asked for)"""
    _fields_ = [("hit_filter", C.POINTER(HitFilterC)), ("taxon_filter", C.POINTER(TaxonFilterC)),
                ("subject_best", C.POINTER(N.SubjectBestC)), ("score_band", C.POINTER(N.ScoreBandC))]


class HitSelectionStats(C.Structure):
    """include/blu_pipeline.h: blu_hit_selection_stats"""
    _fields_ = [("hit_filter", HitFilterStats), ("taxon_filter", TaxonFilterStats), ("subject_best", N.SubjectBestStats),
                ("score_band", N.ScoreBandStats)]


class ConsensusRequest(C.Structure):
    """include/blu_pipeline.h: blu_consensus_request"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("blast_output_file", C.c_char_p),
                ("headers", C.POINTER(C.c_char_p)), ("n_headers", C.c_uint64), ("taxonomies_file", C.c_char_p),
                ("params", C.POINTER(PipelineParams)), ("run_id_text", C.c_char_p), ("config_text", C.c_char_p),
                ("out_path", C.c_char_p), ("report_path", C.c_char_p), ("sample_table_path", C.c_char_p), ("weight", C.c_int32),
                ("min_cover_milli", C.c_int32), ("support_table_path", C.c_char_p), ("selection", HitSelection)]


class ConsensusOutcome(C.Structure):
    """include/blu_pipeline.h: blu_consensus_outcome"""
    _fields_ = [("text", C.c_void_p), ("text_len", C.c_size_t), ("stats", PipelineStats), ("selection", HitSelectionStats)]


class CountTableStats(C.Structure):
    """include/blu_pipeline.h: blu_count_table_stats"""
    _fields_ = [("n_rows", C.c_uint64), ("n_samples", C.c_uint64), ("n_joined", C.c_uint64), ("n_rows_unclassified", C.c_uint64)]


class ConsensusExtras(C.Structure):
    """include/blu_pipeline.h: blu_consensus_extras"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("count_table_path", C.c_char_p),
                ("count_table_stats", C.POINTER(CountTableStats))]


TABLE_LAYOUT_NO_COLUMN = 0xFFFFFFFF
TABLE_LAYOUT_MAX_COLUMNS = 64
REFERENCE_OUTFMT = "6 qseqid saccver staxid pident length mismatch gapopen qstart qend sstart send evalue bitscore"


class TableLayoutC(C.Structure):
    """include/blu_pipeline.h: blu_table_layout"""
    _fields_ = [("struct_size", C.c_uint32), ("n_columns", C.c_uint32), ("query", C.c_uint32), ("accession", C.c_uint32),
                ("taxid", C.c_uint32), ("perc_identity", C.c_uint32), ("align_length", C.c_uint32), ("bit_score", C.c_uint32),
                ("e_value", C.c_uint32), ("taxid_is_list", C.c_uint32)]

    def as_dict(self) -> dict:
        d = {f: int(getattr(self, f)) for f, _ in self._fields_ if f != "struct_size"}
        d["e_value"] = None if d["e_value"] == TABLE_LAYOUT_NO_COLUMN else d["e_value"]
        d["taxid_is_list"] = bool(d["taxid_is_list"])
        return d

    def is_reference(self) -> bool:
        """the reference's thirteen columns in the reference's order: the call without a layout"""
        return self.as_dict() == {"n_columns": 13, "query": 0, "accession": 1, "taxid": 2, "perc_identity": 3, "align_length": 4,
                                  "bit_score": 12, "e_value": 11, "taxid_is_list": False}


def table_layout(blast_outfmt: str) -> TableLayoutC:
    """BLAST's own format string (`6 std staxids`, `qseqid sacc staxid pident length bitscore qcovs`, ...) -> the column layout
    (include/blu_pipeline.h: blu_table_layout_parse).  A string the library refuses is a BluError whose message
    names the offending token."""
    L = _bind()
    lay = TableLayoutC(struct_size=C.sizeof(TableLayoutC))
    rc = L.blu_table_layout_parse(str(blast_outfmt).encode(), C.byref(lay))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_table_layout_parse")
    return lay


def _layout(blast_outfmt) -> Optional[TableLayoutC]:
    """None, or a string that names the reference's own columns -> None (today's calls); else the C struct."""
    if blast_outfmt is None:
        return None
    lay = blast_outfmt if isinstance(blast_outfmt, TableLayoutC) else table_layout(blast_outfmt)
    return None if lay.is_reference() else lay


QUERY_COVER_SOURCE = {"auto": 0, "qcovhsp": 1, "qlen": 2, "qcovs": 3}
QUERY_COVER_SOURCE_NAME = {v: k for k, v in QUERY_COVER_SOURCE.items()}


def min_query_cover_milli(value) -> int:
    """A --min-query-cover value -> thousandths of a percent (0 .. 100000), exactly: a decimal with at most three decimals in
    0 .. 100, read as top_percent_milli reads --top-percent (never through a float)."""
    try:
        return top_percent_milli(value)
    except ValueError as e:
        raise ValueError(str(e).replace("top_percent", "min_query_cover", 1))


@dataclasses.dataclass(frozen=True)
class QueryCover:
    """Lines dropped by their query coverage, in the parser (include/blu_pipeline.h: blu_query_cover; the
    reference has it only as `-q` of its own blastn call).  percent: a decimal string or Decimal with at most three decimals,
    0 .. 100, read exactly.  source: `qcovhsp` (that column, BLAST's per-HSP integer percent c: kept iff c * 1000 >= 1000 *
    percent), `qlen` (the columns qstart, qend, qlen: kept iff (|qend - qstart| + 1) * 100000 >= 1000 * percent * qlen — the
    exact ratio, not BLAST's rounded percent), `qcovs` (that column, the coarser per-subject figure) or `auto`: the first of the
    three the format string has.  Needs blast_outfmt, which names the columns."""
    percent: Union[str, decimal.Decimal] = "0"
    source: str = "auto"


class QueryCoverStats(C.Structure):
    """include/blu_pipeline.h: blu_query_cover_stats"""
    _fields_ = [("n_lines", C.c_uint64), ("n_below", C.c_uint64)]


class QueryCoverC(C.Structure):
    """include/blu_pipeline.h: blu_query_cover"""
    _fields_ = [("struct_size", C.c_uint32), ("source", C.c_uint32), ("min_cover_milli", C.c_uint32), ("cover_column", C.c_uint32),
                ("qstart", C.c_uint32), ("qend", C.c_uint32), ("qlen", C.c_uint32), ("reserved", C.c_uint32),
                ("stats", C.POINTER(QueryCoverStats))]


class _Cover:
    """The C cover of one call, resolved against the format string, and the stats it points to."""

    def __init__(self, query_cover, blast_outfmt):
        if isinstance(query_cover, dict):
            unknown = set(query_cover) - {"percent", "source"}
            if unknown:
                raise ValueError(f"query_cover: unknown keys {sorted(unknown)}")
            query_cover = QueryCover(**query_cover)
        elif not isinstance(query_cover, QueryCover):
            query_cover = QueryCover(query_cover)
        if query_cover.source not in QUERY_COVER_SOURCE:
            raise ValueError(f"query_cover: source must be one of {sorted(QUERY_COVER_SOURCE)}, got {query_cover.source!r}")
        if not isinstance(blast_outfmt, str):
            raise ValueError("query_cover: the reference's columns hold no query length; blast_outfmt has to name the table's "
                             "columns, as the format string itself")
        self.milli = min_query_cover_milli(query_cover.percent)
        self.percent = str(query_cover.percent).strip()
        self.st = QueryCoverStats()
        self.c = QueryCoverC(struct_size=C.sizeof(QueryCoverC), min_cover_milli=self.milli, stats=C.pointer(self.st))
        self.layout = table_layout(blast_outfmt)          # (never turned into None: the cover reads through it)
        rc = _bind().blu_query_cover_parse(blast_outfmt.encode(), QUERY_COVER_SOURCE[query_cover.source], C.byref(self.c))
        if rc != N.BLU_OK:
            raise N.BluError(rc, "blu_query_cover_parse")

    def counts(self) -> dict:
        return {"n_lines": int(self.st.n_lines), "n_below": int(self.st.n_below), "percent": self.percent,
                "source": QUERY_COVER_SOURCE_NAME[int(self.c.source)]}


def query_cover_columns(blast_outfmt: str, source: str = "auto", percent="0") -> dict:
    """The cover a format string and a source resolve to (blu_query_cover_parse): source, cover_column, qstart, qend, qlen
    (None for the columns the source does not read) and min_cover_milli.  A refusal is a BluError naming the missing specifiers."""
    c = _Cover(QueryCover(percent, source), blast_outfmt).c
    col = lambda v: None if v == TABLE_LAYOUT_NO_COLUMN else int(v)
    return {"source": QUERY_COVER_SOURCE_NAME[int(c.source)], "cover_column": col(c.cover_column), "qstart": col(c.qstart),
            "qend": col(c.qend), "qlen": col(c.qlen), "min_cover_milli": int(c.min_cover_milli)}


class _Selection:
    """The keywords hit_filter / taxon_filter / score_band / best_hit_per_subject as the C struct, with what it points to kept
    alive, and the stats keys each of them adds."""

    def __init__(self, hit_filter, taxon_filter, score_band, best_hit_per_subject):
        self.flt, self.tf, self.band = _hit_filter(hit_filter), _taxon_filter(taxon_filter), _score_band(score_band)
        self.sel = N.SubjectBestC(N.SUBJECT_BEST_PER_QUERY, 0) if best_hit_per_subject else None
        ptr = lambda x: C.pointer(x) if x is not None else None
        self.c = HitSelection(ptr(self.flt), ptr(self.tf.filter) if self.tf is not None else None, ptr(self.sel), ptr(self.band))

    def stats(self) -> HitSelectionStats:
        st = HitSelectionStats()
        if self.tf is not None:
            st.taxon_filter.excluded_by = self.tf.by
        return st

    def counts(self, st: HitSelectionStats) -> dict:
        out = {}
        if self.flt is not None or self.tf is not None:
            out["n_lines"], out["n_kept"] = int(st.hit_filter.n_lines), int(st.hit_filter.n_kept)
        if self.tf is not None:
            out["taxon_filter"] = self.tf.counts(st.taxon_filter)
        if self.band is not None:
            out["score_band"] = N.band_counts(st.score_band)
        if self.sel is not None:
            out["subject_best"] = N.subject_counts(st.subject_best)
        return out


def last_min_cover_stats() -> dict:
    """blu_last_min_cover_stats: the minimum cover's counts of this thread's last blu_build_consensus (zeros when that run had no
    min_cover or failed)"""
    st = N.MinCoverStats()
    rc = N.lib().blu_last_min_cover_stats(C.byref(st))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_last_min_cover_stats")
    return N.cover_counts(st)


DISTANCE_DROP_UNCLASSIFIED = 1
DISTANCE_METRIC = {"bray-curtis": 0, "jaccard": 1}


class DistanceFeatures(C.Structure):
    """include/blu_pipeline.h: blu_distance_features"""
    _fields_ = [("n_features", C.c_uint64), ("n_samples", C.c_uint32), ("reserved", C.c_uint32), ("row_ptr", C.POINTER(C.c_uint64)),
                ("sample", C.POINTER(C.c_uint32)), ("count", C.POINTER(C.c_uint64)), ("sample_names", C.POINTER(C.c_char_p)),
                ("feature_text", C.POINTER(C.c_char_p)), ("n_dropped", C.c_uint64)]


class DistanceStats(C.Structure):
    """include/blu_pipeline.h: blu_distance_stats"""
    _fields_ = [("n_features", C.c_uint64), ("n_samples", C.c_uint64), ("n_nonzeros", C.c_uint64), ("n_dropped", C.c_uint64)]


class DistanceOptions(C.Structure):
    """include/blu_pipeline.h: blu_distance_options"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("depth", C.c_uint64), ("seed", C.c_uint64),
                ("rarefied_table_path", C.c_char_p)]


class DistanceStats2(C.Structure):
    """include/blu_pipeline.h: blu_distance_stats2"""
    _fields_ = [(f, C.c_uint64) for f in ("n_features", "n_samples", "n_nonzeros", "n_dropped", "depth", "n_samples_kept",
                                          "n_samples_dropped", "n_features_emptied", "n_reads_hashed")]


class AlphaOptions(C.Structure):
    """include/blu_pipeline.h: blu_alpha_options"""
    _fields_ = [("struct_size", C.c_uint32), ("n_depths", C.c_uint32), ("depths", C.POINTER(C.c_uint64)), ("seed", C.c_uint64)]


class AlphaStats(C.Structure):
    """include/blu_pipeline.h: blu_alpha_stats"""
    _fields_ = [(f, C.c_uint64) for f in ("n_features", "n_samples", "n_nonzeros", "n_dropped", "n_depths", "n_rows")] + [("t_device_ms", C.c_double)]


def _bind():
    L = N.lib()
    if hasattr(L, "blu_alpha_table_file"):       # (an A/B library of an older build: BLU_CONSENSUS_LIB)
        L.blu_alpha_render.restype = C.c_int
        L.blu_alpha_render.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(N.Alpha),
                                       C.c_char_p]
        L.blu_alpha_table_file.restype = C.c_int
        L.blu_alpha_table_file.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.c_int, C.c_char_p, C.POINTER(AlphaOptions),
                                           C.POINTER(AlphaStats)]
    if hasattr(L, "blu_distance_matrix_file_with"):   # (an A/B library of an older build: BLU_CONSENSUS_LIB)
        L.blu_distance_matrix_file_with.restype = C.c_int
        L.blu_distance_matrix_file_with.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_int, C.c_char_p,
                                                    C.POINTER(DistanceOptions), C.POINTER(DistanceStats2)]
    if hasattr(L, "blu_distance_matrix_file"):   # (an A/B library of an older build: BLU_CONSENSUS_LIB)
        L.blu_distance_features_from_table.restype = C.c_int
        L.blu_distance_features_from_table.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(DistanceFeatures)]
        L.blu_distance_features_free.argtypes = [C.POINTER(DistanceFeatures)]
        L.blu_distance_render.restype = C.c_int
        L.blu_distance_render.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(N.SampleDistance), C.c_char_p]
        L.blu_distance_matrix_file.restype = C.c_int
        L.blu_distance_matrix_file.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_int, C.c_char_p, C.POINTER(DistanceStats)]
    L.blu_build_consensus.restype = C.c_int
    L.blu_build_consensus.argtypes = [C.POINTER(ConsensusRequest), C.POINTER(ConsensusOutcome)]
    L.blu_build_consensus_with.restype = C.c_int
    L.blu_build_consensus_with.argtypes = [C.POINTER(ConsensusRequest), C.POINTER(ConsensusExtras), C.POINTER(ConsensusOutcome)]
    L.blu_ingest_columns_selected.restype = C.c_int
    L.blu_ingest_columns_selected.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(HitSelection),
                                              C.POINTER(IngestColumns), C.POINTER(HitSelectionStats)]
    L.blu_ingest_columns_free.argtypes = [C.POINTER(IngestColumns)]
    if hasattr(L, "blu_table_layout_parse"):     # (an A/B library of an older build: BLU_CONSENSUS_LIB)
        L.blu_table_layout_parse.restype = C.c_int
        L.blu_table_layout_parse.argtypes = [C.c_char_p, C.POINTER(TableLayoutC)]
        L.blu_build_consensus_laid_out.restype = C.c_int
        L.blu_build_consensus_laid_out.argtypes = [C.POINTER(ConsensusRequest), C.POINTER(ConsensusExtras), C.POINTER(TableLayoutC),
                                                   C.POINTER(ConsensusOutcome)]
        L.blu_ingest_columns_laid_out.restype = C.c_int
        L.blu_ingest_columns_laid_out.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(TableLayoutC), C.POINTER(HitSelection),
                                                  C.POINTER(IngestColumns), C.POINTER(HitSelectionStats)]
    if hasattr(L, "blu_query_cover_parse"):      # (an A/B library of an older build: BLU_CONSENSUS_LIB)
        L.blu_query_cover_parse.restype = C.c_int
        L.blu_query_cover_parse.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(QueryCoverC)]
        L.blu_build_consensus_covered.restype = C.c_int
        L.blu_build_consensus_covered.argtypes = [C.POINTER(ConsensusRequest), C.POINTER(ConsensusExtras), C.POINTER(TableLayoutC),
                                                  C.POINTER(QueryCoverC), C.POINTER(ConsensusOutcome)]
        L.blu_ingest_columns_covered.restype = C.c_int
        L.blu_ingest_columns_covered.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(TableLayoutC), C.POINTER(QueryCoverC),
                                                 C.POINTER(HitSelection), C.POINTER(IngestColumns), C.POINTER(HitSelectionStats)]
    L.blu_free_text.argtypes = [C.c_void_p]
    L.blu_custom_taxon_from_file.restype = C.c_int
    L.blu_custom_taxon_from_file.argtypes = [C.c_char_p, C.POINTER(N.CutoffConfig)]
    return L


def distance_matrix_file(table_path: str, out_path: str, rank: Optional[str] = None, metric: str = "bray-curtis",
                         drop_unclassified: bool = False, device: int = 0) -> dict:
    """blu_distance_matrix_file: the features of a sample-table file at `rank` (None: every row by its direct counts), the pair
    integers counted on the GPU, the matrix of `metric` written to out_path.  Returns the counts of blu_distance_stats."""
    if metric not in DISTANCE_METRIC:
        raise ValueError(f"unknown metric `{metric}`: bray-curtis or jaccard")
    st = DistanceStats()
    rc = _bind().blu_distance_matrix_file(table_path.encode(), None if rank is None else rank.encode(), DISTANCE_METRIC[metric],
                                          DISTANCE_DROP_UNCLASSIFIED if drop_unclassified else 0, int(device), out_path.encode(),
                                          C.byref(st))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_distance_matrix_file")
    return {f: int(getattr(st, f)) for f, _ in DistanceStats._fields_}


def distance_matrix_file_with(table_path: str, out_path: str, rank: Optional[str] = None, metric: str = "bray-curtis",
                              drop_unclassified: bool = False, device: int = 0, depth: int = 0, seed: int = 0,
                              rarefied_table: Optional[str] = None, struct_size: Optional[int] = None) -> dict:
    """blu_distance_matrix_file_with: the same with every sample rarefied to `depth` reads first (0: not at all), the rarefied
    features written to rarefied_table.  Returns the counts of blu_distance_stats2."""
    if metric not in DISTANCE_METRIC:
        raise ValueError(f"unknown metric `{metric}`: bray-curtis or jaccard")
    opt = DistanceOptions(struct_size=C.sizeof(DistanceOptions) if struct_size is None else struct_size, depth=int(depth), seed=int(seed),
                          rarefied_table_path=None if rarefied_table is None else rarefied_table.encode())
    st = DistanceStats2()
    rc = _bind().blu_distance_matrix_file_with(table_path.encode(), None if rank is None else rank.encode(), DISTANCE_METRIC[metric],
                                               DISTANCE_DROP_UNCLASSIFIED if drop_unclassified else 0, int(device), out_path.encode(),
                                               C.byref(opt), C.byref(st))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_distance_matrix_file_with")
    return {f: int(getattr(st, f)) for f, _ in DistanceStats2._fields_}


def alpha_table_file(table_path: str, out_path: str, rank: Optional[str] = None, drop_unclassified: bool = False, device: int = 0,
                     depths=(), seed: int = 0, struct_size: Optional[int] = None) -> dict:
    """blu_alpha_table_file: the features of a sample-table file at `rank`, the alpha integers of every sample counted on the GPU
    (raw without depths, else at every depth of the ladder a sample reaches), the text written to out_path.  Returns
    blu_alpha_stats."""
    depths = [int(d) for d in depths]
    arr = (C.c_uint64 * max(len(depths), 1))(*depths)
    opt = AlphaOptions(struct_size=C.sizeof(AlphaOptions) if struct_size is None else struct_size, n_depths=len(depths), depths=arr,
                       seed=int(seed))
    st = AlphaStats()
    rc = _bind().blu_alpha_table_file(table_path.encode(), None if rank is None else rank.encode(),
                                      DISTANCE_DROP_UNCLASSIFIED if drop_unclassified else 0, int(device), out_path.encode(),
                                      C.byref(opt), C.byref(st))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_alpha_table_file")
    return {f: getattr(st, f) for f, _ in AlphaStats._fields_}


def ingest_only(blast_output: str, taxonomies_file: str, use_taxid: bool = False, device: int = -1):
    """Text ingest alone: returns (stats, checksum of the SoA columns).  device < 0: CPU ingest (no GPU needed);
    device >= 0: the GPU parser where it applies (same columns, same checksum)."""
    L = _bind()
    L.blu_ingest_only_on.restype = C.c_int
    L.blu_ingest_only_on.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(PipelineStats), C.POINTER(C.c_uint64)]
    st, ck = PipelineStats(), C.c_uint64()
    rc = L.blu_ingest_only_on(blast_output.encode(), taxonomies_file.encode(), 1 if use_taxid else 0, device, C.byref(st), C.byref(ck))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_ingest_only")
    return {f: getattr(st, f) for f, _ in PipelineStats._fields_}, ck.value


class IngestColumns(C.Structure):
    _fields_ = [("n_hits", C.c_uint64), ("n_queries", C.c_uint64), ("n_accessions", C.c_uint64), ("seg_off", C.POINTER(C.c_uint64)),
                ("bitscore", C.POINTER(C.c_int32)), ("align_len", C.POINTER(C.c_int32)), ("tax_desc_row", C.POINTER(C.c_uint32)),
                ("acc_rank", C.POINTER(C.c_uint32)), ("pident", C.POINTER(C.c_double)), ("query_names", C.c_void_p),
                ("query_names_bytes", C.c_uint64), ("accessions", C.c_void_p), ("accessions_bytes", C.c_uint64)]


def ingest_columns(blast_output: str, taxonomies_file: str, use_taxid: bool = False, device: int = -1,
                   hit_filter: Union[None, dict, HitFilter] = None,
                   taxon_filter: Union[None, dict, TaxonFilter] = None,
                   score_band: Union[None, dict, ScoreBand] = None, best_hit_per_subject: bool = False,
                   blast_outfmt: Optional[str] = None, query_cover=None) -> dict:
    """The SoA columns of the ingest (include/blu_pipeline.h: blu_ingest_columns_selected) as numpy arrays + the two string
    tables.  hit_filter (a dict or HitFilter): the columns of the lines it keeps, plus `n_lines` and `n_kept`.  taxon_filter (a
    dict or TaxonFilter): the same under a taxon filter, alone or beside hit_filter, plus `taxon_filter`: its counts (n_lines,
    n_excluded, n_not_only, exclude, excluded_by).  score_band (a dict or ScoreBand): the bitscore column with the band applied
    (needs device >= 0), plus `score_band`: its counts (n_hits, n_raised, n_queries, n_widened).  best_hit_per_subject: the
    columns with only the best row of every (query, subject accession) pair, selected before the band (needs
    device >= 0), plus `subject_best`: its counts (n_hits, n_kept, n_queries, n_thinned).  blast_outfmt: the format string the table
    was written with, when it is not the reference's (blu_ingest_columns_laid_out): the columns are those of the
    table rewritten to the reference's columns.  query_cover (a QueryCover, a dict of its fields, or the percent alone; needs
    blast_outfmt as the format string; blu_ingest_columns_covered): the columns of the lines at or above the cover,
    plus `n_lines`, `n_kept` and `query_cover`: its counts (n_lines, n_below, percent, source)."""
    import numpy as np
    L = _bind()
    c = IngestColumns()
    sel = _Selection(hit_filter, taxon_filter, score_band, best_hit_per_subject)
    st = sel.stats()
    cover = _Cover(query_cover, blast_outfmt) if query_cover is not None else None
    lay = _layout(blast_outfmt) if cover is None else cover.layout
    if cover is not None:
        # (the sibling entry point: only under a cover)
        rc = L.blu_ingest_columns_covered(blast_output.encode(), taxonomies_file.encode(), 1 if use_taxid else 0, device,
                                          C.byref(lay), C.byref(cover.c), C.byref(sel.c), C.byref(c), C.byref(st))
    elif lay is None:
        rc = L.blu_ingest_columns_selected(blast_output.encode(), taxonomies_file.encode(), 1 if use_taxid else 0, device,
                                           C.byref(sel.c), C.byref(c), C.byref(st))
    else:
        rc = L.blu_ingest_columns_laid_out(blast_output.encode(), taxonomies_file.encode(), 1 if use_taxid else 0, device,
                                           C.byref(lay), C.byref(sel.c), C.byref(c), C.byref(st))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_ingest_columns_covered" if cover is not None else
                         "blu_ingest_columns_selected" if lay is None else "blu_ingest_columns_laid_out")
    try:
        nh, nq = int(c.n_hits), int(c.n_queries)
        arr = lambda p, n, dt: np.ctypeslib.as_array(p, shape=(max(n, 1),))[:n].astype(dt, copy=True)
        out = {"seg_off": arr(c.seg_off, nq + 1, np.uint64), "bitscore": arr(c.bitscore, nh, np.int32),
               "align_len": arr(c.align_len, nh, np.int32), "tax_desc_row": arr(c.tax_desc_row, nh, np.uint32),
               "acc_rank": arr(c.acc_rank, nh, np.uint32), "pident": arr(c.pident, nh, np.float64)}
        split = lambda p, n: C.string_at(p, n).split(b"\0")[:-1] if n else []
        out["query_names"] = split(c.query_names, int(c.query_names_bytes))
        out["accessions"] = split(c.accessions, int(c.accessions_bytes))
        out.update(sel.counts(st))
        if cover is not None:
            out["n_lines"], out["n_kept"] = int(st.hit_filter.n_lines), int(st.hit_filter.n_kept)
            out["query_cover"] = cover.counts()
        return out
    finally:
        L.blu_ingest_columns_free(C.byref(c))


def last_ingest_path() -> str:
    """'gpu' or 'cpu': the parser the last ingest of this thread used."""
    return "gpu" if N.lib().blu_last_ingest_path() == 1 else "cpu"


def build_db_cache(taxonomies_file: str, cache_file: str, use_taxid: bool = False) -> None:
    """Writes the binary cache of a `*.blutils.json` (include/blu_pipeline.h: blu_db_cache_build); pass the cache file
    wherever a taxonomies file is expected."""
    L = _bind()
    L.blu_db_cache_build.restype = C.c_int
    L.blu_db_cache_build.argtypes = [C.c_char_p, C.c_int, C.c_char_p]
    rc = L.blu_db_cache_build(taxonomies_file.encode(), 1 if use_taxid else 0, cache_file.encode())
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_db_cache_build")


def custom_taxon_from_file(path: str) -> dict:
    """CustomTaxon::from_file (domain/dtos/taxon.rs:28-66)."""
    cfg = N.CutoffConfig()
    rc = _bind().blu_custom_taxon_from_file(path.encode(), C.byref(cfg))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_custom_taxon_from_file")
    return {k: int(cfg.custom[i]) for i, k in enumerate(N.CUSTOM_FIELDS) if cfg.custom_has[i]}


REPORT_WEIGHT = {"one": 0, "size": 1}


def build_consensus_identities(blast_output: str, taxonomies_file: str, taxon: str = "bacteria",
                               strategy: str = "relaxed", use_taxid: Optional[bool] = None,
                               custom_taxon_values: Optional[dict] = None, headers: Optional[Sequence[str]] = None,
                               out_format: str = "json", device: int = 0, lenient: bool = False, parse: bool = True,
                               config=None, out_path: Optional[str] = None, hit_filter: Union[None, dict, HitFilter] = None,
                               taxon_filter: Union[None, dict, TaxonFilter] = None,
                               score_band: Union[None, dict, ScoreBand] = None, best_hit_per_subject: bool = False,
                               min_cover=None, blast_outfmt: Optional[str] = None, query_cover=None):
    """Returns (results, stats).  With out_path the document is written there by the library (no copy through Python) and
    (None, stats) is returned.  results: the parsed `results` list (json) / list of records (jsonl), sorted by
    query, or the raw text when parse=False.  config: Some(BlastBuilder) of the run-with-consensus path
    (blutils_amd.blast.BlastBuilder): its run id goes on every result and it is written as the document's config.
    hit_filter (a dict or HitFilter; None = no filter): only the lines it keeps take part; stats then
    also has `n_lines` and `n_kept`.  taxon_filter (a dict or TaxonFilter; None = no filter): only the lines whose lineage
    passes take part; stats then also has `taxon_filter`, its counts.  score_band (a dict or ScoreBand; None =
    exact ties): the hits inside the band under a query's top bit-score count as tied with it, after the
    filters; stats then also has `score_band`, its counts (n_hits, n_raised, n_queries, n_widened).  best_hit_per_subject: of
    the lines of one (query, subject accession) pair only the best takes part — the highest truncated bit-score, the first in
    file order among equals — after the filters and before the band; stats then also has `subject_best`, its
    counts (n_hits, n_kept, n_queries, n_thinned), and n_hits / n_unmatched_rows count the kept lines.  min_cover (a decimal
    string or Decimal above 50 and at most 100, at most three decimals; None = strict agreement): of the lines on a query's top
    bit-score, the band's included, those outside the deepest taxon that still covers that percentage of them do not take part
    (DESIGN.md §20), after everything above; stats then also has `min_cover`, its counts (n_hits, n_kept, n_queries,
    n_narrowed, n_unresolved), and n_hits / n_unmatched_rows count the kept lines.  blast_outfmt (BLAST's own format string, e.g.
    `6 std staxids`; None = the reference's thirteen columns): the column list the table was written with; the
    run gives what it gives on a copy of the table rewritten to the reference's columns.  query_cover (a QueryCover, a dict of
    its fields, or the percent alone; None = no cover; needs blast_outfmt as the format string): only the lines whose query
    coverage is at least the percent take part, decided by the parser with the filters; stats then also has
    `n_lines`, `n_kept` and `query_cover`, its counts (n_lines, n_below, percent, source)."""
    return _build(blast_output, taxonomies_file, taxon, strategy, use_taxid, custom_taxon_values, headers, out_format, device,
                  lenient, parse, config, out_path, None, "one", hit_filter=hit_filter, taxon_filter=taxon_filter,
                  score_band=score_band, best_hit_per_subject=best_hit_per_subject, min_cover=min_cover, blast_outfmt=blast_outfmt,
                  query_cover=query_cover)


def build_consensus_identities_with_report(blast_output: str, taxonomies_file: str, taxon: str = "bacteria",
                                           strategy: str = "relaxed", use_taxid: Optional[bool] = None,
                                           custom_taxon_values: Optional[dict] = None,
                                           headers: Optional[Sequence[str]] = None, out_format: str = "json",
                                           device: int = 0, lenient: bool = False, parse: bool = True, config=None,
                                           out_path: Optional[str] = None, report_path: str = "report.tsv",
                                           report_weight: str = "one", hit_filter: Union[None, dict, HitFilter] = None,
                                           taxon_filter: Union[None, dict, TaxonFilter] = None,
                                           score_band: Union[None, dict, ScoreBand] = None,
                                           best_hit_per_subject: bool = False, min_cover=None,
                                           count_table: Optional[str] = None, blast_outfmt: Optional[str] = None,
                                           query_cover=None):
    """build_consensus_identities plus the taxon abundance report of its results, counted on the GPU and written to
    report_path after the document (include/blu_pipeline.h: blu_consensus_request.report_path).
    report_weight: "one" (results) or "size" (dereplicated reads named in the query).  count_table: a feature x sample count
    table whose row sums weigh the queries instead (with report_weight "one" only); stats then also has
    `count_table`, its counts (n_rows, n_samples, n_joined, n_rows_unclassified)."""
    return _build(blast_output, taxonomies_file, taxon, strategy, use_taxid, custom_taxon_values, headers, out_format, device,
                  lenient, parse, config, out_path, report_path, report_weight, hit_filter=hit_filter, taxon_filter=taxon_filter,
                  score_band=score_band, best_hit_per_subject=best_hit_per_subject, min_cover=min_cover, count_table=count_table,
                  blast_outfmt=blast_outfmt, query_cover=query_cover)


def build_consensus_identities_with_tables(blast_output: str, taxonomies_file: str, taxon: str = "bacteria",
                                           strategy: str = "relaxed", use_taxid: Optional[bool] = None,
                                           custom_taxon_values: Optional[dict] = None,
                                           headers: Optional[Sequence[str]] = None, out_format: str = "json",
                                           device: int = 0, lenient: bool = False, parse: bool = True, config=None,
                                           out_path: Optional[str] = None, report_path: Optional[str] = None,
                                           sample_table_path: Optional[str] = None, report_weight: str = "one",
                                           hit_filter: Union[None, dict, HitFilter] = None,
                                           support_table_path: Optional[str] = None,
                                           taxon_filter: Union[None, dict, TaxonFilter] = None,
                                           score_band: Union[None, dict, ScoreBand] = None,
                                           best_hit_per_subject: bool = False, min_cover=None,
                                           count_table: Optional[str] = None, blast_outfmt: Optional[str] = None,
                                           query_cover=None):
    """build_consensus_identities plus the taxon abundance report (report_path), the per-sample table (sample_table_path,
    DESIGN.md §13), or both, counted on the GPU and written in the order document, report, table
    (include/blu_pipeline.h: blu_consensus_request).  report_weight serves both files.  A query whose name
    names no sample fails the call before any file is written.  support_table_path: also the per-query support table
    (DESIGN.md §15), counted on the GPU and written last; it combines with the
    other files and with hit_filter, and may be the only one asked for.  Under a score_band its top_hits is the band's size
    and bits / support_bits sum the raised scores.  count_table: a feature x sample count table (with
    report_weight "one" only): the samples and counts of a query are those of the row with its key (its name up to the first
    ';') instead of what its name says; a row no query has counts as unclassified; stats then also has `count_table`, its
    counts (n_rows, n_samples, n_joined, n_rows_unclassified)."""
    return _build(blast_output, taxonomies_file, taxon, strategy, use_taxid, custom_taxon_values, headers, out_format, device,
                  lenient, parse, config, out_path, report_path, report_weight, sample_table_path, hit_filter=hit_filter,
                  support_table_path=support_table_path, taxon_filter=taxon_filter, score_band=score_band,
                  best_hit_per_subject=best_hit_per_subject, min_cover=min_cover, count_table=count_table,
                  blast_outfmt=blast_outfmt, query_cover=query_cover)


def _build(blast_output, taxonomies_file, taxon, strategy, use_taxid, custom_taxon_values, headers, out_format, device, lenient,
           parse, config, out_path, report_path, report_weight, sample_table_path=None, hit_filter=None,
           support_table_path=None, taxon_filter=None, score_band=None, best_hit_per_subject=False, min_cover=None,
           count_table=None, blast_outfmt=None, query_cover=None):
    L = _bind()
    qcov = _Cover(query_cover, blast_outfmt) if query_cover is not None else None
    lay = _layout(blast_outfmt) if qcov is None else qcov.layout
    cover = min_cover_milli(min_cover) if min_cover is not None else 0
    sel = _Selection(hit_filter, taxon_filter, score_band, best_hit_per_subject)
    p = PipelineParams()
    p.cutoffs.taxon = N.TAXON[taxon]
    p.cutoffs.has_custom = 1 if custom_taxon_values is not None else 0
    if custom_taxon_values is not None:
        for i, k in enumerate(N.CUSTOM_FIELDS):
            if custom_taxon_values.get(k) is not None:
                p.cutoffs.custom[i] = int(custom_taxon_values[k])
                p.cutoffs.custom_has[i] = 1
    p.strategy = N.STRATEGY[strategy]
    p.use_taxid = 1 if use_taxid else 0
    p.device = device
    p.out_format = OUT_FORMAT[out_format]
    p.lenient = 1 if lenient else 0
    enc = lambda x: str(x).encode() if x is not None else None
    rq = ConsensusRequest(struct_size=C.sizeof(ConsensusRequest), blast_output_file=blast_output.encode(),
                          taxonomies_file=taxonomies_file.encode(), params=C.pointer(p), out_path=enc(out_path),
                          report_path=enc(report_path), sample_table_path=enc(sample_table_path),
                          support_table_path=enc(support_table_path), selection=sel.c)
    if headers is not None:
        names = [h.encode() for h in headers]
        rq.headers, rq.n_headers = (C.c_char_p * max(1, len(names)))(*names), len(names)
    if config is not None:
        rq.run_id_text, rq.config_text = str(config.run_id).encode(), config.render(out_format).encode()
    if report_path is not None or sample_table_path is not None or count_table is not None:
        rq.weight = REPORT_WEIGHT[report_weight]
    rq.min_cover_milli = cover
    oc = ConsensusOutcome(selection=sel.stats())
    ex = None
    if count_table is not None:
        # (what the request has no room for travels in the extras)
        cst = CountTableStats()
        ex = ConsensusExtras(struct_size=C.sizeof(ConsensusExtras), count_table_path=enc(count_table), count_table_stats=C.pointer(cst))
    if qcov is not None:
        # (the sibling entry point: only under a cover)
        rc = L.blu_build_consensus_covered(C.byref(rq), C.byref(ex) if ex is not None else None, C.byref(lay), C.byref(qcov.c), C.byref(oc))
    elif lay is not None:
        # (the sibling entry point: only under a layout that is not the reference's own)
        rc = L.blu_build_consensus_laid_out(C.byref(rq), C.byref(ex) if ex is not None else None, C.byref(lay), C.byref(oc))
    elif ex is None:
        rc = L.blu_build_consensus(C.byref(rq), C.byref(oc))
    else:
        rc = L.blu_build_consensus_with(C.byref(rq), C.byref(ex), C.byref(oc))
    if rc != N.BLU_OK:
        raise N.BluError(rc, "blu_build_consensus")
    stats = {f: getattr(oc.stats, f) for f, _ in PipelineStats._fields_}
    stats.update(sel.counts(oc.selection))
    if count_table is not None:
        stats["count_table"] = {f: int(getattr(cst, f)) for f, _ in CountTableStats._fields_}
    if cover:
        stats["min_cover"] = last_min_cover_stats()
    if qcov is not None:
        stats["n_lines"], stats["n_kept"] = int(oc.selection.hit_filter.n_lines), int(oc.selection.hit_filter.n_kept)
        stats["query_cover"] = qcov.counts()
    if out_path is not None:
        return None, stats
    try:
        raw = C.string_at(oc.text, oc.text_len).decode("utf-8")
    finally:
        L.blu_free_text(oc.text)
    if not parse:
        return raw, stats
    if out_format in ("json", "json-compact"):
        return json.loads(raw)["results"], stats
    if out_format == "yaml":
        import yaml
        return yaml.safe_load(raw)["results"], stats
    lines = raw.splitlines()
    assert config is not None or lines[0] == "null"   # the config line comes first (write_blutils_output.rs:169-175)
    return [json.loads(l) for l in lines[1:]], stats
