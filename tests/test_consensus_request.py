"""blu_build_consensus and blu_ingest_columns_selected (include/blu_pipeline.h) where no GPU is needed: the size check of the
request struct, the NULL refusals, the refusals that the older per-feature entry points made (DESIGN.md §19 lists them), and the
zeroing of the caller's counts when a call fails early."""
import ctypes as C

import pytest

from blutils_amd import _native as N
from blutils_amd import pipeline

ABSENT_TABLE, ABSENT_DB = b"/nonexistent/b.tsv", b"/nonexistent/t.json"


def _request(**fields):
    p = pipeline.PipelineParams()
    p.cutoffs.taxon, p.strategy, p.device = N.TAXON["bacteria"], N.STRATEGY["relaxed"], -1
    rq = pipeline.ConsensusRequest(struct_size=C.sizeof(pipeline.ConsensusRequest), blast_output_file=ABSENT_TABLE,
                                   taxonomies_file=ABSENT_DB, params=C.pointer(p))
    for k, v in fields.items():
        setattr(rq, k, v)
    return rq


def _call(rq, oc=None):
    oc = oc if oc is not None else pipeline.ConsensusOutcome()
    return pipeline._bind().blu_build_consensus(C.byref(rq), C.byref(oc))


def test_struct_mirrors():
    # (x86-64 / LP64, as the library is built: the sizes the C compiler gives the structs of include/blu_pipeline.h)
    assert C.sizeof(pipeline.HitSelection) == 32 and C.sizeof(pipeline.HitSelectionStats) == 16 + 32 + 32 + 32
    assert C.sizeof(pipeline.ConsensusRequest) == 136 and pipeline.ConsensusRequest.selection.offset == 104
    assert C.sizeof(pipeline.ConsensusOutcome) == 16 + 64 + 112


@pytest.mark.parametrize("size", [0, C.sizeof(pipeline.ConsensusRequest) + 8])
def test_a_struct_size_the_library_does_not_know_is_refused(size):
    assert _call(_request(struct_size=size)) == N.BLU_ERR_INVALID_ARG
    assert "struct_size" in N.last_error() and str(size) in N.last_error()


def test_a_null_request_or_outcome_is_refused():
    L = pipeline._bind()
    assert L.blu_build_consensus(None, C.byref(pipeline.ConsensusOutcome())) == N.BLU_ERR_INVALID_ARG and "null" in N.last_error()
    assert L.blu_build_consensus(C.byref(_request()), None) == N.BLU_ERR_INVALID_ARG and "null" in N.last_error()
    assert L.blu_ingest_columns_selected(ABSENT_TABLE, ABSENT_DB, 0, -1, None, None, None) == N.BLU_ERR_INVALID_ARG and "null" in N.last_error()


def test_the_refusals_of_the_older_entry_points_are_kept():
    """Each with its code and message, and before any file is opened: the files named here do not exist, and a call that got
    as far as opening one fails with another code."""
    refused = lambda rq, word: _call(rq) == N.BLU_ERR_INVALID_ARG and word in N.last_error()
    # a report or a sample table with a weight that is neither of the two
    assert refused(_request(report_path=b"/nonexistent/r.tsv", weight=2), "weight")
    assert refused(_request(sample_table_path=b"/nonexistent/s.tsv", weight=-1), "weight")
    # (the weight is read only when one of the two files is asked for: this call goes on to the taxonomies file)
    assert _call(_request(weight=7)) not in (N.BLU_OK, N.BLU_ERR_INVALID_ARG)
    assert _call(_request(support_table_path=b"/nonexistent/u.tsv", weight=7)) not in (N.BLU_OK, N.BLU_ERR_INVALID_ARG)
    # no table, no taxonomies file, no parameters
    for field in ("blast_output_file", "taxonomies_file", "params"):
        assert refused(_request(**{field: None}), "null argument")
    # the selection's masks and the band's values
    sel = lambda **kw: pipeline.HitSelection(**{k: C.pointer(v) for k, v in kw.items()})
    flt = pipeline.HitFilterC(mask=16)
    assert refused(_request(selection=sel(hit_filter=flt)), "hit filter")
    assert refused(_request(selection=sel(score_band=N.ScoreBandC(0, 4, 0))), "score band")
    assert refused(_request(selection=sel(score_band=N.ScoreBandC(100001, 1, 0))), "top_percent_milli")
    assert refused(_request(selection=sel(subject_best=N.SubjectBestC(2, 0))), "best hit per subject")
    # in the order of before: the table's path, then the hit filter, the band, the selection, the weight
    everything = _request(report_path=b"/nonexistent/r.tsv", weight=2,
                          selection=sel(hit_filter=flt, score_band=N.ScoreBandC(0, 4, 0), subject_best=N.SubjectBestC(2, 0)))
    assert refused(everything, "hit filter")
    everything.blast_output_file = None
    assert refused(everything, "null argument")
    # the same masks through the ingest-columns call
    L, cols = pipeline._bind(), pipeline.IngestColumns()
    for s, word in ((sel(hit_filter=flt), "hit filter"), (sel(score_band=N.ScoreBandC(0, 4, 0)), "score band"),
                    (sel(subject_best=N.SubjectBestC(2, 0)), "best hit per subject")):
        assert L.blu_ingest_columns_selected(ABSENT_TABLE, ABSENT_DB, 0, -1, C.byref(s), C.byref(cols), None) == N.BLU_ERR_INVALID_ARG
        assert word in N.last_error()
    # the reference's signatures: nowhere to put the text, no path to write to
    p = pipeline.PipelineParams()
    L.blu_build_consensus_identities_cfg.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_char_p, C.POINTER(pipeline.PipelineParams),
                                                     C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.blu_build_consensus_identities_to_file.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_char_p, C.POINTER(pipeline.PipelineParams),
                                                         C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p]
    assert L.blu_build_consensus_identities_cfg(ABSENT_TABLE, None, 0, ABSENT_DB, C.byref(p), None, None, None, None, None) == N.BLU_ERR_INVALID_ARG
    assert "null argument" in N.last_error()
    assert L.blu_build_consensus_identities_to_file(ABSENT_TABLE, None, 0, ABSENT_DB, C.byref(p), None, None, None, None) == N.BLU_ERR_INVALID_ARG
    assert "null argument" in N.last_error()


def _dirty_stats(by):
    st = pipeline.HitSelectionStats()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    st.taxon_filter.excluded_by = by
    return st


def _all_zero(st, by):
    flat = [int(getattr(getattr(st, part), f)) for part, t in pipeline.HitSelectionStats._fields_ for f, ft in t._fields_ if f != "excluded_by"]
    return not any(flat) and list(by) == [0] * len(by) and C.addressof(st.taxon_filter.excluded_by.contents) == C.addressof(by)


def test_the_callers_counts_are_zeroed_when_the_call_fails_early():
    """The files do not exist: the call fails at the taxonomies file, and the counts the caller passed in — the excluded_by
    array it owns too — read zero, not what they held."""
    names = (C.c_char_p * 2)(b"s__a", b"g__b*")
    taxa = pipeline.TaxonFilterC(names, 2, None, 0)
    sel = pipeline.HitSelection(hit_filter=C.pointer(pipeline.HitFilterC(min_perc_identity=97.0, mask=1)), taxon_filter=C.pointer(taxa),
                                subject_best=C.pointer(N.SubjectBestC(N.SUBJECT_BEST_PER_QUERY, 0)),
                                score_band=C.pointer(N.ScoreBandC(0, N.BAND_TOP_BITS, 2)))
    by = (C.c_uint64 * 2)(5, 6)
    oc = pipeline.ConsensusOutcome(text=0x1234, text_len=99, selection=_dirty_stats(by))
    oc.stats.n_hits, oc.stats.t_render_s = 7, 1.5
    rc = _call(_request(selection=sel), oc)
    assert rc not in (N.BLU_OK, N.BLU_ERR_INVALID_ARG) and "nonexistent" in N.last_error()
    assert oc.text is None and oc.text_len == 0
    assert [getattr(oc.stats, f) for f, _ in pipeline.PipelineStats._fields_] == [0] * 8
    assert _all_zero(oc.selection, by)
    # a refusal leaves them zeroed as well
    by[:] = [5, 6]
    oc = pipeline.ConsensusOutcome(selection=_dirty_stats(by))
    assert _call(_request(selection=sel, blast_output_file=None), oc) == N.BLU_ERR_INVALID_ARG and _all_zero(oc.selection, by)
    # the ingest-columns call
    by[:] = [5, 6]
    st, cols = _dirty_stats(by), pipeline.IngestColumns()
    rc = pipeline._bind().blu_ingest_columns_selected(ABSENT_TABLE, ABSENT_DB, 0, -1, C.byref(sel), C.byref(cols), C.byref(st))
    assert rc not in (N.BLU_OK, N.BLU_ERR_INVALID_ARG) and "nonexistent" in N.last_error()
    assert _all_zero(st, by) and cols.n_hits == 0 and not cols.bitscore
