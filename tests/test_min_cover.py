"""The minimum cover where no GPU is needed: the parsing of the percentage, the restatement
(tests/min_cover_reference.py) at the edges of `need` and on its invariants, the ctypes mirrors, the command line's flag and the
C ABI's refusals, which come before any file or device is asked for."""
import ctypes as C
import decimal

import numpy as np
import pytest

from blutils_amd import _native as N
from blutils_amd import blast, cli, engine, pipeline
from tests import min_cover_reference as ref


def test_the_percentage_is_read_exactly():
    for bad in ("50", "50.0001", "100.001", "nan", 50.5, True, "inf", "", "49.999", "-60", "6e1x", "50.000"):
        with pytest.raises(ValueError):
            pipeline.min_cover_milli(bad)
    assert pipeline.min_cover_milli("50.001") == 50001 == N.MIN_COVER_MILLI_LOW
    assert pipeline.min_cover_milli("66.667") == 66667
    assert pipeline.min_cover_milli("100") == 100000 == N.MIN_COVER_MILLI_HIGH
    assert pipeline.min_cover_milli(decimal.Decimal("80.5")) == 80500 and pipeline.min_cover_milli(" 90 ") == 90000
    assert pipeline.min_cover_milli(75) == 75000 and pipeline.min_cover_milli("7.5e1") == 75000


def test_need_at_its_edges():
    assert ref.need_rows(3, 66666) == 2 and ref.need_rows(3, 66667) == 3
    assert ref.need_rows(2, 50001) == 2
    assert ref.need_rows((1 << 32) - 2, 100000) == (1 << 32) - 2
    assert ref.need_rows(41, 80000) == 33 and ref.need_rows(5, 80000) == 4 and ref.need_rows(100000, 50001) == 50001
    for n in range(1, 200):
        for milli in (50001, 66667, 75000, 99999, 100000):
            need = ref.need_rows(n, milli)
            assert need * 100000 >= n * milli > (need - 1) * 100000 and n / 2 < need <= n


def test_the_restatement_on_hand_cases():
    a, b, c = (1, 2, 3), (1, 2, 4), (1, 9, 9)
    # forty of one species and one of another phylum: the forty stay
    v, d, what = ref.decide([a] * 20 + [c] + [a] * 20, 80000)
    assert v == [True] * 20 + [False] + [True] * 20 and (d, what) == (3, "decided")
    # two species of one genus and an outlier: the genus covers 4 of 5 at 80 %, the species do not
    assert ref.decide([a, a, b, b, c], 80000) == ([True, True, True, True, False], 2, "decided")
    # at 80.001 % need is 5: only the first level covers, nothing goes
    assert ref.decide([a, a, b, b, c], 80001) == ([True] * 5, 1, "decided")
    # nothing in common: the empty prefix
    assert ref.decide([(1,), (2,), (3,)], 66667) == ([True] * 3, 0, "decided")
    # a lineage that is a prefix of the others, as the majority's ancestor and as the outlier
    assert ref.decide([(1, 2), (1, 2, 3), (1, 2, 3), (7,)], 75000) == ([True, True, True, False], 2, "decided")
    assert ref.decide([(1,), (1, 2, 3), (1, 2, 3), (1, 2, 3)], 75000) == ([False, True, True, True], 3, "decided")
    # one row, no row, a row without a lineage
    assert ref.decide([a], 60000) == ([True], ref.NONE_U8, "alone") and ref.decide([], 60000) == ([], ref.NONE_U8, "alone")
    assert ref.decide([a, None, a], 60000)[2] == "unresolved" and ref.decide([a, (), a], 60000)[2] == "unresolved"
    # columns: the rows under the top are never touched, whatever they are; rows that no segment names get 0
    lin = [a, c, a, a, None, a, None, b]
    v, depth, counts = ref.keep([0, 5, 5, 7, 40, 6], [9, 9, 9, 9, 3, 7, 7, 1], lin, 75000)
    assert v == [1, 0, 1, 1, 1, 1, 1, 1] and depth == [3, ref.NONE_U8, ref.NONE_U8, ref.NONE_U8, ref.NONE_U8]
    assert counts == {"n_hits": 8, "n_kept": 7, "n_queries": 5, "n_narrowed": 1, "n_unresolved": 1}
    assert ref.keep([0], [1, 2], [a, a], 75000)[0] == [0, 0]


def test_invariants_of_the_restatement():
    rng = np.random.default_rng(5)
    for trial in range(300):
        n = int(rng.integers(2, 30))
        depth = int(rng.integers(1, 6))
        lins = [tuple(int(x) for x in rng.integers(0, 2, int(rng.integers(1, depth + 1)))) for _ in range(n)]
        milli = int(rng.choice([50001, 60000, 66667, 80000, 99999, 100000]))
        v, d, what = ref.decide(lins, milli)
        assert what == "decided" and sum(v) >= ref.need_rows(n, milli)                  # at least `need` rows stay
        kept = [l for l, k in zip(lins, v) if k]
        assert all(l[:d] == kept[0][:d] for l in kept)                                   # the kept rows all start with c
        if len(kept) > 1:
            # a second pass: its prefix extends c (it may be deeper: the group shrank and `need` with it, see below), and at
            # 100 % — or when the first pass dropped nothing — it drops nothing
            v2, d2, _ = ref.decide(kept, milli)
            assert d2 >= d and (all(v2) or not all(v))
            assert all(ref.decide(kept, 100000)[0])
        full, d100, _ = ref.decide(lins, 100000)
        assert all(full)                                                                 # P = 100 drops nothing
        assert all(l[:d100] == lins[0][:d100] for l in lins)


def test_a_second_pass_may_go_deeper():
    """The rule is stated for one pass.  Ten top rows at 60 %: need 6, the first level covers six (four of 1;2, two of 1;3) and
    the four others go.  Of the six that stay need is 4, which 1;2 covers by itself: a second pass drops the two rows of 1;3."""
    rows = [(1, 2)] * 4 + [(1, 3)] * 2 + [(9,)] * 4
    v, d, _ = ref.decide(rows, 60000)
    assert (v, d) == ([True] * 6 + [False] * 4, 1)
    assert ref.decide(rows[:6], 60000) == ([True] * 4 + [False] * 2, 2, "decided")
    assert ref.decide(rows[:4], 60000) == ([True] * 4, 2, "decided")                    # and there it rests


def test_struct_mirrors_and_exports():
    assert C.sizeof(N.MinCoverStats) == 40
    assert [getattr(N.MinCoverStats, f).offset for f in ("n_hits", "n_kept", "n_queries", "n_narrowed", "n_unresolved")] == [0, 8, 16, 24, 32]
    # the request keeps its size and offsets: the field took the place of a reserved word
    rq = pipeline.ConsensusRequest
    assert C.sizeof(rq) == 136 and C.sizeof(pipeline.HitSelection) == 32 and C.sizeof(pipeline.ConsensusOutcome) == 192
    assert (rq.weight.offset, rq.min_cover_milli.offset, rq.min_cover_milli.size, rq.support_table_path.offset, rq.selection.offset) == (88, 92, 4, 96, 104)
    assert not hasattr(rq, "reserved2")
    assert {"blu_hits_cover_keep", "blu_hits_cover_apply"} <= set(N.EXPORTS) and "blu_last_min_cover_stats" in N.PIPELINE_EXPORTS
    L = N.lib()
    for name in ("blu_hits_cover_keep", "blu_hits_cover_apply", "blu_last_min_cover_stats"):
        assert hasattr(L, name)
    assert L.blu_abi_version() == 5


def _request(**fields):
    p = pipeline.PipelineParams()
    p.device = -1
    rq = pipeline.ConsensusRequest(struct_size=C.sizeof(pipeline.ConsensusRequest), blast_output_file=b"/nonexistent/b.tsv",
                                   taxonomies_file=b"/nonexistent/t.json", params=C.pointer(p))
    for k, v in fields.items():
        setattr(rq, k, v)
    return rq, p


def test_the_request_refuses_a_value_out_of_range_before_the_weight_and_before_any_file():
    L = pipeline._bind()
    for milli in (-1, 50000, 100001, 1, 1 << 30, -(1 << 31)):
        rq, _p = _request(min_cover_milli=milli, report_path=b"/nonexistent/r.tsv", weight=7)
        oc = pipeline.ConsensusOutcome()
        assert L.blu_build_consensus(C.byref(rq), C.byref(oc)) == N.BLU_ERR_INVALID_ARG
        assert "min cover" in N.last_error() and "weight" not in N.last_error(), milli
    # a good value: the weight's refusal is next, still with no file opened
    rq, _p = _request(min_cover_milli=80000, report_path=b"/nonexistent/r.tsv", weight=7)
    oc = pipeline.ConsensusOutcome()
    assert L.blu_build_consensus(C.byref(rq), C.byref(oc)) == N.BLU_ERR_INVALID_ARG and "weight" in N.last_error()
    # the selection's mask comes first
    sel = pipeline.HitSelection(subject_best=C.pointer(N.SubjectBestC(4, 0)))
    rq, _p = _request(min_cover_milli=3, selection=sel)
    assert L.blu_build_consensus(C.byref(rq), C.byref(oc)) == N.BLU_ERR_INVALID_ARG and "mask" in N.last_error()
    # the struct did not grow
    rq, _p = _request(min_cover_milli=80000)
    rq.struct_size = 144
    assert L.blu_build_consensus(C.byref(rq), C.byref(oc)) == N.BLU_ERR_INVALID_ARG and "struct_size" in N.last_error()


def test_last_stats_are_zeros_after_a_failed_call():
    L = pipeline._bind()
    zeros = {"n_hits": 0, "n_kept": 0, "n_queries": 0, "n_narrowed": 0, "n_unresolved": 0}
    rq, _p = _request(min_cover_milli=80000)                              # refused files: the call fails
    oc = pipeline.ConsensusOutcome()
    assert L.blu_build_consensus(C.byref(rq), C.byref(oc)) != N.BLU_OK
    assert pipeline.last_min_cover_stats() == zeros
    rq, _p = _request(min_cover_milli=7)
    assert L.blu_build_consensus(C.byref(rq), C.byref(oc)) == N.BLU_ERR_INVALID_ARG and pipeline.last_min_cover_stats() == zeros
    assert L.blu_last_min_cover_stats(None) == N.BLU_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        pipeline.build_consensus_identities("/nonexistent/b.tsv", "/nonexistent/t.json", min_cover="50")


def _host_only_taxonomy():
    lineages = [[1, 2, 3], [1, 2, 4], [1, 5], [6]]
    lin_off = np.concatenate([[0], np.cumsum([len(l) for l in lineages])]).astype(np.uint64)
    node = np.array([x for l in lineages for x in l], np.uint32)
    return engine.Taxonomy(lin_off, node, np.zeros(len(node), np.uint16), ["clade"], taxon="bacteria", device=-1)


def test_engine_calls_refuse_before_they_ask_for_a_device():
    tax = _host_only_taxonomy()
    fwd = tax.row_map()[0]
    seg, bs, rows = [0, 3], [5, 5, 5], fwd[[0, 1, 3]]
    cols = dict(align_len=[1, 2, 3], acc_rank=[0, 1, 2], pident=[99.0, 98.0, 97.0])
    for milli in (0, 50000, 100001, 1 << 31):
        with pytest.raises(N.BluError) as e:
            engine.cover_keep_host(tax, seg, bs, rows, milli)
        assert e.value.code == N.BLU_ERR_INVALID_ARG and "min cover" in str(e.value)
        with pytest.raises(N.BluError) as e:
            engine.cover_apply_host(tax, seg, bs, cols["align_len"], rows, cols["acc_rank"], cols["pident"], milli)
        assert e.value.code == N.BLU_ERR_INVALID_ARG and "min cover" in str(e.value)
    L = N.lib()
    b, r, s, k = (np.array(x, dt) for x, dt in ((bs, np.int32), (rows, np.uint32), (seg, np.uint64), ([0, 0, 0], np.uint32)))
    st = N.MinCoverStats()
    p = lambda a: a.ctypes.data
    # a NULL array with a non-zero count; counts of 2^32 and more (the arrays are not read)
    for args in ((None, p(r), p(s), p(k)), (p(b), None, p(s), p(k)), (p(b), p(r), None, p(k)), (p(b), p(r), p(s), None)):
        rc = L.blu_hits_cover_keep(tax.handle, args[0], args[1], None, args[2], 3, 1, 0, 80000, None, args[3], None, C.byref(st))
        assert rc == N.BLU_ERR_INVALID_ARG and "null" in N.last_error()
    for n_hits, n_queries, word in ((1 << 32, 1, "n_hits"), (3, 1 << 32, "n_queries")):
        rc = L.blu_hits_cover_keep(tax.handle, p(b), p(r), None, p(s), n_hits, n_queries, 0, 80000, None, p(k), None, C.byref(st))
        assert rc == N.BLU_ERR_INVALID_ARG and word in N.last_error()
    # everything in order: the host-only handle is the one thing left to refuse
    with pytest.raises(N.BluError) as e:
        engine.cover_keep_host(tax, seg, bs, rows, 80000)
    assert e.value.code == N.BLU_ERR_NO_DEVICE
    with pytest.raises(N.BluError) as e:
        engine.cover_apply_host(tax, seg, bs, cols["align_len"], rows, cols["acc_rank"], cols["pident"], 80000, row_map=None)
    assert e.value.code == N.BLU_ERR_NO_DEVICE


def test_cli_flag_parses_and_reaches_the_pipeline(tmp_path, monkeypatch, capsys):
    ap = cli.build_parser()
    common = ["-t", "t.json", "--taxon", "bacteria", "--strategy", "relaxed"]
    for head in (["blastn", "build-consensus", "b.tsv"],
                 ["blastn", "run-with-consensus", "q.fa", "-d", "db", "--blast-out-file", "b.tsv"]):
        assert ap.parse_args(head + common + ["--min-cover", "66.667"]).min_cover == decimal.Decimal("66.667")
        assert ap.parse_args(head + common).min_cover is None
        for bad in ("50", "100.001", "80.0001", "nan", "x"):
            with pytest.raises(SystemExit):
                ap.parse_args(head + common + ["--min-cover", bad])
    capsys.readouterr()
    for sub in ("build-tabular", "build-report"):
        with pytest.raises(SystemExit):
            ap.parse_args(["blastn", sub, "doc.json", "--min-cover", "80"])
    seen = []
    counts = {"n_hits": 9, "n_kept": 7, "n_queries": 3, "n_narrowed": 2, "n_unresolved": 1}

    def fake(*a, **kw):
        seen.append(kw)
        return "{}", {"min_cover": counts} if kw.get("min_cover") is not None else {}

    monkeypatch.setattr(pipeline, "build_consensus_identities", fake)
    base = ["blastn", "build-consensus", "b.tsv"] + common
    capsys.readouterr()
    assert cli.main(base + ["--min-cover", "80"]) == 0 and seen[-1].get("min_cover") == decimal.Decimal("80")
    assert "min cover: kept 7 of 9 lines, narrowed 2 of 3 queries, 1 left alone" in capsys.readouterr().err
    assert cli.main(base) == 0 and "min_cover" not in seen[-1] and "min cover" not in capsys.readouterr().err
    seen_b = []
    monkeypatch.setattr(blast, "run_blast_and_build_consensus", lambda *a, **kw: seen_b.append(kw) or "{}")
    run = ["blastn", "run-with-consensus", "q.fa", "-d", "db", "--blast-out-file", str(tmp_path / "b.tsv")] + common
    assert cli.main(run + ["--min-cover", "90.5"]) == 0 and seen_b[-1].get("min_cover") == decimal.Decimal("90.5")
    assert cli.main(run) == 0 and "min_cover" not in seen_b[-1]
    # the count line follows the band's
    cli._say_kept({"score_band": {"n_hits": 9, "n_raised": 1, "n_queries": 3, "n_widened": 1}, "min_cover": counts})
    err = capsys.readouterr().err
    assert err.index("score band: raised 1 of 9 lines") < err.index("min cover: kept 7 of 9 lines")
