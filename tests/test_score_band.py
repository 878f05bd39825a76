"""The bit-score band where no GPU is needed: the restatement (tests/score_band_reference.py) against hand
cases, the ctypes mirrors of the two structs, the C ABI's argument refusals, and the command line's readers."""
import ctypes as C
import decimal

import numpy as np
import pytest

from blutils_amd import _native as N
from blutils_amd import cli, pipeline
from tests import score_band_reference as ref


def test_the_restatement_on_hand_cases():
    # t = 1000, P = 0.1: 1000 * 99900 = 99 900 000 -> 999 in, 998 out (the double form 1000 * (1 - 0.1 / 100) misses 999)
    assert ref.in_band(999, 1000, m=100) and not ref.in_band(998, 1000, m=100)
    assert 1000 * ((100 - 0.1) / 100) > 999
    # t = 370, P = 5: 370 * 95000 = 35 150 000 = 351.5 * 100000
    assert ref.in_band(352, 370, m=5000) and not ref.in_band(351, 370, m=5000)
    assert ref.in_band(1932735283, 2147483647, m=10000) and not ref.in_band(1932735282, 2147483647, m=10000)
    assert ref.in_band(497, 500, D=3) and not ref.in_band(496, 500, D=3)
    # both criteria: both must hold
    assert ref.in_band(999, 1000, m=100, D=1) and not ref.in_band(998, 1000, m=1000, D=1) and not ref.in_band(998, 1000, m=100, D=5)
    # the top itself and anything above are not `in the band`; no criterion: nothing is
    assert not ref.in_band(1000, 1000, m=100000, D=5) and not ref.in_band(999, 1000)
    # a negative top: no row qualifies under percent, bits still does; m = 100000 takes every row >= 0
    assert not ref.in_band(-6, -5, m=100000) and ref.in_band(-6, -5, D=1)
    assert ref.in_band(0, 7, m=100000) and not ref.in_band(-1, 7, m=100000)
    # zero widths: today's exact ties
    assert not ref.in_band(999, 1000, m=0) and not ref.in_band(999, 1000, D=0)
    seg = [0, 3, 3, 7, 9]
    bs = [1000, 999, 998, 370, 352, 351, 370, 5, 5]
    assert ref.raise_scores(seg, bs, m=100) == ([1000, 1000, 998, 370, 352, 351, 370, 5, 5], 1, 1)
    assert ref.raise_scores(seg, bs, m=5000) == ([1000] * 3 + [370, 370, 351, 370, 5, 5], 3, 2)
    assert ref.raise_scores(seg, bs, D=2) == ([1000] * 3 + [370, 352, 351, 370, 5, 5], 2, 1)
    assert ref.raise_scores(seg, bs) == (bs, 0, 0) and ref.raise_scores(seg, bs, m=0, D=0) == (bs, 0, 0)
    once = ref.raise_scores(seg, bs, m=5000)[0]
    assert ref.raise_scores(seg, once, m=5000) == (once, 0, 0)                   # idempotent
    # offsets as the library reads them: clamped to the column, a decreasing pair empty
    assert ref.raise_scores([0, 2, 1, 50], [10, 9, 8], D=1) == ([10, 10, 8], 1, 1)
    assert ref.raise_scores([0, 2, 1, 50], [10, 9, 8], D=2) == ([10, 10, 10], 2, 2)


def test_rewrite_table_rewrites_column_12_of_in_band_lines_only(tmp_path):
    line = lambda q, bs, eol="\n": f"{q}\tA.1\t100\t99.0\t400\t0\t0\t1\t400\t1\t400\t1e-50\t{bs}{eol}"
    src, dst = tmp_path / "a.tsv", tmp_path / "b.tsv"
    body = [line("a", "500.9"), line("b", "8"), line("a", "499.2", "\r\n"), "\n", line("a", "498"), line("b", "9.99e0"), line("a", "900")]
    src.write_text("".join(body), newline="")
    assert ref.rewrite_table(str(src), str(dst), D=1) == (6, 1, 1, 2)
    got = dst.read_bytes().decode().splitlines(keepends=True)
    assert got == [body[0], line("b", "9")] + body[2:]                           # (a's top is 900: nothing near it)
    kept = [True, True, True, True, True, False]
    assert ref.rewrite_table(str(src), str(dst), D=1, kept=kept) == (5, 2, 2, 2)
    got = dst.read_bytes().decode().splitlines(keepends=True)
    assert got == [body[0], line("b", "9"), line("a", "500", "\r\n"), "\n", body[4], body[5]]
    assert ref.rewrite_table(str(src), str(dst), m=100000, kept=kept) == (5, 3, 2, 2)


def test_struct_mirrors():
    assert C.sizeof(N.ScoreBandC) == 16 and C.sizeof(N.ScoreBandStats) == 32
    assert [getattr(N.ScoreBandC, f).offset for f in ("top_percent_milli", "mask", "top_bits")] == [0, 4, 8]
    assert [getattr(N.ScoreBandStats, f).offset for f in ("n_hits", "n_raised", "n_queries", "n_widened")] == [0, 8, 16, 24]
    assert (N.BAND_TOP_PERCENT, N.BAND_TOP_BITS) == (1, 2)
    assert "blu_hits_score_band" in N.EXPORTS
    assert {"blu_build_consensus", "blu_ingest_columns_selected"} <= set(N.PIPELINE_EXPORTS)
    L = N.lib()
    for name in ("blu_hits_score_band", "blu_build_consensus", "blu_ingest_columns_selected"):
        assert hasattr(L, name)


def _call(band, bs, seg, out=True, on_device=0):
    L = N.lib()
    st = N.ScoreBandStats()
    res = np.zeros(3, np.int32)
    rc = L.blu_hits_score_band(0, bs.ctypes.data if bs is not None else None, seg.ctypes.data if seg is not None else None,
                               len(bs) if bs is not None else 3, len(seg) - 1 if seg is not None else 1, on_device,
                               C.byref(band) if band is not None else None, None, res.ctypes.data if out else None, C.byref(st))
    return rc, res, st


def test_c_abi_refusals_need_no_device():
    bs, seg = np.array([5, 4, 3], np.int32), np.array([0, 3], np.uint64)
    for band, word in ((N.ScoreBandC(100001, 1, 0), "top_percent_milli"), (N.ScoreBandC(0, 2, 1 << 32), "top_bits"),
                       (N.ScoreBandC(0, 4, 0), "mask"), (N.ScoreBandC(0, 7, 0), "mask"), (N.ScoreBandC(100001, 0, 0), "top_percent_milli"),
                       (N.ScoreBandC(0, 0, 1 << 32), "top_bits")):
        rc, _, _ = _call(band, bs, seg)
        assert rc == N.BLU_ERR_INVALID_ARG and word in N.last_error()
    ok = N.ScoreBandC(1000, 3, 2)
    for kw in (dict(bs=None, seg=seg), dict(bs=bs, seg=None), dict(bs=bs, seg=seg, out=False)):
        rc, _, _ = _call(ok, kw["bs"], kw["seg"], kw.get("out", True))
        assert rc == N.BLU_ERR_INVALID_ARG and "null" in N.last_error()
    # no band and an empty mask, host pointers: the column as it is, no device asked for
    for band in (None, N.ScoreBandC(0, 0, 0)):
        rc, res, st = _call(band, bs, seg)
        assert rc == N.BLU_OK and res.tolist() == [5, 4, 3]
        assert (st.n_hits, st.n_raised, st.n_queries, st.n_widened) == (3, 0, 1, 0)
    # the pipeline's entry points refuse the same values before they read a file
    cols = pipeline.IngestColumns()
    L = pipeline._bind()
    sel = pipeline.HitSelection(score_band=C.pointer(N.ScoreBandC(0, 8, 0)))
    rc = L.blu_ingest_columns_selected(b"/nonexistent.tsv", b"/nonexistent.json", 0, -1, C.byref(sel), C.byref(cols), None)
    assert rc == N.BLU_ERR_INVALID_ARG and "mask" in N.last_error()


def test_python_band_arguments():
    assert pipeline.top_percent_milli("0.1") == 100 and pipeline.top_percent_milli(decimal.Decimal("100")) == 100000
    assert pipeline.top_percent_milli("1e1") == 10000 and pipeline.top_percent_milli("0") == 0 and pipeline.top_percent_milli(5) == 5000
    assert pipeline.top_percent_milli("12.500") == 12500 and pipeline.top_percent_milli("0.0010") == 1
    for bad in ("0.1234", "101", "nan", "-1", "inf", "1e-4", "x", "", 0.1, "100.001", "-0.001"):
        with pytest.raises(ValueError):
            pipeline.top_percent_milli(bad)
    assert pipeline.top_bits_value("3") == 3 and pipeline.top_bits_value((1 << 32) - 1) == (1 << 32) - 1
    for bad in ("-1", str(1 << 32), "1.5", "x", 2.0):
        with pytest.raises(ValueError):
            pipeline.top_bits_value(bad)
    assert not pipeline.ScoreBand().active() and pipeline.ScoreBand(top_percent="0").active() and pipeline.ScoreBand(top_bits=0).active()
    assert pipeline._score_band(None) is None and pipeline._score_band({}) is None and pipeline._score_band(pipeline.ScoreBand()) is None
    b = pipeline._score_band(pipeline.ScoreBand("0.1", 7))
    assert (b.top_percent_milli, b.mask, b.top_bits) == (100, 3, 7)
    b = pipeline._score_band({"top_bits": 0})
    assert (b.top_percent_milli, b.mask, b.top_bits) == (0, 2, 0)
    with pytest.raises(ValueError):
        pipeline._score_band({"top_percentage": "1"})


def test_cli_readers():
    ap = cli.build_parser()
    for sub, head in (("build-consensus", ["blastn", "build-consensus", "b.tsv"]),
                      ("run-with-consensus", ["blastn", "run-with-consensus", "q.fa", "-d", "db", "--blast-out-file", "b.tsv"])):
        common = ["-t", "t.json", "--taxon", "bacteria", "--strategy", "relaxed"]
        a = ap.parse_args(head + common + ["--top-percent", "0.1", "--top-bits", "3"])
        assert a.top_percent == decimal.Decimal("0.1") and a.top_bits == 3
        assert cli._score_band(a) == pipeline.ScoreBand(decimal.Decimal("0.1"), 3)
        a = ap.parse_args(head + common)
        assert a.top_percent is None and a.top_bits is None and cli._score_band(a) is None
        a = ap.parse_args(head + common + ["--top-percent", "0", "--top-bits", "4294967295"])
        assert cli._score_band(a).active() and a.top_bits == 4294967295
        for bad in (["--top-percent", "0.1234"], ["--top-percent", "101"], ["--top-percent", "nan"], ["--top-percent", "-1"],
                    ["--top-percent", "1e-4"], ["--top-bits", "4294967296"], ["--top-bits", "-1"], ["--top-bits", "1.5"]):
            with pytest.raises(SystemExit):
                ap.parse_args(head + common + bad)
    for sub in ("build-tabular", "build-report"):
        for flag in (["--top-percent", "1"], ["--top-bits", "1"]):
            with pytest.raises(SystemExit):
                ap.parse_args(["blastn", sub, "doc.json"] + flag)
