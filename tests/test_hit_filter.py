"""Hit filters on the host parser (device=-1, no GPU): a filtered ingest gives the columns an independent
reading (tests/ingest_reference.py) gives of the table from which tests/hit_filter_reference.py deleted the dropped lines."""
import os

import numpy as np
import pytest

from blutils_amd import _native as N
from blutils_amd import cli, pipeline
from tests import hit_filter_reference as hf
from tests import ingest_reference as ref


def _check(src, tj, flt, tmp_path, device=-1):
    """filtered ingest of src == unfiltered independent reading of filter_text's copy; returns (columns, lines, kept)"""
    dst = str(tmp_path / "filtered_copy.tsv")
    n_lines, n_kept = hf.filter_text(src, dst, flt)
    got = pipeline.ingest_columns(src, tj, device=device, hit_filter=flt)
    hf.assert_columns_equal(got, ref.read_table(dst, tj))
    assert (got["n_lines"], got["n_kept"]) == (n_lines, n_kept)
    return got, n_lines, n_kept


def _table(tmp_path, rows, name="b.tsv", eol="\n", final=True):
    bt = tmp_path / name
    bt.write_bytes((eol.join(rows) + (eol if final else "")).encode())
    return str(bt)


@pytest.mark.parametrize("layout", ["grouped", "scrambled"])
@pytest.mark.parametrize("which", list(hf.FILTERS))
def test_filtered_ingest_is_the_ingest_of_the_filtered_copy(tmp_path, layout, which):
    rng = np.random.default_rng(31)
    rows = hf.make_rows(1500, 8, rng)
    if layout == "scrambled":
        rows = hf.scramble(rows, rng)
    src, tj = _table(tmp_path, rows), hf.write_db(tmp_path / "t.json")
    got, n_lines, n_kept = _check(src, tj, hf.FILTERS[which], tmp_path)
    assert n_lines == len(rows) and 0 < n_kept < n_lines                 # the threshold cuts
    assert int((got["tax_desc_row"] == ref.UNMATCHED).sum()) > 0


@pytest.mark.parametrize("threads", ["1", "4", "7"])
def test_a_table_cut_into_chunks(tmp_path, threads):
    """Above 1 MiB the host parser cuts the file into one chunk per thread: a query's first KEPT line may sit in any chunk."""
    rng = np.random.default_rng(32)
    rows = hf.scramble(hf.make_rows(6000, 6, rng), rng)
    src, tj = _table(tmp_path, rows), hf.write_db(tmp_path / "t.json")
    assert os.path.getsize(src) > (1 << 20)
    old = os.environ.get("BLU_INGEST_THREADS")
    os.environ["BLU_INGEST_THREADS"] = threads
    try:
        _, n_lines, n_kept = _check(src, tj, hf.FILTERS["all"], tmp_path)
    finally:
        if old is None:
            os.environ.pop("BLU_INGEST_THREADS", None)
        else:
            os.environ["BLU_INGEST_THREADS"] = old
    assert 0 < n_kept < n_lines


def test_a_taxid_listed_twice_multiplies_kept_rows_only(tmp_path):
    rng = np.random.default_rng(33)
    rows = hf.make_rows(400, 6, rng)
    rows += [f"qdup\tNR_000150.1\t150\t{pid}\t700\t1\t0\t1\t400\t1\t400\t1e-60\t500" for pid in ("99.000", "85.000", "95.500")]
    src, tj = _table(tmp_path, rows), hf.write_db(tmp_path / "t.json", duplicate=150)
    got, _, _ = _check(src, tj, {"min_perc_identity": 90.0}, tmp_path)
    q = got["query_names"].index(b"qdup")
    assert int(got["seg_off"][q + 1] - got["seg_off"][q]) == 4          # two kept lines, each joined twice


def _line(q, pid="99.0", aln="400", ev="1e-50", bs="700", acc="A.1", taxid="100"):
    return f"{q}\t{acc}\t{taxid}\t{pid}\t{aln}\t0\t0\t1\t400\t1\t400\t{ev}\t{bs}"


@pytest.mark.parametrize("eol,final", [("\n", True), ("\r\n", True), ("\n", False), ("\r\n", False)])
def test_boundaries(tmp_path, eol, final):
    tj = hf.write_db(tmp_path / "t.json")
    # a value equal to its threshold is kept
    rows = [_line("a", pid="97.000"), _line("a", pid="96.999"), _line("b", pid="97"), _line("c", pid="9.7e1")]
    got, _, kept = _check(_table(tmp_path, rows, eol=eol, final=final), tj, {"min_perc_identity": 97.0}, tmp_path)
    assert kept == 3
    rows = [_line("a", aln="199"), _line("a", aln="200"), _line("b", aln="0200"), _line("c", aln="-5")]
    _, _, kept = _check(_table(tmp_path, rows, eol=eol, final=final), tj, {"min_align_length": 200}, tmp_path)
    assert kept == 2
    # the bit-score as written: 99.5 fails 99.6 although both truncate to 99
    rows = [_line("a", bs="99.5"), _line("a", bs="99.6"), _line("b", bs="99.7"), _line("c", bs="1.0e2"), _line("d", bs="99")]
    got, _, kept = _check(_table(tmp_path, rows, eol=eol, final=final), tj, {"min_bit_score": 99.6}, tmp_path)
    assert kept == 3 and got["bitscore"].tolist() == [99, 99, 100]
    # e-value spellings around 1e-5; the first and the last line dropped
    forms = ["1.01e-05", "0.0", "1e-05", "1E-5", "0.00001", "9.99e-06", "3e-180", "5e-324", "1e-400", "1.0000000000001e-5", "2e-5"]
    rows = [_line(f"q{i}", ev=e) for i, e in enumerate(forms)]
    got, _, kept = _check(_table(tmp_path, rows, eol=eol, final=final), tj, {"max_e_value": 1e-5}, tmp_path)
    assert kept == 8 and got["query_names"] == [f"q{i}".encode() for i in range(1, 9)]
    _, _, kept = _check(_table(tmp_path, rows, eol=eol, final=final), tj, {"max_e_value": 0.0}, tmp_path)
    assert kept == 2                                                    # "0.0" and "1e-400" (strtod gives 0)


def test_a_query_without_kept_lines_disappears(tmp_path):
    tj = hf.write_db(tmp_path / "t.json")
    rows = [_line("first", pid="80"), _line("second", pid="99"), _line("first", pid="81"), _line("third", pid="98"), _line("second", pid="70")]
    got, _, _ = _check(_table(tmp_path, rows), tj, {"min_perc_identity": 90.0}, tmp_path)
    assert got["query_names"] == [b"second", b"third"] and got["seg_off"].tolist() == [0, 1, 2]
    # nothing kept: the result of a zero-byte file
    empty = tmp_path / "empty.tsv"
    empty.write_bytes(b"")
    exp = pipeline.ingest_columns(str(empty), tj, device=-1)
    got = pipeline.ingest_columns(_table(tmp_path, rows), tj, device=-1, hit_filter={"min_perc_identity": 100.0})
    hf.assert_columns_equal(got, exp)
    assert exp["seg_off"].tolist() == [0] and exp["query_names"] == [] and (got["n_lines"], got["n_kept"]) == (5, 0)


def test_column_11_is_read_only_under_its_threshold(tmp_path):
    tj = hf.write_db(tmp_path / "t.json")
    rows = [_line("a"), _line("b"), _line("c", ev="n/a"), _line("d")]
    src = _table(tmp_path, rows)
    assert pipeline.ingest_columns(src, tj, device=-1)["query_names"] == [b"a", b"b", b"c", b"d"]
    got = pipeline.ingest_columns(src, tj, device=-1, hit_filter={"min_perc_identity": 50.0})
    assert got["n_kept"] == 4
    with pytest.raises(N.BluError, match=r"line 3\b.*numeric") as ei:
        pipeline.ingest_columns(src, tj, device=-1, hit_filter={"max_e_value": 1.0})
    assert ei.value.code == 8                                           # BLU_ERR_PARSE
    # a malformed line the filter would drop is refused with the unfiltered call's message
    for bad, what in ((_line("x", pid="10", aln="4x0"), "numeric"), ("x\tA.1\t100\t10.0\t400", "columns"), (_line("x", pid="10", bs="1e12"), "32-bit")):
        src = _table(tmp_path, [_line("a"), bad, _line("b")], name="bad.tsv")
        with pytest.raises(N.BluError) as plain:
            pipeline.ingest_columns(src, tj, device=-1)
        with pytest.raises(N.BluError, match=what) as filtered:
            pipeline.ingest_columns(src, tj, device=-1, hit_filter={"min_perc_identity": 90.0})
        text = lambda e: str(e.value).split(": ", 1)[1]               # (the library's message, without the entry point's name)
        assert text(plain) == text(filtered) and plain.value.code == filtered.value.code


def test_no_filter_and_an_empty_filter_are_todays_call(tmp_path):
    rng = np.random.default_rng(34)
    src, tj = _table(tmp_path, hf.scramble(hf.make_rows(300, 6, rng), rng)), hf.write_db(tmp_path / "t.json")
    today = pipeline.ingest_columns(src, tj, device=-1)
    assert "n_kept" not in today
    hf.assert_columns_equal(today, ref.read_table(src, tj))
    for flt in (None, {}, pipeline.HitFilter(), {"max_e_value": None}):
        hf.assert_columns_equal(pipeline.ingest_columns(src, tj, device=-1, hit_filter=flt), today)
    with pytest.raises(ValueError):
        pipeline.ingest_columns(src, tj, device=-1, hit_filter={"min_query_cov": 80})
    with pytest.raises(ValueError):
        pipeline.ingest_columns(src, tj, device=-1, hit_filter={"min_align_length": 10.5})


def test_nan_and_infinite_thresholds(tmp_path):
    tj = hf.write_db(tmp_path / "t.json")
    src = _table(tmp_path, [_line("a"), _line("b", ev="0.0"), _line("c", ev="1e300")])
    assert pipeline.ingest_columns(src, tj, device=-1, hit_filter={"max_e_value": float("nan")})["n_kept"] == 0
    assert pipeline.ingest_columns(src, tj, device=-1, hit_filter={"max_e_value": float("inf")})["n_kept"] == 3
    assert pipeline.ingest_columns(src, tj, device=-1, hit_filter={"max_e_value": -1.0})["n_kept"] == 0
    assert pipeline.ingest_columns(src, tj, device=-1, hit_filter={"min_bit_score": float("nan")})["n_kept"] == 0


def test_cli_flags():
    ap = cli.build_parser()
    common = ["-t", "t.json", "--taxon", "bacteria", "--strategy", "relaxed"]
    flags = ["--min-perc-identity", "97.5", "--min-align-length", "200", "--max-e-value", "1e-20", "--min-bit-score", "99.6"]
    for head in (["blastn", "build-consensus", "b.tsv"], ["blastn", "run-with-consensus", "q.fa", "-d", "db", "--blast-out-file", "b.tsv"]):
        a = ap.parse_args(head + common + flags)
        assert (a.min_perc_identity, a.min_align_length, a.max_e_value, a.min_bit_score) == (97.5, 200, 1e-20, 99.6)
        assert cli._hit_filter(a) == pipeline.HitFilter(97.5, 200, 1e-20, 99.6)
        a = ap.parse_args(head + common)
        assert cli._hit_filter(a) is None
        a = ap.parse_args(head + common + ["--max-e-value", "0"])
        assert cli._hit_filter(a) == pipeline.HitFilter(max_e_value=0.0)
        for bad in (["--min-align-length", "-1"], ["--min-align-length", "10.5"], ["--max-e-value", "nan"], ["--min-perc-identity", "NaN"],
                    ["--min-bit-score", "high"], ["--min-query-cov", "80"]):
            with pytest.raises(SystemExit):
                ap.parse_args(head + common + bad)
    for sub in ("build-report", "build-tabular"):
        with pytest.raises(SystemExit):
            ap.parse_args(["blastn", sub, "doc.json", "--max-e-value", "1e-5"])
    # the help texts say that the flags are additions
    bc = [a for a in ap._subparsers._group_actions[0].choices["blastn"]._subparsers._group_actions[0].choices["build-consensus"]._actions
          if a.dest in ("min_perc_identity", "min_align_length", "max_e_value", "min_bit_score")]
    assert len(bc) == 4 and all("not in the reference CLI" in a.help for a in bc)
