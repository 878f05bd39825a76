"""Abundances from a count table where no GPU is needed: the restatement (tests/count_table_reference.py)
against hand-computed tables and reports, `blastn build-report --count-table` (blutils_amd/report.py) against the restatement,
both against the pooled zymo document, every refusal of the parser and the join, and the refusals, struct layout and exports
of blu_build_consensus_with."""
import ctypes as C
import gzip
import json
import os
import re

import pytest

from blutils_amd import _native as N
from blutils_amd import cli, pipeline, report
from tests import count_table_reference as ref
from tests import report_reference as rref
from tests import sample_table_reference as sref


def _r(query, taxonomy="null-taxon"):
    if taxonomy == "null-taxon":
        return {"query": query, "taxon": None}
    return {"query": query, "taxon": {"taxonomy": taxonomy, "identifier": "x"}}


RESULTS = [_r("otu1;size=9", "d__b;g__x"), _r("otu2", "d__b;g__y"), _r("otu3", "d__b"), _r("otu4", ""), _r("otu5"),
           _r("otu6", "d__c;g__z")]
TABLE = ("# Constructed from biom file\n"
         "#OTU ID\tS2\tS10\tempty\ta\n"
         "otu1\t3\t2.0\t0\t0\n"
         "\n"
         "otu2;size=4\t0\t1\t0\t0\r\n"
         "otu3\t1\t0\t0\t1\n"
         "otu4\t0\t0\t0\t5\n"
         "otu5\t7\t0\t0\t0\n"
         "otu6\t0\t0\t0.000\t0\n"
         "no_blast_line\t0\t4\t0\t2")
HAND_TABLE = ("#rank\tidentifier\ttaxonomy\ttotal\tS10\tS2\ta\tempty\n"
              "-\tunclassified\t\t13\t4\t7\t2\t0\n"
              "-\tunplaced\t\t5\t0\t0\t5\t0\n"
              "d\tb\td__b\t8\t3\t4\t1\t0\n"
              "g\tx\td__b;g__x\t5\t2\t3\t0\t0\n"
              "g\ty\td__b;g__y\t1\t1\t0\t0\t0\n"
              "d\tc\td__c\t0\t0\t0\t0\t0\n"
              "g\tz\td__c;g__z\t0\t0\t0\t0\t0\n")
HAND_REPORT = ("#percent\tclade\tdirect\trank\tidentifier\ttaxonomy\n"
               "50.00\t13\t13\t-\tunclassified\t\n"
               "19.23\t5\t5\t-\tunplaced\t\n"
               "30.77\t8\t2\td\tb\td__b\n"
               "19.23\t5\t5\tg\tx\td__b;g__x\n"
               "3.85\t1\t1\tg\ty\td__b;g__y\n"
               "0.00\t0\t0\td\tc\td__c\n"
               "0.00\t0\t0\tg\tz\td__c;g__z\n")
HAND_LINE = "count table: 7 rows, 4 samples, 6 joined to results, 1 without a result counted as unclassified"


def _write(tmp_path, results, table, name="c.tsv"):
    doc, tab = tmp_path / "doc.json", tmp_path / name
    doc.write_text(json.dumps({"results": results, "config": None}))
    tab.write_bytes(table.encode())
    return str(doc), str(tab)


def _product(tmp_path, results, table):
    """the host route, through the functions and through the CLI: (table, report, stats)"""
    doc, tab = _write(tmp_path, results, table)
    st = {}
    t = report.sample_table_from_results(results, "one", tab, st)
    r = report.report_from_results(results, "one", tab)
    for flags, want in ((["--by-sample"], t), ([], r)):
        out = tmp_path / "out.tsv"
        assert cli.main(["blastn", "build-report", doc, "--count-table", tab, "-o", str(out)] + flags) == 0
        assert out.read_text() == want
    return t, r, st


def test_hand_computed_table_and_report(tmp_path, capsys):
    """12.0, CRLF, the comment line, a blank line, a row key cut at ';', an all-zero sample, a path only zeros reach, an
    unplaced result, a result without taxon and a row without a result"""
    assert ref.table(RESULTS, TABLE) == HAND_TABLE
    assert ref.report(RESULTS, TABLE) == HAND_REPORT
    assert ref.stderr_line(RESULTS, TABLE) == HAND_LINE
    t, r, st = _product(tmp_path, RESULTS, TABLE)
    assert (t, r) == (HAND_TABLE, HAND_REPORT)
    assert st == {"n_rows": 7, "n_samples": 4, "n_joined": 6, "n_rows_unclassified": 1}
    assert HAND_LINE in capsys.readouterr().err
    # the total column is the report's clade column
    assert [l.split("\t")[3] for l in t.splitlines()[1:]] == [l.split("\t")[1] for l in r.splitlines()[1:]]


def test_no_unplaced_line_without_unplaced_counts_and_sibling_order(tmp_path):
    results = [_r("a", "d__b;g__alpha"), _r("b", "d__b;g__Zeta"), _r("c", "d__b;g__beta"), _r("d", "")]
    table = "OTU\tx\ty\na\t1\t1\nb\t1\t1\nc\t2\t1\nd\t0\t0\n"
    t, r, _ = _product(tmp_path, results, table)
    assert (t, r) == (ref.table(results, table), ref.report(results, table))
    assert "unplaced" not in t and "unplaced" not in r
    assert [l.split("\t")[1] for l in t.splitlines()[2:]] == ["b", "beta", "Zeta", "alpha"]
    assert t.splitlines()[1] == "-\tunclassified\t\t0\t0\t0"


def _zymo_results(golden_dir):
    with gzip.open(os.path.join(golden_dir, "zymo_mock_distilled.json.gz"), "rt") as f:
        cases = json.load(f)["cases"]
    with gzip.open(os.path.join(golden_dir, "zymo_mock_queries.json.gz"), "rt") as f:
        rows = json.load(f)["results"]
    return [{"query": q, "taxon": None if i is None else cases[i]["taxon"]} for q, i in rows]


def test_zymo_document_with_a_table_that_restates_its_names(golden_dir, tmp_path):
    """One row per query of the pooled reference document, its `size` in the column of the sample its name gives: the count
    table route must then give what the name route gives under `size` weighting (tests/sample_table_reference.py and
    tests/report_reference.py, which know nothing of count tables)."""
    results = _zymo_results(golden_dir)
    samples = sorted({sref.sample(r["query"]) for r in results}, reverse=True)      # (the file's order is not the table's)
    lines = ["#OTU ID\t" + "\t".join(samples)]
    for r in reversed(results):
        s, w = sref.sample(r["query"]), sref.weight(r["query"], "size")
        lines.append(r["query"] + "\t" + "\t".join(str(w) + ".0" if x == s else "0" for x in samples))
    table = "\n".join(lines) + "\n"
    want_t, want_r = sref.table(results, "size"), rref.report(results, "size")
    assert ref.table(results, table) == want_t and ref.report(results, table) == want_r
    t, r, st = _product(tmp_path, results, table)
    assert (t, r) == (want_t, want_r)
    assert st == {"n_rows": 3626, "n_samples": 9, "n_joined": 3626, "n_rows_unclassified": 0}
    # a second table: other counts, two more samples, forty rows without a result
    samples2 = samples + ["extra", "Zero"]
    lines = ["OTU\t" + "\t".join(samples2)]
    for k, r in enumerate(results):
        lines.append(r["query"] + "\t" + "\t".join(str((k * 7 + j * 3) % 11 if (k + j) % 4 else 0) if x != "Zero" else "0"
                                                    for j, x in enumerate(samples2)))
    lines += [f"unseen_{k}\t" + "\t".join(str(k + j) if x != "Zero" else "0" for j, x in enumerate(samples2)) for k in range(40)]
    table2 = "\n".join(lines)
    t, r, st = _product(tmp_path, results, table2)
    assert (t, r) == (ref.table(results, table2), ref.report(results, table2))
    assert st == {"n_rows": 3666, "n_samples": 11, "n_joined": 3626, "n_rows_unclassified": 40}
    assert t.splitlines()[0].split("\t")[4:] == sorted(samples2, key=str.encode)
    zero = t.splitlines()[0].split("\t").index("Zero")
    assert all(l.split("\t")[zero] == "0" for l in t.splitlines()[1:])


HEADER = "OTU\tA\tB\n"
PARSE_REFUSALS = [
    (HEADER + "x\t1.5\t0\n", 2, 2), (HEADER + "x\t1\t-1\n", 2, 3), (HEADER + "x\t\t1\n", 2, 2), (HEADER + "x\t1\n", 2, 3),
    (HEADER + "x\t1\t2\t3\n", 2, 4), (HEADER + "x\t1\t2\n\ny\t1\t1e3\n", 4, 3), (HEADER + "x\t1\t4294967296\n", 2, 3),
    (HEADER + "x\t1\t99999999999999999999999\n", 2, 3), (HEADER + "x\t1.\t1\n", 2, 2), (HEADER + "x\t.0\t1\n", 2, 2),
    (HEADER + "x\t1\t 2\n", 2, 3), (HEADER + "x\t+1\t2\n", 2, 2), (HEADER + "x\t1.00x\t2\n", 2, 2),
    ("#c\n#OTU ID\tA\tB\ttaxonomy\nx\t1\t2\tk__Bacteria; p__x\n", 3, 4),      # a trailing taxonomy column
    ("OTU\tA\t\tB\nx\t1\t2\t3\n", 1, 3), ("OTU\tA\tB\tA\nx\t1\t2\t3\n", 1, 4), ("# only\n\nOTU\n", 3, 2),
    ("# a\n# b\n", 3, 1), ("", 1, 1), (HEADER + "x\t1\t2\n# late comment\n", 3, 2), (HEADER + "x\t1\t2\r\r\n", 2, 3),
]


@pytest.mark.parametrize("text,line,column", PARSE_REFUSALS)
def test_parse_refusals_name_line_and_column(tmp_path, text, line, column):
    with pytest.raises(ref.ParseError) as e:
        ref.parse(text)
    assert (e.value.line, e.value.column) == (line, column)
    with pytest.raises(report.ReportError, match=rf"line {line}, column {column}:"):
        report.parse_count_table(text)
    doc, tab = _write(tmp_path, [_r("x", "d__b")], text)
    out = tmp_path / "o.tsv"
    with pytest.raises(SystemExit) as x:
        cli.main(["blastn", "build-report", doc, "--count-table", tab, "--by-sample", "-o", str(out)])
    assert f"line {line}, column {column}:" in str(x.value.code) and not out.exists()


def test_accepted_spellings():
    text = "\r\n# c\r\n\tB\tA\r\nx;a=b\t4294967295\t007.000\r\n\r\ny\t0.0\t0\r\n#z\t1\t1"
    assert ref.parse(text) == (["B", "A"], [("x;a=b", [4294967295, 7]), ("y", [0, 0]), ("#z", [1, 1])])
    assert report.parse_count_table(text) == (["A", "B"], [("x;a=b", {"B": 4294967295, "A": 7}), ("y", {}), ("#z", {"B": 1, "A": 1})])


def _join_refused(tmp_path, results, table, what, *names):
    with pytest.raises(ref.JoinError) as e:
        ref.table(results, table)
    assert e.value.what == what and e.value.names == names
    _, tab = _write(tmp_path, results, table)
    for f in (report.sample_table_from_results, report.report_from_results):
        with pytest.raises(report.ReportError) as p:
            f(results, "one", tab)
        for n in names:
            assert f"`{n}`" in str(p.value)


def test_join_refusals(tmp_path):
    res = [_r("q1;size=2", "d__b"), _r("q2", "d__b")]
    _join_refused(tmp_path, res, HEADER + "q1\t1\t1\nq2\t1\t1\nq1;x\t0\t0\n", "rows", "q1", "q1;x")
    _join_refused(tmp_path, res + [_r("q2;b")], HEADER + "q1\t1\t1\nq2\t1\t1\n", "queries", "q2", "q2;b")
    _join_refused(tmp_path, res + [_r("q3")], HEADER + "q1\t1\t1\nq2\t1\t1\n", "no row", "q3")
    _join_refused(tmp_path, res, HEADER + "Q1\t1\t1\nq2\t1\t1\n", "no row", "q1;size=2")
    _join_refused(tmp_path, res, HEADER + "q1\t4294967295\t1\nq2\t1\t1\n", "row sum", "q1")
    _join_refused(tmp_path, res, HEADER + "q1\t1\t1\nq2\t1\t1\nnobody\t2147483648\t2147483648\n", "row sum", "nobody")
    # just below the limit is fine
    table = HEADER + "q1\t4294967294\t1\nq2\t1\t1\n"
    _, tab = _write(tmp_path, res, table)
    assert report.report_from_results(res, "one", tab) == ref.report(res, table)


def test_weight_size_is_refused_with_a_count_table(tmp_path):
    doc, tab = _write(tmp_path, RESULTS, TABLE)
    for f in (report.sample_table_from_results, report.report_from_results):
        with pytest.raises(report.ReportError, match="weight"):
            f(RESULTS, "size", tab)
    with pytest.raises(SystemExit) as e:
        cli.main(["blastn", "build-report", doc, "--count-table", tab, "--weight", "size", "-o", str(tmp_path / "o.tsv")])
    assert "--weight size" in str(e.value.code) and not (tmp_path / "o.tsv").exists()
    with pytest.raises(SystemExit) as e:
        cli.main(["blastn", "build-report", doc, "--count-table", str(tmp_path / "absent.tsv")])
    assert "absent.tsv" in str(e.value.code)


def test_cli_refusals_of_build_consensus_and_run_with_consensus(tmp_path):
    """before anything is opened: the files named do not exist"""
    bc = ["blastn", "build-consensus", "/nonexistent/b.tsv", "-t", "/nonexistent/t.json", "--taxon", "bacteria", "--strategy", "relaxed",
          "--count-table", "/nonexistent/c.tsv"]
    rw = ["blastn", "run-with-consensus", "/nonexistent/q.fa", "-d", "/nonexistent/db", "-t", "/nonexistent/t.json", "--blast-out-file",
          str(tmp_path / "b.tsv"), "--taxon", "bacteria", "--strategy", "relaxed", "--count-table", "/nonexistent/c.tsv"]
    for base in (bc, rw):
        with pytest.raises(SystemExit) as e:
            cli.main(base)
        assert "--report or --sample-table" in str(e.value.code)
        with pytest.raises(SystemExit) as e:
            cli.main(base + ["--support-table", str(tmp_path / "u.tsv")])
        assert "--report or --sample-table" in str(e.value.code)
        for flag in ("--report", "--sample-table"):
            with pytest.raises(SystemExit) as e:
                cli.main(base + [flag, str(tmp_path / "r.tsv"), "--report-weight", "size"])
            assert "--report-weight size" in str(e.value.code)
    assert list(tmp_path.iterdir()) == []
    args = cli.build_parser().parse_args(bc + ["--report", "r.tsv"])
    assert args.count_table == "/nonexistent/c.tsv"
    assert "--count-table" in cli.__doc__ and "count table: R rows, S samples" in cli.__doc__


# ---- blu_build_consensus_with ------------------------------------------------------------------------------------------

ABSENT_TABLE, ABSENT_DB, ABSENT_COUNTS = b"/nonexistent/b.tsv", b"/nonexistent/t.json", b"/nonexistent/c.tsv"


def _request(**fields):
    p = pipeline.PipelineParams()
    p.cutoffs.taxon, p.strategy, p.device = N.TAXON["bacteria"], N.STRATEGY["relaxed"], -1
    rq = pipeline.ConsensusRequest(struct_size=C.sizeof(pipeline.ConsensusRequest), blast_output_file=ABSENT_TABLE,
                                   taxonomies_file=ABSENT_DB, params=C.pointer(p))
    for k, v in fields.items():
        setattr(rq, k, v)
    return rq


def _extras(**fields):
    ex = pipeline.ConsensusExtras(struct_size=C.sizeof(pipeline.ConsensusExtras), count_table_path=ABSENT_COUNTS)
    for k, v in fields.items():
        setattr(ex, k, v)
    return ex


def _call(rq, ex):
    oc = pipeline.ConsensusOutcome()
    return pipeline._bind().blu_build_consensus_with(C.byref(rq), C.byref(ex) if ex is not None else None, C.byref(oc))


def test_extras_layout_and_exports():
    ex = pipeline.ConsensusExtras
    assert C.sizeof(ex) == 24 and C.sizeof(pipeline.CountTableStats) == 32
    assert [getattr(ex, f).offset for f in ("struct_size", "reserved", "count_table_path", "count_table_stats")] == [0, 4, 8, 16]
    assert [getattr(pipeline.CountTableStats, f).offset for f in ("n_rows", "n_samples", "n_joined", "n_rows_unclassified")] == [0, 8, 16, 24]
    assert [f for f, _ in report.CountRows._fields_] == ["row_ptr", "sample", "count"] and C.sizeof(report.CountRows) == 24
    assert C.sizeof(pipeline.ConsensusRequest) == 136                        # the request did not grow
    assert "blu_build_consensus_with" in N.PIPELINE_EXPORTS and "blu_consensus_sample_table_counts" in N.EXPORTS
    L = N.lib()
    assert hasattr(L, "blu_build_consensus_with") and hasattr(L, "blu_consensus_sample_table_counts")
    assert L.blu_abi_version() == 5
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "blu_pipeline.h")).read()
    assert re.search(r"typedef struct blu_consensus_extras \{\s*uint32_t struct_size; uint32_t reserved;", hdr)
    assert "blu_consensus_sample_table_counts(" in open(os.path.join(root, "include", "blu_consensus.h")).read()


@pytest.mark.parametrize("size", [0, C.sizeof(pipeline.ConsensusExtras) + 8])
def test_an_extras_size_the_library_does_not_know_is_refused(size):
    rq = _request(report_path=b"/nonexistent/r.tsv")
    assert _call(rq, _extras(struct_size=size)) == N.BLU_ERR_INVALID_ARG
    assert "struct_size" in N.last_error() and str(size) in N.last_error() and "blu_consensus_extras" in N.last_error()


def test_refusals_before_any_file_is_opened():
    refused = lambda rq, ex, word: _call(rq, ex) == N.BLU_ERR_INVALID_ARG and word in N.last_error()
    # a count table nothing would use
    assert refused(_request(), _extras(), "neither a report nor a sample table")
    assert refused(_request(support_table_path=b"/nonexistent/u.tsv"), _extras(), "neither a report nor a sample table")
    # a count table beside the weight `size`
    for field in ("report_path", "sample_table_path"):
        assert refused(_request(**{field: b"/nonexistent/r.tsv", "weight": pipeline.REPORT_WEIGHT["size"]}), _extras(), "weight")
    # the request's own refusals stay: its size, a null file
    assert refused(_request(struct_size=144, report_path=b"/nonexistent/r.tsv"), _extras(), "struct_size 144")
    assert refused(_request(blast_output_file=None, report_path=b"/nonexistent/r.tsv"), _extras(), "null argument")
    # accepted so far: the call goes on to the taxonomies file, with extras, with empty extras and with none
    for ex in (_extras(), _extras(count_table_path=None), None):
        rc = _call(_request(report_path=b"/nonexistent/r.tsv"), ex)
        assert rc not in (N.BLU_OK, N.BLU_ERR_INVALID_ARG) and "nonexistent" in N.last_error()
    assert not os.path.exists("/nonexistent")


def test_the_callers_count_table_stats_are_zeroed_when_the_call_begins():
    st = pipeline.CountTableStats(5, 6, 7, 8)
    rc = _call(_request(report_path=b"/nonexistent/r.tsv"), _extras(count_table_stats=C.pointer(st)))
    assert rc not in (N.BLU_OK, N.BLU_ERR_INVALID_ARG)
    assert [int(getattr(st, f)) for f, _ in pipeline.CountTableStats._fields_] == [0, 0, 0, 0]
    st = pipeline.CountTableStats(5, 6, 7, 8)
    assert _call(_request(), _extras(count_table_stats=C.pointer(st))) == N.BLU_ERR_INVALID_ARG
    assert [int(getattr(st, f)) for f, _ in pipeline.CountTableStats._fields_] == [0, 0, 0, 0]


def test_a_host_only_taxonomy_is_refused():
    import numpy as np

    from blutils_amd import engine, synth
    tax = synth.make_taxonomy(50, 3)
    t = engine.Taxonomy(tax.lin_off, tax.lin_node, tax.lin_rank, tax.rank_names, taxon="bacteria", device=-1)
    recs = np.zeros(2, engine.RESULT_DTYPE)
    with pytest.raises(N.BluError, match="host-only") as e:
        report.consensus_sample_table_counts(t, np.zeros(2, np.uint32), recs, 2, np.array([0, 1, 2], np.uint64), np.zeros(2, np.uint32),
                                             np.ones(2, np.uint32), 1)
    assert e.value.code == N.BLU_ERR_NO_DEVICE
