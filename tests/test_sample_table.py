"""Per-sample taxon table on the host (`blastn build-report --by-sample`, blutils_amd/report.py): the restatement
(tests/sample_table_reference.py) against hand-computed tables, the product against the restatement, and both against
the reference's own pooled document (rebuilt from tests/golden/zymo_mock_queries.json.gz + zymo_mock_distilled.json.gz)."""
import gzip
import json
import os

import pytest
import yaml

from blutils_amd import cli, report
from tests import sample_table_reference as ref

ZYMO_RUNS = ["SRR20752596", "SRR20752610", "SRR25644443", "SRR25644557", "SRR25707968", "SRR25707969", "SRR25708007",
             "SRR25708008", "SRR25708009"]


def _r(query, taxonomy="absent"):
    if taxonomy == "absent":
        return {"query": query}
    if taxonomy == "null-taxon":
        return {"query": query, "taxon": None}
    return {"query": query, "taxon": {"taxonomy": taxonomy, "identifier": "x"}}


def _both(results, mode="one"):
    a = ref.table(results, mode)
    b = report.sample_table_from_results(results, mode)
    assert a == b
    return a


@pytest.mark.parametrize("query,sample", [
    ("SRR20752596.1002_size_3", "SRR20752596"), ("Soil.A.12;size=3", "Soil.A"), ("x;sample=B;size=2", "B"),
    ("sample=S9;x.1", "S9"), ("a.1;sample=C", "C"), ("S1.12_size_", None), ("S.1_size_2;size=4", "S"),
    ("abc", None), ("S1.", None), (".12", None), ("S1.x12", None), ("S1_12", None), ("q;sample=", None),
    ("q;sample=;r.4", None), ("x.7;sample=", "x"), ("A.B.C.9", "A.B.C"), ("a b.12", "a b"),
])
def test_label_rules(query, sample):
    if sample is None:
        with pytest.raises(ref.NoSample):
            ref.sample(query)
        with pytest.raises(report.ReportError, match=query.replace(".", r"\.").replace(";", ";")):
            report.sample_of(query)
    else:
        assert ref.sample(query) == sample
        assert report.sample_of(query) == sample


def test_hand_computed_table_columns_unplaced_and_zero_weight_sample():
    results = [_r("S2.1_size_3", "d__b;g__x"), _r("S10.1_size_2", "d__b;g__x"), _r("S10.2", "d__b;g__y"),
               _r("a.1", "d__b"), _r("B.1", ""), _r("B.2", "null-taxon"), _r("S2.9"), _r("Z.1_size_0", "d__c")]
    assert _both(results) == (
        "#rank\tidentifier\ttaxonomy\ttotal\tB\tS10\tS2\tZ\ta\n"
        "-\tunclassified\t\t2\t1\t0\t1\t0\t0\n"
        "-\tunplaced\t\t1\t1\t0\t0\t0\t0\n"
        "d\tb\td__b\t4\t0\t2\t1\t0\t1\n"
        "g\tx\td__b;g__x\t2\t0\t1\t1\t0\t0\n"
        "g\ty\td__b;g__y\t1\t0\t1\t0\t0\t0\n"
        "d\tc\td__c\t1\t0\t0\t0\t1\t0\n")
    assert _both(results, "size") == (
        "#rank\tidentifier\ttaxonomy\ttotal\tB\tS10\tS2\tZ\ta\n"
        "-\tunclassified\t\t2\t1\t0\t1\t0\t0\n"
        "-\tunplaced\t\t1\t1\t0\t0\t0\t0\n"
        "d\tb\td__b\t7\t0\t3\t3\t0\t1\n"
        "g\tx\td__b;g__x\t5\t0\t2\t3\t0\t0\n"
        "g\ty\td__b;g__y\t1\t0\t1\t0\t0\t0\n"
        "d\tc\td__c\t0\t0\t0\t0\t0\t0\n")


def test_no_unplaced_row_when_zero_and_rows_follow_the_report():
    results = [_r("s;sample=b", "d__b;g__alpha"), _r("t;sample=b", "d__b;g__Zeta"), _r("u;sample=a", "d__b"),
               _r("v;sample=a", "d__b;g__beta"), _r("w;sample=b", "d__b;g__beta"), _r("x;sample=b;size=0", "")]
    text = _both(results, "size")
    assert "unplaced" not in text
    rep = report.report_from_results(results, "size").splitlines()[1:]
    tab = text.splitlines()[1:]
    assert len(rep) == len(tab)
    for a, b in zip(rep, tab):
        a, b = a.split("\t"), b.split("\t")
        assert a[1] == b[3] and a[3:] == [b[0], b[1], b[2]] if a[4] != "unclassified" else a[1] == b[3]
        assert sum(int(v) for v in b[4:]) == int(b[3])


def test_a_query_without_sample_is_an_error_naming_it(tmp_path):
    results = [_r("S1.1", "d__b"), _r("orphan_12", "d__b")]
    with pytest.raises(report.ReportError, match="orphan_12"):
        report.sample_table_from_results(results)
    p = tmp_path / "doc.json"
    p.write_text(json.dumps({"results": results, "config": None}))
    with pytest.raises(SystemExit) as e:
        cli.main(["blastn", "build-report", str(p), "--by-sample", "-o", str(tmp_path / "t.tsv")])
    assert "orphan_12" in str(e.value.code)
    assert not (tmp_path / "t.tsv").exists()


def test_cli_by_sample_same_bytes_from_json_jsonl_yaml(tmp_path):
    results = [_r("S1.1_size_4", "d__b;p__f;g__x"), _r("S2.1_size_2", "d__b;p__f"), _r("S2.2", "null-taxon"),
               _r("S1.3", ""), _r("T.1;size=9", "d__a")]
    (tmp_path / "d.json").write_text(json.dumps({"results": results, "config": None}, indent=2))
    (tmp_path / "d.jsonl").write_text("".join(json.dumps(r) + "\n" for r in results))
    (tmp_path / "d.yaml").write_text(yaml.safe_dump({"results": results, "config": None}))
    for weight in ("one", "size"):
        want = ref.table(results, weight)
        for fmt in ("json", "jsonl", "yaml"):
            out = tmp_path / f"t_{fmt}.tsv"
            assert cli.main(["blastn", "build-report", str(tmp_path / f"d.{fmt}"), "-i", fmt, "--by-sample", "--weight", weight,
                             "-o", str(out)]) == 0
            assert out.read_text() == want


def _zymo_results(golden_dir):
    with gzip.open(os.path.join(golden_dir, "zymo_mock_distilled.json.gz"), "rt") as f:
        cases = json.load(f)["cases"]
    with gzip.open(os.path.join(golden_dir, "zymo_mock_queries.json.gz"), "rt") as f:
        rows = json.load(f)["results"]
    return [{"query": q, "taxon": None if i is None else cases[i]["taxon"]} for q, i in rows], cases


def test_reference_document_nine_runs(golden_dir, tmp_path):
    results, cases = _zymo_results(golden_dir)
    assert len(results) == 3626
    # the fixture agrees with the distilled one: every case's query count
    per_case = {}
    for r in results:
        if r["taxon"] is not None:
            per_case[json.dumps(r["taxon"], sort_keys=True)] = per_case.get(json.dumps(r["taxon"], sort_keys=True), 0) + 1
    assert sorted(per_case.values()) == sorted(c["n_queries"] for c in cases)
    text = ref.table(results, "one")
    lines = [l.split("\t") for l in text.splitlines()]
    assert lines[0][4:] == ZYMO_RUNS
    assert lines[1][:4] == ["-", "unclassified", "", "1343"]
    assert lines[1][4:] == ["0", "0", "116", "349", "116", "97", "246", "115", "304"]
    for l in lines[2:]:
        assert l[1] != "unplaced"
        if len(l[2].split(";")) == 1:                   # first-level rows: all classified weight in the first two runs
            assert all(v == "0" for v in l[6:])
    assert sum(int(l[3]) for l in lines[2:] if ";" not in l[2]) == 2283
    assert sum(int(l[4]) + int(l[5]) for l in lines[2:] if ";" not in l[2]) == 2283
    for weight in ("one", "size"):
        assert report.sample_table_from_results(results, weight) == ref.table(results, weight)
    doc = tmp_path / "zymo.json"
    doc.write_text(json.dumps({"results": results, "config": None}))
    out = tmp_path / "z.tsv"
    assert cli.main(["blastn", "build-report", str(doc), "--by-sample", "--weight", "size", "-o", str(out)]) == 0
    assert out.read_text() == ref.table(results, "size")
