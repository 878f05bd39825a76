"""Taxon abundance report on the host (`blastn build-report`, blutils_amd/report.py): the restatement
(tests/report_reference.py) against hand-computed reports, the product against the restatement."""
import json
import os

import pytest
import yaml

from blutils_amd import cli, report
from tests import report_reference as ref

H = "#percent\tclade\tdirect\trank\tidentifier\ttaxonomy\n"


def _r(query, taxonomy="absent"):
    if taxonomy == "absent":
        return {"query": query}
    if taxonomy == "null-taxon":
        return {"query": query, "taxon": None}
    return {"query": query, "taxon": {"taxonomy": taxonomy, "identifier": "x"}}


def _both(results, mode="one"):
    a = ref.report(results, mode)
    b = report.report_from_results(results, mode)
    assert a == b
    return a


def test_skipped_level_shared_identifier_and_unplaced():
    results = [_r("a", "d__bac;p__fir;f__f1;g__uncultured"), _r("b", "d__bac;p__fir;f__f2;g__uncultured"),
               _r("c", "d__bac;g__skip"), _r("d", ""), _r("e", None), _r("f", "null-taxon"), _r("g")]
    assert _both(results) == H + (
        "28.57\t2\t2\t-\tunclassified\t\n"
        "28.57\t2\t2\t-\tunplaced\t\n"
        "42.86\t3\t0\td\tbac\td__bac\n"
        "28.57\t2\t0\tp\tfir\td__bac;p__fir\n"
        "14.29\t1\t0\tf\tf1\td__bac;p__fir;f__f1\n"
        "14.29\t1\t1\tg\tuncultured\td__bac;p__fir;f__f1;g__uncultured\n"
        "14.29\t1\t0\tf\tf2\td__bac;p__fir;f__f2\n"
        "14.29\t1\t1\tg\tuncultured\td__bac;p__fir;f__f2;g__uncultured\n"
        "14.29\t1\t1\tg\tskip\td__bac;g__skip\n")


def test_ties_go_by_text_bytewise_and_inner_paths_count_direct():
    results = [_r("1", "d__b;g__alpha"), _r("2", "d__b;g__Zeta"), _r("3", "d__b"), _r("4", "d__b;g__beta"),
               _r("5", "d__b;g__beta")]
    assert _both(results) == H + (
        "0.00\t0\t0\t-\tunclassified\t\n"
        "100.00\t5\t1\td\tb\td__b\n"
        "40.00\t2\t2\tg\tbeta\td__b;g__beta\n"
        "20.00\t1\t1\tg\tZeta\td__b;g__Zeta\n"
        "20.00\t1\t1\tg\talpha\td__b;g__alpha\n")


def test_percent_half_way_case():
    # 100 * 1 / 800 = 0.125 and 100 * 799 / 800 = 99.875, both exact in binary: "%.2f" rounds them to even
    results = [_r("hit", "d__x")] + [_r(f"u{i}") for i in range(799)]
    assert _both(results) == H + "99.88\t799\t799\t-\tunclassified\t\n0.12\t1\t1\td\tx\td__x\n"


@pytest.mark.parametrize("name,w", [("x;size=0", 0), ("x;size=7;", 7), ("x;size=12;y", 12), ("x;size=abc", 1),
                                    ("x_size_3", 3), ("x_size_3a", 1), ("x;size=5;y_size_9", 5), ("size=4", 4),
                                    ("x;size=", 1), ("x_size_", 1), ("plain", 1), ("x;size=4294967295", 4294967295),
                                    ("SRR20752596.1002_size_3", 3), ("a_size_3_size_4", 4)])
def test_size_weights(name, w):
    assert ref.weight(name, "size") == w
    assert report.weight_of(name, "size") == w
    assert report.weight_of(name, "one") == 1


@pytest.mark.parametrize("name", ["x;size=4294967296", "x_size_99999999999999999999"])
def test_a_size_of_2_to_the_32_is_an_error_naming_the_query(name):
    with pytest.raises(ref.WeightTooLarge):
        ref.weight(name, "size")
    with pytest.raises(report.ReportError, match=name):
        report.weight_of(name, "size")


def test_size_weights_in_a_report_and_a_zero_weight_path_is_listed():
    results = [_r("r1;size=5", "d__a;s__one"), _r("r2_size_3", "d__a;s__two"), _r("r3;size=0", "d__z"), _r("r4;size=2")]
    assert _both(results, "size") == H + (
        "20.00\t2\t2\t-\tunclassified\t\n"
        "80.00\t8\t0\td\ta\td__a\n"
        "50.00\t5\t5\ts\tone\td__a;s__one\n"
        "30.00\t3\t3\ts\ttwo\td__a;s__two\n"
        "0.00\t0\t0\td\tz\td__z\n")


def test_empty_document():
    assert _both([]) == H + "0.00\t0\t0\t-\tunclassified\t\n"
    assert _both([], "size") == H + "0.00\t0\t0\t-\tunclassified\t\n"


def _write_forms(tmp_path, results):
    (tmp_path / "d.json").write_text(json.dumps({"results": results, "config": None}, indent=2))
    (tmp_path / "d.jsonl").write_text("".join(json.dumps(r) + "\n" for r in results))
    (tmp_path / "d.yaml").write_text(yaml.safe_dump({"results": results, "config": None}))


def test_build_report_gives_the_same_bytes_for_json_jsonl_and_yaml(tmp_path, golden_dir, capsys):
    doc = json.load(open(os.path.join(golden_dir, "docs_worked_example.json")))
    results = doc["results"] + [_r("a;size=4", "d__bac;p__fir;f__f1;g__uncultured"), _r("b", ""), _r("c_size_2")]
    _write_forms(tmp_path, results)
    for weight in ("one", "size"):
        outs = []
        for fmt in ("json", "jsonl", "yaml"):
            out = tmp_path / f"r.{fmt}.{weight}.tsv"
            assert cli.main(["blastn", "build-report", str(tmp_path / f"d.{fmt}"), "-o", str(out), "-i", fmt,
                             "--weight", weight]) == 0
            outs.append(out.read_bytes())
        assert outs[0] == outs[1] == outs[2]
        assert outs[0].decode() == ref.report(results, weight)
    # stdout without -o
    capsys.readouterr()
    assert cli.main(["blastn", "build-report", str(tmp_path / "d.json")]) == 0
    assert capsys.readouterr().out == ref.report(results, "one")


def test_build_report_on_the_reference_worked_example(tmp_path, golden_dir):
    """tests/golden/docs_worked_example.json is reference blutils output: one query, `SRR20752596.1002_size_3`."""
    path = os.path.join(golden_dir, "docs_worked_example.json")
    results = json.load(open(path))["results"]
    for weight, n in (("one", 1), ("size", 3)):
        out = tmp_path / f"r.{weight}.tsv"
        assert cli.main(["blastn", "build-report", path, "-o", str(out), "--weight", weight]) == 0
        text = out.read_text()
        assert text == ref.report(results, weight)
        lines = text.splitlines()
        assert lines[1] == "0.00\t0\t0\t-\tunclassified\t"
        assert lines[2].startswith(f"100.00\t{n}\t0\tcellular-root\tcellular-organisms\t")
        assert lines[-1].split("\t")[:3] == ["100.00", str(n), str(n)]
        assert lines[-1].split("\t")[5] == results[0]["taxon"]["taxonomy"]


def test_build_report_errors(tmp_path):
    with pytest.raises(SystemExit, match="does not exist"):
        cli.main(["blastn", "build-report", str(tmp_path / "missing.json")])
    (tmp_path / "big.json").write_text(json.dumps({"results": [_r("q;size=4294967296", "d__a")], "config": None}))
    with pytest.raises(SystemExit, match="q;size=4294967296"):
        cli.main(["blastn", "build-report", str(tmp_path / "big.json"), "--weight", "size"])


def test_report_flags_parse():
    ap = cli.build_parser()
    a = ap.parse_args(["blastn", "build-consensus", "b.tsv", "-t", "t.json", "--taxon", "bacteria", "--strategy", "relaxed",
                       "--report", "r.tsv", "--report-weight", "size"])
    assert a.report == "r.tsv" and a.report_weight == "size"
    a = ap.parse_args(["blastn", "run-with-consensus", "q.fa", "-d", "db", "-t", "t.json", "--blast-out-file", "b",
                       "--taxon", "fungi", "--strategy", "cautious", "--report", "r.tsv"])
    assert a.report == "r.tsv" and a.report_weight == "one"
