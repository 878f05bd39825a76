"""`build-db lineages` without a GPU: the restatement (tests/lineage_db_reference.py) against the hand-written rule cases and
the reference tree's mock lineage table, the round trip through the QIIME taxonomy TSV, the command line's argument errors and
the output names."""
import json
import os
import re
import subprocess

import pytest

from blutils_amd import cli, lineagedb, synth_lineages
from oracle import taxdb_oracle as orc
from tests import lineage_db_cases as LC
from tests import lineage_db_reference as R
from tests import seqdb_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "golden", "mock_16S_taxonomies.tsv")
DOCS = os.path.join(ROOT, "tests", "golden", "taxdb_docs_example")


def units_of(doc: bytes):
    return [(e["taxid"], e["rank"], e["numericLineage"], e["textLineage"], [(a["accession"], a["oid"]) for a in e["accessions"]])
            for e in json.loads(doc)["taxonomies"]]


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_restatement_rule_cases(name):
    table, replace, expected = LC.CASES[name]
    if "error" in expected:
        with pytest.raises(R.LineageError) as e:
            R.build(table, "t.tsv", replace)
        assert (e.value.line, e.value.kind) == expected["error"]
        return
    got = R.build(table, "t.tsv", replace)
    assert units_of(got["doc"]) == expected["units"]
    assert got["tsv"] == expected["tsv"] and got["map"] == expected["map"]
    st = got["stats"]
    assert st["taxonomies"] == len(expected["units"]) and st["empty"] == expected["tsv"].count(b"\n")
    assert st["data_lines"] == expected["tsv"].count(b"\n") + expected["map"].count(b"\n")


def test_restatement_literal_document():
    got = R.build(LC.LITERAL_TABLE, "silva.tsv", [("sk", "d")])
    assert got["doc"] == LC.LITERAL_DOC
    assert R.build(b"", "x", None)["doc"].endswith(b'"replaceRank": null,\n  "dropNonLinnaeanTaxonomies": null,\n'
                                                   b'  "sourceDatabase": "x",\n  "taxonomies": []\n}')
    assert b'"replaceRank": {},\n' in R.build(b"", "x", [])["doc"]


def test_restatement_depth_limit():
    assert R.build(LC.depth_table(64), "t", None)["stats"]["max_depth"] == 64
    with pytest.raises(R.LineageError) as e:
        R.build(b"a\td__A\n" + LC.depth_table(65), "t", None)
    assert (e.value.line, e.value.kind) == (2, "depth")


def test_restatement_mock_fixture():
    """The ids and units the issue quotes for the reference's mock table."""
    data = open(MOCK, "rb").read()
    assert data.count(b"\n") == 53
    got = R.build(data, "mock", None)
    taxa = got["taxa"]
    first = [b"d__2", b"d__2;p__1224", b"d__2;p__1224;c__1236", b"d__2;p__1224;c__1236;o__135622",
             b"d__2;p__1224;c__1236;o__135622;f__267890", b"d__2;p__1224;c__1236;o__135622;f__267890;g__22",
             b"d__2;p__1224;c__1236;o__135622;f__267890;g__22;s__93973", b"d__2;p__1224;c__1236;o__135622;f__267890;g__22;s__135626",
             b"d__2;p__1224;c__1236;o__135622;f__267890;g__22;s__150120"]
    assert [taxa[p] for p in first] == list(range(1, 10))
    second = b"d__2;p__201174;c__1760;o__85006;f__1268;g__1742989;s__256701".split(b";")
    assert [taxa[b";".join(second[:k + 1])] for k in range(1, 7)] == list(range(10, 16))
    units = units_of(got["doc"])
    assert units[0] == (5, "f", "d__1;p__2;c__3;o__4;f__5", "d__2;p__1224;c__1236;o__135622;f__267890", [("NR025123.135626.Bacb", "3")])
    seven = next(u for u in units if u[0] == 7)
    assert seven[1] == "s" and seven[2] == "d__1;p__2;c__3;o__4;f__5;g__6;s__7"
    assert seven[4][:2] == [("NR025012.93973.Bac", "0"), ("NR025012.93973.Bac", "1")]
    assert got["stats"] == {"data_lines": 53, "taxonomies": len(units), "taxa": len(taxa), "empty": 0, "truncated": 0, "max_depth": 10}
    assert got["tsv"] == b"" and got["map"].startswith(b"NR025012.93973.Bac 7\nNR025012.93973.Bac 7\nNR025123.135626.Baca 8\nNR025123.135626.Bacb 5\n")
    assert [u[0] for u in units] == sorted(u[0] for u in units)


def test_round_trip_of_a_build_db_blu_document():
    """qiime_tsv of a `build-db blu` document (both restated), fed back in, gives the same set of textLineage strings."""
    doc, _, _ = orc.build(DOCS, os.path.join(DOCS, "accessions.txt"), source_database="db")
    before = {e["textLineage"] for e in json.loads(doc)["taxonomies"]}
    table = SR.qiime2_taxonomies(doc, False)
    assert table.startswith(b"Feature ID\tTaxon\n")
    got = R.build(table, "roundtrip.tsv", None)
    assert {u[3] for u in units_of(got["doc"])} == before and len(before) > 1
    assert got["stats"]["empty"] == 0 and got["stats"]["truncated"] == 0


def test_synthetic_tables_are_seeded_and_cover_their_knobs(tmp_path):
    a = synth_lineages.write_table(str(tmp_path / "a.tsv"), 500, 60, depth=7, seed=4, ragged=0.2, empty=0.05, greengenes=0.2, noise=0.3,
                                   header=True, confidence=True)
    b = synth_lineages.write_table(str(tmp_path / "b.tsv"), 500, 60, depth=7, seed=4, ragged=0.2, empty=0.05, greengenes=0.2, noise=0.3,
                                   header=True, confidence=True)
    data = open(a, "rb").read()
    assert data == open(b, "rb").read()
    st = R.build(data, a, None)["stats"]
    assert st["data_lines"] == 500 and st["empty"] > 0 and st["truncated"] > 0 and st["max_depth"] == 7
    plain = synth_lineages.write_table(str(tmp_path / "c.tsv"), 300, 300, depth=5, seed=1)
    st = R.build(open(plain, "rb").read(), plain, None)["stats"]
    assert st["taxonomies"] <= 300 and st["taxa"] > st["taxonomies"] and st["empty"] == 0
    # noise respells a line without changing its taxon
    quiet = synth_lineages.write_table(str(tmp_path / "d.tsv"), 200, 40, seed=9)
    loud = synth_lineages.write_table(str(tmp_path / "e.tsv"), 200, 40, seed=9, noise=1.0)
    q, l = R.build(open(quiet, "rb").read(), "x", None), R.build(open(loud, "rb").read(), "x", None)
    assert q["doc"] == l["doc"] and open(quiet, "rb").read() != open(loud, "rb").read()


def test_cli_argument_errors(tmp_path, capsys):
    table = tmp_path / "t.tsv"
    table.write_bytes(b"a\td__A\n")
    for argv in (["build-db", "lineages"], ["build-db", "lineages", str(table)],
                 ["build-db", "lineages", str(table), str(tmp_path / "o"), "--taxid-map"],
                 ["build-db", "lineages", str(table), str(tmp_path / "o"), "--device", "x"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2
    capsys.readouterr()
    for bad in ("d", "a=b=c"):
        with pytest.raises(SystemExit, match="Invalid replace rank option"):
            cli.main(["build-db", "lineages", str(table), str(tmp_path / "o"), "-r", bad])
    with pytest.raises(SystemExit, match="Invalid lineage table path"):
        cli.main(["build-db", "lineages", str(tmp_path / "missing.tsv"), str(tmp_path / "o")])
    assert not any(p.name.startswith("o") for p in tmp_path.iterdir())


def test_replace_rank_and_output_names():
    assert lineagedb.parse_replace_rank(None) is None
    assert lineagedb.parse_replace_rank(["SK=Domain", "clade=no rank"]) == [("sk", "Domain"), ("clade", "no rank")]
    assert lineagedb.output_paths("out/silva.json") == ("out/silva.blutils.json", "out/silva.non-mapped.tsv")
    assert lineagedb.output_paths("silva_138.1") == ("silva_138.blutils.json", "silva_138.non-mapped.tsv")
    assert lineagedb.output_paths("db") == ("db.blutils.json", "db.non-mapped.tsv")
    st = dict(data_lines=5, taxonomies=2, taxa=9, empty=1, truncated=3, max_depth=7)
    assert lineagedb.summary(st) == "lineage table: 5 lines, 2 taxonomies, 9 taxa, 1 without a lineage, 3 truncated, deepest 7 levels"


def test_the_abi_is_declared_and_bound():
    from blutils_amd import _native
    assert "blu_lineage_db_build" in _native.PIPELINE_EXPORTS
    header = open(os.path.join(ROOT, "include", "blu_pipeline.h")).read()
    assert "int blu_lineage_db_build(const blu_lineage_db_desc* desc, blu_lineage_db_stats* stats);" in header
    import ctypes
    assert ctypes.sizeof(lineagedb.LineageDbDesc) == 80 and ctypes.sizeof(lineagedb.LineageDbStats) == 13 * 8 + 6 * 8


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_lineage_db_kernels_build_for_gfx950_without_scratch():
    """csrc/lineage_db_gpu.hip compiles for gfx950 under the Makefile's flags without a warning; every lindb_* kernel reports
    no scratch and no LDS (DESIGN.md 25.2 records the registers)."""
    csrc = os.path.join(ROOT, "blutils_amd", "csrc")
    p = subprocess.run(["make", "-s", "-C", csrc, "resource-usage-of", "SRC=lineage_db_gpu.hip"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "warning:" not in p.stderr
    usage, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: \S*?(lindb_[a-z_]+?)E", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split()[0]] = int(m.group(2))
    assert {"lindb_scan_lines", "lindb_classify", "lindb_write_paths", "lindb_intern", "lindb_mark_first", "lindb_item_ids",
            "lindb_leaf_keys", "lindb_heads", "lindb_segments", "lindb_row_len", "lindb_row_write", "lindb_list_len",
            "lindb_list_write"} == set(usage)
    assert all(u == {"ScratchSize": 0, "LDS": 0} for u in usage.values()), usage
