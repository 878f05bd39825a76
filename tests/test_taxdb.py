"""`build-db blu` without a GPU: the oracle against the reference book and the hand-built rule cases, the command line,
the database check, the blastdbcmd call, and the gfx950 build of csrc/taxdb_gpu.hip."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

from oracle import taxdb_oracle as orc
from tests import taxdb_cases as tc
from blutils_amd import cli, taxdb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS = os.path.join(ROOT, "tests", "golden", "taxdb_docs_example")


def _entries(doc: bytes):
    return {e["taxid"]: e for e in json.loads(doc)["taxonomies"]}


def test_oracle_reproduces_the_book_example():
    """docs/book/01_create_blutils_database.md:179-213"""
    doc, tsv, st = orc.build(DOCS, os.path.join(DOCS, "accessions.txt"), source_database="db")
    e = _entries(doc)
    assert e[259354] == {
        "taxid": 259354, "rank": "s",
        "numericLineage": "no-rank__131567;superkingdom__2;p__200940;c__3024418;o__213118;f__3031627;g__218207;s__259354",
        "textLineage": "no-rank__cellular-organisms;superkingdom__bacteria;p__thermodesulfobacteriota;c__desulfobacteria;"
                       "o__desulfobacterales;f__desulfatibacillaceae;g__desulfatibacillum;s__desulfatibacillum-alkenivorans",
        "accessions": [{"accession": "NR_025795.1", "oid": "1878"}]}
    assert e[1006576] == {
        "taxid": 1006576, "rank": "s",
        "numericLineage": "no-rank__131567;superkingdom__2;p__200918;c__188708;o__1643947;f__1643949;g__1511648;s__1006576",
        "textLineage": "no-rank__cellular-organisms;superkingdom__bacteria;p__thermotogota;c__thermotogae;o__petrotogales;"
                       "f__petrotogaceae;g__defluviitoga;s__defluviitoga-tunisiensis",
        "accessions": [{"accession": "NR_122085.1", "oid": "13670"}]}
    assert tsv == b""
    head = doc.decode().split('  "taxonomies"')[0]
    assert head == ('{\n  "blutilsVersion": "8.3.1",\n  "ignoreTaxids": null,\n  "replaceRank": null,\n'
                    '  "dropNonLinnaeanTaxonomies": false,\n  "sourceDatabase": "db",\n')


@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_oracle_rule_cases(tmp_path, name):
    kw, opts, expected, tsv_expected = tc.CASES[name]
    c = tc.write_case(str(tmp_path / "dump"), **kw)
    doc, tsv, st = orc.build(c["dir"], c["accessions"], **opts)
    e = _entries(doc)
    assert set(e) == set(expected)
    for t, (num, txt) in expected.items():
        assert e[t]["numericLineage"] == num
        assert e[t]["textLineage"] == txt
    assert tsv.decode() == tsv_expected
    if name == "unmapped_ancestor":
        assert st["unmapped_ancestors"] == 1
    if name == "drop_leaf_vs_ancestor":
        assert st["dropped"] == 1 and st["mapped"] == 1
    if name == "merged_keeps_old_id":
        assert e[99]["rank"] == "s" and st["mapped_merged"] == 1
    if name == "accessions_keep_input_order":
        assert [a["accession"] for a in e[50]["accessions"]] == ["Z", "M"]
    if name == "escapes_and_extra_pieces":
        assert e[50]["accessions"] == [{"accession": 'A"\\\x01', "oid": "7"}, {"accession": "B", "oid": ""}]
        assert b'"accession": "A\\"\\\\\\u0001"' in doc


def test_oracle_options_in_the_head(tmp_path):
    c = tc.write_case(str(tmp_path / "d"), accessions="")
    doc, tsv, _ = orc.build(c["dir"], c["accessions"], skip=[5, 3], replace=[("a", "b"), ("c", "d"), ("a", "e")], drop=True)
    assert doc.decode() == ('{\n  "blutilsVersion": "8.3.1",\n  "ignoreTaxids": [\n    5,\n    3\n  ],\n'
                            '  "replaceRank": {\n    "a": "e",\n    "c": "d"\n  },\n  "dropNonLinnaeanTaxonomies": true,\n'
                            '  "sourceDatabase": "",\n  "taxonomies": []\n}')
    assert tsv == b""


def test_oracle_errors_name_file_and_line(tmp_path):
    c = tc.write_case(str(tmp_path / "a"), nodes=tc.dmp(1, 1, "no rank") + "2\t|\t1\n", accessions="")
    with pytest.raises(orc.TaxdbError, match=r"nodes\.dmp:2:"):
        orc.build(c["dir"], c["accessions"])
    c = tc.write_case(str(tmp_path / "b"), accessions="A  1  1\nB 2 3\n")
    with pytest.raises(orc.TaxdbError, match=r"accessions\.txt:2:"):
        orc.build(c["dir"], c["accessions"])
    c = tc.write_case(str(tmp_path / "c"), nodes=tc.dmp("x", 1, "no rank"), accessions="")
    with pytest.raises(orc.TaxdbError, match=r"nodes\.dmp:1: non-numeric"):
        orc.build(c["dir"], c["accessions"])
    c = tc.write_case(str(tmp_path / "d"), nodes=tc.dmp(-3, 1, "no rank"), accessions="")
    with pytest.raises(orc.TaxdbError, match=r"nodes\.dmp:1: id -3 outside"):
        orc.build(c["dir"], c["accessions"])


def test_oracle_stops_reading_accessions_at_invalid_utf8(tmp_path):
    c = tc.write_case(str(tmp_path / "a"), accessions=b"A  50  1\nB\xff  40  2\nC  30  3\n")
    doc, _, st = orc.build(c["dir"], c["accessions"])
    assert set(_entries(doc)) == {50} and st["accession_lines"] == 1


def test_cli_arguments():
    a = cli.build_parser().parse_args(["build-db", "blu", "DB", "TAX", "OUT", "-d", "-s", "131567", "--skip-taxid", "2",
                                       "-r", "superkingdom=d", "--replace-rank", "clade=cl", "--accessions-file", "acc.txt",
                                       "--blastdbcmd", "/x/blastdbcmd", "--device", "3"])
    assert (a.cmd, a.sub, a.blast_database_path, a.taxdump_directory_path, a.output_file_path) == ("build-db", "blu", "DB", "TAX", "OUT")
    assert a.drop_non_linnaean_taxonomies and a.skip_taxid == [131567, 2]
    assert a.replace_rank == ["superkingdom=d", "clade=cl"]
    assert (a.accessions_file, a.blastdbcmd, a.device) == ("acc.txt", "/x/blastdbcmd", 3)
    b = cli.build_parser().parse_args(["build-db", "blu", "DB", "TAX", "OUT"])
    assert not b.drop_non_linnaean_taxonomies and b.skip_taxid is None and b.replace_rank is None
    assert (b.accessions_file, b.blastdbcmd, b.device) == (None, "blastdbcmd", 0)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["build-db", "blu", "DB", "TAX", "OUT", "-s", "-1"])


@pytest.mark.parametrize("bad", ["superkingdom", "a=b=c", "=a=", ""])
def test_cli_malformed_replace_rank(bad, tmp_path):
    """db_builder/mod.rs:25-33: exactly one '='"""
    with pytest.raises(SystemExit, match="Invalid replace rank option"):
        cli.main(["build-db", "blu", "DB", str(tmp_path), str(tmp_path / "o"), "-r", bad, "--accessions-file", "x"])
    assert taxdb.parse_replace_rank(["a=b", "=c", "d="]) == [("a", "b"), ("", "c"), ("d", "")]


@pytest.mark.parametrize("arg,stem", [("out/db", "out/db"), ("out/db.json", "out/db"), ("out/db.tar.gz", "out/db.tar"),
                                      ("db", "db"), ("out/.hidden", "out/.hidden"), ("out/.h.txt", "out/.h")])
def test_output_names(arg, stem):
    """rs:240-270: set_extension("json"), then <stem>.blutils.json and <stem>.non-mapped.tsv"""
    assert taxdb.output_paths(arg) == (stem + ".blutils.json", stem + ".non-mapped.tsv")
    assert orc.output_paths(arg) == taxdb.output_paths(arg)


def test_database_check(tmp_path):
    """shared/validate_blast_database.rs:5-60: <stem>*.nsq, then taxdb.btd beside it"""
    db = str(tmp_path / "16S")
    from blutils_amd import blast
    with pytest.raises(blast.BlastError, match="Blast database not found"):
        taxdb.validate_blast_database_with_taxdb(db)
    (tmp_path / "16S.00.nsq").write_bytes(b"")
    with pytest.raises(taxdb.TaxdbError, match="Taxdb not found"):
        taxdb.validate_blast_database_with_taxdb(db)
    (tmp_path / "taxdb.btd").write_bytes(b"")
    taxdb.validate_blast_database_with_taxdb(db)
    blast.validate_blast_database(db)                 # the existing check is unchanged


def test_blastdbcmd_receives_the_reference_arguments(tmp_path):
    """build_accessions_map.rs:31-38, through the CLI up to the build itself (which needs a GPU)"""
    (tmp_path / "16S.nsq").write_bytes(b"")
    (tmp_path / "taxdb.btd").write_bytes(b"")
    log = tmp_path / "args.json"
    stand_in = tmp_path / "blastdbcmd"
    stand_in.write_text(f"#!{sys.executable}\nimport json, sys\njson.dump(sys.argv[1:], open({str(log)!r}, 'w'))\n"
                        "sys.stdout.write('NR_1.1  50  0\\n')\n")
    stand_in.chmod(0o755)
    c = tc.write_case(str(tmp_path / "dump"))
    try:
        cli.main(["build-db", "blu", str(tmp_path / "16S"), c["dir"], str(tmp_path / "out"), "--blastdbcmd", str(stand_in),
                  "--device", "0"])
    except SystemExit:
        pass                                           # no device on a CPU box: the build itself reports it
    assert json.load(open(log)) == ["-entry", "all", "-db", str(tmp_path / "16S"), "-outfmt", "%a  %T  %o"]


def test_taxdump_directory_and_files_are_checked(tmp_path):
    with pytest.raises(SystemExit, match="Invalid taxdump directory path"):
        cli.main(["build-db", "blu", "DB", str(tmp_path / "none"), str(tmp_path / "o"), "--accessions-file", "x"])
    c = tc.write_case(str(tmp_path / "d"))
    os.remove(os.path.join(c["dir"], "merged.dmp"))
    with pytest.raises(SystemExit, match="Invalid merged path"):
        cli.main(["build-db", "blu", "DB", c["dir"], str(tmp_path / "o"), "--accessions-file", c["accessions"]])


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_taxdb_kernels_build_for_gfx950():
    """csrc/taxdb_gpu.hip compiles for gfx950; the per-kernel resource usage (the PR records it) has every taxdb_* kernel
    at 4 waves per SIMD or more and without scratch."""
    csrc = os.path.join(ROOT, "blutils_amd", "csrc")
    p = subprocess.run(["make", "-s", "-C", csrc, "resource-usage-of", "SRC=taxdb_gpu.hip"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: \S*?(taxdb_[a-z0-9_]+?)E", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split()[0]] = int(m.group(2))
    assert {"taxdb_parse_dump", "taxdb_parse_acc", "taxdb_resolve", "taxdb_lineages", "taxdb_row_len", "taxdb_row_write"} <= set(usage)
    for k, u in usage.items():
        assert u["Occupancy"] >= 4, (k, u)
    for k, u in usage.items():
        assert u["ScratchSize"] == 0, (k, u)
