"""Tables in any outfmt-6 column order (`--blast-outfmt`) on the GPU: the layout builds of the parse kernels
(csrc/ingest_gpu.hip: parse_rows_layout, parse_rows_layout_filtered, parse_rows_layout_taxa and their general forms) held to the
host parser and to the independent reading (tests/ingest_reference.py) of the table rewritten to the reference's columns
(tests/outfmt_reference.py), and the whole run — document, report, sample table, support table, stderr lines — held to the run on
that copy through today's path.  Every accepted case must be read by the GPU parser itself (`last_ingest_path() == "gpu"`): a
fall-back to the host parser would hide the kernel.  tests/test_outfmt.py checks without a GPU that every case is in the plain
form and lies where it claims."""
import os

import pytest

from blutils_amd import blast, cli, pipeline
from tests import ingest_edges as E
from tests import ingest_reference as ref
from tests import outfmt_cases as K
from tests import outfmt_reference as R
from tests.test_ingest_edges import assert_columns_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def force_gpu():
    old = os.environ.get("BLU_INGEST")
    os.environ["BLU_INGEST"] = "gpu"
    yield
    if old is None:
        os.environ.pop("BLU_INGEST", None)
    else:
        os.environ["BLU_INGEST"] = old


def _write(tmp_path, blob, db, name="b.tsv"):
    bt, tj = tmp_path / name, tmp_path / "t.json"
    bt.write_bytes(blob)
    tj.write_text(db)
    return str(bt), str(tj)


# ---- byte-level cases: the stage bound in both forms, the long line, row counts, line ends, the `;` list ---------------------------
@pytest.mark.parametrize("name", sorted(K.ACCEPTED))
def test_accepted_byte_level_case(tmp_path, name):
    spec, case = K.ACCEPTED[name][0], K.accepted_case(name)
    t, ck = K.expected_of(name)
    bt, tj = _write(tmp_path, case.blob, E.db_json())
    got = pipeline.ingest_columns(bt, tj, device=0, blast_outfmt=spec)
    assert pipeline.last_ingest_path() == "gpu"
    assert_columns_equal(got, t)
    assert ref.checksum(got) == ck


# ---- the three builds, on thirteen columns (a wrong kernel choice parses "successfully") and on thirty ------------------------------
@pytest.mark.parametrize("mode", sorted(K.MODES))
@pytest.mark.parametrize("layout", ["std_staxids", "wide"])
def test_modes_agree_with_the_host_parser(tmp_path, layout, mode):
    spec, kw = R.LAYOUTS[layout][0], K.MODES[mode]
    bt, tj = _write(tmp_path, K.modes_table(spec, b";1;2"), E.db_json())
    host = pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec, **kw)
    assert pipeline.last_ingest_path() == "cpu"
    got = pipeline.ingest_columns(bt, tj, device=0, blast_outfmt=spec, **kw)
    assert pipeline.last_ingest_path() == "gpu"
    assert_columns_equal(got, host)
    for key in ("n_lines", "n_kept", "taxon_filter"):
        assert got.get(key) == host.get(key), key


# ---- declined files go to the host parser with the same layout -----------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["std_staxids", "wide"])
@pytest.mark.parametrize("what", ["a_quoted_query", "a_quote_inside_an_accession", "blank_line_in_the_middle", "crlf_only_line_at_the_end",
                                  "a_16_digit_identity", "a_16_digit_taxid_in_a_list"])
def test_declined_files_are_read_by_the_host_parser_with_the_layout(tmp_path, layout, what):
    spec, fillers = R.LAYOUTS[layout]
    if what in E.DECLINED:
        relaid = R.relayout(E.declined_cases()[what].blob, spec, fillers)
    else:
        rows = [E._row(i // 3, i) for i in range(40)]
        f = rows[7].split(b"\t")
        if what == "a_16_digit_identity":
            f[3] = b"99.12345678901234"                  # (sixteen counted digits: beyond the one-operation fast path)
        else:
            f[2] = b"1234567890123456"                   # (in front of the `;` of a list)
        rows[7] = b"\t".join(f)
        relaid = R.relayout(E._table(rows), spec, dict(fillers, **{";": b";77"}))
    assert not K.plain_form(relaid, spec)
    t, ck = E.expected(R.to_reference(relaid, spec), E.db_json())
    bt, tj = _write(tmp_path, relaid, E.db_json())
    got = pipeline.ingest_columns(bt, tj, device=0, blast_outfmt=spec)
    assert pipeline.last_ingest_path() == "cpu"
    assert_columns_equal(got, t)
    assert ref.checksum(got) == ck


# ---- the whole run: byte for byte the run on the reference-order copy --------------------------------------------------------------
_BASELINE = {}


def _run(tmp_path, tag, table, tj, fmt, capsys, **kw):
    """one run with every output file -> {doc, report, table, support, stderr: bytes, counts}"""
    paths = {k: str(tmp_path / f"{tag}.{k}") for k in ("doc", "report", "table", "support")}
    cfg = blast.BlastBuilder.default("/db/ref16s", "bacteria")
    cfg.run_id = "00000000-0000-4000-8000-000000000000"               # (one run id for every document)
    text, _ = pipeline.build_consensus_identities_with_tables(table, tj, "bacteria", "relaxed", out_format=fmt, lenient=True, parse=False,
                                                              config=cfg, **{k: v for k, v in kw.items() if k != "count_table"})
    _, stats = pipeline.build_consensus_identities_with_tables(
        table, tj, "bacteria", "relaxed", out_format=fmt, lenient=True, parse=False, config=cfg, out_path=paths["doc"],
        report_path=paths["report"], sample_table_path=paths["table"], support_table_path=paths["support"], **kw)
    out = {k: open(p, "rb").read() for k, p in paths.items()}
    assert out["doc"] == text.encode()                                  # the text entry gives the same document
    capsys.readouterr()
    cli._say_kept(stats, kw.get("hit_filter") is not None)
    out["stderr"] = capsys.readouterr().err
    out["counts"] = {k: v for k, v in stats.items() if not k.startswith("t_")}
    return out


@pytest.mark.parametrize("parser", ["gpu", "cpu"])
@pytest.mark.parametrize("selection", ["all", "none"])
@pytest.mark.parametrize("layout", sorted(R.LAYOUTS))
def test_the_run_is_the_run_on_the_reference_copy(tmp_path, monkeypatch, capsys, layout, selection, parser):
    monkeypatch.setenv("BLU_INGEST", parser)
    spec, fillers = R.LAYOUTS[layout]
    blob13, db = K.golden_table()
    relaid = R.relayout(blob13, spec, fillers)
    copy = R.to_reference(relaid, spec)
    assert K.plain_form(relaid, spec)
    kw = K.SELECT_ALL if selection == "all" else {}
    fmt = "json" if selection == "all" else "jsonl"
    bt, tj = _write(tmp_path, relaid, db)
    got = _run(tmp_path, "laid", bt, tj, fmt, capsys, blast_outfmt=spec, **kw)
    assert pipeline.last_ingest_path() == parser
    if (copy, selection, parser) not in _BASELINE:                      # (the copies of most layouts are the same bytes: one run for them)
        ct, _ = _write(tmp_path, copy, db, "copy.tsv")
        _BASELINE[(copy, selection, parser)] = _run(tmp_path, "copy", ct, tj, fmt, capsys, **kw)
        assert pipeline.last_ingest_path() == parser
    today = _BASELINE[(copy, selection, parser)]
    for key in ("doc", "report", "table", "support", "stderr", "counts"):
        assert got[key] == today[key], key
    if selection == "all":
        assert got["stderr"].count("\n") >= 5 and got["counts"]["n_kept"] < got["counts"]["n_lines"]


@pytest.mark.parametrize("fmt", ["yaml", "json-compact"])
def test_the_other_document_formats_and_the_count_table(tmp_path, capsys, fmt):
    spec, fillers = R.LAYOUTS["wide"]
    blob13, db = K.golden_table()
    relaid = R.relayout(blob13, spec, fillers)
    bt, tj = _write(tmp_path, relaid, db)
    ct, _ = _write(tmp_path, R.to_reference(relaid, spec), db, "copy.tsv")
    names = sorted({ln.split(b"\t")[0] for ln in blob13.split(b"\n") if ln})
    counts = tmp_path / "counts.tsv"
    counts.write_bytes(b"#OTU ID\tA\tB\n" + b"".join(b"%s\t%d\t%d\n" % (n, i % 5, 1 + i % 3) for i, n in enumerate(names)))
    kw = dict(hit_filter={"min_perc_identity": 90.0}, count_table=str(counts))
    got = _run(tmp_path, "laid", bt, tj, fmt, capsys, blast_outfmt=spec, **kw)
    assert pipeline.last_ingest_path() == "gpu"
    today = _run(tmp_path, "copy", ct, tj, fmt, capsys, **kw)
    for key in ("doc", "report", "table", "support", "stderr", "counts"):
        assert got[key] == today[key], key


def test_the_cli_flag_reaches_the_library(tmp_path, capsys):
    spec, fillers = R.LAYOUTS["std_staxids"]
    blob13, db = K.golden_table()
    blob13 = blob13.replace(b"\t77\t", b"\t1000\t")                    # (the command line is strict: no taxid the database lacks)
    relaid = R.relayout(blob13, spec, fillers)
    bt, tj = _write(tmp_path, relaid, db)
    ct, _ = _write(tmp_path, R.to_reference(relaid, spec), db, "copy.tsv")
    common = ["-t", tj, "--taxon", "bacteria", "--strategy", "relaxed", "--out-format", "jsonl", "--max-e-value", "1e-4", "--report"]
    out = {}
    for tag, argv in (("laid", [bt, "--blast-outfmt", spec]), ("copy", [ct])):
        assert cli.main(["blastn", "build-consensus"] + argv + common + [str(tmp_path / f"{tag}.report"),
                                                                         "--blutils-out-file", str(tmp_path / f"{tag}.jsonl")]) == 0
        assert pipeline.last_ingest_path() == "gpu"
        out[tag] = (open(tmp_path / f"{tag}.report", "rb").read(), capsys.readouterr().err)
    assert out["laid"] == out["copy"] and "hit filter: kept" in out["laid"][1] and len(out["laid"][0].splitlines()) > 10
