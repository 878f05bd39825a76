"""Query coverage (`--min-query-cover`) on the GPU: the cover builds of the layout parse kernels
(csrc/ingest_gpu.hip: parse_rows_layout_qcov, parse_rows_layout_qcov_taxa and their general forms) held to the Python restatement
(tests/query_cover_reference.py: the copy without the lines below the cover, read by tests/ingest_reference.py) and to the host
parser, and the whole run — document, report, sample, support and count tables, the other selections' stderr lines — held to the
run without the flag on that copy.  Every accepted case must be read by the GPU parser itself (`last_ingest_path() == "gpu"`);
only the cases built to be declined take the host path, and they assert that.  tests/test_query_cover.py checks without a GPU that
every byte-level case lies where it claims."""
import os

import pytest

from blutils_amd import _native as N
from blutils_amd import cli, pipeline
from tests import ingest_edges as E
from tests import ingest_reference as ref
from tests import outfmt_cases as K
from tests import outfmt_reference as R
from tests import query_cover_cases as QC
from tests import query_cover_reference as Q
from tests.test_gpu_outfmt import _run, _write
from tests.test_ingest_edges import assert_columns_equal
from tests.test_query_cover import FILLERS, GOLDEN, covered_golden

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


def _expect(blob, spec, cover):
    """(columns, checksum, n_lines, n_below) by the restatement: the independent reading of the copy in the reference's columns"""
    copy, n_below = Q.drop_lines(blob, spec, cover)
    t, ck = E.expected(R.to_reference(copy, spec), E.db_json())
    return t, ck, len([1 for ln, _ in R._lines(blob) if ln]), n_below


def _check(tmp_path, blob, spec, cover, path="gpu", **kw):
    t, ck, n, n_below = _expect(blob, spec, cover)
    bt, tj = _write(tmp_path, blob, E.db_json())
    got = pipeline.ingest_columns(bt, tj, device=0, blast_outfmt=spec, query_cover=cover, **kw)
    assert pipeline.last_ingest_path() == path
    assert got["query_cover"]["n_below"] == n_below and got["query_cover"]["n_lines"] == n == got["n_lines"]
    if not kw:
        assert got["n_kept"] == n - n_below
        assert_columns_equal(got, t)
        assert ref.checksum(got) == ck
    return got, n, n_below


# ---- line counts and byte-level edges, for the three sources ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(QC.ACCEPTED))
def test_accepted_byte_level_case(tmp_path, name):
    source, spec, _ = QC.ACCEPTED[name]
    _, n, n_below = _check(tmp_path, QC.accepted_case(name).blob, spec, QC.SOURCES[source]["cover"])
    assert n == 1 or 0 < n_below < n


# ---- threshold boundaries -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("percent", QC.LEN_PERCENTS)
def test_the_exact_ratio_at_its_boundaries(tmp_path, percent):
    _check(tmp_path, QC.boundary_table(QC.LEN_SPEC), QC.LEN_SPEC, {"percent": percent, "source": "qlen"})


def test_the_boundary_rows_fall_on_both_sides():
    """(no GPU) 80 percent of 1500 is a span of 1200: 1199 is below, 1200 and 1201 are not; one base of three is 33.333.. percent"""
    m = Q.milli
    assert [Q.keeps("qlen", m("80"), v) for v in QC.LEN_ROWS[:6]] == [False, True, True, True, False, True]
    assert Q.keeps("qlen", m("33.333"), (2, 2, 3)) and not Q.keeps("qlen", m("33.334"), (2, 2, 3))
    assert Q.keeps("qlen", m("66.666"), (1, 2, 3)) and not Q.keeps("qlen", m("66.667"), (1, 2, 3))
    assert Q.keeps("qlen", m("100"), (1, 400, 300)) and Q.keeps("qlen", m("100"), (0, QC.TOP, QC.TOP))
    assert [Q.keeps("qcovhsp", m(p), (c,)) for p, c in (("0", 0), ("100", 100), ("100", 99), ("0.001", 0), ("80", 80), ("80.001", 80))] == \
           [True, True, False, False, True, False]


@pytest.mark.parametrize("percent", QC.HSP_PERCENTS)
def test_the_percent_column_at_its_boundaries(tmp_path, percent):
    _check(tmp_path, QC.boundary_table(QC.HSP_SPEC), QC.HSP_SPEC, {"percent": percent})


@pytest.mark.parametrize("spec,fields", [(QC.LEN_SPEC, {"qlen": b"2147483648"}), (QC.LEN_SPEC, {"qend": b"2147483648"}), (QC.LEN_SPEC, {"qlen": b"0"}),
                                         (QC.HSP_SPEC, {"qcovhsp": b"2147483648"}), (QC.HSP_SPEC, {"qcovhsp": b"-1"}), (QC.HSP_SPEC, {"qcovhsp": b"8x"})])
@pytest.mark.parametrize("form", ["staged", "general"])
def test_a_value_out_of_range_is_declined_and_the_error_is_the_hosts(tmp_path, spec, fields, form):
    blob = QC.boundary_table(spec, top=False)
    if form == "general":
        blob = Q.set_fields(blob, spec, lambda i: {"mismatch": b"m" * 200})       # 256 lines of more than 128 bytes: beyond the stage
        assert E.block_forms(blob)[0][1] == "general"                            # (line 151 lies in the first block)
    blob = Q.set_fields(blob, spec, lambda i: fields if i == 150 else {})
    bt, tj = _write(tmp_path, blob, E.db_json())
    errors = []
    for device in (0, -1):
        with pytest.raises(N.BluError, match=r"line 151\b.*query cover column") as e:
            pipeline.ingest_columns(bt, tj, device=device, blast_outfmt=spec, query_cover="0")
        assert e.value.code == 8 and pipeline.last_ingest_path() == "cpu"
        errors.append(str(e.value))
    assert errors[0] == errors[1]


# ---- combinations -------------------------------------------------------------------------------------------------------------------------
def _modes_table(spec):
    """tests/outfmt_cases.py's table of the parse modes (both forms, e-values spelled like the threshold, taxa on and off the
    lists) with coverage fields: every third line below 80 percent"""
    cols = R.columns_of(spec)
    fields = lambda i: {"qlen": (b"500", b"400", b"501")[i % 3], "qstart": b"1", "qend": b"400", "qcovhsp": (b"80", b"100", b"79")[i % 3]}
    return Q.set_fields(K.modes_table(spec), spec, lambda i: {k: v for k, v in fields(i).items() if k in cols})


@pytest.mark.parametrize("mode", [m for m in sorted(K.MODES) if m != "plain"])
@pytest.mark.parametrize("spec", [QC.LEN_SPEC, QC.HSP_SPEC])
def test_beside_the_other_filters_both_parsers_agree(tmp_path, spec, mode):
    blob, kw = _modes_table(spec), K.MODES[mode]
    got, n, n_below = _check(tmp_path, blob, spec, {"percent": "80"}, **kw)
    assert n_below == 200 and n == 600
    bt, tj = _write(tmp_path, blob, E.db_json())
    host = pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec, query_cover="80", **kw)
    assert pipeline.last_ingest_path() == "cpu"
    assert_columns_equal(got, host)
    for key in ("n_lines", "n_kept", "taxon_filter", "query_cover"):
        assert got.get(key) == host.get(key), key
    # and both give the run without the flag on the copy: the e-values spelled like the threshold are still decided
    copy, _ = Q.drop_lines(blob, spec, {"percent": "80"})
    ct, _ = _write(tmp_path, copy, E.db_json(), "copy.tsv")
    today = pipeline.ingest_columns(ct, tj, device=0, blast_outfmt=spec, **kw)
    assert pipeline.last_ingest_path() == "gpu"
    assert_columns_equal(got, today)
    assert got["n_kept"] == today["n_kept"] and 0 < got["n_kept"] < 400
    if "taxon_filter" in kw:                                 # counted over every line, as without the cover
        alone = pipeline.ingest_columns(bt, tj, device=0, blast_outfmt=spec, **kw)
        assert got["taxon_filter"] == alone["taxon_filter"] and got["taxon_filter"]["n_excluded"] > today["taxon_filter"]["n_excluded"]


def test_a_cover_that_keeps_nothing_goes_to_the_host_parser(tmp_path):
    blob = QC.boundary_table(QC.HSP_SPEC, top=False)
    blob = Q.set_fields(blob, QC.HSP_SPEC, lambda i: {"qcovhsp": b"%d" % (i % 80)})
    got, n, n_below = _check(tmp_path, blob, QC.HSP_SPEC, {"percent": "80"}, path="cpu")
    assert n_below == n == 300 and got["n_kept"] == 0 and got["pident"].size == 0


@pytest.mark.parametrize("spec", [QC.LEN_SPEC, QC.HSP_SPEC])
def test_a_cover_that_keeps_everything_gives_the_columns_without_it(tmp_path, spec):
    blob = QC.boundary_table(spec)
    got, n, n_below = _check(tmp_path, blob, spec, {"percent": "0"})
    assert n_below == 0 and got["n_kept"] == n
    bt, tj = _write(tmp_path, blob, E.db_json())
    plain = pipeline.ingest_columns(bt, tj, device=0, blast_outfmt=spec)
    assert pipeline.last_ingest_path() == "gpu"
    assert_columns_equal(got, plain)


# ---- the whole run: byte for byte the run without the flag on the copy ---------------------------------------------------------------------------
PARSER_LINES = ("taxon filter:", "  ", "query cover:", "hit filter:")     # counted by the parser over the table's lines: not the copy's


def _others(stderr):
    return [ln for ln in stderr.splitlines() if not ln.startswith(PARSER_LINES)]


@pytest.mark.parametrize("parser", ["gpu", "cpu"])
@pytest.mark.parametrize("selection", ["all", "cover_alone"])
@pytest.mark.parametrize("name", ["qlen", "qcovhsp", "qcovs"])
def test_the_run_is_the_run_on_the_copy(tmp_path, monkeypatch, capsys, name, selection, parser):
    monkeypatch.setenv("BLU_INGEST", parser)
    spec, cover, relaid, copy, n_below, db = covered_golden(name)
    assert K.plain_form(relaid, spec)
    kw = K.SELECT_ALL if selection == "all" else {}
    fmt = "json" if selection == "all" else "jsonl"
    names = sorted({ln.split(b"\t")[R.parse_spec(spec)["query"]] for ln in relaid.split(b"\n") if ln})
    counts = tmp_path / "counts.tsv"
    counts.write_bytes(b"#OTU ID\tA\tB\n" + b"".join(b"%s\t%d\t%d\n" % (q, i % 5, 1 + i % 3) for i, q in enumerate(names)))
    bt, tj = _write(tmp_path, relaid, db)
    ct, _ = _write(tmp_path, copy, db, "copy.tsv")
    got = _run(tmp_path, "covered", bt, tj, fmt, capsys, blast_outfmt=spec, query_cover=cover, count_table=str(counts), **kw)
    assert pipeline.last_ingest_path() == parser
    today = _run(tmp_path, "copy", ct, tj, fmt, capsys, blast_outfmt=spec, count_table=str(counts), **kw)
    assert pipeline.last_ingest_path() == parser
    for key in ("doc", "report", "table", "support"):
        assert got[key] == today[key], key
    assert _others(got["stderr"]) == _others(today["stderr"]) and len(_others(got["stderr"])) == (4 if selection == "all" else 1)
    n = relaid.count(b"\n")
    assert f"query cover: {n_below} of {n} lines under {cover['percent']} percent (from {got['counts']['query_cover']['source']})\n" in got["stderr"]
    assert f"hit filter: kept {got['counts']['n_kept']} of {n} lines\n" in got["stderr"]          # also when coverage is the only filter
    assert got["stderr"].index("query cover:") < got["stderr"].index("hit filter:")
    if selection == "all":
        assert got["stderr"].index("taxon filter:") < got["stderr"].index("query cover:")
    else:
        assert got["counts"]["n_kept"] == n - n_below
    skip = ("n_lines", "n_kept", "taxon_filter", "query_cover")         # (the parser's counts: over the table's lines, not the copy's)
    assert got["counts"]["n_kept"] == today["counts"].get("n_kept", n - n_below)
    assert {k: v for k, v in got["counts"].items() if k not in skip} == {k: v for k, v in today["counts"].items() if k not in skip}
    assert got["counts"]["query_cover"] == {"n_lines": n, "n_below": n_below, "percent": cover["percent"], "source": Q.resolve(spec, cover.get("source", "auto"))["source"]}


def test_the_cli_gives_the_bytes_of_the_run_on_the_filtered_copy(tmp_path, capsys):
    spec = "6 std staxids qlen"
    blob13, db = K.golden_table()
    blob13 = blob13.replace(b"\t77\t", b"\t1000\t")                    # (the command line is strict: no taxid the database lacks)
    relaid = R.relayout(blob13, spec, FILLERS)
    copy, n_below = Q.drop_lines(relaid, spec, {"percent": "80"})
    bt, tj = _write(tmp_path, relaid, db)
    ct, _ = _write(tmp_path, copy, db, "copy.tsv")
    common = ["-t", tj, "--taxon", "bacteria", "--strategy", "relaxed", "--out-format", "jsonl", "--blast-outfmt", spec, "--report"]
    out = {}
    for tag, argv in (("covered", [bt, "--min-query-cover", "80"]), ("copy", [ct])):
        assert cli.main(["blastn", "build-consensus"] + argv + common + [str(tmp_path / f"{tag}.report"),
                                                                         "--blutils-out-file", str(tmp_path / f"{tag}.jsonl")]) == 0
        assert pipeline.last_ingest_path() == "gpu"
        # (every result of a document carries the call's fresh run id: the documents are compared in the test above, under one id)
        out[tag] = (len(open(tmp_path / f"{tag}.jsonl", "rb").read().splitlines()), open(tmp_path / f"{tag}.report", "rb").read(), capsys.readouterr().err)
    assert out["covered"][0] == out["copy"][0] > 10 and out["covered"][1] == out["copy"][1] and len(out["copy"][1].splitlines()) > 10
    n = relaid.count(b"\n")
    assert out["covered"][2] == f"query cover: {n_below} of {n} lines under 80 percent (from qlen)\nhit filter: kept {n - n_below} of {n} lines\n"
    assert out["copy"][2] == ""
