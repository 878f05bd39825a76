"""Query coverage (`--min-query-cover`) without a GPU: the resolver against its Python restatement
(tests/query_cover_reference.py), the C ABI's new structs and refusals, and the host parser (device=-1) on relaid golden tables
with coverage fields — its columns against the independent reading (tests/ingest_reference.py) of the copy without the failing
lines, alone and beside the hit and taxon filters.  The document-level contract needs the engine: tests/test_gpu_query_cover.py."""
import ctypes as C
import re

import pytest

from blutils_amd import _native as N
from blutils_amd import cli, pipeline
from tests import ingest_edges as E
from tests import ingest_reference as ref
from tests import outfmt_cases as K
from tests import outfmt_reference as R
from tests import query_cover_reference as Q
from tests.test_ingest_edges import assert_columns_equal

BLU_ERR_PARSE = 8
LEN_SPEC, HSP_SPEC, SUBJ_SPEC = "6 std staxid qlen", "6 std staxid qcovhsp", "6 std staxids qcovs"
ALL_SPEC = "6 qcovs std staxid qlen qcovhsp"                  # every source at once: qcovs first, qcovhsp last


def _write(tmp_path, blob, db, name="b.tsv"):
    bt, tj = tmp_path / name, tmp_path / "t.json"
    bt.write_bytes(blob)
    tj.write_text(db)
    return str(bt), str(tj)


# ---- the resolver -------------------------------------------------------------------------------------------------------------------------
RESOLVED = [
    (HSP_SPEC, "auto", "qcovhsp"), (LEN_SPEC, "auto", "qlen"), (SUBJ_SPEC, "auto", "qcovs"), (ALL_SPEC, "auto", "qcovhsp"),
    (ALL_SPEC, "qlen", "qlen"), (ALL_SPEC, "qcovs", "qcovs"), (ALL_SPEC, "qcovhsp", "qcovhsp"),
    ("6 std staxids qcovs qlen", "auto", "qlen"), ("6 qcovs std staxid qcovhsp", "auto", "qcovhsp"),
    ("qlen qseqid sseqid staxid pident length bitscore qend qstart qcovs", "auto", "qlen"),
    ("qseqid sseqid staxid pident length bitscore qstart qend qcovs", "auto", "qcovs"),          # (no qlen: the pair alone is no source)
]
REFUSED = [
    ("6 std staxid", "auto", ("qcovhsp", "qlen", "qcovs")), ("6 std staxid", "qlen", ("qlen",)), ("6 std staxid", "qcovhsp", ("qcovhsp",)),
    ("6 std staxid qlen", "qcovs", ("qcovs",)), ("6 std staxid qcovs", "qcovhsp", ("qcovhsp",)),
    ("qseqid sseqid staxid pident length bitscore qlen", "qlen", ("qstart", "qend")),
    ("qseqid sseqid staxid pident length bitscore", "auto", ("qcovhsp", "qstart", "qend", "qlen", "qcovs")),
]


@pytest.mark.parametrize("spec,source,resolved", RESOLVED)
def test_the_source_resolves_as_restated(spec, source, resolved):
    exp = Q.resolve(spec, source)
    got = pipeline.query_cover_columns(spec, source, "12.5")
    assert exp["source"] == resolved == got["source"] and got["min_cover_milli"] == 12500
    named = {"qcovhsp": "cover_column", "qcovs": "cover_column"}
    for name in ("qstart", "qend", "qlen", "qcovhsp", "qcovs"):
        if name in exp["columns"]:
            assert got[named.get(name, name)] == exp["columns"][name], name
    unused = {"qstart", "qend", "qlen"} if resolved != "qlen" else {"cover_column"}
    assert all(got[k] is None for k in unused)


@pytest.mark.parametrize("spec,source,missing", REFUSED)
def test_a_source_the_format_string_lacks_names_the_specifiers(spec, source, missing):
    with pytest.raises(Q.CoverError) as r:
        Q.resolve(spec, source)
    assert set(missing) <= set(r.value.missing)
    with pytest.raises(N.BluError) as e:
        pipeline.query_cover_columns(spec, source)
    assert e.value.code == N.BLU_ERR_INVALID_ARG
    tail = str(e.value).split("lacks", 1)[1]
    assert set(re.findall(r"`(\w+)`", tail)) == set(r.value.missing), str(e.value)


@pytest.mark.parametrize("spec,token", [("7 std staxid qlen", "7"), ("std std staxid qlen", "qseqid"), ("std staxid qlen qlen", "qlen"),
                                        ("std qlen", "staxid"), ("std staxid q-len", "q-len")])
def test_the_layouts_refusals_are_the_resolvers(spec, token):
    with pytest.raises(R.SpecError):
        Q.resolve(spec)
    with pytest.raises(N.BluError, match=re.escape(f"`{token}`")) as e:
        pipeline.query_cover_columns(spec)
    assert e.value.code == N.BLU_ERR_INVALID_ARG


@pytest.mark.parametrize("text,value", [("0", 0), ("100", 100000), ("80", 80000), ("33.333", 33333), ("0.001", 1), (" 99.5 ", 99500), ("100.000", 100000)])
def test_the_percent_is_read_exactly(text, value):
    assert pipeline.min_query_cover_milli(text) == value
    assert Q.milli(text.strip()) == value


@pytest.mark.parametrize("text", ["100.001", "-1", "33.3333", "nan", "inf", "", "eighty", 80.0, True])
def test_a_percent_that_is_refused(text):
    with pytest.raises(ValueError, match="min_query_cover"):
        pipeline.min_query_cover_milli(text)


# ---- the structs --------------------------------------------------------------------------------------------------------------------------
def test_struct_sizes_exports_and_abi():
    L = pipeline._bind()
    assert C.sizeof(pipeline.QueryCoverC) == 40 and C.sizeof(pipeline.QueryCoverStats) == 16
    assert [getattr(pipeline.QueryCoverC, f).offset for f, _ in pipeline.QueryCoverC._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32]
    assert C.sizeof(pipeline.ConsensusRequest) == 136 and C.sizeof(pipeline.ConsensusExtras) == 24 and C.sizeof(pipeline.TableLayoutC) == 40
    assert C.sizeof(pipeline.HitFilterC) == 40 and L.blu_abi_version() == 5
    for name in ("blu_query_cover_parse", "blu_build_consensus_covered", "blu_ingest_columns_covered"):
        assert name in N.PIPELINE_EXPORTS and hasattr(L, name)
    for size in (0, 36, 44):
        c = pipeline.QueryCoverC(struct_size=size)
        assert L.blu_query_cover_parse(LEN_SPEC.encode(), 0, C.byref(c)) == N.BLU_ERR_INVALID_ARG and "struct_size" in N.last_error()
    good = pipeline.QueryCoverC(struct_size=40)
    assert L.blu_query_cover_parse(None, 0, C.byref(good)) == N.BLU_ERR_INVALID_ARG
    assert L.blu_query_cover_parse(LEN_SPEC.encode(), 0, None) == N.BLU_ERR_INVALID_ARG
    assert L.blu_query_cover_parse(LEN_SPEC.encode(), 4, C.byref(good)) == N.BLU_ERR_INVALID_ARG and "source" in N.last_error()


def test_a_cover_struct_the_library_does_not_take(tmp_path):
    """every refusal comes before a file is opened: the table does not exist"""
    bt, tj = str(tmp_path / "absent.tsv"), str(tmp_path / "absent.json")
    L = pipeline._bind()
    lay = pipeline.table_layout(LEN_SPEC)                     # qstart 6, qend 7, qlen 13; 14 columns
    good = pipeline._Cover({"percent": "80"}, LEN_SPEC).c
    assert (good.source, good.qstart, good.qend, good.qlen, good.cover_column) == (2, 6, 7, 13, pipeline.TABLE_LAYOUT_NO_COLUMN)
    cols, st = pipeline.IngestColumns(), pipeline.HitSelectionStats()
    call = lambda cov, layout=lay: L.blu_ingest_columns_covered(bt.encode(), tj.encode(), 0, -1, C.byref(layout) if layout is not None else None,
                                                                C.byref(cov), None, C.byref(cols), C.byref(st))
    for field, value, word in (("struct_size", 36, "struct_size"), ("struct_size", 44, "struct_size"), ("source", 0, "source"), ("source", 4, "source"),
                               ("min_cover_milli", 100001, "thousandths"), ("qlen", 14, "qlen column 14"), ("qstart", 0xFFFFFFFF, "qstart column"),
                               ("qend", 0, "query column"), ("qlen", 10, "e_value column"), ("qend", 6, "both column 6")):
        cov = pipeline.QueryCoverC.from_buffer_copy(good)
        setattr(cov, field, value)
        assert call(cov) == N.BLU_ERR_INVALID_ARG and word in N.last_error(), (field, value, N.last_error())
    one = pipeline._Cover({"percent": "80"}, HSP_SPEC).c
    for value, word in ((14, "cover column 14"), (2, "perc_identity column")):
        cov = pipeline.QueryCoverC.from_buffer_copy(one)
        cov.cover_column = value
        assert call(cov, pipeline.table_layout(HSP_SPEC)) == N.BLU_ERR_INVALID_ARG and word in N.last_error(), (value, N.last_error())
    assert call(good, None) == N.BLU_ERR_INVALID_ARG and "no query length" in N.last_error()          # a cover without a layout
    assert call(good) == 7 and "absent" in N.last_error()                                              # accepted: the files are looked for (BLU_ERR_IO)
    # the use-case's entry point refuses the same way
    rq, oc, p = pipeline.ConsensusRequest(struct_size=136), pipeline.ConsensusOutcome(), pipeline.PipelineParams()
    rq.blast_output_file, rq.taxonomies_file, rq.params = bt.encode(), tj.encode(), C.pointer(p)
    bad = pipeline.QueryCoverC.from_buffer_copy(good)
    bad.min_cover_milli = 100001
    assert L.blu_build_consensus_covered(C.byref(rq), None, C.byref(lay), C.byref(bad), C.byref(oc)) == N.BLU_ERR_INVALID_ARG and "thousandths" in N.last_error()
    assert L.blu_build_consensus_covered(C.byref(rq), None, None, C.byref(good), C.byref(oc)) == N.BLU_ERR_INVALID_ARG and "no query length" in N.last_error()


def test_the_keyword_needs_the_format_string():
    for kw in ({}, {"blast_outfmt": None}, {"blast_outfmt": pipeline.table_layout(LEN_SPEC)}):
        with pytest.raises(ValueError, match="no query length"):
            pipeline.ingest_columns("absent.tsv", "absent.json", query_cover="80", **kw)
    with pytest.raises(ValueError, match="source"):
        pipeline.ingest_columns("absent.tsv", "absent.json", query_cover={"percent": "80", "source": "slen"}, blast_outfmt=LEN_SPEC)
    with pytest.raises(ValueError, match="unknown keys"):
        pipeline.ingest_columns("absent.tsv", "absent.json", query_cover={"percent": "80", "from": "qlen"}, blast_outfmt=LEN_SPEC)


# ---- the host parser on golden tables with coverage fields ------------------------------------------------------------------------------------
# the golden table's qstart / qend are 1 / 400 on every line: span 400
FILLERS = {"qlen": lambda i: (b"400", b"450", b"500", b"501", b"1500", b"399")[i % 6], "qcovhsp": lambda i: (b"100", b"80", b"79", b"0", b"81")[i % 5],
           "qcovs": lambda i: (b"79", b"100", b"80")[i % 3], ";": lambda i: (b"", b";9606")[i % 2]}
GOLDEN = {"qlen": (LEN_SPEC, {"percent": "80", "source": "auto"}), "qcovhsp": (HSP_SPEC, {"percent": "80"}),
          "qcovs": (SUBJ_SPEC, {"percent": "80", "source": "qcovs"}), "qlen_of_all": (ALL_SPEC, {"percent": "79.999", "source": "qlen"}),
          "qcovs_of_all": (ALL_SPEC, {"percent": "80", "source": "qcovs"})}


def covered_golden(name):
    spec, cover = GOLDEN[name]
    blob13, db = K.golden_table()
    relaid = R.relayout(blob13, spec, FILLERS)
    copy, n_below = Q.drop_lines(relaid, spec, cover)
    return spec, cover, relaid, copy, n_below, db


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_the_host_parser_gives_the_columns_of_the_copy(tmp_path, name):
    spec, cover, relaid, copy, n_below, db = covered_golden(name)
    n = relaid.count(b"\n")
    assert 0 < n_below < n and copy.count(b"\n") == n - n_below
    bt, tj = _write(tmp_path, relaid, db)
    ct, _ = _write(tmp_path, R.to_reference(copy, spec), db, "copy13.tsv")
    exp = ref.read_table(ct, tj)
    got = pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec, query_cover=cover)
    assert pipeline.last_ingest_path() == "cpu"
    assert_columns_equal(got, exp)
    assert ref.checksum(got) == ref.checksum(exp)
    assert (got["n_lines"], got["n_kept"]) == (n, n - n_below)
    assert got["query_cover"] == {"n_lines": n, "n_below": n_below, "percent": cover["percent"], "source": Q.resolve(spec, cover.get("source", "auto"))["source"]}
    # beside the hit and taxon filters: the library's own columns and counts on the copy, through the path without the flag
    lt, _ = _write(tmp_path, copy, db, "copy.tsv")
    got = pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec, query_cover=cover, **K.SELECT_HOST)
    today = pipeline.ingest_columns(lt, tj, device=-1, blast_outfmt=spec, **K.SELECT_HOST)
    assert_columns_equal(got, today)
    assert got["n_kept"] == today["n_kept"] and 0 < got["n_kept"] < n - n_below
    assert got["query_cover"]["n_below"] == n_below                   # whatever the other filters say
    # the taxon verdict is counted as without the cover: over every line of the table
    alone = pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec, taxon_filter=K.SELECT_HOST["taxon_filter"])
    assert got["taxon_filter"] == alone["taxon_filter"] and got["taxon_filter"]["n_excluded"] > today["taxon_filter"]["n_excluded"] > 0


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_percent_zero_is_the_call_without_the_flag(tmp_path, name):
    spec, cover, relaid, _, _, db = covered_golden(name)
    bt, tj = _write(tmp_path, relaid, db)
    zero = pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec, query_cover=dict(cover, percent="0"))
    plain = pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec)
    assert_columns_equal(zero, plain)
    assert ref.checksum(zero) == ref.checksum(plain)
    assert zero["query_cover"]["n_below"] == 0 and zero["n_kept"] == zero["n_lines"] == relaid.count(b"\n")


def test_a_cover_over_the_references_own_columns_by_other_names(tmp_path):
    """thirteen columns in the reference's order are no layout (§23) — under a cover they are still read through it"""
    spec = "qacc sacc staxid pident length qcovhsp b c d e f evalue bitscore"
    assert pipeline._layout(spec) is None
    blob13, db = K.golden_table()
    relaid = R.relayout(blob13, spec, FILLERS)
    copy, n_below = Q.drop_lines(relaid, spec, {"percent": "80"})
    bt, tj = _write(tmp_path, relaid, db)
    ct, _ = _write(tmp_path, copy, db, "copy.tsv")
    got = pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec, query_cover="80")
    assert_columns_equal(got, ref.read_table(ct, tj))
    assert got["query_cover"]["n_below"] == n_below > 0


def test_quotes_blank_lines_and_crlf(tmp_path):
    rows = [K.line(HSP_SPEC, b"q%d" % (i // 2), b"A%d.1" % i, pid=90 + i) for i in range(8)]
    blob = Q.set_fields(E._table(rows), HSP_SPEC, lambda i: {"qcovhsp": (b"80", b"+80", b"079", b"79", b"100", b"0", b"00080", b"81")[i]})
    blob = blob.replace(b"\n", b"\r\n").replace(b"q1\t", b'"q1"\t', 1) + b"\r\n"                 # CR LF, a quoted query, a CR-LF-only line
    copy, n_below = Q.drop_lines(blob, HSP_SPEC, {"percent": "80"})
    assert n_below == 3
    bt, tj = _write(tmp_path, blob, E.db_json())
    got = pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=HSP_SPEC, query_cover="80")
    assert_columns_equal(got, E.expected(R.to_reference(copy, HSP_SPEC), E.db_json())[0])
    assert got["pident"].tolist() == [90.0, 91.0, 94.0, 96.0, 97.0] and got["query_cover"]["n_below"] == 3 and got["n_lines"] == 8


# ---- parse errors: on kept and dropped lines alike, and only under the flag --------------------------------------------------------------------
BAD_FIELDS = [b"abc", b"", b"-1", b"2147483648", b"80.0", b"8e1", b" 80", b'"80"', b"99999999999999999999"]


@pytest.mark.parametrize("field", BAD_FIELDS)
@pytest.mark.parametrize("source", ["qcovhsp", "qlen", "qcovs"])
def test_a_coverage_field_that_is_refused_names_the_line(tmp_path, source, field):
    spec = ALL_SPEC
    names = Q.NEEDS[source]
    for which in names:
        for line_kept in (True, False):
            rows = [K.line(spec, b"q%d" % i, b"A.1") for i in range(6)]
            ok = {"qcovhsp": b"90", "qcovs": b"90", "qstart": b"1", "qend": b"90", "qlen": b"100"} if line_kept else \
                 {"qcovhsp": b"10", "qcovs": b"10", "qstart": b"1", "qend": b"10", "qlen": b"100"}
            blob = Q.set_fields(E._table(rows), spec, lambda i: dict(ok, **({which: field} if i == 3 else {})))
            bt, tj = _write(tmp_path, blob, E.db_json())
            with pytest.raises(Q.FieldError) as r:
                Q.drop_lines(blob, spec, {"percent": "50", "source": source})
            assert r.value.line == 4
            with pytest.raises(N.BluError, match=r"line 4\b.*query cover column.*\(%s" % which) as e:
                pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec, query_cover={"percent": "50", "source": source})
            assert e.value.code == BLU_ERR_PARSE
            # the fields of the other sources, and all of them without the flag, are columns nobody reads
            others = [s for s in ("qcovhsp", "qlen", "qcovs") if which not in Q.NEEDS[s]]
            for s in others:
                assert pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec, query_cover={"percent": "50", "source": s})["n_lines"] == 6
            assert pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec)["pident"].size == 6


def test_qlen_zero_names_the_line_and_the_largest_values_pass(tmp_path):
    rows = [K.line(LEN_SPEC, b"q%d" % i, b"A.1") for i in range(4)]
    top = b"%d" % Q.INT32_MAX
    blob = Q.set_fields(E._table(rows), LEN_SPEC, lambda i: {"qstart": (b"1", b"0", top, b"5")[i], "qend": (b"10", top, b"0", b"5")[i],
                                                             "qlen": (b"10", top, top, b"0")[i]})
    bt, tj = _write(tmp_path, blob, E.db_json())
    with pytest.raises(N.BluError, match=r"line 4\b.*query cover column.*\(qlen") as e:
        pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=LEN_SPEC, query_cover="100")
    assert e.value.code == BLU_ERR_PARSE
    blob = blob.rsplit(b"\n", 2)[0] + b"\n"                              # without the fourth line: a span of 2^31 over qlen 2^31 - 1 passes
    bt, tj = _write(tmp_path, blob, E.db_json())
    got = pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=LEN_SPEC, query_cover="100")
    assert got["n_kept"] == 3 == Q.drop_lines(blob, LEN_SPEC, {"percent": "100"})[0].count(b"\n")


# ---- the byte-level cases of tests/test_gpu_query_cover.py, without a GPU: each lies where it claims, and the host parser reads it ------------
from tests import query_cover_cases as QC


@pytest.mark.parametrize("name", sorted(QC.ACCEPTED))
def test_byte_level_case_lies_where_it_claims(tmp_path, name):
    source, spec, _ = QC.ACCEPTED[name]
    case, cover = QC.accepted_case(name), QC.SOURCES[source]["cover"]
    c, blob = case.claims, case.blob
    assert K.plain_form(blob, spec)                        # the GPU parser has no reason to decline it
    got_source = Q.resolve(spec, cover["source"])
    assert got_source["source"] == source
    at = sorted(got_source["columns"].values())
    assert at[0] == 0 if "/first/" in name else at[-1] == R.parse_spec(spec)["n_columns"] - 1      # a coverage field first, or last
    forms = E.block_forms(blob)
    if "span" in c:
        assert forms[2] == (c["span"], c["form"]) and c["form"] == ("general" if c["span"] > E.STAGE_BYTES else "staged")
        if "crlf" in name:
            assert blob.count(b"\r\n") == blob.count(b"\n")
        if "open" in name:
            assert not blob.endswith(b"\n")
    if "forms" in c:
        assert [f for _, f in forms] == c["forms"]
    if "rows" in c:
        assert len(E.line_starts(blob)) - 1 == c["rows"]
    copy, n_below = Q.drop_lines(blob, spec, cover)
    n = len(E.line_starts(blob)) - 1
    assert n == 1 or 0.2 * n < n_below < 0.8 * n
    bt, tj = _write(tmp_path, blob, E.db_json())
    got = pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec, query_cover=cover)
    t, ck = E.expected(R.to_reference(copy, spec), E.db_json())
    assert_columns_equal(got, t)
    assert ref.checksum(got) == ck and got["query_cover"]["n_below"] == n_below and got["n_kept"] == n - n_below


@pytest.mark.parametrize("spec", [QC.LEN_SPEC, QC.HSP_SPEC])
def test_the_boundary_table_on_the_host_parser(tmp_path, spec):
    blob = QC.boundary_table(spec)
    bt, tj = _write(tmp_path, blob, E.db_json())
    for percent in (QC.LEN_PERCENTS if spec == QC.LEN_SPEC else QC.HSP_PERCENTS):
        copy, n_below = Q.drop_lines(blob, spec, {"percent": percent})
        got = pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec, query_cover=percent)
        assert got["query_cover"]["n_below"] == n_below, percent
        assert_columns_equal(got, E.expected(R.to_reference(copy, spec), E.db_json())[0])


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
COMMON = ["-t", "t.json", "--taxon", "bacteria", "--strategy", "relaxed"]


def test_cli_flags(tmp_path, capsys):
    import decimal
    ap = cli.build_parser()
    a = ap.parse_args(["blastn", "build-consensus", "b.tsv"] + COMMON + ["--blast-outfmt", LEN_SPEC, "--min-query-cover", "80.5"])
    assert a.min_query_cover == decimal.Decimal("80.5") and a.query_cover_from == "auto"
    a = ap.parse_args(["blastn", "build-consensus", "b.tsv"] + COMMON)
    assert a.min_query_cover is None and a.query_cover_from == "auto"
    for bad in (["--min-query-cover", "100.001"], ["--min-query-cover", "80", "--query-cover-from", "slen"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["blastn", "build-consensus", "b.tsv"] + COMMON + bad)
    with pytest.raises(SystemExit):                           # run-with-consensus has -q for blastn itself
        ap.parse_args(["blastn", "run-with-consensus", "q.fa", "-d", "db", "--blast-out-file", "b.tsv"] + COMMON + ["--min-query-cover", "80"])
    capsys.readouterr()
    absent = str(tmp_path / "absent.tsv")
    with pytest.raises(SystemExit, match="--min-query-cover needs --blast-outfmt.*no query length.*columns have to be named"):
        cli.main(["blastn", "build-consensus", absent] + COMMON + ["--min-query-cover", "80"])
    with pytest.raises(SystemExit, match="--min-query-cover: .*`qcovhsp`.*`qlen`.*`qcovs`"):
        cli.main(["blastn", "build-consensus", absent] + COMMON + ["--blast-outfmt", "6 std staxids", "--min-query-cover", "80"])
    with pytest.raises(SystemExit, match="--min-query-cover: .*source qlen.*lacks `qlen`"):
        cli.main(["blastn", "build-consensus", absent] + COMMON + ["--blast-outfmt", "6 std staxids qcovs", "--min-query-cover", "80", "--query-cover-from", "qlen"])
    with pytest.raises(SystemExit, match="--query-cover-from needs --min-query-cover"):
        cli.main(["blastn", "build-consensus", absent] + COMMON + ["--blast-outfmt", LEN_SPEC, "--query-cover-from", "qlen"])


def test_the_stderr_lines(capsys):
    stats = {"n_lines": 10, "n_kept": 6, "query_cover": {"n_lines": 10, "n_below": 3, "percent": "80.5", "source": "qlen"},
             "taxon_filter": {"n_lines": 10, "n_excluded": 1, "n_not_only": 0, "exclude": ["s__x"], "excluded_by": [1]}}
    cli._say_kept(stats, False)                               # coverage the only threshold: the kept line is still printed
    assert capsys.readouterr().err.splitlines() == ["taxon filter: excluded 1, not in --only-taxon 0, of 10 lines", "  s__x: 1",
                                                    "query cover: 3 of 10 lines under 80.5 percent (from qlen)", "hit filter: kept 6 of 10 lines"]
    cli._say_kept({"n_lines": 10, "n_kept": 9, "taxon_filter": stats["taxon_filter"]}, False)
    assert "hit filter" not in capsys.readouterr().err        # (as before: a taxon filter alone prints no kept line)
