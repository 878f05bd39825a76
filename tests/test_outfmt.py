"""Tables in any outfmt-6 column order (`--blast-outfmt`) without a GPU: the format-string parser against its
Python restatement (tests/outfmt_reference.py), the C ABI's pinned sizes, and the host parser (device=-1) on relaid tables — the
columns of the independent reading (tests/ingest_reference.py) of the table rewritten to the reference's columns, and the
library's own columns on that copy through today's path.  The document-level equivalence needs the engine and is in
tests/test_gpu_outfmt.py."""
import ctypes as C
import re

import numpy as np
import pytest

from blutils_amd import _native as N
from blutils_amd import cli, pipeline
from tests import ingest_edges as E
from tests import ingest_reference as ref
from tests import outfmt_cases as K
from tests import outfmt_reference as R
from tests.test_ingest_edges import assert_columns_equal

def _write(tmp_path, blob, db, name="b.tsv"):
    bt, tj = tmp_path / name, tmp_path / "t.json"
    bt.write_bytes(blob)
    tj.write_text(db)
    return str(bt), str(tj)


# ---- the format string ----------------------------------------------------------------------------------------------------------------
ACCEPTED_SPECS = [
    "6 std staxids", "std staxids", "std staxid", R.REFERENCE_SPEC, " ".join(R.REFERENCE), "  6   std \t staxid  ", R.REVERSED, R.MINIMAL, R.WIDE,
    R.TAXID_LAST, R.EMPTY_IN_FRONT, "qseqid saccver staxid pident length bitscore", "6 qseqid sacc staxid pident length bitscore qcovs",
    "sseqid saccver qacc qseqid staxids staxid pident length bitscore", "saccver sseqid qseqid qacc staxid staxids length pident bitscore evalue",
    "sacc saccver qaccver qacc staxid pident length bitscore", "saccver sacc qacc qaccver staxid pident length bitscore",
    "sseqid sacc qaccver qseqid staxid pident length bitscore", "sacc sseqid qseqid qaccver staxid pident length bitscore",
    "qseqid sseqid staxids pident length bitscore 6 7 std_", "STD qseqid sseqid staxid pident length bitscore",
    "std staxid " + " ".join(f"c{k}" for k in range(51)),                                       # 64 columns
]
REFUSED_SPECS = [
    ("7 std staxid", "7"), ("0 std staxid", "0"), ("66 std staxid", "66"), ("06 std staxid", "06"),
    ("std staxid " + " ".join(f"c{k}" for k in range(51)) + " last", "last"),                  # 65 columns
    ("std std staxid", "qseqid"), ("std staxid qseqid", "qseqid"), ("std staxid staxid", "staxid"), ("std staxid qcovs qlen qcovs", "qcovs"),
    ("sseqid staxid pident length bitscore", "qseqid"), ("qseqid staxid pident length bitscore", "saccver"),
    ("std", "staxid"), ("qseqid sseqid staxid length bitscore", "pident"), ("qseqid sseqid staxid pident bitscore", "length"),
    ("qseqid sseqid staxid pident length evalue", "bitscore"), ("", "qseqid"), ("6", "qseqid"),
    ("std sta-xid staxid", "sta-xid"), ("std staxid,qlen", "staxid,qlen"), ("std staxid q%s", "q%s"),
]


@pytest.mark.parametrize("spec", ACCEPTED_SPECS)
def test_accepted_format_strings_give_the_restated_layout(spec):
    exp = R.parse_spec(spec)
    got = pipeline.table_layout(spec)
    assert got.as_dict() == exp
    assert got.struct_size == C.sizeof(pipeline.TableLayoutC) == 40
    assert got.is_reference() == R.is_reference(exp)


@pytest.mark.parametrize("spec,token", REFUSED_SPECS)
def test_refused_format_strings_name_the_token(spec, token):
    with pytest.raises(R.SpecError) as r:
        R.parse_spec(spec)
    assert r.value.token == token
    with pytest.raises(N.BluError, match=re.escape(f"`{token}`")) as e:
        pipeline.table_layout(spec)
    assert e.value.code == N.BLU_ERR_INVALID_ARG


def test_priorities_do_not_depend_on_position():
    for a, b in (("saccver", "sseqid"), ("saccver", "sacc"), ("sacc", "sseqid")):
        for first, second in ((a, b), (b, a)):
            lay = pipeline.table_layout(f"qseqid {first} {second} staxid pident length bitscore").as_dict()
            assert lay["accession"] == (1 if first == a else 2), (first, second)
    for a, b in (("qseqid", "qacc"), ("qseqid", "qaccver"), ("qacc", "qaccver")):
        for first, second in ((a, b), (b, a)):
            lay = pipeline.table_layout(f"{first} {second} sseqid staxid pident length bitscore").as_dict()
            assert lay["query"] == (0 if first == a else 1), (first, second)
    for first, second in (("staxid", "staxids"), ("staxids", "staxid")):
        lay = pipeline.table_layout(f"qseqid sseqid {first} {second} pident length bitscore").as_dict()
        assert lay["taxid"] == (2 if first == "staxid" else 3) and lay["taxid_is_list"] is False
    assert pipeline.table_layout("std staxids").as_dict()["taxid_is_list"] is True


def test_the_reference_string_is_no_layout():
    assert pipeline._layout(None) is None
    assert pipeline._layout(pipeline.REFERENCE_OUTFMT) is None and pipeline.REFERENCE_OUTFMT == R.REFERENCE_SPEC
    assert pipeline._layout("qacc sacc staxid pident length a b c d e f evalue bitscore") is None       # (the same columns by other names)
    assert pipeline._layout("6 std staxid") is not None
    assert pipeline._layout("qseqid saccver staxids pident length mismatch gapopen qstart qend sstart send evalue bitscore") is not None


def test_struct_sizes_exports_and_abi():
    L = pipeline._bind()
    assert C.sizeof(pipeline.ConsensusRequest) == 136 and C.sizeof(pipeline.ConsensusExtras) == 24 and L.blu_abi_version() == 5
    for name in ("blu_table_layout_parse", "blu_build_consensus_laid_out", "blu_ingest_columns_laid_out"):
        assert name in N.PIPELINE_EXPORTS and hasattr(L, name)
    for size in (0, 36, 44):
        lay = pipeline.TableLayoutC(struct_size=size)
        assert L.blu_table_layout_parse(b"std staxid", C.byref(lay)) == N.BLU_ERR_INVALID_ARG
        assert "struct_size" in N.last_error()
    assert L.blu_table_layout_parse(None, C.byref(pipeline.TableLayoutC(struct_size=40))) == N.BLU_ERR_INVALID_ARG
    assert L.blu_table_layout_parse(b"std staxid", None) == N.BLU_ERR_INVALID_ARG


def test_a_layout_struct_the_library_does_not_take(tmp_path):
    bt, tj = _write(tmp_path, E._table([E.line(b"q", b"A.1")]), E.db_json())
    good = pipeline.table_layout("std staxid")
    cols, st = pipeline.IngestColumns(), pipeline.HitSelectionStats()
    call = lambda lay: pipeline._bind().blu_ingest_columns_laid_out(bt.encode(), tj.encode(), 0, -1, C.byref(lay), None, C.byref(cols), C.byref(st))
    for field, value, word in (("struct_size", 36, "struct_size"), ("n_columns", 0, "columns"), ("n_columns", 65, "columns"),
                               ("query", 13, "query"), ("bit_score", 0, "both column"), ("e_value", 13, "e_value"), ("taxid_is_list", 2, "taxid_is_list")):
        lay = pipeline.TableLayoutC.from_buffer_copy(good)
        setattr(lay, field, value)
        assert call(lay) == N.BLU_ERR_INVALID_ARG and word in N.last_error(), (field, N.last_error())
    rq, oc = pipeline.ConsensusRequest(struct_size=136), pipeline.ConsensusOutcome()
    p = pipeline.PipelineParams()
    rq.blast_output_file, rq.taxonomies_file, rq.params = bt.encode(), tj.encode(), C.pointer(p)
    bad = pipeline.TableLayoutC.from_buffer_copy(good)
    bad.struct_size = 44
    assert pipeline._bind().blu_build_consensus_laid_out(C.byref(rq), None, C.byref(bad), C.byref(oc)) == N.BLU_ERR_INVALID_ARG
    assert "struct_size" in N.last_error()


# ---- the host parser on relaid tables -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.LAYOUTS))
def test_relaid_golden_table_gives_the_columns_of_the_reference_copy(tmp_path, name):
    spec, fillers = R.LAYOUTS[name]
    blob13, db = K.golden_table()
    relaid = R.relayout(blob13, spec, fillers)
    copy = R.to_reference(relaid, spec)
    assert relaid != blob13 and len(relaid.split(b"\n")[0].split(b"\t")) == R.parse_spec(spec)["n_columns"]
    bt, tj = _write(tmp_path, relaid, db)
    ct, _ = _write(tmp_path, copy, db, "copy.tsv")
    exp = ref.read_table(ct, tj)
    assert_columns_equal(exp, ref.read_table(_write(tmp_path, blob13, db, "b13.tsv")[0], tj))        # (the relayout loses nothing the parse reads)
    # once with no selection: the independent reading, and its checksum over the columns that came back
    got = pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec)
    assert_columns_equal(got, exp)
    assert ref.checksum(got) == ref.checksum(exp) == pipeline.ingest_only(ct, tj, False)[1]
    # once with the filters: the library's own columns and counts on the copy, through today's path
    got = pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec, **K.SELECT_HOST)
    today = pipeline.ingest_columns(ct, tj, device=-1, **K.SELECT_HOST)
    assert_columns_equal(got, today)
    assert (got["n_lines"], got["n_kept"], got["taxon_filter"]) == (today["n_lines"], today["n_kept"], today["taxon_filter"])
    assert 0 < got["n_kept"] < got["n_lines"] and got["taxon_filter"]["n_excluded"] > 0


@pytest.mark.parametrize("name", ["eol_crlf", "eol_open_last_line", "eol_open_last_line_ending_in_cr", "a_14th_column", "a_trailing_tab"])
@pytest.mark.parametrize("layout", ["reversed", "wide", "taxid_last"])
def test_line_ends_and_further_fields(tmp_path, layout, name):
    """CR LF, the open last line and fields beyond the layout's, relaid: a string role or a `;` list is then the last field."""
    spec, fillers = R.LAYOUTS[layout]
    case = E.placement_cases()[name]
    blob = case.blob if "column" not in name and "tab" not in name else None
    if blob is None:                                     # (the further field is added behind the relaid line)
        base = R.relayout(E.placement_cases()["eol_lf"].blob, spec, fillers).split(b"\n")[:-1]
        relaid = b"".join(ln + (b"\textra" if name == "a_14th_column" and i % 3 else b"\t" if i % 2 else b"") + b"\n" for i, ln in enumerate(base))
    else:
        relaid = R.relayout(blob, spec, fillers)
    bt, tj = _write(tmp_path, relaid, E.db_json())
    t, ck = E.expected(R.to_reference(relaid, spec), E.db_json())
    got = pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec)
    assert_columns_equal(got, t)
    assert ref.checksum(got) == ck


def test_quotes_and_blank_lines_apply_to_whichever_field_holds_the_role(tmp_path):
    spec = R.REVERSED
    for name in ("blank_line_in_the_middle", "crlf_only_line_at_the_end", "a_quoted_query", "a_quote_inside_an_accession"):
        relaid = R.relayout(E.declined_cases()[name].blob, spec)
        bt, tj = _write(tmp_path, relaid, E.db_json())
        t, _ = E.expected(R.to_reference(relaid, spec), E.db_json())
        assert_columns_equal(pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec), t)


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def test_a_short_line_names_the_line_and_the_layouts_count(tmp_path):
    for spec in (R.STD_STAXIDS, R.WIDE, R.MINIMAL):
        n = R.parse_spec(spec)["n_columns"]
        rows = [K.line(spec, b"q%d" % i, b"A.1") for i in range(5)]
        rows[3] = b"\t".join(rows[3].split(b"\t")[:n - 1])
        bt, tj = _write(tmp_path, E._table(rows), E.db_json())
        with pytest.raises(N.BluError, match=r"line 4\b.* has %d columns, outfmt-6 with %d expected" % (n - 1, n)) as e:
            pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec)
        assert e.value.code == 8                                            # BLU_ERR_PARSE
    # a table of the reference's thirteen columns under a wider layout, and the other way round
    bt, tj = _write(tmp_path, E._table([E.line(b"q", b"A.1")]), E.db_json())
    with pytest.raises(N.BluError, match=r"line 1\b.* has 13 columns, outfmt-6 with 30 expected"):
        pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=R.WIDE)
    bt, tj = _write(tmp_path, E._table([K.line(R.MINIMAL, b"q", b"A.1")]), E.db_json())
    with pytest.raises(N.BluError, match=r"line 1\b.* has 7 columns, outfmt-6 with 13 expected"):
        pipeline.ingest_columns(bt, tj, device=-1)


@pytest.mark.parametrize("field", [b"N/A", b";5", b"", b";", b"5x;6", b" 5;6", b"1.0;2"])
def test_a_staxids_field_without_an_int64_in_front(tmp_path, field):
    rows = [K.line(R.STD_STAXIDS, b"q", b"A.1", tail=b";7"), K.line(R.STD_STAXIDS, b"q", b"B.1").rsplit(b"\t", 1)[0] + b"\t" + field]
    bt, tj = _write(tmp_path, E._table(rows), E.db_json())
    with pytest.raises(N.BluError, match=r"line 2\b.*numeric") as e:
        pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=R.STD_STAXIDS)
    assert e.value.code == 8


def test_a_semicolon_is_read_only_in_a_staxids_column(tmp_path):
    bt, tj = _write(tmp_path, E._table([K.line("std staxid", b"q", b"A.1", tax=b"105;7")]), E.db_json())
    with pytest.raises(N.BluError, match="numeric"):
        pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt="std staxid")
    assert pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt="std staxids")["tax_desc_row"].tolist() == [5]


def test_the_e_value_column_is_needed_only_by_its_threshold(tmp_path):
    spec = "qseqid sseqid staxid pident length bitscore"
    assert R.parse_spec(spec)["e_value"] is None and pipeline.table_layout(spec).e_value == pipeline.TABLE_LAYOUT_NO_COLUMN
    bt, tj = _write(tmp_path, E._table([K.line(spec, b"q%d" % i, b"A.1", pid=90 + i) for i in range(4)]), E.db_json())
    assert pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec)["pident"].tolist() == [90.0, 91.0, 92.0, 93.0]
    assert pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec, hit_filter={"min_perc_identity": 92.0})["n_kept"] == 2
    with pytest.raises(N.BluError, match="`evalue`") as e:
        pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec, hit_filter={"max_e_value": 1.0})
    assert e.value.code == N.BLU_ERR_INVALID_ARG


# ---- the command line --------------------------------------------------------------------------------------------------------------------
def test_cli_flag(tmp_path, capsys):
    ap = cli.build_parser()
    common = ["-t", "t.json", "--taxon", "bacteria", "--strategy", "relaxed"]
    a = ap.parse_args(["blastn", "build-consensus", "b.tsv"] + common + ["--blast-outfmt", "6 std staxids"])
    assert a.blast_outfmt == "6 std staxids"
    assert ap.parse_args(["blastn", "build-consensus", "b.tsv"] + common).blast_outfmt is None
    with pytest.raises(SystemExit):                         # run-with-consensus writes the reference's format itself
        ap.parse_args(["blastn", "run-with-consensus", "q.fa", "-d", "db", "--blast-out-file", "b.tsv"] + common + ["--blast-outfmt", "6 std staxids"])
    capsys.readouterr()
    # the flag reaches the library: its refusals are the library's messages, before any file is opened
    with pytest.raises(SystemExit, match="--blast-outfmt: .*`qseqid` is named twice"):
        cli.main(["blastn", "build-consensus", str(tmp_path / "absent.tsv")] + common + ["--blast-outfmt", "6 std std"])
    with pytest.raises(SystemExit, match="--blast-outfmt: .*`evalue`"):
        cli.main(["blastn", "build-consensus", str(tmp_path / "absent.tsv")] + common
                 + ["--blast-outfmt", "qseqid sseqid staxid pident length bitscore", "--max-e-value", "1e-5"])


# ---- the failure the feature removes ---------------------------------------------------------------------------------------------------
def test_a_std_staxids_table_read_as_the_reference_columns_is_silently_wrong(tmp_path):
    """Thirteen columns, every number parses in the wrong place: pident is read as the taxid, length as the identity."""
    rows = [K.line(R.STD_STAXIDS, b"q%d" % (i // 2), b"NR_%06d.1" % i, tax=100 + i, pid="%d" % (100 + i % 3), aln=300 + i, bs=500 + i) for i in range(12)]
    blob = E._table(rows)
    bt, tj = _write(tmp_path, blob, E.db_json())
    without = pipeline.ingest_columns(bt, tj, device=-1)                    # no error: nothing tells the user
    with_flag = pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=R.STD_STAXIDS)
    assert_columns_equal(with_flag, E.expected(R.to_reference(blob, R.STD_STAXIDS), E.db_json())[0])
    assert not np.array_equal(without["tax_desc_row"], with_flag["tax_desc_row"])
    assert not np.array_equal(without["pident"], with_flag["pident"]) and not np.array_equal(without["bitscore"], with_flag["bitscore"])


# ---- the byte-level cases of tests/test_gpu_outfmt.py, without a GPU: each lies where it claims, and the host parser reads it ---------
@pytest.mark.parametrize("name", sorted(K.ACCEPTED))
def test_byte_level_case_lies_where_it_claims(tmp_path, name):
    spec, case = K.ACCEPTED[name][0], K.accepted_case(name)
    c, blob = case.claims, case.blob
    assert K.plain_form(blob, spec)                        # the GPU parser has no reason to decline it
    forms = E.block_forms(blob)
    if "span" in c:
        assert forms[2] == (c["span"], c["form"]) and c["form"] == ("general" if c["span"] > E.STAGE_BYTES else "staged")
        assert all(f == c["others"] for j, (_, f) in enumerate(forms) if j != 2) and len(forms) >= 3
        assert E.line_starts(blob)[512] % 16 == c["start_mod16"]
        lay = R.parse_spec(spec)
        if "crlf" in name:
            assert blob.count(b"\r\n") == blob.count(b"\n")
            if not name.startswith("wide/"):              # a string role, or the `;` list, ends at the CR
                assert max(lay["query"], lay["taxid"]) == lay["n_columns"] - 1
        if "open" in name:
            assert not blob.endswith(b"\n") and len(forms) == 3
    if "forms" in c:
        assert [f for _, f in forms] == c["forms"]
    if "rows" in c:
        assert len(E.line_starts(blob)) - 1 == c["rows"]
    if "line_len" in c:
        assert len(blob) == c["rows"] * c["line_len"] and c["line_len"] == 2 * 7 - 1     # seven fields of at most one byte
    t, ck = K.expected_of(name)
    bt, tj = _write(tmp_path, blob, E.db_json())
    got = pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec)
    assert_columns_equal(got, t)
    assert ref.checksum(got) == ck


@pytest.mark.parametrize("layout", ["std_staxids", "wide"])
def test_modes_table_cuts_under_every_mode(tmp_path, layout):
    """The table of the GPU mode tests: both forms, e-values the device leaves to the host, every count above zero — and the host
    parser gives, under each mode, its own result on the reference copy."""
    spec = R.LAYOUTS[layout][0]
    blob = K.modes_table(spec, b";1;2")
    assert K.plain_form(blob, spec) and {f for _, f in E.block_forms(blob)} == {"staged", "general"}
    e_at = R.parse_spec(spec)["e_value"]
    assert sum(ln.split(b"\t")[e_at] in (b"1e-30", b"1.0e-30") for ln in blob.split(b"\n")[:-1]) > 100
    bt, tj = _write(tmp_path, blob, E.db_json())
    ct, _ = _write(tmp_path, R.to_reference(blob, spec), E.db_json(), "copy.tsv")
    for mode, kw in K.MODES.items():
        got, today = pipeline.ingest_columns(bt, tj, device=-1, blast_outfmt=spec, **kw), pipeline.ingest_columns(ct, tj, device=-1, **kw)
        assert_columns_equal(got, today)
        if kw:
            assert (got["n_lines"], got["n_kept"]) == (today["n_lines"], today["n_kept"]) and 0 < got["n_kept"] < 600, mode
        if "taxon_filter" in kw:
            assert got["taxon_filter"] == today["taxon_filter"] and all(n > 0 for n in got["taxon_filter"]["excluded_by"]), mode
