"""Taxon filters in the GPU parser (csrc/ingest_gpu.hip: parse_rows_taxa, the per-wave counts, the compaction it
shares with the hit filters) and end to end.  The rule: a run under the filter gives what the run without it gives on the copy
of the table from which tests/taxon_filter_reference.py deleted the dropped lines — columns against tests/ingest_reference.py,
the four counts against that restatement, documents, reports, sample and support tables byte for byte."""
import json
import os
import re

import numpy as np
import pytest

from blutils_amd import blast, cli, pipeline
from tests import hit_filter_reference as hf
from tests import ingest_reference as ref
from tests import taxon_filter_reference as tf

pytestmark = pytest.mark.gpu


@pytest.fixture()
def force_gpu():
    old = os.environ.get("BLU_INGEST")
    os.environ["BLU_INGEST"] = "gpu"
    yield
    if old is None:
        os.environ.pop("BLU_INGEST", None)
    else:
        os.environ["BLU_INGEST"] = old


def _table(tmp_path, rows, name="b.tsv", eol="\n", final=True):
    bt = tmp_path / name
    bt.write_bytes((eol.join(rows) + (eol if final else "")).encode())
    return str(bt)


def _check(src, tj, tmp_path, exclude=(), only=(), hit=None, path="gpu", use_taxid=False):
    """GPU ingest of src under the filter == independent reading of filter_text's copy, and the counts; the GPU parser did it"""
    dst = str(tmp_path / "taxon_copy.tsv")
    keep = (lambda f: hf.keep(f, hit)) if hit else None
    c = tf.filter_text(src, dst, tj, exclude, only, use_taxid, keep)
    got = pipeline.ingest_columns(src, tj, use_taxid=use_taxid, device=0, hit_filter=hit, taxon_filter={"exclude": exclude, "only": only})
    assert pipeline.last_ingest_path() == path
    hf.assert_columns_equal(got, ref.read_table(dst, tj))
    t = got["taxon_filter"]
    assert (t["n_lines"], t["n_excluded"], t["n_not_only"]) == (c["n_lines"], c["n_excluded"], c["n_not_only"])
    assert t["excluded_by"] == c["excluded_by"]
    assert (got["n_lines"], got["n_kept"]) == (c["n_lines"], c["n_kept"])
    return got, c


LISTS = {"exclude": (tf.EXCLUDE, ()), "only": ((), tf.ONLY), "both": (tf.EXCLUDE, tf.ONLY)}
THRESHOLDS = {"pid": {"min_perc_identity": 90.0}, "aln": {"min_align_length": 1000}, "evalue": {"max_e_value": 1e-30},
              "bits": {"min_bit_score": 60000.0}}


@pytest.mark.parametrize("layout", ["grouped", "scrambled"])
@pytest.mark.parametrize("which", list(LISTS) + [f"both+{k}" for k in THRESHOLDS])
def test_gpu_filtered_ingest_is_the_ingest_of_the_filtered_copy(tmp_path, force_gpu, layout, which):
    """3000 queries x 8 rows: 94 parse blocks of 256 lines, whose waves' counts meet in the same counters."""
    rng = np.random.default_rng(71)
    rows = tf.make_rows(3000, 8, rng, exact=True)
    if layout == "scrambled":
        rows = hf.scramble(rows, rng)
    src, tj = _table(tmp_path, rows), tf.write_db(tmp_path / "t.json")
    lists, _, thr = which.partition("+")
    exclude, only = LISTS[lists]
    got, c = _check(src, tj, tmp_path, exclude, only, hit=THRESHOLDS.get(thr))
    assert c["n_lines"] == len(rows) == 24000 and 0 < c["n_kept"] < c["n_lines"]
    assert (c["n_excluded"] > 0) == bool(exclude) and (c["n_not_only"] > 0) == bool(only) and all(n > 0 for n in c["excluded_by"])
    assert (int((got["tax_desc_row"] == ref.UNMATCHED).sum()) > 0) == (not only)
    if thr:                                                               # the threshold cuts too, and the taxon counts ignore it
        alone = pipeline.ingest_columns(src, tj, device=0, taxon_filter={"exclude": exclude, "only": only})
        assert c["n_kept"] < alone["n_kept"] and alone["taxon_filter"] == got["taxon_filter"]


def test_gpu_numeric_lineages_and_spellings(tmp_path, force_gpu):
    rng = np.random.default_rng(72)
    src, tj = _table(tmp_path, hf.scramble(tf.make_rows(400, 8, rng), rng)), tf.write_db(tmp_path / "t.json")
    _, c = _check(src, tj, tmp_path, tf.EXCLUDE_NUMERIC, tf.ONLY_NUMERIC, use_taxid=True)
    assert 0 < c["n_kept"] < c["n_lines"]
    _, c = _check(src, tj, tmp_path, ["species__uncultured-organism", "O__*"], ["Domain__Bacteria"])
    assert 0 < c["n_kept"] < c["n_lines"] and all(c["excluded_by"])


# ---- where the verdict falls: by line index, over hf.write_db's flat database (taxid 100 + t is `d__b;g__g<t // 7>;s__s<t>`) ----
def _lines(n, taxid_of, long_names=False):
    """n lines, three per query, line i naming taxid_of(i)"""
    rows = []
    for i in range(n):
        q = f"q{i // 3:05d}"
        if long_names:
            q = f"query_with_a_very_long_identifier_for_the_general_form_of_the_parse_kernel_{i // 3:07d}/1_" + "x" * 60
        t = taxid_of(i)
        rows.append(f"{q}\tNR_{t:06d}.1\t{t}\t{90 + i % 10}.{i % 7}00\t{300 + i % 500}\t1\t0\t1\t400\t1\t400\t1e-{20 + i % 60}\t{200 + i % 900}")
    return rows


KEPT = lambda i: 100 + 500 + i % 300          # taxids no list below names
N_SHAPE = 1800
SHAPES = {
    # name: (excluded(i) -> taxid or None, exclude list)
    "a_whole_parse_block_excluded": (lambda i: 100 if 256 <= i < 512 or i % 7 == 0 else None, ["s__s0"]),
    "one_line_kept": (lambda i: 100 + i % 3 if i != 777 else None, ["s__s0", "s__s1", "s__s2"]),
    "alternating": (lambda i: 100 + 14 + i % 5 if i % 2 else None, ["g__g2"]),
    "first_and_last_excluded": (lambda i: 107 if i in (0, N_SHAPE - 1) else None, ["g__g1"]),
    # lines 64 .. 127: one wave whose lanes carry 64 different codes; 128 .. 191: one whose lanes all carry the same; 192 .. 255: a
    # wave with two codes and kept lanes between them; then a few elsewhere
    "codes_within_a_wave": (lambda i: 100 + (i - 64) if 64 <= i < 128 else 105 if 128 <= i < 192 else
                            (100 + 60 + i % 2 if i % 3 else None) if 192 <= i < 256 else (100 + i % 64 if i % 11 == 0 else None),
                            [f"s__s{k}" for k in range(64)]),
}


@pytest.mark.parametrize("eol,final", [("\n", True), ("\n", False), ("\r\n", True)])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_verdict_placement(tmp_path, force_gpu, shape, eol, final):
    excluded, exclude = SHAPES[shape]
    rows = _lines(N_SHAPE, lambda i: excluded(i) or KEPT(i))
    src, tj = _table(tmp_path, rows, eol=eol, final=final), hf.write_db(tmp_path / "t.json")
    _, c = _check(src, tj, tmp_path, exclude)
    assert c["n_excluded"] == sum(1 for i in range(N_SHAPE) if excluded(i)) and 0 < c["n_kept"] == N_SHAPE - c["n_excluded"]
    if shape == "codes_within_a_wave":
        assert all(n > 0 for n in c["excluded_by"]) and c["excluded_by"][5] >= 65
    # the same lines under an only list that the kept ones hold: the dropped lines are `not only` instead
    only = sorted({f"s__s{KEPT(i) - 100}" for i in range(N_SHAPE) if not excluded(i)})
    _, c2 = _check(src, tj, tmp_path, (), only)
    assert (c2["n_not_only"], c2["n_kept"]) == (c["n_excluded"], c["n_kept"])


@pytest.mark.parametrize("shape", ["alternating", "codes_within_a_wave"])
def test_verdict_placement_in_the_general_form(tmp_path, force_gpu, shape):
    """Long query names: no 256-line block fits the LDS stage, every line goes through the one-state-machine form."""
    excluded, exclude = SHAPES[shape]
    rows = _lines(N_SHAPE, lambda i: excluded(i) or KEPT(i), long_names=True)
    assert sum(map(len, rows)) / len(rows) >= 128
    src, tj = _table(tmp_path, rows, final=False), hf.write_db(tmp_path / "t.json")
    _, c = _check(src, tj, tmp_path, exclude, ["d__b"])
    assert 0 < c["n_kept"] < c["n_lines"] and c["n_not_only"] == 0
    _, c = _check(src, tj, tmp_path, exclude, hit={"min_align_length": 500, "max_e_value": 1e-30})
    assert 0 < c["n_kept"] < c["n_lines"] - c["n_excluded"]


def test_code_values_at_both_ends(tmp_path, force_gpu):
    """65 534 exclude elements over a database of 65 600 taxids: element 0, element 65 533 (code 0xFFFE), the 0xFFFF code from
    the table and from the constant of unmatched lines, and lines whose row is the last of the taxonomy."""
    n_tax = 65600
    tj = hf.write_db(tmp_path / "big.json", n=n_tax)
    exclude = [f"s__s{k}" for k in range(65534)]
    only = [f"s__s{n_tax - 1}", "s__s65534"]
    pick = [100, 100 + 65533, 100 + n_tax - 1, 100 + 65540, 99999999, 100 + 65534, 100 + 65533, 100 + 7]
    rows = _lines(1500, lambda i: pick[(i * 7 + i // 64) % len(pick)])
    src = _table(tmp_path, rows)
    got, c = _check(src, tj, tmp_path, exclude, only)
    by = c["excluded_by"]
    assert by[0] > 0 and by[65533] > 0 and by[7] > 0 and sum(by) == c["n_excluded"] and sum(1 for n in by if n) == 3
    assert c["n_not_only"] > 0 and set(got["tax_desc_row"].tolist()) == {n_tax - 1, 65534}
    # without the only list the unmatched lines and row 65 540 stay
    got, c = _check(src, tj, tmp_path, exclude)
    assert set(got["tax_desc_row"].tolist()) == {n_tax - 1, 65534, 65540, ref.UNMATCHED}


def test_tables_of_unmatched_lines_only(tmp_path, force_gpu):
    tj = tf.write_db(tmp_path / "t.json")
    rows = _lines(1500, lambda i: 5000 + i % 40)
    src = _table(tmp_path, rows)
    got, c = _check(src, tj, tmp_path, tf.EXCLUDE)                       # every line kept: no compaction
    assert c["n_kept"] == c["n_lines"] == 1500 and c["n_excluded"] == 0
    hf.assert_columns_equal(got, pipeline.ingest_columns(src, tj, device=0))
    got, c = _check(src, tj, tmp_path, (), tf.ONLY, path="cpu")          # nothing kept: the host parser returns the empty table
    assert c["n_kept"] == 0 and c["n_not_only"] == 1500 and got["seg_off"].tolist() == [0]


def test_an_excluded_line_never_asks_the_host_for_its_e_value(tmp_path, force_gpu):
    """Against 1e-30 a field spelled `1e-30` is left to the host's number reader — unless the taxon verdict dropped the line
    first.  Here every such line is excluded: the call's trace shows no e-value round trip, and the counts match."""
    tj = hf.write_db(tmp_path / "t.json")
    rows = []
    for i, r in enumerate(_lines(1600, lambda i: 100 + i % 4 if i % 3 == 0 else KEPT(i))):
        c = r.split("\t")
        c[11] = ("1e-30", "1.0e-30", "10e-31")[i // 3 % 3] if i % 3 == 0 else ("1e-40", "3e-12")[i % 2]
        rows.append("\t".join(c))
    src = _table(tmp_path, rows)
    exclude, hit = ["s__s0", "s__s1", "s__s2", "s__s3"], {"max_e_value": 1e-30}
    _, c = _check(src, tj, tmp_path, exclude, hit=hit)
    assert c["n_excluded"] == 534 and 0 < c["n_kept"] < c["n_lines"] - c["n_excluded"]
    # (without the taxon filter those lines do reach the host, and are kept)
    plain = pipeline.ingest_columns(src, tj, device=0, hit_filter=hit)
    assert pipeline.last_ingest_path() == "gpu" and plain["n_kept"] == c["n_kept"] + c["n_excluded"]


def test_the_trace_shows_no_e_value_round_trip_for_excluded_lines(tmp_path, force_gpu, capfd):
    tj = hf.write_db(tmp_path / "t.json")
    rows = []
    for i, r in enumerate(_lines(600, lambda i: 100 if i % 3 == 0 else KEPT(i))):
        c = r.split("\t")
        c[11] = "1e-30" if i % 3 == 0 else "1e-40"
        rows.append("\t".join(c))
    src = _table(tmp_path, rows)
    old = os.environ.get("BLU_INGEST_TRACE")
    os.environ["BLU_INGEST_TRACE"] = "1"
    try:
        capfd.readouterr()
        with_taxa = pipeline.ingest_columns(src, tj, device=0, hit_filter={"max_e_value": 1e-30}, taxon_filter={"exclude": ["s__s0"]})
        err_taxa = capfd.readouterr().err
        plain = pipeline.ingest_columns(src, tj, device=0, hit_filter={"max_e_value": 1e-30})
        err_plain = capfd.readouterr().err
    finally:
        if old is None:
            os.environ.pop("BLU_INGEST_TRACE", None)
        else:
            os.environ["BLU_INGEST_TRACE"] = old
    assert with_taxa["n_kept"] == 400 and plain["n_kept"] == 600
    assert "e-values decided on the host" in err_plain and "e-values decided on the host" not in err_taxa


def test_either_parser(tmp_path, force_gpu):
    rng = np.random.default_rng(73)
    src, tj = _table(tmp_path, hf.scramble(tf.make_rows(1500, 8, rng), rng)), tf.write_db(tmp_path / "t.json")
    for hit in (None, hf.FILTERS["all"]):
        flt = {"exclude": tf.EXCLUDE, "only": tf.ONLY}
        gpu = pipeline.ingest_columns(src, tj, device=0, hit_filter=hit, taxon_filter=flt)
        assert pipeline.last_ingest_path() == "gpu"
        host = pipeline.ingest_columns(src, tj, device=-1, hit_filter=hit, taxon_filter=flt)
        assert pipeline.last_ingest_path() == "cpu"
        hf.assert_columns_equal(gpu, host)
        assert gpu["taxon_filter"] == host["taxon_filter"] and (gpu["n_lines"], gpu["n_kept"]) == (host["n_lines"], host["n_kept"])
    # no filter and an empty one: today's call, today's kernel
    today = pipeline.ingest_columns(src, tj, device=0)
    assert pipeline.last_ingest_path() == "gpu" and "taxon_filter" not in today
    hf.assert_columns_equal(pipeline.ingest_columns(src, tj, device=0, taxon_filter={"exclude": [], "only": []}), today)
    # the binary cache on the GPU path
    cache = str(tmp_path / "t.cache")
    pipeline.build_db_cache(tj, cache)
    cached = pipeline.ingest_columns(src, cache, device=0, taxon_filter={"exclude": tf.EXCLUDE, "only": tf.ONLY})
    assert pipeline.last_ingest_path() == "gpu"
    hf.assert_columns_equal(cached, pipeline.ingest_columns(src, tj, device=0, taxon_filter={"exclude": tf.EXCLUDE, "only": tf.ONLY}))


GOOD_TAXIDS = [t for t in range(tf.FIRST_TAXID, tf.FIRST_TAXID + tf.N_TAXIDS) if t not in (tf.BAD_TAXID, tf.EMPTY_TAXID)]


def _end_to_end_rows(rng, n_q=1500):
    """sample-named queries; queries 0 .. 39 name an excluded taxon on every line"""
    rows = hf.scramble(tf.make_rows(n_q, 8, rng, sample_names=True), rng)
    return ["\t".join(c[:2] + ["1002"] + c[3:]) if int(c[0].split(".")[1]) < 40 else "\t".join(c) for c in (r.split("\t") for r in rows)]


@pytest.mark.parametrize("host_columns", [False, True])
@pytest.mark.parametrize("strategy,fmt", [("relaxed", "json"), ("cautious", "jsonl")])
def test_documents_reports_and_tables_are_those_of_the_filtered_copy(tmp_path, force_gpu, strategy, fmt, host_columns):
    rng = np.random.default_rng(74)
    rows = _end_to_end_rows(rng)
    src, tj = _table(tmp_path, rows), tf.write_db(tmp_path / "t.json")
    flt = {"exclude": tf.EXCLUDE, "only": tf.ONLY}
    copy = str(tmp_path / "copy.tsv")
    c = tf.filter_text(src, copy, tj, tf.EXCLUDE, tf.ONLY)
    assert 0 < c["n_kept"] < c["n_lines"]
    headers = sorted({r.split("\t")[0] for r in rows}) + ["s1.999999"]
    cfg = blast.BlastBuilder.default("/db/ref16s", "bacteria")             # (one run id for both documents)
    old = os.environ.get("BLU_PIPELINE_HOST_COLUMNS")
    if host_columns:
        os.environ["BLU_PIPELINE_HOST_COLUMNS"] = "1"
    try:
        out = {}
        for tag, table, extra in (("filtered", src, {"taxon_filter": flt}), ("copy", copy, {})):
            paths = {k: str(tmp_path / f"{tag}.{k}") for k in ("doc", "report", "table", "support")}
            _, stats = pipeline.build_consensus_identities_with_tables(
                table, tj, "bacteria", strategy, headers=headers, out_format=fmt, lenient=True, parse=False, config=cfg,
                out_path=paths["doc"], report_path=paths["report"], sample_table_path=paths["table"],
                support_table_path=paths["support"], **extra)
            assert pipeline.last_ingest_path() == "gpu"
            out[tag] = ({k: open(p, "rb").read() for k, p in paths.items()}, stats)
            text, _ = pipeline.build_consensus_identities(table, tj, "bacteria", strategy, headers=headers, out_format=fmt,
                                                          lenient=True, parse=False, config=cfg, **extra)
            assert text.encode() == out[tag][0]["doc"]                    # text and file entry: the same document
    finally:
        if old is None:
            os.environ.pop("BLU_PIPELINE_HOST_COLUMNS", None)
        else:
            os.environ["BLU_PIPELINE_HOST_COLUMNS"] = old
    assert out["filtered"][0] == out["copy"][0] and all(len(v) > 1000 for v in out["copy"][0].values())
    fs, cs = out["filtered"][1], out["copy"][1]
    t = fs["taxon_filter"]
    assert (t["n_lines"], t["n_excluded"], t["n_not_only"], t["excluded_by"]) == (c["n_lines"], c["n_excluded"], c["n_not_only"], c["excluded_by"])
    assert (fs["n_lines"], fs["n_kept"]) == (c["n_lines"], c["n_kept"]) and "taxon_filter" not in cs
    assert all(fs[k] == cs[k] for k in ("n_hits", "n_queries", "n_unmatched_rows")) and fs["n_hits"] == c["n_kept"]
    # with headers, the queries that lost every line are NoConsensusFound entries
    doc = out["filtered"][0]["doc"].decode()
    results = json.loads(doc)["results"] if fmt == "json" else [json.loads(l) for l in doc.splitlines()[1:]]
    by = {r["query"]: r for r in results}
    kept_queries = {l.split(b"\t")[0].decode() for l in open(copy, "rb").read().splitlines()}
    lost = [h for h in headers if h not in kept_queries]
    assert len(lost) >= 41 and all(by[q]["taxon"] is None for q in lost) and len(by) == len(headers)
    assert sum(r["taxon"] is not None for r in results) > 100


def test_the_command_line(tmp_path, force_gpu, capsys):
    """Strict mode there: a table whose every taxid the database knows, with a sound lineage."""
    rng = np.random.default_rng(75)
    rows = hf.scramble(tf.make_rows(1200, 8, rng, sample_names=True, taxids=GOOD_TAXIDS), rng)
    src, tj = _table(tmp_path, rows), tf.write_db(tmp_path / "t.json")
    hit = {"min_perc_identity": 85.0}
    copy = str(tmp_path / "copy.tsv")
    c = tf.filter_text(src, copy, tj, tf.EXCLUDE, tf.ONLY, keep=lambda f: hf.keep(f, hit))
    only_file = tmp_path / "only.txt"
    only_file.write_text("# the two domains of interest\nd__Bacteria\n\nd__Archaea\n")
    args = ["--exclude-taxon", tf.EXCLUDE[0], "--exclude-taxon", tf.EXCLUDE[1], "--only-taxon-file", str(only_file), "--min-perc-identity", "85"]
    common = ["-t", tj, "--taxon", "bacteria", "--strategy", "relaxed", "--out-format", "jsonl"]
    files = {}
    for tag, table, more in (("cli_filtered", src, args), ("cli_copy", copy, [])):
        paths = {k: str(tmp_path / f"{tag}.{k}") for k in ("doc", "report", "table", "support")}
        assert cli.main(["blastn", "build-consensus", table, "--blutils-out-file", paths["doc"], "--report", paths["report"],
                         "--sample-table", paths["table"], "--support-table", paths["support"]] + common + more) == 0
        assert pipeline.last_ingest_path() == "gpu"
        err = capsys.readouterr().err
        if more:
            exp = [f"taxon filter: excluded {c['n_excluded']}, not in --only-taxon {c['n_not_only']}, of {c['n_lines']} lines"]
            exp += [f"  {el}: {n}" for el, n in zip(tf.EXCLUDE, c["excluded_by"])]
            exp += [f"hit filter: kept {c['n_kept']} of {c['n_lines']} lines"]
            assert [l for l in err.splitlines() if "filter" in l or l.startswith("  ")] == exp and all(c["excluded_by"])
        else:
            assert "filter" not in err
        d = open(os.path.splitext(paths["doc"])[0] + ".jsonl", "rb").read()
        files[tag] = (re.sub(rb'"runId":\s*"[0-9a-f-]{36}"', b'"runId":""', d),) + tuple(open(paths[k], "rb").read() for k in ("report", "table", "support"))
    assert files["cli_filtered"] == files["cli_copy"] and len(files["cli_copy"][0]) > 50000
    # an unknown element: a non-zero exit with the library's message
    with pytest.raises(SystemExit, match="s__uncultured-bacterum"):
        cli.main(["blastn", "build-consensus", src, "--exclude-taxon", "s__uncultured-bacterum"] + common)
