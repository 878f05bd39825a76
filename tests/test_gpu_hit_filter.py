"""Hit filters in the GPU parser (csrc/ingest_gpu.hip: parse_rows_filtered, the e-value verdicts, the stable
compaction) and end to end.  The rule: a filtered run gives what the unfiltered run gives on the copy of the table from
which tests/hit_filter_reference.py deleted the dropped lines — columns against tests/ingest_reference.py, documents,
reports and per-sample tables byte for byte."""
import json
import os
import stat
import sys

import numpy as np
import pytest

from blutils_amd import blast, cli, pipeline
from tests import hit_filter_reference as hf
from tests import ingest_reference as ref

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


def _check(src, tj, flt, tmp_path, path="gpu"):
    """filtered GPU ingest of src == independent reading of filter_text's copy; the GPU parser did it"""
    dst = str(tmp_path / "filtered_copy.tsv")
    n_lines, n_kept = hf.filter_text(src, dst, flt)
    got = pipeline.ingest_columns(src, tj, device=0, hit_filter=flt)
    assert pipeline.last_ingest_path() == path
    hf.assert_columns_equal(got, ref.read_table(dst, tj))
    assert (got["n_lines"], got["n_kept"]) == (n_lines, n_kept)
    return got, n_lines, n_kept


def _line(q, pid="99.0", aln="400", ev="1e-50", bs="700", acc="A.1", taxid="100"):
    return f"{q}\t{acc}\t{taxid}\t{pid}\t{aln}\t0\t0\t1\t400\t1\t400\t{ev}\t{bs}"


@pytest.mark.parametrize("layout", ["grouped", "scrambled"])
@pytest.mark.parametrize("which", list(hf.FILTERS))
def test_gpu_filtered_ingest_is_the_ingest_of_the_filtered_copy(tmp_path, force_gpu, layout, which):
    rng = np.random.default_rng(41)
    rows = hf.make_rows(3000, 8, rng)
    if layout == "scrambled":
        rows = hf.scramble(rows, rng)
    src, tj = _table(tmp_path, rows), hf.write_db(tmp_path / "t.json")
    got, n_lines, n_kept = _check(src, tj, hf.FILTERS[which], tmp_path)
    assert n_lines == len(rows) and 0 < n_kept < n_lines
    assert int((got["tax_desc_row"] == ref.UNMATCHED).sum()) > 0


@pytest.mark.parametrize("eol,final", [("\n", True), ("\r\n", True), ("\r\n", False)])
def test_gpu_boundaries_and_e_value_spellings(tmp_path, force_gpu, eol, final):
    tj = hf.write_db(tmp_path / "t.json")
    rows = [_line("a", pid="97.000"), _line("a", pid="96.999"), _line("b", pid="97"), _line("c", pid="9.7e1")]
    _, _, kept = _check(_table(tmp_path, rows, eol=eol, final=final), tj, {"min_perc_identity": 97.0}, tmp_path)
    assert kept == 3
    rows = [_line("a", bs="99.5"), _line("a", bs="99.6"), _line("b", bs="99.7"), _line("c", bs="1.0e2"), _line("d", bs="99")]
    got, _, kept = _check(_table(tmp_path, rows, eol=eol, final=final), tj, {"min_bit_score": 99.6}, tmp_path)
    assert kept == 3 and got["bitscore"].tolist() == [99, 99, 100]
    forms = ["1.01e-05", "0.0", "1e-05", "1E-5", "0.00001", "9.99e-06", "3e-180", "5e-324", "1e-400", "1.0000000000001e-5", "2e-5"]
    rows = [_line(f"q{i}", ev=e) for i, e in enumerate(forms)]
    got, _, kept = _check(_table(tmp_path, rows, eol=eol, final=final), tj, {"max_e_value": 1e-5}, tmp_path)
    assert kept == 8 and got["query_names"] == [f"q{i}".encode() for i in range(1, 9)]
    _, _, kept = _check(_table(tmp_path, rows, eol=eol, final=final), tj, {"max_e_value": 0.0}, tmp_path)
    assert kept == 2
    # thresholds whose neighbourhood the device cannot compute in one operation: 1e-30 (two steps: bracket, then the host for the
    # threshold's own spellings), 1e-300 and 5e-324 (outside the band: the host decides the near ones), infinity, NaN, negative
    forms = ["1e-30", "1.0e-30", "0.00000000000001e-16", "9.9999999999e-31", "1.00000000001e-30", "10e-31", "1e-29", "3e-300", "1e-300",
             "1.0e-300", "0.9e-300", "4e-324", "5e-324", "2e-324", "3e-324", "1e-323", "0", "1e308", "1e309", "12345.678", "1e-31", "100e-32"]
    rows = [_line(f"q{i}", ev=e) for i, e in enumerate(forms)]
    for E in (1e-30, 1e-300, 5e-324, float("inf"), float("nan"), -1.0, 1e-29, 1e300, 12345.678):
        got = pipeline.ingest_columns(_table(tmp_path, rows, eol=eol, final=final), tj, device=0, hit_filter={"max_e_value": E})
        exp = [f"q{i}".encode() for i, e in enumerate(forms) if float(e) <= E]
        assert got["query_names"] == exp, E
        assert pipeline.last_ingest_path() == ("gpu" if exp else "cpu")      # (nothing kept: handed to the host parser)


def test_a_few_thousand_lines_spelled_like_the_threshold(tmp_path, force_gpu):
    """Fields spelled like the threshold are an ordinary case: against 1e-5 the device decides them exactly (one operation),
    against 1e-30 they go to the host as a list and come back as decisions; the GPU parser keeps the file either way."""
    rng = np.random.default_rng(42)
    rows = hf.make_rows(4000, 6, rng)
    own = {1e-5: ["1e-05", "1E-5", "0.00001", "1.0e-05"], 1e-30: ["1e-30", "1.0e-30", "10e-31", "0.1e-29"]}
    tj = hf.write_db(tmp_path / "t.json")
    for E, spellings in own.items():
        lines = []
        for i, r in enumerate(rows):
            c = r.split("\t")
            if i % 4 == 0:
                c[11] = spellings[(i // 4) % len(spellings)]
            lines.append("\t".join(c))
        assert sum(1 for r in lines if r.split("\t")[11] in spellings) > 3000
        _check(_table(tmp_path, hf.scramble(lines, rng)), tj, {"max_e_value": E}, tmp_path)


@pytest.mark.parametrize("shape", ["a_whole_parse_block_dropped", "one_line_kept", "alternating", "first_and_last_dropped", "general_form"])
def test_compaction_shapes(tmp_path, force_gpu, shape):
    rng = np.random.default_rng(43)
    rows = hf.make_rows(700, 6, rng, long_names=shape == "general_form")
    if shape == "general_form":
        assert sum(map(len, rows)) / len(rows) >= 128                    # no 256-line block fits the LDS stage
    n = len(rows)
    assert n > 1500
    low = {"a_whole_parse_block_dropped": lambda i: 256 <= i < 512 or i % 7 == 0, "one_line_kept": lambda i: i != 777,
           "alternating": lambda i: i % 2 == 1, "first_and_last_dropped": lambda i: i in (0, n - 1),
           "general_form": lambda i: i % 3 == 0}[shape]
    lines = []
    for i, r in enumerate(rows):
        c = r.split("\t")
        c[3] = "50.000" if low(i) else c[3]
        lines.append("\t".join(c))
    src, tj = _table(tmp_path, lines, final=shape != "first_and_last_dropped"), hf.write_db(tmp_path / "t.json")
    got, n_lines, n_kept = _check(src, tj, {"min_perc_identity": 60.0}, tmp_path)
    assert n_kept == sum(1 for i in range(n) if not low(i))
    if shape == "general_form":
        _check(src, tj, hf.FILTERS["all"], tmp_path)


def test_several_million_lines(tmp_path, force_gpu):
    """3 M lines: the prefix sum over the keep words spans 700 blocks of the device scan, the parse 11 000 blocks.  The
    expected columns of so large a table come from the block it repeats (Python reads 20 000 lines, not 3 M): grouped
    queries in file order, so every column is the kept lines' values in file order."""
    rng = np.random.default_rng(44)
    block = hf.make_rows(4000, 9, rng)
    reps = 3_000_000 // len(block) + 1
    flt = hf.FILTERS["all"]
    fields = [r.split("\t") for r in block]
    keep = np.array([hf.keep(c, flt) for c in fields])
    src = tmp_path / "big.tsv"
    with open(src, "wb") as f:
        body = ("\n".join(block) + "\n").encode()
        for r in range(reps):
            f.write(body.replace(b"q0", b"r%03d_" % r))                  # the queries of every repetition are new ones
    tj = hf.write_db(tmp_path / "t.json")
    got = pipeline.ingest_columns(str(src), tj, device=0, hit_filter=flt)
    assert pipeline.last_ingest_path() == "gpu"
    assert (got["n_lines"], got["n_kept"]) == (len(block) * reps, int(keep.sum()) * reps) and got["n_lines"] >= 3_000_000
    pid = np.array([float(c[3]) for c in fields])[keep]
    aln = np.array([int(c[4]) for c in fields], dtype=np.int32)[keep]
    bs = np.array([int(float(c[12])) for c in fields], dtype=np.int32)[keep]
    assert np.array_equal(got["pident"], np.tile(pid, reps)) and np.array_equal(got["align_len"], np.tile(aln, reps))
    assert np.array_equal(got["bitscore"], np.tile(bs, reps))
    kept_queries = []
    for c, k in zip(fields, keep):
        if k and (not kept_queries or kept_queries[-1] != c[0]):
            kept_queries.append(c[0])
    assert len(got["query_names"]) == len(kept_queries) * reps
    assert got["query_names"][:3] == [q.replace("q0", "r000_").encode() for q in kept_queries[:3]]
    # and the host parser gives the same table
    os.environ["BLU_INGEST"] = "cpu"
    host = pipeline.ingest_columns(str(src), tj, device=0, hit_filter=flt)
    assert pipeline.last_ingest_path() == "cpu"
    hf.assert_columns_equal(got, host)
    assert (host["n_lines"], host["n_kept"]) == (got["n_lines"], got["n_kept"])


def test_either_parser_and_a_declined_file(tmp_path, force_gpu):
    rng = np.random.default_rng(45)
    rows = hf.scramble(hf.make_rows(2500, 8, rng), rng)
    tj = hf.write_db(tmp_path / "t.json")
    src = _table(tmp_path, rows)
    for which, flt in hf.FILTERS.items():
        gpu = pipeline.ingest_columns(src, tj, device=0, hit_filter=flt)
        assert pipeline.last_ingest_path() == "gpu"
        host = pipeline.ingest_columns(src, tj, device=-1, hit_filter=flt)
        assert pipeline.last_ingest_path() == "cpu"
        hf.assert_columns_equal(gpu, host)
        assert (gpu["n_lines"], gpu["n_kept"]) == (host["n_lines"], host["n_kept"])
    # quotes: the GPU parser declines the file as it does without a filter; the host path applies the filter
    rows[17] = '"' + rows[17].replace("\t", '"\t', 1)
    _check(_table(tmp_path, rows, name="quoted.tsv"), tj, hf.FILTERS["all"], tmp_path, path="cpu")
    # junk in column 11: loads without its threshold, is a parse error naming the line with it — whichever parser came first
    from blutils_amd import _native as N
    rows[17] = _line("x", ev="n/a")
    src = _table(tmp_path, rows, name="junk.tsv")
    assert pipeline.ingest_columns(src, tj, device=0, hit_filter={"min_perc_identity": 90.0})["n_lines"] == len(rows)
    assert pipeline.last_ingest_path() == "gpu"
    with pytest.raises(N.BluError, match=r"line 18\b.*numeric"):
        pipeline.ingest_columns(src, tj, device=0, hit_filter={"max_e_value": 1e-5})
    # no filter and an empty filter: today's call, today's kernel
    today = pipeline.ingest_columns(_table(tmp_path, rows[:17]), tj, device=0)
    assert pipeline.last_ingest_path() == "gpu" and "n_kept" not in today
    hf.assert_columns_equal(pipeline.ingest_columns(_table(tmp_path, rows[:17]), tj, device=0, hit_filter={}), today)


@pytest.mark.parametrize("strategy,fmt", [("relaxed", "json"), ("cautious", "jsonl")])
def test_documents_reports_and_tables_are_those_of_the_filtered_copy(tmp_path, force_gpu, strategy, fmt, capsys):
    rng = np.random.default_rng(46)
    rows = hf.scramble(hf.make_rows(2500, 8, rng, sample_names=True), rng)
    # (queries 0 .. 39 lose every line under the filter)
    rows = ["\t".join(c[:3] + ["70.000"] + c[4:]) if int(c[0].split(".")[1]) < 40 else "\t".join(c) for c in (r.split("\t") for r in rows)]
    src, tj = _table(tmp_path, rows), hf.write_db(tmp_path / "t.json")
    flt = hf.FILTERS["all"]
    copy = str(tmp_path / "copy.tsv")
    n_lines, n_kept = hf.filter_text(src, copy, flt)
    headers = sorted({r.split("\t")[0] for r in rows}) + ["s1.999999"]
    cfg = blast.BlastBuilder.default("/db/ref16s", "bacteria")             # (one run id for both documents)
    out = {}
    for tag, table, extra in (("filtered", src, {"hit_filter": flt}), ("copy", copy, {})):
        paths = {k: str(tmp_path / f"{tag}.{k}") for k in ("doc", "report", "table")}
        _, stats = pipeline.build_consensus_identities_with_tables(
            table, tj, "bacteria", strategy, headers=headers, out_format=fmt, lenient=True, parse=False, config=cfg,
            out_path=paths["doc"], report_path=paths["report"], sample_table_path=paths["table"], **extra)
        assert pipeline.last_ingest_path() == "gpu"
        out[tag] = ({k: open(p, "rb").read() for k, p in paths.items()}, stats)
        text, stats2 = pipeline.build_consensus_identities(table, tj, "bacteria", strategy, headers=headers, out_format=fmt,
                                                           lenient=True, parse=False, config=cfg, **extra)
        assert text.encode() == out[tag][0]["doc"]                        # text and file entry: the same document
    assert out["filtered"][0] == out["copy"][0]
    fs, cs = out["filtered"][1], out["copy"][1]
    assert (fs["n_lines"], fs["n_kept"]) == (n_lines, n_kept) and "n_kept" not in cs
    assert all(fs[k] == cs[k] for k in ("n_hits", "n_queries", "n_unmatched_rows")) and fs["n_hits"] == n_kept
    # with headers, the queries that lost every line are NoConsensusFound entries
    doc = out["filtered"][0]["doc"].decode()
    results = json.loads(doc)["results"] if fmt == "json" else [json.loads(l) for l in doc.splitlines()[1:]]
    by = {r["query"]: r for r in results}
    kept_queries = {l.split(b"\t")[0].decode() for l in open(copy, "rb").read().splitlines()}
    lost = [h for h in headers if h not in kept_queries]
    assert len(lost) >= 41 and all(by[q]["taxon"] is None for q in lost) and len(by) == len(headers)
    assert sum(r["taxon"] is not None for r in results) > 1000
    # through the command line (strict mode there: a DB that knows every taxid of the table): the same three files, the run
    # ids apart, and the count on stderr
    import re
    tj_full = hf.write_db(tmp_path / "full.json", n=3100)
    args = ["--min-perc-identity", "85", "--min-align-length", "500", "--max-e-value", "1e-30", "--min-bit-score", "20000.25"]
    common = ["-t", tj_full, "--taxon", "bacteria", "--strategy", strategy, "--out-format", fmt]
    files = {}
    for tag, table, more in (("cli_filtered", src, args), ("cli_copy", copy, [])):
        paths = {k: str(tmp_path / f"{tag}.{k}") for k in ("doc", "report", "table")}
        assert cli.main(["blastn", "build-consensus", table, "--blutils-out-file", paths["doc"], "--report", paths["report"],
                         "--sample-table", paths["table"]] + common + more) == 0
        assert pipeline.last_ingest_path() == "gpu"
        err = capsys.readouterr().err
        assert (f"hit filter: kept {n_kept} of {n_lines} lines" in err) == bool(more)
        d = open(os.path.splitext(paths["doc"])[0] + "." + fmt, "rb").read()
        files[tag] = (re.sub(rb'"runId":\s*"[0-9a-f-]{36}"', b'"runId":""', d), open(paths["report"], "rb").read(), open(paths["table"], "rb").read())
    assert files["cli_filtered"] == files["cli_copy"] and len(files["cli_copy"][0]) > 100000


def test_run_with_consensus_filters_the_consensus_step_only(tmp_path, force_gpu, capsys):
    """FASTA -> stand-in `blastn` executable -> the table written in full -> filtered consensus."""
    rng = np.random.default_rng(47)
    rows = hf.make_rows(130, 8, rng)
    rows = ["\t".join(c[:3] + ["70.000"] + c[4:]) if c[0] in ("q000003", "q000077") else "\t".join(c) for c in (r.split("\t") for r in rows)]
    bt, tj = _table(tmp_path, rows), hf.write_db(tmp_path / "t.json", n=3100)     # (strict mode: every taxid of the table is known)
    fa = tmp_path / "queries.fa"
    fa.write_text("".join(f">q{i:06d} read {i}\nACGTACGTAC\nGGTT\n" for i in range(130)) + ">fasta_only\nAC\n")
    os.mkdir(tmp_path / "db")
    (tmp_path / "db" / "ref16s.nsq").write_text("")
    exe = tmp_path / "blastn"
    exe.write_text(f"#!{sys.executable}\nimport sys\n"
                   f"want = {{l[1:].split()[0] for l in sys.stdin.read().split(chr(10)) if l.startswith('>')}}\n"
                   f"sys.stdout.write(''.join(l for l in open({bt!r}) if l.split(chr(9))[0] in want))\n")
    exe.chmod(exe.stat().st_mode | stat.S_IEXEC)
    flt = {"min_perc_identity": 85.0, "max_e_value": 1e-5}
    copy = str(tmp_path / "copy.tsv")
    n_lines, n_kept = hf.filter_text(bt, copy, flt)
    argv = ["blastn", "run-with-consensus", str(fa), "-d", str(tmp_path / "db" / "ref16s"), "-t", tj, "--blast-out-file",
            str(tmp_path / "work" / "hits.tsv"), "--blutils-out-file", str(tmp_path / "res" / "consensus.json"), "--taxon", "bacteria",
            "--strategy", "relaxed", "--threads", "2", "--blastn", str(exe), "--min-perc-identity", "85", "--max-e-value", "1e-5"]
    assert cli.main(argv) == 0
    assert f"hit filter: kept {n_kept} of {n_lines} lines" in capsys.readouterr().err
    assert sorted(open(tmp_path / "work" / "hits.out").read().splitlines()) == sorted(rows)      # the BLAST table: in full
    doc = json.load(open(tmp_path / "res" / "consensus.json"))
    by = {r["query"]: r["taxon"] for r in doc["results"]}
    assert sorted(by) == sorted([f"q{i:06d}" for i in range(130)] + ["fasta_only"])
    assert by["q000003"] is None and by["q000077"] is None and by["fasta_only"] is None
    exp, _ = pipeline.build_consensus_identities(copy, tj, "bacteria", "relaxed", lenient=False)
    assert all(by[r["query"]] == r["taxon"] for r in exp) and sum(t is not None for t in by.values()) > 60
