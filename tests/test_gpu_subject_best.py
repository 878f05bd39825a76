"""The best hit per subject end to end.  The rule: a run with best_hit_per_subject gives, byte for byte, what
the run without it gives on the copy of the (filtered) table from which tests/subject_best_reference.py deleted every line but
the best of its (query, subject) pair — the document, the report, the per-sample table, the support table and the ingest
columns, through either parser, the host-column path, both strategies and the command line."""
import json
import os
import re
import stat
import sys

import numpy as np
import pytest

from blutils_amd import _native as N
from blutils_amd import blast, cli, pipeline
from tests import hit_filter_reference as hf
from tests import score_band_reference as band_ref
from tests import subject_best_reference as ref

pytestmark = pytest.mark.gpu

MODES = {"gpu": {"BLU_INGEST": "gpu"}, "cpu": {"BLU_INGEST": "cpu"},
         "host_columns": {"BLU_INGEST": "gpu", "BLU_PIPELINE_HOST_COLUMNS": "1"}}
RUN_ID = re.compile(rb'"runId":\s*"[0-9a-f-]{36}"')


def _set(monkeypatch, mode):
    monkeypatch.delenv("BLU_PIPELINE_HOST_COLUMNS", raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)


def make_rows(n_q, rng, sample_names=False):
    """BLAST-shaped lines in which a subject occurs once, twice, three or seven times under a query (HSPs), often on one
    truncated score (a third of the scores carry a decimal), sometimes under another taxid, in a shuffled order inside the
    query; a subject in twelve, never the first of its query and always 40 bits under the rest, has a taxid the taxonomy lacks."""
    rows = []
    for q in range(n_q):
        name = f"s{q % 3}.{q}" if sample_names else f"q{q:06d}"
        top, g = int(rng.integers(100, 3000)), int(rng.integers(1, 420))
        mine = []
        for k in range(int(rng.integers(1, 6))):
            t = min(2999, 7 * g + int(rng.integers(-3, 10)))
            lacking = k > 0 and rng.random() < 0.08                      # (never a query's only subject, and always under its top:
            if lacking:                                                  #  a top hit without a lineage ends a strict run)
                t = 3000 + int(rng.integers(0, 50))
            for h in range(int(rng.choice([1, 1, 1, 2, 3, 7]))):
                b = top - int(rng.choice([0, 0, 1, 2, 5, 30])) - (40 if lacking else 0)
                text = f"{b}.{int(rng.integers(0, 10))}" if rng.random() < 0.33 else str(b)
                taxid = 100 + t + (1 if h and t < 2990 and rng.random() < 0.2 else 0)
                mine.append(f"{name}\tNR_{t:06d}.1\t{taxid}\t{97 + int(rng.integers(0, 3001)) / 1000:.3f}\t{int(rng.integers(300, 500))}"
                            f"\t1\t0\t1\t400\t1\t400\t1e-{int(rng.integers(50, 150))}\t{text}")
        rows += [mine[i] for i in rng.permutation(len(mine))]
    return rows


def _table(tmp_path, rows, name="b.tsv"):
    p = tmp_path / name
    p.write_bytes(("\n".join(rows) + "\n").encode())
    return str(p)


def _run(tmp_path, tag, table, tj, fmt, headers, cfg, strategy="relaxed", **extra):
    """one run with every output file -> ({doc, report, table, support: bytes}, stats); the text entry gives the same document"""
    paths = {k: str(tmp_path / f"{tag}.{k}") for k in ("doc", "report", "table", "support")}
    kw = dict(headers=headers, out_format=fmt, lenient=True, parse=False, config=cfg, **extra)
    _, stats = pipeline.build_consensus_identities_with_tables(
        table, tj, "bacteria", strategy, out_path=paths["doc"], report_path=paths["report"], sample_table_path=paths["table"],
        support_table_path=paths["support"], **kw)
    files = {k: open(p, "rb").read() for k, p in paths.items()}
    text, _ = pipeline.build_consensus_identities(table, tj, "bacteria", strategy, **kw)
    assert text.encode() == files["doc"]                                 # text and file entry: the same document
    return files, stats


def _subject_stats(counts):
    n_in, n_kept, n_thinned, n_q = counts
    return {"n_hits": n_in, "n_kept": n_kept, "n_queries": n_q, "n_thinned": n_thinned}


@pytest.mark.parametrize("mode,fmt,layout,strategy", [("gpu", "json", "grouped", "relaxed"), ("gpu", "jsonl", "scrambled", "cautious"),
                                                      ("cpu", "jsonl", "grouped", "cautious"), ("cpu", "json", "scrambled", "relaxed"),
                                                      ("host_columns", "json", "scrambled", "cautious"),
                                                      ("host_columns", "jsonl", "grouped", "relaxed")])
def test_every_output_is_that_of_the_copy(tmp_path, monkeypatch, mode, fmt, layout, strategy):
    _set(monkeypatch, mode)
    rng = np.random.default_rng(111)
    rows = make_rows(60, rng, sample_names=True)
    if layout == "scrambled":                                            # a pair's lines far apart, a query's lines not contiguous
        rows = hf.scramble(rows, rng)
    src, tj = _table(tmp_path, rows), hf.write_db(tmp_path / "t.json")
    copy = str(tmp_path / "copy.tsv")
    counts = ref.rewrite_table(src, copy)
    assert counts[0] == len(rows) and counts[1] < len(rows) and 0 < counts[2] < counts[3] == 60
    headers = sorted({r.split("\t")[0] for r in rows}) + ["s1.777777", "s0.888888"]      # two FASTA ids without a hit
    cfg = blast.BlastBuilder.default("/db/ref16s", "bacteria")           # (one run id for every document)
    best, bstats = _run(tmp_path, "best", src, tj, fmt, headers, cfg, strategy, best_hit_per_subject=True)
    assert pipeline.last_ingest_path() == ("cpu" if mode == "cpu" else "gpu")
    plain, pstats = _run(tmp_path, "copy", copy, tj, fmt, headers, cfg, strategy)
    assert best == plain
    assert bstats["subject_best"] == _subject_stats(counts) and "subject_best" not in pstats
    assert (bstats["n_hits"], bstats["n_queries"], bstats["n_unmatched_rows"]) == (pstats["n_hits"], pstats["n_queries"], pstats["n_unmatched_rows"])
    # the selection made a difference: the run without it on the table as it stands is another document and another support table
    full, fstats = _run(tmp_path, "full", src, tj, fmt, headers, cfg, strategy)
    assert full["doc"] != best["doc"] and full["support"] != best["support"]
    assert fstats["n_hits"] == len(rows) and fstats["n_unmatched_rows"] > bstats["n_unmatched_rows"] > 0
    hits = lambda f: sum(int(l.split(b"\t")[3]) for l in f["support"].splitlines()[1:])
    assert hits(best) == counts[1] and hits(full) == len(rows)           # the support table counts each subject once


def _by_query(cols):
    """the columns of every query under its name (the order of the queries left aside)"""
    seg = cols["seg_off"]
    return {name: tuple(cols[k][int(seg[q]):int(seg[q + 1])].tobytes() for k in ("bitscore", "align_len", "tax_desc_row", "acc_rank", "pident"))
            for q, name in enumerate(cols["query_names"])}


@pytest.mark.parametrize("mode", ["gpu", "cpu"])
def test_columns_are_those_of_the_copy(tmp_path, monkeypatch, mode):
    _set(monkeypatch, mode)
    rng = np.random.default_rng(112)
    rows = make_rows(80, rng)
    tj = hf.write_db(tmp_path / "t.json")
    # a grouped file: the columns of the copy, byte for byte
    src, copy = _table(tmp_path, rows), str(tmp_path / "copy.tsv")
    counts = ref.rewrite_table(src, copy)
    got = pipeline.ingest_columns(src, tj, device=0, best_hit_per_subject=True)
    assert pipeline.last_ingest_path() == mode
    hf.assert_columns_equal(got, pipeline.ingest_columns(copy, tj, device=0))
    assert got["subject_best"] == _subject_stats(counts) and counts[1] < counts[0]
    # a scrambled file: the queries are numbered by their first line in the file, and where that line is one of the deleted
    # ones the copy numbers them differently — every query's rows, and the accessions, are the copy's
    src = _table(tmp_path, hf.scramble(rows, rng), "s.tsv")
    counts = ref.rewrite_table(src, copy)
    got, exp = pipeline.ingest_columns(src, tj, device=0, best_hit_per_subject=True), pipeline.ingest_columns(copy, tj, device=0)
    assert _by_query(got) == _by_query(exp) and got["accessions"] == exp["accessions"]
    assert got["query_names"] == pipeline.ingest_columns(src, tj, device=0)["query_names"]
    assert got["subject_best"] == _subject_stats(counts)
    # under a band as well: the band acts on the thinned table
    c2 = str(tmp_path / "copy2.tsv")
    bcounts = band_ref.rewrite_table(copy, c2, D=2)
    got = pipeline.ingest_columns(src, tj, device=0, best_hit_per_subject=True, score_band={"top_bits": 2})
    assert _by_query(got) == _by_query(pipeline.ingest_columns(c2, tj, device=0))
    assert got["score_band"] == {"n_hits": bcounts[0], "n_raised": bcounts[1], "n_queries": bcounts[3], "n_widened": bcounts[2]}
    assert "subject_best" not in pipeline.ingest_columns(src, tj, device=0, best_hit_per_subject=False)


@pytest.mark.parametrize("mode", ["gpu", "cpu", "host_columns"])
def test_order_of_stages_filters_then_subjects_then_band(tmp_path, monkeypatch, mode):
    """a.1: subject X's best line (700.5 bits, species s5, 98 % identity) goes under an identity threshold or a taxon filter;
    X's next best (650) then survives, X's 645 is deleted, and the 1 % band under 650 takes Y's 649 — two subjects in the top
    group, where the band before the selection would have counted X twice."""
    _set(monkeypatch, mode)
    line = lambda q, acc, taxid, bs, pid="99.000": f"{q}\t{acc}.1\t{taxid}\t{pid}\t400\t0\t0\t1\t400\t1\t400\t1e-50\t{bs}"
    rows = [line("a.1", "X", 105, "700.5", "98.000"), line("a.1", "X", 108, "645"), line("a.1", "X", 108, "650"),
            line("a.1", "Y", 106, "649"), line("a.1", "Z", 107, "600")]
    rows += make_rows(30, np.random.default_rng(113), sample_names=True)
    src, tj = _table(tmp_path, rows), hf.write_db(tmp_path / "t.json")
    fields = [r.split("\t") for r in rows]
    cfg = blast.BlastBuilder.default("/db/ref16s", "bacteria")
    flt = {"min_perc_identity": 98.5}
    cases = [("identity", dict(hit_filter=flt), [hf.keep(f, flt) for f in fields], ("3", "2", "650")),
             ("taxon", dict(taxon_filter={"exclude": ["s__s5"]}), [f[2] != "105" for f in fields], ("3", "2", "650")),
             ("none", {}, None, ("3", "1", "700"))]
    for tag, extra, kept, first in cases:
        c1, c2 = str(tmp_path / f"c1_{tag}.tsv"), str(tmp_path / f"c2_{tag}.tsv")
        counts = ref.rewrite_table(src, c1, kept=kept)
        bcounts = band_ref.rewrite_table(c1, c2, m=1000)
        got, stats = _run(tmp_path, f"best_{tag}", src, tj, "json", None, cfg, best_hit_per_subject=True,
                          score_band=pipeline.ScoreBand(top_percent="1"), **extra)
        plain, _ = _run(tmp_path, f"copy_{tag}", c2, tj, "json", None, cfg)
        assert got == plain, tag
        assert stats["subject_best"] == _subject_stats(counts), tag
        assert stats["score_band"] == {"n_hits": bcounts[0], "n_raised": bcounts[1], "n_queries": bcounts[3], "n_widened": bcounts[2]}, tag
        if kept is not None:
            assert (stats["n_lines"], stats["n_kept"]) == (len(rows), sum(kept)), tag       # the filters' counts are theirs
        sup = {l.split("\t")[0]: l.split("\t") for l in got["support"].decode().splitlines()}
        assert (sup["a.1"][3], sup["a.1"][5], sup["a.1"][8]) == first, tag                  # hits, top_hits, bit_score


def test_the_case_it_exists_for(tmp_path, monkeypatch, capsys):
    """Two HSPs of one subject tie on the top truncated score (500.4 and 500), a second subject lies lower: today the
    reference's multi-taxa path runs on a group of two; with the flag the group is one line and the single match is reported."""
    _set(monkeypatch, "gpu")
    line = lambda q, acc, taxid, bs: f"{q}\t{acc}.1\t{taxid}\t100.000\t400\t0\t0\t1\t400\t1\t400\t1e-50\t{bs}"
    rows = [line("q", "X", 114, "500.4"), line("q", "X", 114, "500"), line("q", "Y", 115, "480")]
    src, tj = _table(tmp_path, rows), hf.write_db(tmp_path / "t.json")
    copy = str(tmp_path / "copy.tsv")
    assert ref.rewrite_table(src, copy) == (3, 2, 1, 1)
    assert open(copy).read().splitlines() == [rows[0], rows[2]]
    kw = dict(out_format="json", lenient=False)
    today, tstats = pipeline.build_consensus_identities(src, tj, "bacteria", "relaxed", **kw)
    best, stats = pipeline.build_consensus_identities(src, tj, "bacteria", "relaxed", best_hit_per_subject=True, **kw)
    of_copy, _ = pipeline.build_consensus_identities(copy, tj, "bacteria", "relaxed", **kw)
    t, b, c = today[0]["taxon"], best[0]["taxon"], of_copy[0]["taxon"]
    print("today:", json.dumps(t), "\nbest: ", json.dumps(b))
    assert b == c and b != t
    assert t["singleMatch"] is False and b["singleMatch"] is True
    assert b["identifier"] == t["identifier"] == "s14" and b["bitScore"] == t["bitScore"] == 500.0
    assert stats["subject_best"] == {"n_hits": 3, "n_kept": 2, "n_queries": 1, "n_thinned": 1}
    assert (tstats["n_hits"], stats["n_hits"]) == (3, 2)
    # through the command line
    capsys.readouterr()
    base = ["blastn", "build-consensus", "-t", tj, "--taxon", "bacteria", "--strategy", "relaxed"]
    outs = {}
    for tag, argv in (("today", [src]), ("best", [src, "--best-hit-per-subject"]), ("copy", [copy]), ("again", [copy, "--best-hit-per-subject"])):
        assert cli.main(base + argv) == 0
        cap = capsys.readouterr()
        outs[tag] = (RUN_ID.sub(b'"runId":""', cap.out.encode()), cap.err)
    assert outs["best"][0] == outs["copy"][0] == outs["again"][0] != outs["today"][0]
    assert "subject best hit" not in outs["today"][1] and "subject best hit" not in outs["copy"][1]
    assert "subject best hit: kept 2 of 3 lines, thinned 1 of 1 queries" in outs["best"][1]
    assert "subject best hit: kept 2 of 2 lines, thinned 0 of 1 queries" in outs["again"][1]       # idempotent


def test_cli_files_counts_and_the_place_of_the_count_line(tmp_path, monkeypatch, capsys):
    _set(monkeypatch, "gpu")
    rng = np.random.default_rng(114)
    rows = make_rows(50, rng, sample_names=True)
    src, tj = _table(tmp_path, rows), hf.write_db(tmp_path / "t.json")
    flt = {"min_perc_identity": 97.5}
    kept = [hf.keep(r.split("\t"), flt) for r in rows]
    c1, c2 = str(tmp_path / "c1.tsv"), str(tmp_path / "c2.tsv")
    counts = ref.rewrite_table(src, c1, kept=kept)
    bcounts = band_ref.rewrite_table(c1, c2, D=2)
    assert counts[0] == sum(kept) < len(rows) and counts[1] < counts[0] and bcounts[1] > 0
    common = ["-t", tj, "--taxon", "bacteria", "--strategy", "cautious", "--out-format", "jsonl"]
    files = {}
    for tag, table, more in (("best", src, ["--min-perc-identity", "97.5", "--best-hit-per-subject", "--top-bits", "2"]), ("copy", c2, [])):
        paths = {k: str(tmp_path / f"{tag}.{k}") for k in ("doc", "report", "table", "support")}
        assert cli.main(["blastn", "build-consensus", table, "--blutils-out-file", paths["doc"], "--report", paths["report"],
                         "--sample-table", paths["table"], "--support-table", paths["support"]] + common + more) == 0
        err = capsys.readouterr().err
        line = f"subject best hit: kept {counts[1]} of {counts[0]} lines, thinned {counts[2]} of {counts[3]} queries"
        assert (line in err) == bool(more)
        if more:
            band_line = f"score band: raised {bcounts[1]} of {bcounts[0]} lines in {bcounts[2]} of {bcounts[3]} queries"
            assert err.index(f"hit filter: kept {counts[0]} of {len(rows)} lines") < err.index(line) < err.index(band_line)
        d = open(os.path.splitext(paths["doc"])[0] + ".jsonl", "rb").read()
        files[tag] = (RUN_ID.sub(b'"runId":""', d),) + tuple(open(paths[k], "rb").read() for k in ("report", "table", "support"))
    assert files["best"] == files["copy"] and len(files["copy"][0]) > 5000
    # n_unmatched_rows is that of the copy: deleted lines with a taxid the taxonomy lacks are no longer counted
    copy = str(tmp_path / "copy.tsv")
    ref.rewrite_table(src, copy)
    kw = dict(out_format="jsonl", lenient=True, parse=False)
    for mode in ("gpu", "cpu", "host_columns"):
        _set(monkeypatch, mode)
        _, full = pipeline.build_consensus_identities(src, tj, "bacteria", "relaxed", **kw)
        _, best = pipeline.build_consensus_identities(src, tj, "bacteria", "relaxed", best_hit_per_subject=True, **kw)
        _, of_copy = pipeline.build_consensus_identities(copy, tj, "bacteria", "relaxed", **kw)
        assert full["n_unmatched_rows"] > best["n_unmatched_rows"] == of_copy["n_unmatched_rows"] > 0, mode
        assert best["n_hits"] == of_copy["n_hits"] < full["n_hits"], mode


def test_run_with_consensus_passes_the_flag_through(tmp_path, monkeypatch, capsys):
    """FASTA -> stand-in `blastn` executable -> the table written as it is, in full -> consensus on the best hit per subject."""
    _set(monkeypatch, "gpu")
    rng = np.random.default_rng(115)
    rows = make_rows(40, rng)
    bt, tj = _table(tmp_path, rows), hf.write_db(tmp_path / "t.json")
    fa = tmp_path / "queries.fa"
    fa.write_text("".join(f">q{i:06d} read {i}\nACGTACGTAC\n" for i in range(40)) + ">fasta_only\nAC\n")
    os.mkdir(tmp_path / "db")
    (tmp_path / "db" / "ref16s.nsq").write_text("")
    exe = tmp_path / "blastn"
    exe.write_text(f"#!{sys.executable}\nimport sys\n"
                   f"want = {{l[1:].split()[0] for l in sys.stdin.read().split(chr(10)) if l.startswith('>')}}\n"
                   f"sys.stdout.write(''.join(l for l in open({bt!r}) if l.split(chr(9))[0] in want))\n")
    exe.chmod(exe.stat().st_mode | stat.S_IEXEC)
    copy = str(tmp_path / "copy.tsv")
    counts = ref.rewrite_table(bt, copy)
    sup = tmp_path / "support.tsv"
    argv = ["blastn", "run-with-consensus", str(fa), "-d", str(tmp_path / "db" / "ref16s"), "-t", tj, "--blast-out-file",
            str(tmp_path / "work" / "hits.tsv"), "--blutils-out-file", str(tmp_path / "res" / "consensus.json"), "--taxon", "bacteria",
            "--strategy", "relaxed", "--threads", "2", "--blastn", str(exe), "--best-hit-per-subject", "--support-table", str(sup)]
    assert cli.main(argv) == 0
    assert f"subject best hit: kept {counts[1]} of {counts[0]} lines, thinned {counts[2]} of {counts[3]} queries" in capsys.readouterr().err
    assert counts[1] < counts[0]
    assert sorted(open(tmp_path / "work" / "hits.out").read().splitlines()) == sorted(rows)      # the BLAST table: in full
    doc = json.load(open(tmp_path / "res" / "consensus.json"))
    by = {r["query"]: r["taxon"] for r in doc["results"]}
    assert by["fasta_only"] is None and len(by) == 41
    exp, _ = pipeline.build_consensus_identities(copy, tj, "bacteria", "relaxed", lenient=True)
    assert all(by[r["query"]] == r["taxon"] for r in exp)
    sup_copy = tmp_path / "support_copy.tsv"
    pipeline.build_consensus_identities_with_tables(copy, tj, "bacteria", "relaxed", headers=["fasta_only"], out_path=str(tmp_path / "c.json"),
                                                    lenient=True, support_table_path=str(sup_copy))
    assert sup.read_bytes() == sup_copy.read_bytes()


@pytest.mark.parametrize("mode", ["gpu", "host_columns"])
def test_an_empty_selection_is_the_run_without_the_flag(tmp_path, monkeypatch, mode):
    """blu_build_consensus with a subject_best whose mask is empty (what a NULL member becomes inside): the bytes and the
    counts of the run without the keyword."""
    _set(monkeypatch, mode)
    rows = make_rows(40, np.random.default_rng(116), sample_names=True)
    src, tj = _table(tmp_path, rows), hf.write_db(tmp_path / "t.json")
    cfg = blast.BlastBuilder.default("/db/ref16s", "bacteria")
    plain, pstats = _run(tmp_path, "plain", src, tj, "json", None, cfg, score_band={"top_bits": 1})
    monkeypatch.setattr(N, "SUBJECT_BEST_PER_QUERY", 0)                  # the keyword now sends {mask = 0} through the new entry point
    empty, estats = _run(tmp_path, "empty", src, tj, "json", None, cfg, score_band={"top_bits": 1}, best_hit_per_subject=True)
    assert empty == plain
    assert estats["subject_best"] == {"n_hits": len(rows), "n_kept": len(rows), "n_queries": 40, "n_thinned": 0}
    assert estats["score_band"] == pstats["score_band"] and estats["n_hits"] == pstats["n_hits"] == len(rows)
    hf.assert_columns_equal(pipeline.ingest_columns(src, tj, device=0, best_hit_per_subject=True), pipeline.ingest_columns(src, tj, device=0))
