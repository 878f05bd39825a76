"""The minimum cover end to end.  The rule: a run with min_cover gives, byte for byte, what the run with the same
options before it gives on the copy of the table from which tests/min_cover_reference.py deleted the top lines outside the
covering prefix — the document, the report, the per-sample table and the support table, through either parser, the host-column
path, both strategies and the command line."""
import os
import re

import numpy as np
import pytest

from blutils_amd import _native as N
from blutils_amd import blast, cli, pipeline
from tests import hit_filter_reference as hf
from tests import min_cover_reference as ref
from tests import score_band_reference as band_ref
from tests import subject_best_reference as subj_ref

pytestmark = pytest.mark.gpu

MODES = {"gpu": {"BLU_INGEST": "gpu"}, "cpu": {"BLU_INGEST": "cpu"},
         "host_columns": {"BLU_INGEST": "gpu", "BLU_PIPELINE_HOST_COLUMNS": "1"}}
RUN_ID = re.compile(rb'"runId":\s*"[0-9a-f-]{36}"')


def _set(monkeypatch, mode):
    monkeypatch.delenv("BLU_PIPELINE_HOST_COLUMNS", raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)


def _table(tmp_path, rows, name="b.tsv"):
    p = tmp_path / name
    p.write_bytes(("\n".join(rows) + "\n").encode())
    return str(p)


def _run(tmp_path, tag, table, tj, fmt, headers, cfg, strategy="relaxed", lenient=True, **extra):
    """one run with every output file -> ({doc, report, table, support: bytes}, stats); the text entry gives the same document"""
    paths = {k: str(tmp_path / f"{tag}.{k}") for k in ("doc", "report", "table", "support")}
    kw = dict(headers=headers, out_format=fmt, lenient=lenient, parse=False, config=cfg, **extra)
    _, stats = pipeline.build_consensus_identities_with_tables(
        table, tj, "bacteria", strategy, out_path=paths["doc"], report_path=paths["report"], sample_table_path=paths["table"],
        support_table_path=paths["support"], **kw)
    files = {k: open(p, "rb").read() for k, p in paths.items()}
    text, tstats = pipeline.build_consensus_identities(table, tj, "bacteria", strategy, **kw)
    assert text.encode() == files["doc"]                                 # text and file entry: the same document
    assert tstats.get("min_cover") == stats.get("min_cover")
    return files, stats


@pytest.mark.parametrize("mode,fmt,layout,strategy", [("gpu", "json", "grouped", "relaxed"), ("gpu", "jsonl", "scrambled", "cautious"),
                                                      ("cpu", "jsonl", "grouped", "cautious"), ("cpu", "json", "scrambled", "relaxed"),
                                                      ("host_columns", "json", "scrambled", "cautious"),
                                                      ("host_columns", "jsonl", "grouped", "relaxed")])
def test_every_output_is_that_of_the_copy(tmp_path, monkeypatch, mode, fmt, layout, strategy):
    _set(monkeypatch, mode)
    rng = np.random.default_rng(211)
    rows = ref.make_rows(60, rng, sample_names=True)
    if layout == "scrambled":                                            # a query's lines not contiguous
        rows = hf.scramble(rows, rng)
    src, tj = _table(tmp_path, rows), ref.write_db(tmp_path / "t.json")
    copy = str(tmp_path / "copy.tsv")
    counts = ref.rewrite_table(src, copy, tj, False, 80000)
    assert counts["n_hits"] == len(rows) > counts["n_kept"] and counts["n_queries"] == 60
    assert 5 < counts["n_narrowed"] < 50 and counts["n_unresolved"] >= 5
    headers = sorted({r.split("\t")[0] for r in rows}) + ["s1.777777", "s0.888888"]      # two FASTA ids without a hit
    cfg = blast.BlastBuilder.default("/db/ref16s", "bacteria")           # (one run id for every document)
    cover, cstats = _run(tmp_path, "cover", src, tj, fmt, headers, cfg, strategy, min_cover="80")
    assert pipeline.last_ingest_path() == ("cpu" if mode == "cpu" else "gpu")
    plain, pstats = _run(tmp_path, "copy", copy, tj, fmt, headers, cfg, strategy)
    assert cover == plain
    assert cstats["min_cover"] == counts and "min_cover" not in pstats
    assert (cstats["n_hits"], cstats["n_queries"], cstats["n_unmatched_rows"]) == (pstats["n_hits"], pstats["n_queries"], pstats["n_unmatched_rows"])
    assert pipeline.last_min_cover_stats() == {k: 0 for k in counts}     # (the last run was the one without the keyword)
    # the option made a difference: the run without it on the table as it stands is another document and another support table
    full, fstats = _run(tmp_path, "full", src, tj, fmt, headers, cfg, strategy)
    assert full["doc"] != cover["doc"] and full["support"] != cover["support"] and full["report"] != cover["report"]
    assert fstats["n_hits"] == len(rows)
    hits = lambda f: sum(int(l.split(b"\t")[3]) for l in f["support"].splitlines()[1:])
    assert hits(cover) == counts["n_kept"] and hits(full) == len(rows)   # the support table counts the kept lines
    # 100 %: the bytes of the run without the keyword
    all_of_it, astats = _run(tmp_path, "hundred", src, tj, fmt, headers, cfg, strategy, min_cover="100")
    assert all_of_it == full
    assert astats["min_cover"] == dict(counts, n_kept=len(rows), n_narrowed=0)
    # under use_taxid the numeric lineages decide, and give the same verdicts here
    if mode == "gpu" and fmt == "json":
        ncounts = ref.rewrite_table(src, str(tmp_path / "ncopy.tsv"), tj, True, 80000)
        assert ncounts == counts
        ncover, nstats = _run(tmp_path, "ncover", src, tj, fmt, headers, cfg, strategy, min_cover="80", use_taxid=True)
        nplain, _ = _run(tmp_path, "nplain", copy, tj, fmt, headers, cfg, strategy, use_taxid=True)
        assert ncover == nplain and nstats["min_cover"] == counts


@pytest.mark.parametrize("mode", ["gpu", "cpu", "host_columns"])
def test_after_the_best_hit_per_subject_and_the_band(tmp_path, monkeypatch, mode):
    """q.1: the line with the highest score (700) is of another family than the ten lines of one genus at 695 .. 699; X's second
    line (650) goes with the best hit per subject.  The 5-bit band raises the ten to 700, the top group is eleven lines, and at
    80 % (need 9) the genus covers it: the ORIGINAL top line is the one dropped.  Had the cover come before the band it would
    have seen a top group of one and done nothing — which is why its contract is stated on the table the band leaves."""
    _set(monkeypatch, mode)
    line = lambda q, acc, t, bs: f"{q}\t{acc}.1\t{ref.FIRST_TAXID + t}\t99.000\t400\t0\t0\t1\t400\t1\t400\t1e-50\t{bs}"
    rows = [line("q.1", "OUT", 200, "700.2")] + [line("q.1", f"G{k}", 8 + k % 4, str(695 + k % 5)) for k in range(10)]
    rows += [line("q.1", "G3", 9, "650"), line("q.1", "LOW", 300, "500")]
    rows += ref.make_rows(30, np.random.default_rng(212), sample_names=True)
    src, tj = _table(tmp_path, rows), ref.write_db(tmp_path / "t.json")
    c1, c2, c3 = (str(tmp_path / f"c{k}.tsv") for k in (1, 2, 3))
    scounts = subj_ref.rewrite_table(src, c1)
    bcounts = band_ref.rewrite_table(c1, c2, D=5)
    counts = ref.rewrite_table(c2, c3, tj, False, 80000)
    assert scounts[1] < scounts[0] and bcounts[1] >= 10 and counts["n_narrowed"] > 1
    kept_q1 = [l.split("\t") for l in open(c3).read().splitlines() if l.startswith("q.1\t")]
    assert len(kept_q1) == 11 and not any(f[1] == "OUT.1" for f in kept_q1) and sum(f[12] == "700" for f in kept_q1) == 10
    cfg = blast.BlastBuilder.default("/db/ref16s", "bacteria")
    got, stats = _run(tmp_path, "all", src, tj, "json", None, cfg, best_hit_per_subject=True, score_band={"top_bits": 5}, min_cover="80")
    plain, pstats = _run(tmp_path, "copy", c3, tj, "json", None, cfg)
    assert got == plain
    assert stats["min_cover"] == counts
    assert stats["subject_best"] == {"n_hits": scounts[0], "n_kept": scounts[1], "n_queries": scounts[3], "n_thinned": scounts[2]}
    assert stats["score_band"] == {"n_hits": bcounts[0], "n_raised": bcounts[1], "n_queries": bcounts[3], "n_widened": bcounts[2]}
    assert (stats["n_hits"], stats["n_unmatched_rows"]) == (pstats["n_hits"], pstats["n_unmatched_rows"])
    sup = {l.split("\t")[0]: l.split("\t") for l in got["support"].decode().splitlines()}
    assert (sup["q.1"][3], sup["q.1"][5], sup["q.1"][8]) == ("11", "10", "700")            # hits, top_hits, bit_score
    # without the band the cover sees q.1's single top line and leaves the query as it is
    alone, astats = _run(tmp_path, "noband", src, tj, "json", None, cfg, best_hit_per_subject=True, min_cover="80")
    sup = {l.split("\t")[0]: l.split("\t") for l in alone["support"].decode().splitlines()}
    assert (sup["q.1"][3], sup["q.1"][5]) == ("12", "1")


def test_strict_mode_still_fails_on_a_query_left_alone_and_lenient_writes_null(tmp_path, monkeypatch):
    _set(monkeypatch, "gpu")
    line = lambda q, acc, t, bs: f"{q}\t{acc}.1\t{t}\t99.000\t400\t0\t0\t1\t400\t1\t400\t1e-50\t{bs}"
    rows = [line("ok", f"A{k}", ref.FIRST_TAXID + 8 + k % 4, "500") for k in range(9)] + [line("ok", "OUT", ref.FIRST_TAXID + 300, "500")]
    rows += [line("lacking", f"B{k}", ref.FIRST_TAXID + 8, "500") for k in range(9)] + [line("lacking", "L", ref.LACKING_TAXID, "500")]
    src, tj = _table(tmp_path, rows), ref.write_db(tmp_path / "t.json")
    with pytest.raises(N.BluError) as e:
        pipeline.build_consensus_identities(src, tj, "bacteria", "relaxed", min_cover="80")
    assert e.value.code == 9 and "lacking" in str(e.value)               # BLU_ERR_REFERENCE_PANIC, as without the keyword
    assert pipeline.last_min_cover_stats() == {k: 0 for k in ("n_hits", "n_kept", "n_queries", "n_narrowed", "n_unresolved")}
    res, stats = pipeline.build_consensus_identities(src, tj, "bacteria", "relaxed", min_cover="80", lenient=True)
    by = {r["query"]: r["taxon"] for r in res}
    assert by["lacking"] is None and by["ok"] is not None
    assert stats["min_cover"] == {"n_hits": 20, "n_kept": 19, "n_queries": 2, "n_narrowed": 1, "n_unresolved": 1}
    plain, _ = pipeline.build_consensus_identities(src, tj, "bacteria", "relaxed", lenient=True)
    assert {r["query"]: r["taxon"] for r in plain}["ok"] != by["ok"]     # ten tied hits, one of another phylum: a higher rank


def test_through_the_command_line(tmp_path, monkeypatch, capsys):
    _set(monkeypatch, "gpu")
    rows = ref.make_rows(50, np.random.default_rng(214), sample_names=True, lacking=False)
    src, tj = _table(tmp_path, rows), ref.write_db(tmp_path / "t.json")
    c1, copy = str(tmp_path / "c1.tsv"), str(tmp_path / "copy.tsv")
    bcounts = band_ref.rewrite_table(src, c1, m=2000)
    counts = ref.rewrite_table(c1, copy, tj, False, 66667)
    assert counts["n_narrowed"] > 5 and counts["n_unresolved"] == 0
    common = ["-t", tj, "--taxon", "bacteria", "--strategy", "cautious", "--out-format", "jsonl"]
    files = {}
    for tag, table, more in (("cover", src, ["--top-percent", "2", "--min-cover", "66.667"]), ("copy", copy, [])):
        paths = {k: str(tmp_path / f"{tag}.{k}") for k in ("doc", "report", "table", "support")}
        assert cli.main(["blastn", "build-consensus", table, "--blutils-out-file", paths["doc"], "--report", paths["report"],
                         "--sample-table", paths["table"], "--support-table", paths["support"]] + common + more) == 0
        err = capsys.readouterr().err
        line = (f"min cover: kept {counts['n_kept']} of {counts['n_hits']} lines, narrowed {counts['n_narrowed']} of "
                f"{counts['n_queries']} queries, {counts['n_unresolved']} left alone")
        assert (line in err) == bool(more)
        if more:
            assert err.index(f"score band: raised {bcounts[1]} of {bcounts[0]} lines") < err.index(line)
        d = open(os.path.splitext(paths["doc"])[0] + ".jsonl", "rb").read()
        files[tag] = (RUN_ID.sub(b'"runId":""', d),) + tuple(open(paths[k], "rb").read() for k in ("report", "table", "support"))
    assert files["cover"] == files["copy"] and len(files["copy"][0]) > 5000
