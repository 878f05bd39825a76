"""The bit-score band end to end.  The rule: a run with a band gives, byte for byte, what the run without one
gives on the copy of the (filtered) table in which tests/score_band_reference.py replaced column 12 of every in-band line by
its query's top score — the document, the report, the per-sample table and the support table, through either parser, the
host-column path, both entry forms and the command line."""
import json
import os
import re
import stat
import sys

import numpy as np
import pytest

from blutils_amd import blast, cli, pipeline
from tests import hit_filter_reference as hf
from tests import score_band_reference as ref

pytestmark = pytest.mark.gpu

MODES = {"gpu": {"BLU_INGEST": "gpu"}, "cpu": {"BLU_INGEST": "cpu"},
         "host_columns": {"BLU_INGEST": "gpu", "BLU_PIPELINE_HOST_COLUMNS": "1"}}
BANDS = {"percent": (dict(top_percent="1"), dict(m=1000)), "bits": (dict(top_bits=2), dict(D=2)),
         "both": (dict(top_percent="0.5", top_bits=3), dict(m=500, D=3))}
RUN_ID = re.compile(rb'"runId":\s*"[0-9a-f-]{36}"')


def _set(monkeypatch, mode):
    monkeypatch.delenv("BLU_PIPELINE_HOST_COLUMNS", raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)


def make_rows(n_q, rng, sample_names=False, hits=8):
    """BLAST-shaped lines whose scores crowd under each query's top: differences of 0 .. 100 bits under tops of 100 .. 3000,
    a third of them written with a decimal (truncated away by the parser), over the species of a genus and its neighbours."""
    rows = []
    for q in range(n_q):
        name = f"s{q % 3}.{q}" if sample_names else f"q{q:06d}"
        top, g = int(rng.integers(100, 3000)), int(rng.integers(1, 420))
        for j in range(int(rng.integers(1, hits + 1))):
            t = min(2999, 7 * g + int(rng.integers(-3, 10)))
            b = top - int(rng.choice([0, 0, 1, 1, 2, 3, 5, 10, 30, 100]))
            text = f"{b}.{int(rng.integers(0, 10))}" if j % 3 == 0 else str(b)
            rows.append(f"{name}\tNR_{t:06d}.1\t{100 + t}\t{97 + int(rng.integers(0, 3001)) / 1000:.3f}\t{int(rng.integers(300, 500))}"
                        f"\t1\t0\t1\t400\t1\t400\t1e-{int(rng.integers(50, 150))}\t{text}")
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


def _band_stats(counts):
    n_kept, n_raised, n_widened, n_q = counts
    return {"n_hits": n_kept, "n_raised": n_raised, "n_queries": n_q, "n_widened": n_widened}


@pytest.mark.parametrize("mode,fmt,layout,band", [("gpu", "json", "grouped", "percent"), ("gpu", "jsonl", "scrambled", "both"),
                                                  ("cpu", "jsonl", "grouped", "bits"), ("cpu", "json", "scrambled", "percent"),
                                                  ("host_columns", "json", "scrambled", "bits"),
                                                  ("host_columns", "jsonl", "grouped", "both")])
def test_every_output_is_that_of_the_rewritten_copy(tmp_path, monkeypatch, mode, fmt, layout, band):
    _set(monkeypatch, mode)
    rng = np.random.default_rng(81)
    rows = make_rows(60, rng, sample_names=True)
    if layout == "scrambled":                                            # queries not contiguous: the GPU ingest's radix-sort path
        rows = hf.scramble(rows, rng)
    src, tj = _table(tmp_path, rows), hf.write_db(tmp_path / "t.json")
    given, restated = BANDS[band]
    copy = str(tmp_path / "copy.tsv")
    counts = ref.rewrite_table(src, copy, **restated)
    assert counts[0] == len(rows) and 0 < counts[1] < len(rows) and 0 < counts[2] < counts[3] == 60
    headers = sorted({r.split("\t")[0] for r in rows}) + ["s1.777777", "s0.888888"]      # two FASTA ids without a hit
    cfg = blast.BlastBuilder.default("/db/ref16s", "bacteria")           # (one run id for every document)
    banded, bstats = _run(tmp_path, "band", src, tj, fmt, headers, cfg, score_band=pipeline.ScoreBand(**given))
    assert pipeline.last_ingest_path() == ("cpu" if mode == "cpu" else "gpu")
    plain, pstats = _run(tmp_path, "copy", copy, tj, fmt, headers, cfg)
    assert banded == plain
    assert bstats["score_band"] == _band_stats(counts) and "score_band" not in pstats
    # the band made a difference: the run without it on the table as it stands is another document and another support table
    exact, _ = _run(tmp_path, "exact", src, tj, fmt, headers, cfg)
    assert exact["doc"] != banded["doc"] and exact["support"] != banded["support"]
    top_hits = lambda f: sum(int(l.split(b"\t")[5]) for l in f["support"].splitlines()[1:])
    assert top_hits(banded) == top_hits(exact) + counts[1]               # top_hits is the band's size
    assert b"s1.777777\t-\tunclassified\t0\t0\t0" in banded["support"]


@pytest.mark.parametrize("mode", ["gpu", "cpu"])
def test_columns_are_those_of_the_rewritten_copy(tmp_path, monkeypatch, mode):
    _set(monkeypatch, mode)
    rng = np.random.default_rng(82)
    rows = hf.scramble(make_rows(80, rng), rng)
    src, tj = _table(tmp_path, rows), hf.write_db(tmp_path / "t.json")
    for given, restated in BANDS.values():
        copy = str(tmp_path / "copy.tsv")
        counts = ref.rewrite_table(src, copy, **restated)
        got = pipeline.ingest_columns(src, tj, device=0, score_band=given)
        assert pipeline.last_ingest_path() == mode
        exp = pipeline.ingest_columns(copy, tj, device=0)
        hf.assert_columns_equal(got, exp)
        assert got["score_band"] == _band_stats(counts) and counts[1] > 0
    # no criterion: the call without a band
    assert "score_band" not in pipeline.ingest_columns(src, tj, device=0, score_band=pipeline.ScoreBand())


@pytest.mark.parametrize("mode", ["gpu", "cpu"])
def test_the_band_hangs_from_the_top_the_filters_leave(tmp_path, monkeypatch, mode):
    """The band comes after the filters.  a.1's top line (700.5 bits, species s5, 98 % identity) goes under an identity threshold
    or a taxon filter: the band then hangs from 640 and 639 joins it.  (--min-bit-score keeps the scores at or above its
    threshold, so it cannot take a top line and leave a lower one; what it can take is a line of the band: a.2's 639.9.)"""
    _set(monkeypatch, mode)
    line = lambda q, taxid, bs, pid="99.000": f"{q}\tA{taxid}.1\t{taxid}\t{pid}\t400\t0\t0\t1\t400\t1\t400\t1e-50\t{bs}"
    rows = [line("a.1", 105, "700.5", "98.000"), line("a.1", 106, "640"), line("a.1", 107, "639"), line("a.1", 108, "600"),
            line("a.2", 120, "640.2"), line("a.2", 121, "639.9"), line("a.2", 122, "639.1"), line("a.2", 123, "100")]
    rows += make_rows(30, np.random.default_rng(83), sample_names=True)
    src, tj = _table(tmp_path, rows), hf.write_db(tmp_path / "t.json")
    fields = [r.split("\t") for r in rows]
    cfg = blast.BlastBuilder.default("/db/ref16s", "bacteria")
    no_s5 = [f[2] != "105" for f in fields]
    # (per case: the filters, the kept-line verdicts, a.1's and a.2's expected hits / top_hits / bit_score in the support table)
    cases = [("identity", dict(hit_filter={"min_perc_identity": 98.5}), [hf.keep(f, {"min_perc_identity": 98.5}) for f in fields],
              ("3", "2", "640"), ("4", "3", "640")),
             ("min_bit_score", dict(hit_filter={"min_bit_score": 639.5}), [hf.keep(f, {"min_bit_score": 639.5}) for f in fields],
              ("2", "1", "700"), ("2", "2", "640")),
             ("taxon", dict(taxon_filter={"exclude": ["s__s5"]}), no_s5, ("3", "2", "640"), ("4", "3", "640")),
             ("both", dict(hit_filter={"min_bit_score": 639.5}, taxon_filter={"exclude": ["s__s5"]}),
              [a and hf.keep(f, {"min_bit_score": 639.5}) for a, f in zip(no_s5, fields)], ("1", "1", "640"), ("2", "2", "640")),
             ("none", {}, None, ("4", "1", "700"), ("4", "3", "640"))]
    for tag, extra, kept, first, second in cases:
        copy = str(tmp_path / f"copy_{tag}.tsv")
        counts = ref.rewrite_table(src, copy, D=1, kept=kept)
        banded, bstats = _run(tmp_path, f"band_{tag}", src, tj, "json", None, cfg, score_band=pipeline.ScoreBand(top_bits=1), **extra)
        plain, _ = _run(tmp_path, f"copy_{tag}", copy, tj, "json", None, cfg)
        assert banded == plain, tag
        assert bstats["score_band"] == _band_stats(counts), tag
        sup = {l.split("\t")[0]: l.split("\t") for l in banded["support"].decode().splitlines()}
        assert (sup["a.1"][3], sup["a.1"][5], sup["a.1"][8]) == first, tag
        assert (sup["a.2"][3], sup["a.2"][5], sup["a.2"][8]) == second, tag


def test_the_case_the_band_exists_for(tmp_path, monkeypatch, capsys):
    """Two species of one genus at 500 and 499 bits: a single-match species call today, a call from both hits under --top-bits 1."""
    _set(monkeypatch, "gpu")
    line = lambda q, taxid, bs: f"{q}\tA{taxid}.1\t{taxid}\t100.000\t400\t0\t0\t1\t400\t1\t400\t1e-50\t{bs}"
    rows = [line("q", 114, "500"), line("q", 115, "499")]                # taxids 114, 115: species s14, s15 of genus g2
    src, tj = _table(tmp_path, rows), hf.write_db(tmp_path / "t.json")
    copy = str(tmp_path / "copy.tsv")
    assert ref.rewrite_table(src, copy, D=1) == (2, 1, 1, 1)
    assert open(copy).read().splitlines()[1].endswith("\t500")
    kw = dict(out_format="json", lenient=False)
    today, _ = pipeline.build_consensus_identities(src, tj, "bacteria", "relaxed", **kw)
    banded, stats = pipeline.build_consensus_identities(src, tj, "bacteria", "relaxed", score_band={"top_bits": 1}, **kw)
    of_copy, _ = pipeline.build_consensus_identities(copy, tj, "bacteria", "relaxed", **kw)
    t, b, c = today[0]["taxon"], banded[0]["taxon"], of_copy[0]["taxon"]
    assert t["singleMatch"] is True and t["reachedRank"] == "species" and t["identifier"] == "s14"
    assert b == c and b != t
    assert b["singleMatch"] is False and b["reachedRank"] != "species" and b["bitScore"] == t["bitScore"] == 500.0
    assert stats["score_band"] == {"n_hits": 2, "n_raised": 1, "n_queries": 1, "n_widened": 1}
    # zero widths are today's exact ties: the bytes of the run without the flag, with the count line on stderr
    cfg = blast.BlastBuilder.default("/db/ref16s", "bacteria")
    raw = lambda **extra: pipeline.build_consensus_identities(src, tj, "bacteria", "relaxed", parse=False, config=cfg, **extra)[0]
    assert raw(score_band={"top_percent": "0"}) == raw(score_band={"top_bits": 0}) == raw(score_band={"top_percent": "0.000", "top_bits": 0}) == raw()
    assert raw(score_band={"top_bits": 1}) != raw()
    # through the command line
    capsys.readouterr()
    base = ["blastn", "build-consensus", "-t", tj, "--taxon", "bacteria", "--strategy", "relaxed"]
    outs = {}
    for tag, argv in (("today", [src]), ("zero", [src, "--top-percent", "0", "--top-bits", "0"]), ("band", [src, "--top-bits", "1"]),
                      ("percent", [src, "--top-percent", "0.2"]), ("copy", [copy])):
        assert cli.main(base + argv) == 0
        cap = capsys.readouterr()
        outs[tag] = (RUN_ID.sub(b'"runId":""', cap.out.encode()), cap.err)
    assert outs["zero"][0] == outs["today"][0] and outs["band"][0] == outs["percent"][0] == outs["copy"][0] != outs["today"][0]
    assert "score band" not in outs["today"][1] and "score band" not in outs["copy"][1]
    assert "score band: raised 0 of 2 lines in 0 of 1 queries" in outs["zero"][1]
    assert "score band: raised 1 of 2 lines in 1 of 1 queries" in outs["band"][1]
    assert "score band: raised 1 of 2 lines in 1 of 1 queries" in outs["percent"][1]    # 499 * 100000 >= 500 * 99800


def test_cli_files_and_the_count_line_after_the_filter_lines(tmp_path, monkeypatch, capsys):
    _set(monkeypatch, "gpu")
    rng = np.random.default_rng(84)
    rows = make_rows(50, rng, sample_names=True)
    src, tj = _table(tmp_path, rows), hf.write_db(tmp_path / "t.json")
    flt = {"min_perc_identity": 97.5}
    kept = [hf.keep(r.split("\t"), flt) for r in rows]
    copy = str(tmp_path / "copy.tsv")
    counts = ref.rewrite_table(src, copy, m=1500, D=20, kept=kept)
    assert 0 < counts[1] and counts[0] < len(rows)
    common = ["-t", tj, "--taxon", "bacteria", "--strategy", "cautious", "--out-format", "jsonl"]
    files = {}
    for tag, table, more in (("band", src, ["--min-perc-identity", "97.5", "--top-percent", "1.5", "--top-bits", "20"]), ("copy", copy, [])):
        paths = {k: str(tmp_path / f"{tag}.{k}") for k in ("doc", "report", "table", "support")}
        assert cli.main(["blastn", "build-consensus", table, "--blutils-out-file", paths["doc"], "--report", paths["report"],
                         "--sample-table", paths["table"], "--support-table", paths["support"]] + common + more) == 0
        err = capsys.readouterr().err
        line = f"score band: raised {counts[1]} of {counts[0]} lines in {counts[2]} of {counts[3]} queries"
        assert (line in err) == bool(more)
        if more:
            assert err.index(f"hit filter: kept {counts[0]} of {len(rows)} lines") < err.index(line)
        d = open(os.path.splitext(paths["doc"])[0] + ".jsonl", "rb").read()
        files[tag] = (RUN_ID.sub(b'"runId":""', d),) + tuple(open(paths[k], "rb").read() for k in ("report", "table", "support"))
    assert files["band"] == files["copy"] and len(files["copy"][0]) > 5000


def test_run_with_consensus_passes_the_band_through(tmp_path, monkeypatch, capsys):
    """FASTA -> stand-in `blastn` executable -> the table written as it is -> consensus under the band."""
    _set(monkeypatch, "gpu")
    rng = np.random.default_rng(85)
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
    counts = ref.rewrite_table(bt, copy, m=2000)
    sup = tmp_path / "support.tsv"
    argv = ["blastn", "run-with-consensus", str(fa), "-d", str(tmp_path / "db" / "ref16s"), "-t", tj, "--blast-out-file",
            str(tmp_path / "work" / "hits.tsv"), "--blutils-out-file", str(tmp_path / "res" / "consensus.json"), "--taxon", "bacteria",
            "--strategy", "relaxed", "--threads", "2", "--blastn", str(exe), "--top-percent", "2", "--support-table", str(sup)]
    assert cli.main(argv) == 0
    assert f"score band: raised {counts[1]} of {counts[0]} lines in {counts[2]} of {counts[3]} queries" in capsys.readouterr().err
    assert counts[1] > 0
    assert sorted(open(tmp_path / "work" / "hits.out").read().splitlines()) == sorted(rows)      # the BLAST table: as blastn wrote it
    doc = json.load(open(tmp_path / "res" / "consensus.json"))
    by = {r["query"]: r["taxon"] for r in doc["results"]}
    assert by["fasta_only"] is None and len(by) == 41
    exp, _ = pipeline.build_consensus_identities(copy, tj, "bacteria", "relaxed", lenient=False)
    assert all(by[r["query"]] == r["taxon"] for r in exp)
    sup_copy = tmp_path / "support_copy.tsv"
    pipeline.build_consensus_identities_with_tables(copy, tj, "bacteria", "relaxed", headers=["fasta_only"], out_path=str(tmp_path / "c.json"),
                                                    support_table_path=str(sup_copy))
    assert sup.read_bytes() == sup_copy.read_bytes()


def test_several_million_lines(tmp_path, monkeypatch):
    """3 M lines, 669 000 queries: tens of thousands of blocks add to the 64 spread counter words.  The expected column and
    counts come from the block the table repeats (the restatement reads 13 000 lines, not 3 M)."""
    _set(monkeypatch, "gpu")
    rng = np.random.default_rng(86)
    block = make_rows(3000, rng)
    reps = 3_000_000 // len(block) + 1
    seg, scores, last = [0], [], None
    for r in block:
        f = r.split("\t")
        if last is not None and f[0] != last:
            seg.append(len(scores))
        last = f[0]
        scores.append(ref.truncated(f[12]))
    seg.append(len(scores))
    exp, n_raised, n_widened = ref.raise_scores(seg, scores, m=1000, D=4)
    assert n_raised > 1000
    src = tmp_path / "big.tsv"
    with open(src, "wb") as f:
        body = ("\n".join(block) + "\n").encode()
        for r in range(reps):
            f.write(body.replace(b"q00", b"r%03d_" % r))                 # the queries of every repetition are new ones
    tj = hf.write_db(tmp_path / "t.json")
    got = pipeline.ingest_columns(str(src), tj, device=0, score_band={"top_percent": "1.000", "top_bits": 4})
    assert pipeline.last_ingest_path() == "gpu"
    assert got["score_band"] == {"n_hits": len(block) * reps, "n_raised": n_raised * reps, "n_queries": 3000 * reps,
                                 "n_widened": n_widened * reps} and got["score_band"]["n_hits"] >= 3_000_000
    assert np.array_equal(got["bitscore"], np.tile(np.array(exp, np.int32), reps))
    # and the whole use-case on the device path agrees with the counts (the column never leaves the device there)
    _, stats = pipeline.build_consensus_identities(str(src), tj, "bacteria", "relaxed", out_format="jsonl", lenient=True,
                                                   out_path=str(tmp_path / "big.jsonl"), score_band={"top_percent": "1", "top_bits": 4})
    assert stats["score_band"] == got["score_band"]
