"""The hit passes in composition, on the GPU (tests/pass_chain_cases.py): every subset of {best hit per subject, band,
minimum cover} under five parser settings (none, the hit filter, the taxon filter, the query cover under a permuted
`--blast-outfmt`, all three) on the three routes of the use-case — the columns the GPU ingest left on the device, the same
columns downloaded (BLU_PIPELINE_HOST_COLUMNS=1) and the host parser's (BLU_INGEST=cpu).  One test is one (subset, parser
setting, route); `json` / `jsonl`, relaxed / cautious and grouped / scrambled alternate over the subsets and parser settings,
so each value meets each route.  The rule: the run with the options gives, byte for byte, what the run without any gives on the
last copy of the chain of references — the document (file and text entry), the report, the sample table and the support
table — and every stage's counts are the references'.  The run on a copy is made once per module.  tests/test_pass_chain.py
asserts without a GPU that the table holds the queries that change their kernel class between two passes."""
import hashlib
import re

import numpy as np
import pytest

from blutils_amd import _native as N
from blutils_amd import blast, engine, pipeline
from tests import hit_filter_reference as hf
from tests import ingest_reference as ingest_ref
from tests import min_cover_reference as mc
from tests import pass_chain_cases as C

pytestmark = pytest.mark.gpu

ROUTES = {"device": {"BLU_INGEST": "gpu"}, "host_columns": {"BLU_INGEST": "gpu", "BLU_PIPELINE_HOST_COLUMNS": "1"}, "cpu": {"BLU_INGEST": "cpu"}}
PACKED_BLOCKS, F64_BLOCKS = (768, 1024), (704, 768)        # consensus_kernel.hip: BLOCK_A / BLOCK_N and BLOCK_F / BLOCK_A
FILES = ("doc", "report", "table", "support")
ZERO_COVER = {k: 0 for k in ("n_hits", "n_kept", "n_queries", "n_narrowed", "n_unresolved")}


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    return str(tmp_path_factory.mktemp("gpu_pass_chain"))


@pytest.fixture(scope="module")
def main():
    return C.main_table()


@pytest.fixture(scope="module")
def cfg():
    return blast.BlastBuilder.default("/db/ref16s", "bacteria")           # (one run id for every document)


@pytest.fixture(scope="module")
def plain_runs():
    return {}


def _set(monkeypatch, route):
    for k in ("BLU_INGEST", "BLU_PIPELINE_HOST_COLUMNS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)


def _spy(monkeypatch):
    """the selection's counts as the library wrote them, also those of the options that are off (pipeline.py shows only the others)"""
    seen = {}
    counts = pipeline._Selection.counts

    def spy(self, st):
        seen.update(hit_filter=(int(st.hit_filter.n_lines), int(st.hit_filter.n_kept)), subject_best=N.subject_counts(st.subject_best),
                    score_band=N.band_counts(st.score_band))
        return counts(self, st)

    monkeypatch.setattr(pipeline._Selection, "counts", spy)
    return seen


def _run(directory, tag, table, db, headers, cfg, fmt, strategy, count_table=None, **kw):
    """one run with every output file -> ({doc, report, table, support: bytes}, stats); the text entry gives the same document"""
    paths = {k: f"{directory}/{tag}.{k}" for k in FILES}
    common = dict(headers=headers, out_format=fmt, lenient=True, parse=False, config=cfg, **kw)
    _, stats = pipeline.build_consensus_identities_with_tables(
        table, db, "bacteria", strategy, out_path=paths["doc"], report_path=paths["report"], sample_table_path=paths["table"],
        support_table_path=paths["support"], count_table=count_table, **common)
    path = pipeline.last_ingest_path()
    files = {k: open(p, "rb").read() for k, p in paths.items()}
    text, tstats = pipeline.build_consensus_identities(table, db, "bacteria", strategy, **common)
    assert text.encode() == files["doc"]                                 # text and file entry: the same document
    timings = lambda s: {k: v for k, v in s.items() if not k.startswith("t_") and k != "count_table"}
    assert timings(tstats) == timings(stats)
    stats["ingest_path"] = path
    return files, stats


def _plain(plain_runs, directory, copy, db, headers, cfg, fmt, strategy, count_table=None):
    """the run without options on a copy, through the device route: once per distinct copy, format and strategy"""
    key = (hashlib.sha1(open(copy, "rb").read()).hexdigest(), fmt, strategy, count_table)
    if key not in plain_runs:
        plain_runs[key] = _run(directory, "plain_" + key[0][:12], copy, db, headers, cfg, fmt, strategy, count_table=count_table)
    return plain_runs[key]


def _table_counts(path):
    """n_hits, n_queries, n_unmatched_rows of a table in the reference's columns, from its bytes"""
    per = C.by_query(path)
    known = set(range(mc.FIRST_TAXID, mc.FIRST_TAXID + mc.N_TAXIDS))
    return sum(len(v) for v in per.values()), len(per), sum(int(f[2]) not in known for v in per.values() for f in v)


def _expected_counts(directory, table, order, parser, passes):
    """every stage's counts as the references give them; an option that is off: the pass-through counts of Selection::loaded"""
    stages = {s.step: s for s in C.chain(directory, table, order, parser, passes)}
    whole = C.whole_table_counts(directory, table, order)
    n0, n1 = stages["table"].n_out, stages["columns"].n_out
    n_q = len(C.by_query(stages["columns"].path))
    exp = {"hit_filter": (n0, n1) if C.PARSERS[parser] else (n1, n1)}
    n2 = stages["subject"].n_out if "subject" in stages else n1
    exp["subject_best"] = stages["subject"].counts if "subject" in stages else {"n_hits": n1, "n_kept": n1, "n_queries": n_q, "n_thinned": 0}
    exp["score_band"] = stages["band"].counts if "band" in stages else {"n_hits": n2, "n_raised": 0, "n_queries": n_q, "n_widened": 0}
    exp["min_cover"] = stages["min_cover"].counts if "min_cover" in stages else None
    exp["taxon_filter"] = {"n_lines": n0, "n_excluded": whole["n_excluded"], "n_not_only": 0, "exclude": C.EXCLUDE, "excluded_by": whole["excluded_by"]}
    exp["query_cover"] = {"n_lines": n0, "n_below": whole["n_below"], "percent": C.QUERY_COVER["percent"], "source": "qcovhsp"}
    return exp


def _check_counts(exp, stats, raw, parser, passes):
    assert raw == {k: exp[k] for k in ("hit_filter", "subject_best", "score_band")}
    if C.PARSERS[parser]:
        assert (stats["n_lines"], stats["n_kept"]) == exp["hit_filter"]
    else:
        assert "n_lines" not in stats and "n_kept" not in stats
    for key, on in (("taxon_filter", "taxon" in C.PARSERS[parser]), ("query_cover", "cover" in C.PARSERS[parser]), ("subject_best", "subject" in passes),
                    ("score_band", "band" in passes), ("min_cover", "min_cover" in passes)):
        assert (stats.get(key) == exp[key]) if on else (key not in stats), (key, stats.get(key), exp[key])
    assert pipeline.last_min_cover_stats() == (exp["min_cover"] if "min_cover" in passes else ZERO_COVER)


PARAMS = [(s, p, r) for s in range(8) for p in range(5) for r in ROUTES]
IDS = ["+".join(C.SUBSETS[s]) or "no_pass" for s in range(8)]


@pytest.mark.parametrize("s, p, route", PARAMS, ids=[f"{IDS[s]}-{list(C.PARSERS)[p]}-{r}" for s, p, r in PARAMS])
def test_the_run_with_the_options_is_the_plain_run_on_the_last_copy(directory, main, cfg, plain_runs, monkeypatch, s, p, route):
    passes, parser = C.SUBSETS[s], list(C.PARSERS)[p]
    fmt, strategy, order = ("json", "jsonl")[(s + p) % 2], ("relaxed", "cautious")[((s >> 1) + p) % 2], ("grouped", "scrambled")[((s >> 2) + p + (s & 1)) % 2]
    files = C.write(directory, main, order)
    kw = C.options(parser, passes)
    copy = C.chain(directory, main, order, parser, passes)[-1].path
    exp = _expected_counts(directory, main, order, parser, passes)
    counts_file = None
    if s == 7 and p == 4:                                                # --count-table: once per route, under everything
        counts_file = f"{directory}/counts.tsv"
        open(counts_file, "wb").write(b"#OTU ID\tA\tB\n" + b"".join(b"%s\t%d\t%d\n" % (q.split(";")[0].encode(), i % 5, 1 + i % 3) for i, q in enumerate(main.headers)))
    _set(monkeypatch, "device")
    want, pstats = _plain(plain_runs, directory, copy, files["db"], main.headers, cfg, fmt, strategy, counts_file)
    assert pstats["ingest_path"] == "gpu"
    _set(monkeypatch, route)
    raw = _spy(monkeypatch)
    got, stats = _run(directory, f"run_{s}_{p}_{route}", files["perm" if "blast_outfmt" in kw else "base"], files["db"], main.headers, cfg, fmt,
                      strategy, count_table=counts_file, **kw)
    assert stats["ingest_path"] == ("cpu" if route == "cpu" else "gpu")
    for k in FILES:
        assert got[k] == want[k], k
    assert len(want["doc"]) > 100000 and want["support"].count(b"\n") == len(main.headers) + 1
    _check_counts(exp, stats, raw, parser, passes)
    assert (stats["n_hits"], stats["n_queries"], stats["n_unmatched_rows"]) == (pstats["n_hits"], pstats["n_queries"], pstats["n_unmatched_rows"]) == _table_counts(copy)
    if counts_file:
        assert stats["count_table"] == pstats["count_table"] and stats["count_table"]["n_rows"] == len(main.headers)
    if kw:                                                               # the options made a difference: another document, another support table
        none, _ = _plain(plain_runs, directory, files["base"], files["db"], main.headers, cfg, fmt, strategy, counts_file)
        assert got["doc"] != none["doc"] and got["support"] != none["support"]


def _query_columns(t):
    """{query name: its rows}, the accession rank spelled out"""
    seg, out = t["seg_off"].astype(np.int64), {}
    for q, name in enumerate(t["query_names"]):
        r = slice(seg[q], seg[q + 1])
        out[name] = (t["bitscore"][r].tolist(), t["align_len"][r].tolist(), t["tax_desc_row"][r].tolist(), [t["accessions"][k] for k in t["acc_rank"][r]],
                     t["pident"][r].view(np.uint64).tolist())
    return out


@pytest.mark.parametrize("parser", list(C.PARSERS))
@pytest.mark.parametrize("s", range(4), ids=IDS[:4])
def test_the_columns_are_those_of_the_copy(directory, main, monkeypatch, s, parser):
    """blu_ingest_columns* under each subset of {best hit per subject, band} and each parser setting: the independent reading of the
    chain's copy — a grouped file byte for byte, a scrambled one query by query (the numbering is the table's)"""
    _set(monkeypatch, "device")
    passes = C.SUBSETS[s]
    kw = C.options(parser, passes)
    for order in ("grouped", "scrambled"):
        files = C.write(directory, main, order)
        stages = C.chain(directory, main, order, parser, passes)
        exp = ingest_ref.read_table(stages[-1].path, files["db"])
        got = pipeline.ingest_columns(files["perm" if "blast_outfmt" in kw else "base"], files["db"], device=0, **kw)
        assert pipeline.last_ingest_path() == "gpu"
        if order == "grouped":
            hf.assert_columns_equal(got, exp)
        else:
            assert _query_columns(got) == _query_columns(exp) and got["accessions"] == exp["accessions"]
            if "subject" not in passes:
                hf.assert_columns_equal(got, exp)
        counts = _expected_counts(directory, main, order, parser, passes)
        for key in ("subject_best", "score_band"):
            assert (got.get(key) == counts[key]) if ("subject" if key == "subject_best" else "band") in passes else key not in got


def test_the_identity_route_follows_the_rows_the_passes_leave(directory, cfg, monkeypatch):
    """One row with a fourth decimal or with 131.071 keeps the whole table off the packed records (engine_dev.hip:
    pack_side_records) — unless the subject pass or the cover deletes it first.  The run with the options and the run on the copy
    take the same build of the stream kernel: the packed one where the row is deleted, the f64 one where it is kept."""
    _set(monkeypatch, "device")
    block = {}
    for value in C.IDENTITY_VALUES:
        for variant in C.IDENTITY_VARIANTS:
            t = C.identity_table(value, variant)
            files = C.write(directory, t)
            copy = C.chain(directory, t, "grouped", "none", C.PASSES)[-1].path
            got, stats = _run(directory, "identity_run", files["base"], files["db"], t.headers, cfg, "json", "relaxed", **C.options("none", C.PASSES))
            b_run = engine.last_launch()[2]
            want, _ = _run(directory, "identity_copy", copy, files["db"], t.headers, cfg, "json", "relaxed")
            b_copy = engine.last_launch()[2]
            assert stats["ingest_path"] == "gpu" and got == want
            block[value, variant] = (b_run, b_copy)
    print("[pass chain] identity routes: block sizes", block)
    for (value, variant), (b_run, b_copy) in block.items():
        assert b_run == b_copy, (value, variant, block)
        assert b_run in (F64_BLOCKS if variant == "kept" else PACKED_BLOCKS), (value, variant, block)
        assert variant == "kept" or b_run != block[value, "kept"][0], (value, variant, block)       # (one table shape: the builds differ in block size)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("parser", ["hit", "taxon", "cover", "all"])
def test_a_table_the_parser_erases(directory, cfg, monkeypatch, plain_runs, parser, route):
    """every line goes: the headers without a taxon, nothing else, and the counts of an empty table"""
    t = C.erased_table()
    files = C.write(directory, t)
    copy = C.chain(directory, t, "grouped", parser, C.PASSES)[-1].path
    assert open(copy, "rb").read() == b""
    kw = C.options(parser, C.PASSES)
    _set(monkeypatch, route)
    raw = _spy(monkeypatch)
    got, stats = _run(directory, f"erased_{parser}_{route}", files["perm" if "blast_outfmt" in kw else "base"], files["db"], t.headers, cfg, "jsonl", "relaxed", **kw)
    n0 = C.n_lines(files["base"])
    assert raw == {"hit_filter": (n0, 0), "subject_best": {"n_hits": 0, "n_kept": 0, "n_queries": 0, "n_thinned": 0},
                   "score_band": {"n_hits": 0, "n_raised": 0, "n_queries": 0, "n_widened": 0}}
    assert stats["min_cover"] == ZERO_COVER and (stats["n_hits"], stats["n_queries"], stats["n_unmatched_rows"]) == (0, 0, 0)
    _set(monkeypatch, "device")
    want, _ = _plain(plain_runs, directory, copy, files["db"], t.headers, cfg, "jsonl", "relaxed")
    assert got == want
    records = got["doc"].decode().splitlines()[1:]
    assert len(records) == len(t.headers) and all(re.search(r'"taxon": ?null', r) for r in records)
