"""`build-distances` on the host: the feature rule and the rendering through blu_distance_features_from_table
and blu_distance_render, against the restatement in tests/distance_reference.py; the CLI's argument errors.  No GPU."""
import ctypes as C
import gzip
import json
import os

import pytest

from blutils_amd import _native as N
from blutils_amd import cli, distance, pipeline
from tests import distance_reference as ref

HEAD = "#rank\tidentifier\ttaxonomy\ttotal"


def _table(samples, rows):
    """rows: (rank, identifier, taxonomy, cells) -> the table's text; total is the cells' sum"""
    out = [HEAD + "".join("\t" + s for s in samples)]
    for rank, ident, tax, cells in rows:
        out.append("\t".join([rank, ident, tax, str(sum(cells))] + [str(c) for c in cells]))
    return "\n".join(out) + "\n"


# d__B ─ p__P ─ g__G1 ─ s__x ─ g__Gin (a g under a g) ; p__P ─ s__skip (a branch without g) ; d__B ─ p__Q (ends above g);
# d__A: all zero.  Three samples; S3 is empty.
ROWS = [
    ("-", "unclassified", "", [5, 0, 0]),
    ("-", "unplaced", "", [1, 2, 0]),
    ("d", "B", "d__B", [40, 31, 0]),
    ("p", "P", "d__B;p__P", [30, 25, 0]),
    ("g", "G1", "d__B;p__P;g__G1", [20, 10, 0]),
    ("s", "x", "d__B;p__P;g__G1;s__x", [12, 10, 0]),
    ("g", "Gin", "d__B;p__P;g__G1;s__x;g__Gin", [7, 0, 0]),
    ("s", "skip", "d__B;p__P;s__skip", [6, 9, 0]),
    ("p", "Q", "d__B;p__Q", [8, 0, 0]),
    ("d", "A", "d__A", [0, 0, 0]),
]
SAMPLES = ["S1", "S2", "S3"]


def _features(tmp_path, text, rank=None, drop=False):
    p = tmp_path / "table.tsv"
    p.write_text(text)
    got = distance.features_from_table(str(p), rank, drop)
    rp, sm, ct = got["row_ptr"].tolist(), got["sample"].tolist(), got["count"].tolist()
    cells = []
    for k in range(len(rp) - 1):
        row = [0] * len(got["samples"])
        for e in range(rp[k], rp[k + 1]):
            row[sm[e]] = ct[e]
        assert sm[rp[k]:rp[k + 1]] == sorted(set(sm[rp[k]:rp[k + 1]])) and all(ct[rp[k]:rp[k + 1]])
        cells.append(row)
    return got["samples"], list(zip(got["features"], cells)), got["n_dropped"]


def _same(tmp_path, text, rank=None, drop=False):
    got = _features(tmp_path, text, rank, drop)
    names, feats, dropped = ref.features(text, rank, drop)
    assert got == (names, [(t, list(c)) for t, c in feats], dropped)
    return dict(got[1]), got[2]


def test_symbols_struct_sizes_and_constants():
    L = N.lib()
    assert {"blu_sample_distances", "blu_sample_distance_free"} <= set(N.EXPORTS)
    for name in ("blu_distance_features_from_table", "blu_distance_features_free", "blu_distance_render", "blu_distance_matrix_file"):
        assert name in N.PIPELINE_EXPORTS and hasattr(L, name)
    assert C.sizeof(N.DistanceDesc) == 56 and C.sizeof(N.SampleDistance) == 48
    assert C.sizeof(pipeline.DistanceFeatures) == 64 and C.sizeof(pipeline.DistanceStats) == 32
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "blu_consensus.h")).read()
    assert f"#define BLU_DISTANCE_MAX_SAMPLES {N.DISTANCE_MAX_SAMPLES}u" in header
    assert f"#define BLU_DISTANCE_CHUNK {N.DISTANCE_CHUNK}u" in header and f"#define BLU_DISTANCE_PARTNERS {N.DISTANCE_PARTNERS}u" in header
    assert C.sizeof(pipeline.ConsensusRequest) == 136 and C.sizeof(pipeline.ConsensusExtras) == 24 and L.blu_abi_version() == 5


def test_rank_g_outermost_wins_skipped_branches_and_queries_above(tmp_path):
    feats, dropped = _same(tmp_path, _table(SAMPLES, ROWS), "g")
    assert feats == {
        "unclassified": [5, 0, 0], "unplaced": [1, 2, 0],
        "d__B": [2, 6, 0],                      # queries that ended at the domain: direct counts
        "d__B;p__P": [4, 6, 0],                 # ended at the phylum
        "d__B;p__P;g__G1": [20, 10, 0],         # the outermost g with its clade: s__x and the inner g__Gin are in it
        "d__B;p__P;s__skip": [6, 9, 0],         # a branch that skips g
        "d__B;p__Q": [8, 0, 0],
    }
    assert dropped == 1                          # d__A


def test_genus_is_g_and_other_spellings(tmp_path):
    text = _table(SAMPLES, ROWS)
    a = _features(tmp_path, text, "g")
    assert a == _features(tmp_path, text, "genus") == _features(tmp_path, text, " Genus ")
    assert _features(tmp_path, text, "species") == _features(tmp_path, text, "s") != a


def test_no_rank_is_every_row_by_its_direct_counts(tmp_path):
    feats, dropped = _same(tmp_path, _table(SAMPLES, ROWS))
    assert feats["d__B;p__P;g__G1"] == [8, 0, 0] and feats["d__B;p__P;g__G1;s__x"] == [5, 10, 0]
    assert feats["d__B;p__P;g__G1;s__x;g__Gin"] == [7, 0, 0] and "d__A" not in feats and dropped == 1


@pytest.mark.parametrize("rank", [None, "g", "s", "p", "d"])
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("with_unplaced", [True, False])
def test_sum_invariant_unplaced_and_drop_unclassified(tmp_path, rank, drop, with_unplaced):
    rows = [r for r in ROWS if with_unplaced or r[1] != "unplaced"]
    feats, _ = _same(tmp_path, _table(SAMPLES, rows), rank, drop)
    assert ("unclassified" in feats) == (not drop) and ("unplaced" in feats) == (with_unplaced and not drop)
    top = [40, 31, 0]
    fixed = [0, 0, 0] if drop else ([6, 2, 0] if with_unplaced else [5, 0, 0])
    assert [sum(c[s] for c in feats.values()) for s in range(3)] == [t + f for t, f in zip(top, fixed)]


def test_an_all_zero_fixed_row_is_dropped_too(tmp_path):
    rows = [("-", "unclassified", "", [0, 0, 0])] + ROWS[2:]
    feats, dropped = _same(tmp_path, _table(SAMPLES, rows), "g")
    assert "unclassified" not in feats and "unplaced" not in feats and dropped == 3


def _refused(tmp_path, text, line, rank=None, code=8):                 # (BLU_ERR_PARSE)
    p = tmp_path / "bad.tsv"
    p.write_text(text)
    with pytest.raises(N.BluError) as e:
        distance.features_from_table(str(p), rank)
    assert e.value.code == code
    if line is not None:
        assert f"line {line}:" in str(e.value), str(e.value)
        with pytest.raises(ref.Malformed) as r:
            ref.features(text, rank)
        assert r.value.line == line
    return str(e.value)


def test_refusals_name_the_line(tmp_path):
    good = _table(SAMPLES, ROWS)
    lines = good.splitlines()
    # a negative direct count: the children of d__B;p__P (line 5) pass it in S2
    rows = list(ROWS)
    rows[3] = ("p", "P", "d__B;p__P", [30, 18, 0])
    rows[2] = ("d", "B", "d__B", [40, 31, 0])
    assert "negative direct" in _refused(tmp_path, _table(SAMPLES, rows), 5)
    # a missing parent: d__B;p__P removed, its children (first: line 5) hang
    assert "parent" in _refused(tmp_path, "\n".join(lines[:4] + lines[5:]) + "\n", 5)
    # a short line (a cell less), a long one
    short = lines[:6] + [lines[6].rsplit("\t", 1)[0]] + lines[7:]
    assert "cells" in _refused(tmp_path, "\n".join(short) + "\n", 7)
    assert "cells" in _refused(tmp_path, "\n".join(lines[:6] + [lines[6] + "\t0"] + lines[7:]) + "\n", 7)
    # a wrong total
    cells = lines[8].split("\t")
    cells[3] = str(int(cells[3]) + 1)
    assert "total" in _refused(tmp_path, "\n".join(lines[:8] + ["\t".join(cells)] + lines[9:]) + "\n", 9)
    # a cell that is no number
    assert "whole number" in _refused(tmp_path, good.replace("\t12\t10\t0", "\t12\t1x\t0"), 7)
    # a rank no row carries: named, BLU_ERR_INVALID_ARG
    msg = _refused(tmp_path, good, None, rank="family", code=N.BLU_ERR_INVALID_ARG)
    assert "family" in msg
    with pytest.raises(ref.Malformed, match="family"):
        ref.features(good, "family")
    # no header
    assert "header" in _refused(tmp_path, "\n".join(lines[1:]) + "\n", 1)


# ---- rendering ------------------------------------------------------------------------------------------------------------

def _render(tmp_path, metric, names, total, rich, min_sum, shared):
    out = tmp_path / f"{metric}.tsv"
    distance.render(metric, names, total, rich, min_sum, shared, str(out))
    text = out.read_text()
    assert text == ref.render(metric, names, total, rich, min_sum, shared)
    return [l.split("\t") for l in text.splitlines()]


def test_render_identical_disjoint_and_empty_samples(tmp_path):
    # A == B, C disjoint from both, E empty
    cols = [{0: 3, 1: 4}, {0: 3, 1: 4}, {2: 9}, {}]
    names = ["A", "B", "C", "E"]
    ints = ref.integers_dense(cols)
    for metric in ("bray-curtis", "jaccard"):
        m = _render(tmp_path, metric, names, *ints)
        assert m[0] == [""] + names and [r[0] for r in m[1:]] == names
        assert m[1][1] == m[1][2] == m[2][1] == "0.000000"
        assert m[1][3] == m[3][1] == m[2][3] == "1.000000"
        assert m[4][4] == "nan" and m[1][4] == m[4][1] == "1.000000" and m[3][3] == "0.000000"


def test_render_rounds_half_up_in_integers(tmp_path):
    # N = 4 000 000, C = 1 999 999: (N - 2C) / N = 0.0000005 -> 0.000001
    total = [2_000_000, 2_000_000]
    m = _render(tmp_path, "bray-curtis", ["a", "b"], total, [1, 1], [[2_000_000, 1_999_999], [1_999_999, 2_000_000]], [[1, 1], [1, 1]])
    assert m[1][2] == m[2][1] == "0.000001"
    # just under the tie: N = 4 000 002, C = 2 000 000 -> 2 / 4 000 002 = 0.00000049999... -> 0.000000
    total = [2_000_001, 2_000_001]
    m = _render(tmp_path, "bray-curtis", ["a", "b"], total, [1, 1], [[2_000_001, 2_000_000], [2_000_000, 2_000_001]], [[1, 1], [1, 1]])
    assert m[1][2] == "0.000000"
    # jaccard tie: U = 2 000 000, I = 1 999 999 -> 1 / 2 000 000 = 0.0000005 -> 0.000001
    rich = [2_000_000, 1_999_999]
    m = _render(tmp_path, "jaccard", ["a", "b"], [1, 1], rich, [[1, 1], [1, 1]], [[2_000_000, 1_999_999], [1_999_999, 1_999_999]])
    assert m[1][2] == "0.000001"


def test_render_totals_above_2_53(tmp_path):
    # doubles cannot tell these apart: N = 2^62 + 2^61 + 2, C = 2^61 and 2^61 + 1
    a, b = (1 << 62) + 1, (1 << 61) + 1
    for c in ((1 << 61) - 3, (1 << 61) + 1):
        m = _render(tmp_path, "bray-curtis", ["a", "b"], [a, b], [5, 5], [[a, c], [c, b]], [[5, 5], [5, 5]])
        n = a + b
        q = ((n - 2 * c) * 10 ** 6 + n // 2) // n
        assert m[1][2] == f"0.{q:06d}"
    # (2^63 - 1) twice: N = 2^64 - 2 still fits
    t = (1 << 63) - 1
    m = _render(tmp_path, "bray-curtis", ["a", "b"], [t, t], [1, 1], [[t, 1], [1, t]], [[1, 1], [1, 1]])
    assert m[1][2] == "1.000000" and m[1][1] == "0.000000"


def test_render_refuses_integers_that_cannot_be(tmp_path):
    out = str(tmp_path / "x.tsv")
    with pytest.raises(N.BluError, match="min_sum"):
        distance.render("bray-curtis", ["a", "b"], [1, 1], [1, 1], [[1, 2], [2, 1]], [[1, 1], [1, 1]], out)
    with pytest.raises(N.BluError, match="shared"):
        distance.render("jaccard", ["a", "b"], [1, 1], [1, 1], [[1, 1], [1, 1]], [[1, 2], [2, 1]], out)
    with pytest.raises(ValueError):
        distance.render("euclid", ["a"], [1], [1], [[1]], [[1]], out)
    assert not os.path.exists(out)


# ---- the golden table: nine samples --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def zymo_table(tmp_path_factory, golden_dir):
    """the by-sample table of the reference's own pooled document, through build-report --by-sample"""
    with gzip.open(os.path.join(golden_dir, "zymo_mock_distilled.json.gz"), "rt") as f:
        cases = json.load(f)["cases"]
    with gzip.open(os.path.join(golden_dir, "zymo_mock_queries.json.gz"), "rt") as f:
        rows = json.load(f)["results"]
    d = tmp_path_factory.mktemp("zymo")
    doc, tab = d / "doc.json", d / "table.tsv"
    doc.write_text(json.dumps({"results": [{"query": q, "taxon": None if i is None else cases[i]["taxon"]} for q, i in rows]}))
    assert cli.main(["blastn", "build-report", str(doc), "--by-sample", "-o", str(tab)]) == 0
    return str(tab)


@pytest.mark.parametrize("rank", ["g", None])
def test_golden_table_features(tmp_path, zymo_table, rank):
    text = open(zymo_table).read()
    feats, _ = _same(tmp_path, text, rank)
    assert len(text.splitlines()[0].split("\t")) - 4 == 9
    assert feats["unclassified"] == [0, 0, 116, 349, 116, 97, 246, 115, 304]
    names, kept, _ = ref.features(text, rank)
    assert len(names) == 9 and len(kept) > 3
    if rank == "g":
        assert all(";g__" not in t.rsplit(";", 1)[0] for t, _ in kept)      # no feature under a genus


# ---- CLI arguments --------------------------------------------------------------------------------------------------------

def test_cli_argument_errors(tmp_path, capsys):
    base_bc = ["blastn", "build-consensus", "b.tsv", "-t", "t.json", "--taxon", "bacteria", "--strategy", "relaxed"]
    base_rw = ["blastn", "run-with-consensus", "q.fa", "-d", "db", "-t", "t.json", "--blast-out-file", "b.tsv", "--taxon", "bacteria",
               "--strategy", "relaxed"]
    for argv, word in (
            (["blastn", "build-distances", "t.tsv"], "-o"),
            (["blastn", "build-distances", "t.tsv", "-o", "m.tsv", "--metric", "euclid"], "--metric"),
            (["blastn", "build-distances", "-o", "m.tsv"], "table"),
            (base_bc + ["--distance-matrix", "m.tsv"], "--sample-table"),
            (base_rw + ["--distance-matrix", "m.tsv"], "--sample-table"),
            (base_bc + ["--sample-table", "s.tsv", "--distance-rank", "g"], "--distance-matrix"),
            (base_bc + ["--sample-table", "s.tsv", "--distance-matrix", "m.tsv", "--distance-metric", "x"], "--distance-metric"),
            (["blastn", "build-report", "doc.json", "--distance-matrix", "m.tsv"], "--by-sample"),
            (["blastn", "build-report", "doc.json", "--by-sample", "--distance-matrix", "m.tsv"], "-o"),
            (["blastn", "build-report", "doc.json", "-o", "r.tsv", "--distance-matrix", "m.tsv"], "--by-sample"),
            (["blastn", "build-report", "doc.json", "--distance-metric", "jaccard"], "--distance-matrix")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv
        assert word in capsys.readouterr().err, argv
    assert not os.path.exists("m.tsv")


def test_a_table_that_cannot_be_read_and_unknown_flags(tmp_path):
    with pytest.raises(N.BluError) as e:
        distance.features_from_table(str(tmp_path / "absent.tsv"))
    assert e.value.code == 7
    L = pipeline._bind()
    ft = pipeline.DistanceFeatures()
    p = tmp_path / "t.tsv"
    p.write_text(_table(SAMPLES, ROWS))
    assert L.blu_distance_features_from_table(str(p).encode(), None, 2, C.byref(ft)) == N.BLU_ERR_INVALID_ARG
    assert L.blu_distance_features_from_table(None, None, 0, C.byref(ft)) == N.BLU_ERR_INVALID_ARG
    assert L.blu_distance_matrix_file(str(p).encode(), None, 7, 0, 0, str(tmp_path / "o.tsv").encode(), None) == N.BLU_ERR_INVALID_ARG
    assert "metric" in N.last_error() and not (tmp_path / "o.tsv").exists()
