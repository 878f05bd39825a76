"""blu_sample_rarefy on the GPU against the restatement in tests/rarefy_reference.py: equal kept samples, row
offsets, samples and counts, and column sums equal to the depth — at the seams of the read tiles, where a non-zero spans tiles
and where a tile holds many, at the ends of the radix select, under permuted and subset columns; then `build-distances --rarefy`
and `build-consensus --distance-rarefy` end to end, the files byte-equal to the restatement's rendering."""
import json
import random

import numpy as np
import pytest

from blutils_amd import _native as N
from blutils_amd import cli, distance
from tests import distance_reference as dref
from tests import rarefy_reference as ref
from tests.test_gpu_distance import _golden_inputs, _zymo

pytestmark = pytest.mark.gpu

T = N.RAREFY_TILE


def _csr(columns, n_features):
    """per-sample {feature: count} -> CSR over the features"""
    rows = [[] for _ in range(n_features)]
    for s, col in enumerate(columns):
        for f, v in col.items():
            rows[f].append((s, v))
    row_ptr, sample, count = [0], [], []
    for r in rows:
        for s, v in r:
            sample.append(s)
            count.append(v)
        row_ptr.append(len(sample))
    return row_ptr, sample, count


def _columns(got, n_features):
    """a rarefied CSR -> per kept sample {feature: count}"""
    cols = [{} for _ in range(len(got["kept_sample"]))]
    rp = got["row_ptr"].tolist()
    for f in range(n_features):
        for e in range(rp[f], rp[f + 1]):
            cols[int(got["sample"][e])][f] = int(got["count"][e])
    return cols


def _check(csr, names, depth, seed=0):
    got = distance.rarefy(*csr, names, depth, seed)
    kept, rp, sm, ct = ref.rarefy(*csr, names, depth, seed)
    assert got["kept_sample"].tolist() == kept
    assert got["row_ptr"].tolist() == rp and got["sample"].tolist() == sm and got["count"].tolist() == ct
    sums = np.zeros(len(kept), np.uint64)
    np.add.at(sums, got["sample"], got["count"])
    assert (sums == depth).all()
    return got


def _one_sample(counts):
    return list(range(len(counts) + 1)), [0] * len(counts), list(counts)


@pytest.mark.parametrize("n", [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3])
def test_tile_seams_one_sample_one_feature(n):
    for depth in sorted({1, max(n // 2, 1), max(n - 1, 1), n}):
        got = _check(_one_sample([n]), ["only"], depth, seed=n)
        assert got["count"].tolist() == [depth] and got["kept_sample"].tolist() == [0]
    got = _check(_one_sample([n]), ["only"], n + 1)                      # one read short: dropped, K = 0
    assert got["kept_sample"].size == 0 and got["row_ptr"].tolist() == [0, 0] and got["count"].size == 0


@pytest.mark.parametrize("counts", [
    [5, 2 * T + 7, 3],                                 # a non-zero that spans three tiles, one before it and one after
    [T - 10, 10, 7, T - 7, 20],                        # non-zeros that end exactly on the first and the second tile boundary
    [T, T, 1],                                         # whole tiles
    [3, T - 4, 2 * T, 9],                              # a start one read before a boundary, an end one read before the next but one
], ids=["three-tiles", "ends-on-boundary", "whole-tiles", "off-by-one"])
def test_non_zeros_across_tiles(counts):
    n = sum(counts)
    for depth in (1, n // 3, n - 1, n):
        _check(_one_sample(counts), ["wide"], depth, seed=7)


def test_a_tile_that_holds_thousands_of_non_zeros():
    rng = random.Random(3)
    counts = [rng.randrange(1, 4) for _ in range(3000)]
    n = sum(counts)
    for depth in (1, 17, n // 2, n - 1):
        _check(_one_sample(counts), ["many"], depth, seed=depth)
    # and thousands on both sides of a boundary: the second tile starts inside a run of small non-zeros
    counts = [rng.randrange(1, 4) for _ in range(40000)]
    assert sum(counts) > T + 5000
    _check(_one_sample(counts), ["many"], sum(counts) // 2, seed=1)


def test_the_smallest_and_the_largest_key():
    counts = [40, 1, 300, 7, 90, 2]
    n, names, seed = sum(counts), ["S"], 11
    keys = ref.keys(ref.stream(seed, "S"), n)
    ends = np.cumsum(counts)
    f_min = int(np.searchsorted(ends, int(np.argmin(keys)), side="right"))
    f_max = int(np.searchsorted(ends, int(np.argmax(keys)), side="right"))
    got = _check(_one_sample(counts), names, 1, seed)                   # only the read with the smallest key
    assert got["row_ptr"].tolist() == [0] * (f_min + 1) + [1] * (len(counts) - f_min) and got["count"].tolist() == [1]
    got = _check(_one_sample(counts), names, n - 1, seed)               # every read but the one with the largest key
    expect = list(counts)
    expect[f_max] -= 1
    assert [c for c in expect if c] == got["count"].tolist()


def test_every_depth_of_one_small_sample_and_nested_kept_sets():
    rng = random.Random(8)
    counts = [rng.randrange(1, 8) for _ in range(39)]
    counts.append(300 - sum(counts))
    assert sum(counts) == 300 and min(counts) > 0
    csr, before = _one_sample(counts), [0] * len(counts)
    st = ref.stream(2, "nested")
    for depth in range(1, 301):
        got = distance.rarefy(*csr, ["nested"], depth, 2)
        now = [0] * len(counts)
        rp = got["row_ptr"].tolist()
        for f in range(len(counts)):
            if rp[f + 1] > rp[f]:
                now[f] = int(got["count"][rp[f]])
        assert now == ref.kept_by_sort(counts, depth, st), depth
        assert sum(now) == depth and all(a <= b for a, b in zip(before, now)), depth      # the kept sets are nested
        before = now
    assert before == counts


def test_samples_are_independent_of_column_order_and_of_each_other():
    rng = random.Random(21)
    F, depth = 60, 5000
    cols = [{f: rng.randrange(1, 400) for f in rng.sample(range(F), rng.randrange(20, F))} for _ in range(12)]

    def resize(col, total):                             # the same features, the counts adding up to `total`
        fs = sorted(col)
        col.clear()
        col.update({f: total // len(fs) + (1 if i < total % len(fs) else 0) for i, f in enumerate(fs)})

    resize(cols[3], depth - 1)                          # just under: dropped
    resize(cols[5], depth)                              # at the depth: kept whole
    resize(cols[7], depth + 1)                          # just over: one read goes
    resize(cols[0], 3 * depth)
    names = [f"sample-{i}" for i in range(12)]
    totals = [sum(c.values()) for c in cols]
    got = _check(_csr(cols, F), names, depth, seed=4)
    kept = got["kept_sample"].tolist()
    assert 3 not in kept and 5 in kept and 7 in kept and kept == [a for a in range(12) if totals[a] >= depth]
    by_name = {names[a]: c for a, c in zip(kept, _columns(got, F))}
    assert by_name["sample-5"] == cols[5] and sum(by_name["sample-7"].values()) == depth
    order = list(range(12))
    rng.shuffle(order)
    for pick in (order, [7, 5, 3, 0, 11]):
        sub = _check(_csr([cols[a] for a in pick], F), [names[a] for a in pick], depth, seed=4)
        for k, c in zip(sub["kept_sample"].tolist(), _columns(sub, F)):
            assert c == by_name[names[pick[k]]], names[pick[k]]


def test_seeds():
    cols = [{f: 50 + f for f in range(30)}, {f: 10 + 2 * f for f in range(0, 30, 2)}]
    csr, names = _csr(cols, 30), ["a", "b"]
    assert ref.rarefy(*csr, names, 400, 0) != ref.rarefy(*csr, names, 400, 1)
    g0, g1, again = _check(csr, names, 400, 0), _check(csr, names, 400, 1), _check(csr, names, 400, 0)
    assert g0["count"].tobytes() != g1["count"].tobytes() or g0["row_ptr"].tobytes() != g1["row_ptr"].tobytes()
    for k in ("kept_sample", "row_ptr", "sample", "count"):
        assert g0[k].tobytes() == again[k].tobytes()
    _check(csr, names, 400, 2 ** 64 - 1)


def test_empty_samples_empty_features_and_no_features():
    cols = [{0: 9, 3: 4}, {}, {3: 20}]                  # sample 1 has no non-zero; features 1 and 2 have none
    got = _check(_csr(cols, 5), ["x", "y", "z"], 6)
    assert got["kept_sample"].tolist() == [0, 2] and len(got["row_ptr"]) == 6
    assert got["row_ptr"].tolist()[1:4] == [got["row_ptr"][1]] * 3      # the rows of features 1 and 2 stay, empty
    got = distance.rarefy([0], [], [], ["x", "y"], 1)
    assert got["kept_sample"].size == 0 and got["row_ptr"].tolist() == [0]


def _random_columns(S, F, density, seed, top=1000):
    rng = random.Random(seed)
    n = max(1, round(F * density))
    return [{f: rng.randrange(1, top) for f in (range(F) if n >= F else rng.sample(range(F), n))} for _ in range(S)]


@pytest.mark.parametrize("S,F,density", [(70, 20000, 0.01), (12, 8197, 1.0)])
def test_random_csr_and_the_chained_integers(S, F, density):
    cols = _random_columns(S, F, density, S + F)
    depth = int(np.percentile([sum(c.values()) for c in cols], 25))
    names = [f"s{a}" for a in range(S)]
    got = _check(_csr(cols, F), names, depth, seed=S)
    K = len(got["kept_sample"])
    assert 0 < K < S
    rarefied = _columns(got, F)                         # (equal to the restatement's: _check compared the CSR)
    ints = distance.sample_distances(got["row_ptr"], got["sample"], got["count"], K)
    total, rich, min_sum, shared = dref.integers_dense(rarefied)
    assert ints["total"].tolist() == total == [depth] * K and ints["richness"].tolist() == rich
    assert ints["min_sum"].tolist() == min_sum and ints["shared"].tolist() == shared


# ---- end to end ---------------------------------------------------------------------------------------------------------------

def _expected(text, rank, depth, seed, drop=False):
    """the restatement's rarefied features of a sample table's text -> kept names, features, the dropped (name, total)"""
    names, feats, _ = dref.features(text, rank, drop)
    totals = [sum(c[s] for _, c in feats) for s in range(len(names))]
    kept_names, rare = ref.rarefied_features(names, feats, depth, seed)
    return kept_names, rare, [(n, t) for n, t in zip(names, totals) if t < depth], totals


def _matrix(metric, kept_names, rare):
    return dref.render(metric, kept_names, *dref.integers(*dref.csr(rare), len(kept_names)))


def test_build_distances_rarefy_on_the_golden_table(tmp_path, golden_dir, capsys):
    cases, rows = _zymo(golden_dir)
    doc, tab = tmp_path / "doc.json", tmp_path / "table.tsv"
    doc.write_text(json.dumps({"results": [{"query": q, "taxon": None if i is None else cases[i]["taxon"]} for q, i in rows]}))
    assert cli.main(["blastn", "build-report", str(doc), "--by-sample", "-o", str(tab)]) == 0
    text = tab.read_text()
    totals = _expected(text, "g", 1, 0)[3]
    depth = sorted(totals)[2]                           # the third-smallest total: two samples go, one stays whole
    kept_names, rare, dropped, _ = _expected(text, "g", depth, 5)
    assert len(totals) == 9 and len(dropped) == 2 and len(kept_names) == 7 and totals.count(depth) >= 1
    capsys.readouterr()
    for metric in ("bray-curtis", "jaccard"):
        out, table = tmp_path / f"{metric}.tsv", tmp_path / f"{metric}.rarefied.tsv"
        assert cli.main(["blastn", "build-distances", str(tab), "-o", str(out), "--rarefy", str(depth), "--seed", "5", "--rank", "genus",
                         "--metric", metric, "--rarefied-table", str(table)]) == 0
        assert out.read_text() == _matrix(metric, kept_names, rare)
        assert table.read_text() == ref.table_text(kept_names, rare)
        err = capsys.readouterr().err
        left = [c for _, c in rare if any(c)]
        assert (f"distances: {len(left)} features at genus, 7 samples, {sum(sum(1 for v in c if v) for c in left)} non-zeros\n"
                f"rarefy: depth {depth}, seed 5, kept 7 of 9 samples, {len(rare) - len(left)} features emptied\n") in err
        for name, total in dropped:
            assert f"rarefy: dropped {name} ({total} reads)\n" in err
        assert err.count("rarefy: dropped") == 2
    # a sample at the depth is kept whole; another seed is another draw of the others
    names, feats, _ = dref.features(text, "g")
    for name in (n for n, t in zip(names, totals) if t == depth):
        assert [c[kept_names.index(name)] for _, c in rare] == [c[names.index(name)] for _, c in feats]
    out0 = tmp_path / "seed0.tsv"
    assert cli.main(["blastn", "build-distances", str(tab), "-o", str(out0), "--rarefy", str(depth), "--rank", "genus"]) == 0
    kn0, rare0, _, _ = _expected(text, "g", depth, 0)
    assert out0.read_text() == _matrix("bray-curtis", kn0, rare0) and "seed 0" in capsys.readouterr().err
    # a depth above every total: the error names the largest, nothing is written
    with pytest.raises(SystemExit, match=f"has {max(totals)} reads"):
        cli.main(["blastn", "build-distances", str(tab), "-o", str(tmp_path / "no.tsv"), "--rarefy", str(max(totals) + 1), "--rank", "genus",
                  "--rarefied-table", str(tmp_path / "no.rarefied.tsv")])
    assert not (tmp_path / "no.tsv").exists() and not (tmp_path / "no.rarefied.tsv").exists()
    # without --rarefy: what it was
    plain = tmp_path / "plain.tsv"
    capsys.readouterr()
    assert cli.main(["blastn", "build-distances", str(tab), "-o", str(plain), "--rank", "genus"]) == 0
    assert plain.read_text() == dref.matrix_text(text, "g", "bray-curtis")
    names, feats, _ = dref.features(text, "g")
    assert capsys.readouterr().err == f"distances: {len(feats)} features at genus, 9 samples, {dref.csr(feats)[0][-1]} non-zeros\n"


def test_build_consensus_rarefies_the_matrix_of_its_own_sample_table(tmp_path, golden_dir, capsys):
    cases, rows = _zymo(golden_dir)
    cls = [(q, i) for q, i in rows if i is not None]
    bt, tj = _golden_inputs(tmp_path, [cases[i]["taxon"] for _, i in cls], [q for q, _ in cls])
    doc, tab, out, rtab = tmp_path / "doc.json", tmp_path / "table.tsv", tmp_path / "m.tsv", tmp_path / "rarefied.tsv"
    base = ["blastn", "build-consensus", bt, "-t", tj, "--taxon", "bacteria", "--strategy", "relaxed", "--blutils-out-file", str(doc),
            "--sample-table", str(tab)]
    assert cli.main(base) == 0
    totals = _expected(tab.read_text(), "g", 1, 0)[3]
    print("totals of the rebuilt table:", totals)
    depth = sorted(totals)[len(totals) // 2]            # the median total: some samples go, one stays whole
    assert len(totals) >= 2 and min(totals) < depth
    assert cli.main(base + ["--distance-matrix", str(out), "--distance-rank", "g", "--distance-rarefy", str(depth), "--distance-seed", "9",
                            "--distance-rarefied-table", str(rtab)]) == 0
    kept_names, rare, dropped, _ = _expected(tab.read_text(), "g", depth, 9)
    assert out.read_text() == _matrix("bray-curtis", kept_names, rare)
    assert rtab.read_text() == ref.table_text(kept_names, rare)
    err = capsys.readouterr().err
    assert f"rarefy: depth {depth}, seed 9, kept {len(kept_names)} of {len(totals)} samples" in err
    assert all(f"rarefy: dropped {n} ({t} reads)" in err for n, t in dropped) and len(dropped) == sum(t < depth for t in totals)
