"""blu_sample_alpha on the GPU against the restatement in tests/alpha_reference.py: the presence flags and the
six integer arrays equal, exactly — raw, along ladders whose slots share radix prefixes, at the seams of the read tiles of both
passes, for samples that reach different numbers of depths, against the library's own rarefaction, under permuted and subset
columns; then `build-diversity` and `build-consensus --alpha-table` end to end, the files byte-equal to the restatement's
rendering."""
import json
import random

import numpy as np
import pytest

from blutils_amd import _native as N
from blutils_amd import cli, distance, diversity
from tests import alpha_reference as ref
from tests import distance_reference as dref
from tests.test_gpu_distance import _golden_inputs, _zymo

pytestmark = pytest.mark.gpu

T = N.ALPHA_TILE               # reads of one block of the level pass
ST = N.RAREFY_TILE             # reads of one block of the select
ARRAYS = ("present",) + ref.FIELDS


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


def _one_sample(counts):
    return list(range(len(counts) + 1)), [0] * len(counts), list(counts)


def _check(csr, names, depths=(), seed=0):
    """all seven arrays against the restatement; -> the library's"""
    got = diversity.alpha(*csr, names, depths, seed)
    want = ref.alpha(*csr, names, list(depths), seed)
    for f in ARRAYS:
        assert got[f].tolist() == want[f], f
    return got


def _ladder(values, top=None):
    return sorted({v for v in values if v >= 1 and (top is None or v <= top)})


# ---- raw mode -----------------------------------------------------------------------------------------------------------------

def test_raw_the_sample_cap_reads_the_logarithm_off_the_device():
    S = N.DISTANCE_MAX_SAMPLES
    got = _check(([0, S], list(range(S)), list(range(1, S + 1))), [f"s{a}" for a in range(S)])
    assert got["sum_xlog"][:, 0].tolist() == [x * ref.log2_fixed(x) for x in range(1, S + 1)]
    assert got["observed"].sum() == S and got["singletons"].sum() == 1 and got["doubletons"].sum() == 1


def test_raw_one_feature_of_the_most_reads_a_sample_may_have():
    big = 2 ** 32 - 1
    got = _check(_one_sample([big]), ["big"])
    assert got["n"].tolist() == [[big]] and got["sum_sq"].tolist() == [[big * big]] and got["sum_xlog"].tolist() == [[big * 536870911]]


def test_raw_empty_samples_empty_features_and_no_features():
    cols = [{0: 9, 3: 4}, {}, {3: 20, 4: 1, 0: 2}]      # sample 1 has no non-zero; features 1 and 2 have none
    got = _check(_csr(cols, 5), ["x", "y", "z"])
    assert got["present"].tolist() == [[1], [1], [1]] and got["n"].tolist() == [[13], [0], [23]]
    got = diversity.alpha([0], [], [], ["x", "y"])
    assert got["present"].tolist() == [[1], [1]] and not any(got[f].any() for f in ref.FIELDS)
    # the same with a ladder: the empty sample reaches nothing
    got = _check(_csr(cols, 5), ["x", "y", "z"], [1, 13, 14, 23])
    assert got["present"].tolist() == [[1, 1, 0, 0], [0, 0, 0, 0], [1, 1, 1, 1]]


def test_raw_many_non_zeros_of_one_sample():
    rng = random.Random(4)
    counts = [rng.choice((1, 1, 2, 2, 3, 70000, 5)) for _ in range(5000)]       # more than one stride of the block
    _check(_one_sample(counts), ["many"])


# ---- ladders ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, T - 1, T, T + 1, 2 * T + 3])
def test_ladder_one_sample_one_feature(n):
    depths = _ladder([1, n // 2, n - 1, n, n + 1])
    got = _check(_one_sample([n]), ["only"], depths, seed=n)
    assert got["present"].tolist() == [[1] * (len(depths) - 1) + [0]]               # the last depth is one read too many
    assert got["n"][0, :-1].tolist() == depths[:-1] and got["observed"][0, :-1].tolist() == [1] * (len(depths) - 1)


def test_adjacent_depths_beside_far_ones():
    rng = random.Random(12)
    counts = [rng.randrange(1, 900) for _ in range(200)]
    n = sum(counts)
    # neighbours share seven digits of their thresholds or more; 1 and n share none with them
    depths = _ladder([1, 2, 3, n // 7, n // 7 + 1, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1, n, n + 1, n + 2])
    got = _check(_one_sample(counts), ["close"], depths, seed=3)
    assert got["present"].tolist() == [[1] * (len(depths) - 2) + [0, 0]]


def test_every_depth_of_a_small_sample_in_three_calls_of_32():
    rng = random.Random(96)
    counts = [rng.randrange(1, 12) for _ in range(11)]
    counts.append(96 - sum(counts))
    assert len(counts) == 12 and min(counts) > 0 and sum(counts) == 96
    csr, curve = _one_sample(counts), {f: [] for f in ref.FIELDS}
    for lo in (1, 33, 65):
        got = _check(csr, ["small"], list(range(lo, lo + 32)), seed=1)                 # 32 depths: the cap
        assert got["present"].all()
        for f in ref.FIELDS:
            curve[f] += got[f][0].tolist()
    assert curve["n"] == list(range(1, 97))
    assert all(a <= b for a, b in zip(curve["observed"], curve["observed"][1:])) and curve["observed"][-1] == 12
    assert curve["observed"][0] == curve["singletons"][0] == 1
    raw = _check(csr, ["small"])
    assert all(raw[f][0, 0] == curve[f][-1] for f in ref.FIELDS)                     # the full depth is the raw table
    with pytest.raises(N.BluError, match="33 depths"):
        diversity.alpha(*csr, ["small"], list(range(1, 34)))


@pytest.mark.parametrize("counts", [
    [5, 2 * T + 7, 3],                                 # a non-zero that spans three tiles, one before it and one after
    [T - 10, 10, 7, T - 7, 20],                        # non-zeros that end exactly on the first and the second tile boundary
    [T, T, 1],                                         # whole tiles
    [3, T - 4, 2 * T, 9],                              # a start one read before a boundary, an end one read before the next but one
    [ST - 6, 10, 3],                                   # over the seam of the select's tiles
], ids=["three-tiles", "ends-on-boundary", "whole-tiles", "off-by-one", "select-seam"])
def test_non_zeros_across_tiles(counts):
    n = sum(counts)
    got = _check(_one_sample(counts), ["wide"], _ladder([1, 9, n // 3, n // 2, n - 1, n]), seed=7)
    assert got["present"].all()
    assert all(a <= b for a, b in zip(got["observed"][0].tolist(), got["observed"][0].tolist()[1:]))


def test_a_tile_that_holds_thousands_of_non_zeros():
    rng = random.Random(3)
    counts = [rng.randrange(1, 4) for _ in range(3000)]                              # all of them inside one tile
    n = sum(counts)
    assert n < T
    _check(_one_sample(counts), ["many"], _ladder([1, 17, n // 2, n - 1, n]), seed=5)
    counts = [rng.randrange(1, 4) for _ in range(6000)]                              # thousands on both sides of a boundary
    n = sum(counts)
    assert n > T + 2000
    _check(_one_sample(counts), ["many"], _ladder([n // 10 * k for k in range(1, 11)]), seed=1)


def _random_columns(S, F, density, seed, top):
    rng = random.Random(seed)
    n = max(1, round(F * density))
    return [{f: rng.randrange(1, top) for f in (range(F) if n >= F else rng.sample(range(F), n))} for _ in range(S)]


@pytest.fixture(scope="module")
def random_cases():
    """the two random CSRs with a ladder only some samples reach all of, the restatement's integers computed once"""
    cases = {}
    for S, F, density, top in ((70, 20000, 0.01, 1000), (12, 8197, 1.0, 30)):
        cols = _random_columns(S, F, density, S + F, top)
        for a in range(0, S, 5):                        # every fifth sample thinned, so that the totals spread
            cols[a] = {f: v for i, (f, v) in enumerate(sorted(cols[a].items())) if i % (a % 4 + 2) == 0}
        totals = sorted(sum(c.values()) for c in cols)
        depths = _ladder([totals[0] // 2, totals[0], totals[0] + 1, totals[S // 3], totals[S // 2], totals[S // 2] + 1, totals[-1], totals[-1] + 1])
        names = [f"s{a}" for a in range(S)]
        csr = _csr(cols, F)
        cases[S] = (cols, csr, names, depths, ref.alpha(*csr, names, depths, seed=S))
    return cases


@pytest.mark.parametrize("S", [70, 12])
def test_random_csr_with_a_ladder_that_some_samples_only_partly_reach(random_cases, S):
    cols, csr, names, depths, want = random_cases[S]
    got = diversity.alpha(*csr, names, depths, seed=S)
    for f in ARRAYS:
        assert got[f].tolist() == want[f], f
    live = got["present"].sum(axis=1).tolist()
    assert min(live) >= 2 and max(live) == len(depths) - 1 and len(set(live)) >= 3 and not got["present"][:, -1].any()
    for a in range(S):                                  # observed and n do not decrease along a curve
        k = live[a]
        assert got["n"][a, :k].tolist() == depths[:k] and (np.diff(got["observed"][a, :k].astype(np.int64)) >= 0).all()


@pytest.mark.parametrize("S", [70, 12])
def test_agreement_with_the_library_s_rarefaction(random_cases, S):
    """the integers at D are those of the table `--rarefy D --seed N` writes: computed here in numpy from distance.rarefy"""
    cols, csr, names, depths, _ = random_cases[S]
    got = diversity.alpha(*csr, names, depths, seed=S)
    for j in (0, len(depths) // 2, len(depths) - 2):
        r = distance.rarefy(*csr, names, depths[j], seed=S)
        K = len(r["kept_sample"])
        assert r["kept_sample"].tolist() == [a for a in range(S) if got["present"][a, j]]
        x = r["count"]                                  # (uint64; every sum below stays far under 2^64 for these tables)
        log_of = np.array([0] + [ref.log2_fixed(v) for v in range(1, int(x.max()) + 1)], dtype=np.uint64)
        for f, w in (("n", x), ("observed", np.ones_like(x)), ("singletons", (x == 1).astype(np.uint64)),
                     ("doubletons", (x == 2).astype(np.uint64)), ("sum_sq", x * x), ("sum_xlog", x * log_of[x.astype(np.int64)])):
            sums = np.zeros(K, dtype=np.uint64)
            np.add.at(sums, r["sample"], w)
            assert sums.tolist() == [int(v) for v in got[f][r["kept_sample"], j]], (f, depths[j])


def test_seeds():
    cols = [{f: 50 + f for f in range(30)}, {f: 10 + 2 * f for f in range(0, 30, 2)}]
    csr, names, depths = _csr(cols, 30), ["a", "b"], [40, 400, 585]
    g0, g1, again = _check(csr, names, depths, 0), _check(csr, names, depths, 1), _check(csr, names, depths, 0)
    assert any(g0[f].tobytes() != g1[f].tobytes() for f in ref.FIELDS)
    assert all(g0[f].tobytes() == again[f].tobytes() for f in ARRAYS)
    _check(csr, names, depths, 2 ** 64 - 1)
    raw0, raw1 = diversity.alpha(*csr, names, seed=0), diversity.alpha(*csr, names, seed=1)      # no draw: the seed says nothing
    assert all(raw0[f].tobytes() == raw1[f].tobytes() for f in ARRAYS)


def test_samples_are_independent_of_column_order_and_of_each_other():
    rng = random.Random(21)
    F, depths = 60, [100, 2500, 5000, 5001, 9000]
    cols = [{f: rng.randrange(1, 400) for f in rng.sample(range(F), rng.randrange(20, F))} for _ in range(12)]
    names = [f"sample-{i}" for i in range(12)]
    got = _check(_csr(cols, F), names, depths, seed=4)
    by_name = {names[a]: [got[f][a].tolist() for f in ARRAYS] for a in range(12)}
    order = list(range(12))
    rng.shuffle(order)
    for pick in (order, [7, 5, 3, 0, 11]):
        sub = _check(_csr([cols[a] for a in pick], F), [names[a] for a in pick], depths, seed=4)
        for k, a in enumerate(pick):
            assert [sub[f][k].tolist() for f in ARRAYS] == by_name[names[a]], names[a]


# ---- end to end ---------------------------------------------------------------------------------------------------------------

def _summary(names, feats, rank, depths, text):
    totals = [sum(c[s] for _, c in feats) for s in range(len(names))]
    lines = [f"diversity: {len(feats)} features at {rank}, {len(names)} samples, {len(depths)} depths, {len(text.splitlines()) - 1} rows\n"]
    for n, t in zip(names, totals):
        j = sum(1 for d in depths if d <= t)
        if j < len(depths):
            lines.append(f"diversity: {n} ({t} reads) reaches {j} of {len(depths)} depths\n")
    return "".join(lines), totals


def test_build_diversity_on_the_golden_table(tmp_path, golden_dir, capsys):
    cases, rows = _zymo(golden_dir)
    doc, tab, out = tmp_path / "doc.json", tmp_path / "table.tsv", tmp_path / "alpha.tsv"
    doc.write_text(json.dumps({"results": [{"query": q, "taxon": None if i is None else cases[i]["taxon"]} for q, i in rows]}))
    assert cli.main(["blastn", "build-report", str(doc), "--by-sample", "-o", str(tab)]) == 0
    names, feats, _ = dref.features(tab.read_text(), "g")
    assert len(names) == 9
    capsys.readouterr()
    # raw
    assert cli.main(["blastn", "build-diversity", str(tab), "-o", str(out), "--rank", "genus"]) == 0
    want = ref.table_text(names, feats)
    err, totals = _summary(names, feats, "genus", [], want)
    assert out.read_text() == want and len(want.splitlines()) == 10 and capsys.readouterr().err == err
    # --steps 5: up to the largest total, so every smaller sample misses some depths
    depths = ref.ladder(5, max(totals))
    assert cli.main(["blastn", "build-diversity", str(tab), "-o", str(out), "--rank", "genus", "--steps", "5", "--seed", "5"]) == 0
    want = ref.table_text(names, feats, depths, 5)
    err, _ = _summary(names, feats, "genus", depths, want)
    assert out.read_text() == want and capsys.readouterr().err == err and err.count("reaches") >= 1
    assert want != ref.table_text(names, feats, depths, 6)
    # --depths, --max-depth, no rank, --drop-unclassified
    names0, feats0, _ = dref.features(tab.read_text(), None, True)
    assert cli.main(["blastn", "build-diversity", str(tab), "-o", str(out), "--drop-unclassified", "--steps", "4", "--max-depth", "10"]) == 0
    assert out.read_text() == ref.table_text(names0, feats0, [2, 5, 7, 10], 0) and "at no rank" in capsys.readouterr().err
    low = min(totals)
    print("totals of the golden table at genus:", totals)
    assert low >= 2
    assert cli.main(["blastn", "build-diversity", str(tab), "-o", str(out), "--rank", "g", "--depths", f"{low // 2},{low},{low + 1}"]) == 0
    assert out.read_text() == ref.table_text(names, feats, [low // 2, low, low + 1], 0)
    # a first depth above every total: the error names the largest, nothing is written
    out.unlink()
    with pytest.raises(SystemExit, match=f"has {max(totals)} reads"):
        cli.main(["blastn", "build-diversity", str(tab), "-o", str(out), "--rank", "genus", "--depths", f"{max(totals) + 1},{max(totals) + 5}"])
    assert not out.exists()


def test_build_consensus_writes_the_alpha_table_of_its_own_sample_table(tmp_path, golden_dir, capsys):
    cases, rows = _zymo(golden_dir)
    cls = [(q, i) for q, i in rows if i is not None]
    bt, tj = _golden_inputs(tmp_path, [cases[i]["taxon"] for _, i in cls], [q for q, _ in cls])
    doc, tab, out = tmp_path / "doc.json", tmp_path / "table.tsv", tmp_path / "alpha.tsv"
    base = ["blastn", "build-consensus", bt, "-t", tj, "--taxon", "bacteria", "--strategy", "relaxed", "--blutils-out-file", str(doc),
            "--sample-table", str(tab)]
    assert cli.main(base + ["--alpha-table", str(out), "--alpha-rank", "g"]) == 0
    names, feats, _ = dref.features(tab.read_text(), "g")
    want = ref.table_text(names, feats)
    err, totals = _summary(names, feats, "g", [], want)
    assert out.read_text() == want and capsys.readouterr().err.endswith(err)
    depths = ref.ladder(5, max(totals))
    assert cli.main(base + ["--alpha-table", str(out), "--alpha-rank", "g", "--alpha-steps", "5", "--alpha-seed", "9"]) == 0
    want = ref.table_text(names, feats, depths, 9)
    err, _ = _summary(names, feats, "g", depths, want)
    assert out.read_text() == want and capsys.readouterr().err.endswith(err)
    assert cli.main(base + ["--alpha-table", str(out), "--alpha-depths", "1,2"]) == 0
    names0, feats0, _ = dref.features(tab.read_text(), None)
    assert out.read_text() == ref.table_text(names0, feats0, [1, 2], 0)
