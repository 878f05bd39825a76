"""The boundary-table builder of the conformance matrix (tests/conformance_tables.py), on the CPU: its integer thresholds
against a brute-force scan, every boundary kind present with both outcomes in the oracle, and the same table for a seed."""
import numpy as np
import pytest

from tests import conformance_tables as CT
from tests import helpers as H

CONFIGS = [(21, "bacteria", None, True), (22, "fungi", None, True), (23, "custom", H.CUSTOM_16S, False)]


@pytest.fixture(scope="module")
def tables():
    return [CT.build(seed, taxon, custom, deep=deep, grid=grid) for seed, taxon, custom, deep in CONFIGS for grid in (False, True)]


def test_kthr_against_a_brute_force_scan(tables):
    grid = np.arange(CT.KTHR_NEVER, dtype=np.int64) / 1000.0          # every k in [0, 131 071)
    cuts = np.unique(np.concatenate([t.cutoff[t.kind >= 0] for t in tables]))
    assert len(cuts) > 50
    # the interpolated cutoffs, and off-grid values next to them (the "equals" bit clear), and the ends of the range
    probe = np.concatenate([cuts, np.nextafter(cuts, np.inf), np.nextafter(cuts, -np.inf), cuts + 0.0004,
                            [0.0, -1.0, 1e-300, 131.07, np.nextafter(131.07, np.inf), 131.071, 500.0]])
    k = CT.kthr(probe)
    eq = CT.kthr_equal(probe)
    for c, kc, e in zip(probe, k, eq):
        ok = np.nonzero(grid >= c)[0]
        want = int(ok[0]) if len(ok) else CT.KTHR_NEVER
        assert kc == want, (c, kc, want)
        assert e == (want < CT.KTHR_NEVER and grid[want] == c), c
    assert not eq[len(cuts):2 * len(cuts)].any() and not eq[2 * len(cuts):3 * len(cuts)].any()
    # interpolation rounds every cutoff to three decimals: the equals bit is set for each cutoff a taxonomy can have,
    # integral (97) and not (66.667) alike
    assert CT.kthr_equal(cuts).all()
    assert (cuts == np.round(cuts)).any() and (cuts != np.round(cuts)).any()


def test_every_boundary_kind_is_reached_with_both_outcomes(tables):
    total = {k: {"queries": 0, "pass": 0, "fail": 0} for k in CT.KINDS}
    for t in tables:
        c = t.counts()
        for k in CT.KINDS:
            for f in total[k]:
                total[k][f] += c[k][f]
        kinds = set(CT.KINDS[i] for i in np.unique(t.kind[t.kind >= 0]))
        assert kinds == set(CT.MILLI_KINDS if t.grid else CT.KINDS), (t.taxon, t.grid, kinds)
        if t.grid:
            assert t.hits["pident_milli"].dtype == np.uint32
        else:   # off the milli-percent grid: the f64 level tests must run
            assert (np.round(t.hits["pident"] * 1000.0) / 1000.0 != t.hits["pident"]).sum() > 100
        # levels past 16 (the lvl4 loop) on the deep taxonomies; single-hit queries; every segment length
        if t.tax.deep:
            assert (t.level[t.kind >= 0] >= 16).sum() > 50
        lens = np.diff(t.hits["seg_off"])
        assert set(CT.LENGTHS) <= set(lens.tolist())
        assert ((t.kind >= 0) & (lens == 1)).sum() > 50
    for k in CT.KINDS:
        assert total[k]["queries"] > 300 and total[k]["pass"] > 0 and total[k]["fail"] > 0, (k, total[k])
    # which side of the cutoff a kind falls on decides most outcomes
    for k in ("kthr", "kthr+1", "c", "c+ulp"):
        assert total[k]["pass"] > 5 * total[k]["fail"], (k, total[k])
    for k in ("kthr-1", "c-ulp"):
        assert total[k]["fail"] > 5 * total[k]["pass"], (k, total[k])


def test_same_seed_same_table():
    a, b = CT.build(5, "bacteria", deep=True, scale=0.3), CT.build(5, "bacteria", deep=True, scale=0.3)
    c = CT.build(6, "bacteria", deep=True, scale=0.3)
    for k in a.hits:
        assert a.hits[k].tobytes() == b.hits[k].tobytes(), k
    assert a.kind.tobytes() == b.kind.tobytes() and a.level.tobytes() == b.level.tobytes()
    assert a.cutoff.tobytes() == b.cutoff.tobytes()
    assert a.hits["pident"].tobytes() != c.hits["pident"].tobytes()
    # the on-grid variant is the same table with the f64 kinds folded onto the milli-percent ones
    g = CT.build(5, "bacteria", deep=True, scale=0.3, grid=True)
    for k in ("seg_off", "bitscore", "tax_row", "align_len", "acc_rank"):
        assert g.hits[k].tobytes() == a.hits[k].tobytes(), k
    assert (g.kind == np.where(a.kind >= 3, a.kind - 3, a.kind)).all()


def test_recut_segments_keep_the_row_and_query_counts(tables):
    t = tables[0]
    seg = CT.long_segments(t.hits["seg_off"], 1)
    lens = np.diff(seg)
    assert len(seg) == len(t.hits["seg_off"]) and seg[-1] == t.hits["seg_off"][-1]
    assert (lens >= 0).all() and (lens[lens > 0] >= 1100).sum() >= (lens > 0).sum() - 1
    seg = CT.even_segments(t.hits["seg_off"])
    lens = np.diff(seg)
    assert len(seg) == len(t.hits["seg_off"]) and seg[-1] == t.hits["seg_off"][-1] and lens.max() - lens.min() <= 1
