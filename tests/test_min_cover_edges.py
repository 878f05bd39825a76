"""The case families of tests/min_cover_edges.py lie where they claim (no GPU): every claim is computed from the sorted
positions of the groups, nothing is read from a kernel.  The closed form of the large table — share, lcp8, d* from digit
prefixes — is held to tests/min_cover_reference.py, which counts prefix tuples in a dict."""
import collections

import numpy as np
import pytest

from tests import min_cover_edges as mc
from tests import min_cover_reference as ref
from tests import support_edges as se

LARGE = {"spread": mc.spread_family, "digit": mc.digit_family, "bin edge": mc.bin_edge_family, "range": mc.range_family}


def _groups(family):
    if family in LARGE:
        return LARGE[family]()
    if family == "scores":
        return mc.scores_family()
    return [g for groups in mc.queries_family().values() for g in groups] + mc.repeated_block()


def test_the_large_table_is_what_the_closed_form_says():
    m, perm = mc.large_matrix()
    assert m.shape == (mc.LARGE_ROWS, mc.LEVELS) and mc.LARGE_ROWS == (1 << 20) + 40
    for r in (0, 1, 12345, mc.LARGE_ROWS - 1):
        assert tuple(int(x) for x in m[r]) == mc.lineage_of(int(perm[r]))
    order = se.sort_rows(m)                                              # the independent sort: position p holds the digits of p
    assert np.array_equal(perm[order], np.arange(mc.LARGE_ROWS))
    lcp = mc.lcp8()
    assert len(lcp) == mc.LARGE_ROWS - 1
    for i in (0, 6, 7, 8, 62, 63, 64, 511, 4095, (1 << 18) - 1, (1 << 18), (1 << 20) - 1, 1 << 20, mc.LARGE_ROWS - 2):
        a, b = mc.lineage_of(i), mc.lineage_of(i + 1)
        by_tuples = next(k for k in range(mc.LEVELS) if a[k] != b[k])
        assert lcp[i] == mc.share(i, i + 1) == by_tuples, i
    rng = np.random.default_rng(1)
    for a, b in rng.integers(0, mc.LARGE_ROWS, (200, 2)).tolist() + [(5, 5), (0, mc.LARGE_ROWS - 1)]:
        la, lb = mc.lineage_of(a), mc.lineage_of(b)
        assert mc.share(a, b) == next((k for k in range(mc.LEVELS) if la[k] != lb[k]), mc.LEVELS)
        if a < b:
            assert mc.share(a, b) == lcp[a:b].min()                      # share is the range minimum the kernels take
    # the deepest entries sit at the end of a 16-entry block: what range_family says about the right edge
    assert (lcp[np.arange(len(lcp)) % 16 != 15] >= mc.LEVELS - 2).all()
    assert np.flatnonzero(lcp == 0).tolist() == [(1 << 18) * k - 1 for k in (1, 2, 3, 4)]


def test_the_stepped_table_is_what_its_closed_form_says():
    m, perm = mc.stepped_matrix()
    for r in (0, 1, 777, mc.LARGE_ROWS - 1) + tuple(int(x) for x in np.flatnonzero((perm < mc.STEP_1) | (perm >= mc.STEP_2))[:6]):
        assert tuple(int(x) for x in m[r] if x >= 0) == mc.stepped_lineage_of(int(perm[r]))
    assert np.array_equal(perm[se.sort_rows(m)], np.arange(mc.LARGE_ROWS))        # position p holds stepped_lineage_of(p)
    lcp = mc.stepped_lcp8()
    for i in (0, 7, mc.STEP_1 - 2, mc.STEP_1 - 1, mc.STEP_1, 63, (1 << 18) - 1, mc.STEP_2 - 2, mc.STEP_2 - 1, mc.STEP_2, mc.LARGE_ROWS - 2):
        a, b = mc.stepped_lineage_of(i), mc.stepped_lineage_of(i + 1)
        by_tuples = next(k for k in range(len(a) + 1) if k >= min(len(a), len(b)) or a[k] != b[k])
        assert lcp[i] == mc.stepped_share(i, i + 1) == by_tuples, i
    assert np.flatnonzero(lcp < 2).tolist() == [mc.STEP_1 - 1, mc.STEP_2 - 1] and lcp[mc.STEP_1 - 1] == 1 and lcp[mc.STEP_2 - 1] == 0
    rng = np.random.default_rng(2)
    for a, b in rng.integers(0, mc.LARGE_ROWS, (100, 2)).tolist() + [(0, 9), (9, 10), (3, mc.STEP_2), (mc.STEP_2 - 1, mc.STEP_2), (mc.STEP_2, mc.STEP_2 + 5)]:
        if a < b:
            assert mc.stepped_share(a, b) == lcp[a:b].min()
    groups = mc.stepped_range_family()
    seg, v, d, c = mc.reference(groups, 75000)
    assert d == [mc.stepped_share(g.claims["lo"], g.claims["hi"]) for g in groups]
    assert c["n_narrowed"] == sum(1 for x in d if x > 0) >= 150


@pytest.mark.parametrize("family", sorted(LARGE))
def test_closed_form_equals_the_reference(family):
    groups = LARGE[family]()
    for milli in mc.MILLIS[family]:
        seg, v, d, c = mc.reference(groups, milli)
        for q, g in enumerate(groups):
            top = g.top()
            want_d, want_top = mc.closed_form(top, milli)
            assert d[q] == want_d, (g.where(), milli)
            t = max(s for _, s in g.rows)
            got_top = [v[seg[q] + i] for i, (_, s) in enumerate(g.rows) if s == t]
            assert got_top == want_top, (g.where(), milli)
            assert all(v[seg[q] + i] == 1 for i, (_, s) in enumerate(g.rows) if s != t)


def test_family_sizes_and_conditions():
    """every case a family lists is there (none is left out), every spread and digit group is narrowed at
    50.001 %, and every family has a group with need * 100000 == n * milli, where `>=` and `>` in `need` part"""
    spread = mc.spread_family()
    assert collections.Counter((g.claims["n"], g.claims["level"], g.claims["form"]) for g in spread) == \
        {(n, level, form): 4 for n in mc.SPREAD_N for level in range(1, 7) for form in (("short", "long") if n <= 64 else ("long",))}
    assert all(len(g.top()) == g.claims["n"] and (len(g.rows) > 64) == (g.claims["form"] == "long") for g in spread)
    for g in spread:                                                     # exactly `need` rows in one clade of the level
        pre = collections.Counter(p >> (3 * (mc.LEVELS - g.claims["level"])) for p in g.top())
        assert max(pre.values()) >= g.claims["need"] == ref.need_rows(g.claims["n"], 50001)
    digit = mc.digit_family()
    form1 = collections.Counter((g.claims["s"], g.claims["t"], g.claims["low"], g.claims["side"]) for g in digit if g.claims["form"] == 1)
    assert set(form1.values()) == {2}                                    # majority first and majority last
    for s in (18, 12, 6):
        assert {t for (s_, t, _, _) in form1 if s_ == s} == {0, 1, 2, 3, 4}
        assert {side for (s_, _, _, side) in form1 if s_ == s} == {"below", "above", "split"}
        for t in range(5):
            assert len({low for (s_, t_, low, _) in form1 if (s_, t_) == (s, t)}) == 3, (s, t)
    # the arrangements left out are exactly those with an outlier outside the table
    assert len(form1) == 3 * 5 * 3 * 3 - sum(
        1 for s in (18, 12, 6) for t in range(5) for low in ((0, 63, 29) if t < 4 else (0, 32, 16)) for sg in ((-1,), (1,), (-1, 1))
        if any(not 0 <= (((t << 18) | ((low << 12 | low << 6 | low) if t < 4 else low)) & ~7) + off + x * (1 << s) < mc.LARGE_ROWS
               for x in sg for off in ((0, 1, 3, 4) if len(sg) == 1 else ((0, 1) if x < 0 else (3, 4)))))
    assert collections.Counter((g.claims["t"], g.claims["side"]) for g in digit if g.claims["form"] == 2) == \
        {(t, side): 2 for t in range(4) for side in ("below", "above") if (t, side) != (0, "below")}
    assert all(len(g.top()) == 9 and len(g.rows) > 64 for g in digit + mc.bin_edge_family())
    assert len(mc.bin_edge_family()) == 4 * 2 * 2 * 2
    assert sorted(mc.queries_family()) == sorted(mc.QUERY_COUNTS)
    assert all(len(groups) == count for count, groups in mc.queries_family().items())
    for count, groups in mc.queries_family().items():
        if count >= 5:
            longs = [q for q, g in enumerate(groups) if len(g.rows) > 64]
            assert longs[0] == 0 and longs[-1] == count - 1 and (count < 63 or len(longs) >= 3)
    block = mc.repeated_block()
    assert len(block) == mc.REPEAT_BLOCK and mc.REPEAT_BLOCK % 7 == 0
    assert [len(g.rows) > 64 for g in block] == [q % 7 == 3 for q in range(len(block))]
    assert 290000 <= len(block) * mc.REPEAT_TIMES <= 310000 and 2.9e6 <= sum(len(g.rows) for g in block) * mc.REPEAT_TIMES <= 4e6
    for family in ("spread", "digit"):
        seg, v, d, c = mc.reference(_groups(family), 50001)
        assert c["n_narrowed"] == len(_groups(family)), (family, c)
    for family in mc.FAMILIES:
        milli = mc.MILLIS[family][-1]
        assert any(len(g.top()) > 1 and ref.need_rows(len(g.top()), milli) * ref.MILLI_ONE == len(g.top()) * milli
                   for g in _groups(family)), family


def test_scores_family_is_what_it_says():
    groups = {g.name: g for g in mc.scores_family()}
    for form in ("short", "long"):
        assert max(s for _, s in groups[f"INT32_MAX on top, {form}"].rows) == mc.INT32_MAX
        assert {s for _, s in groups[f"every row INT32_MIN, {form}"].rows} == {mc.INT32_MIN}
        assert {s for _, s in groups[f"INT32_MAX over INT32_MIN, {form}"].rows} == {mc.INT32_MIN, mc.INT32_MAX}
        assert max(s for _, s in groups[f"a negative top, {form}"].rows) < 0
        assert all((len(groups[f"{name}, {form}"].rows) > 64) == (form == "long")
                   for name in ("INT32_MAX on top", "every row INT32_MIN", "INT32_MAX over INT32_MIN", "a negative top"))
    for length in (257, 300, 513):
        g = groups[f"the top rows in the last sweep of {length} rows"]
        t = max(s for _, s in g.rows)
        assert len(g.rows) == length and min(i for i, (_, s) in enumerate(g.rows) if s == t) >= (length - 1) // 256 * 256
    assert sorted(len(g.top()) for name, g in groups.items() if name.startswith("a top group of")) == [256, 256, 257, 257]
    seg, v, d, c = mc.reference(list(groups.values()), 80000)
    assert c["n_narrowed"] >= 12 and c["n_unresolved"] == 0


def test_selection_coverage():
    """the sorted medians of the long groups: pass 0 chooses each of the digits 0 .. 4, passes 1 .. 3 choose 0, 63 and at
    least 32 digits each; the bin-edge groups meet the histogram walk where they say"""
    long_groups = [g for f in ("spread", "digit", "bin edge") for g in LARGE[f]() if len(g.rows) > 64]
    seen = [set() for _ in range(4)]
    skipped_on_entry = [set() for _ in range(4)]
    for g in long_groups:
        for p, (dgt, left_in, left_out, in_bin, before) in enumerate(mc.selection_trace(g.top())):
            assert 0 <= left_out < in_bin and left_in == before + left_out
            seen[p].add(dgt)
            skipped_on_entry[p].add(left_in > 0)
    assert seen[0] == {0, 1, 2, 3, 4}
    for p in (1, 2, 3):
        assert {0, 63} <= seen[p] and len(seen[p]) >= 32, (p, sorted(seen[p]))
        assert skipped_on_entry[p] == {False, True}                      # a count carried into the pass, and none
    for g in mc.bin_edge_family():
        dgt, left_in, left_out, in_bin, before = mc.selection_trace(g.top())[g.claims["p"]]
        if g.claims["edge"] == "first":                                  # left == the rows of the bins in front, which are not empty
            assert left_out == 0 and before == left_in > 0, g.where()
        else:
            assert left_out == in_bin - 1, g.where()
    assert {(g.claims["p"], g.claims["edge"]) for g in mc.bin_edge_family()} == {(p, e) for p in range(4) for e in ("first", "last")}
    # the second form of the digit family: the outliers' next digit is smaller than the majority's, under another top digit
    for g in mc.digit_family():
        if g.claims["form"] == 2:
            top = sorted(g.top())
            major = [p for p in top if p >> 18 == g.claims["t"]]
            out = [p for p in top if p >> 18 != g.claims["t"]]
            assert len(major) == 5 and len(out) == 4 and max(mc.digits(p)[1] for p in out) < min(mc.digits(p)[1] for p in major)


def test_range_coverage():
    """every level k = 0 .. 16 of the sparse table is read by some (row, median) pair.  On the digit table the range's unique
    minimum lies in each of the four places it can at k = 5 .. 13, for every depth of boundary j = 2 .. 6 (the right edge never
    holds it, levels 14 .. 16 only in the overlap or not uniquely: mc.range_family); with the stepped table each of the five
    places holds the unique minimum at every k = 5 .. 16, short and long"""
    ks, places, digit_places = set(), collections.Counter(), collections.Counter()
    js = set()
    for g in mc.range_family() + mc.stepped_range_family():
        lcp = mc.lcp8() if g.tree == "large" else mc.stepped_lcp8()
        top = g.top()
        m = mc.median(top)
        assert m == g.claims["hi"] and len(top) == 4
        for p in top:
            if p != m:
                ks.add(mc.range_parts(min(p, m), max(p, m))[2])
        lo, hi = g.claims["lo"], g.claims["hi"]
        part = lcp[lo:hi]
        assert mc.range_parts(lo, hi)[2] == g.claims["k"]
        if g.claims["unique"]:
            z = lo + int(part.argmin())
            assert (part == part.min()).sum() == 1 and z == g.claims["z"]
            assert mc.range_place(lo, hi, z) == g.claims["place"], g.where()
            places[(g.claims["k"], g.claims["place"], g.claims["form"])] += 1
            if g.tree == "large":
                assert part.min() == mc.LEVELS - 1 - g.claims["j"]
                digit_places[(g.claims["k"], g.claims["place"], g.claims["form"])] += 1
                js.add(g.claims["j"])
        else:
            at = {mc.range_place(lo, hi, lo + int(i)) for i in np.flatnonzero(part == part.min())}
            assert g.claims["k"] is None or g.claims["k"] < 15 or len(at) > 1 or at == {"overlap"}
    assert ks - {None} == set(range(17))
    assert js == {2, 3, 4, 5, 6}
    for form in ("short", "long"):
        for k in range(5, 14):
            for place in mc.RANGE_PLACES:
                assert digit_places[(k, place, form)] >= 2, (k, place, form)
        assert digit_places[(14, "overlap", form)] >= 2
        for k in range(5, 17):
            for place in mc.RANGE_PLACES + ("right edge",):
                assert places[(k, place, form)] >= 1, (k, place, form)
    assert not any(place == "right edge" for _, place, _ in digit_places)
    ends = {(g.claims["lo"], g.claims["hi"]) for g in mc.range_family()}
    assert (0, mc.LARGE_ROWS - 1) in ends and any(lo == 0 for lo, _ in ends) and any(hi == mc.LARGE_ROWS - 1 and lo for lo, hi in ends)
    assert {g.claims["k"] for g in mc.range_family() if g.claims["lo"] < 16 and g.claims["hi"] >= (1 << 20) + 16} == {16}
