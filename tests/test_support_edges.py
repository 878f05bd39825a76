"""Keeps tests/support_edges.py honest without a GPU: every coverage set is recomputed from the generated
lineages and the independent sort, the vectorised expected value is held to tests/support_reference.py field for field, and
[lo, hi] to a scan for the rows that share the prefix."""
import numpy as np
import pytest

from tests import support_edges as E
from tests import support_reference as ref


@pytest.fixture
def t(request):
    """The table a test is parametrised with by name (built on first use, not at collection)."""
    return E.table(request.param)


def _sample(t, k=400, seed=0):
    nq = len(t.recs)
    return np.arange(nq) if nq <= k else np.sort(np.random.default_rng(seed).choice(nq, k, replace=False))


# ---- the sort and the ranges ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", E.ALL_TABLES, indirect=True)
def test_sorted_order_and_ranges_against_a_scan(t):
    lineages = None
    if len(t.raw) <= 10000:                                                     # Python's own list order says the same
        lineages = [tuple(l) if not t.length[r] == 0 else () for r, l in enumerate(t.lineages())]
        assert sorted(range(len(lineages)), key=lambda r: (lineages[r], r)) == t.order.tolist()
    assert np.array_equal(np.sort(t.order), np.arange(len(t.raw)))
    assert np.array_equal(t.eng & E.POS_MASK, t.pos_of) and np.array_equal(t.eng >> E.ROW_BITS, t.length)
    assert not np.array_equal(t.order, np.arange(len(t.raw))) or len(t.raw) <= 2
    for q in _sample(t, 300 if len(t.raw) < 100000 else 60):
        if t.recs["status"][q] >= 2:
            assert t.q_lo[q] == -1 and t.q_hi[q] == -1
            continue
        row = int(t.desc[int(t.recs["ref_row"][q])])
        assert t.pos_of[row] == t.q_pos[q], t.where(q)
        need = int(t.recs["level_mask"][q]).bit_length()
        assert need == t.q_need[q]
        got = E.clade_range_brute(t.lin, t.length, t.pos_of, row, need)
        if got is None:
            assert t.q_lo[q] == -1 and t.q_hi[q] == -1, t.where(q)
        else:
            lo, hi, members = got
            assert (lo, hi) == (t.q_lo[q], t.q_hi[q]) and members == hi - lo + 1, t.where(q)
            assert lo <= t.q_pos[q] <= hi


# ---- every hit of an edge query matters -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", E.SMALL_TABLES + ("high_levels",), indirect=True)
def test_edge_queries_hold_their_probe_rows_and_every_one_of_them_counts(t):
    n = len(t.raw)
    for q in _sample(t, 500):
        a, b = int(t.seg[q]), int(t.seg[q + 1])
        rows, sc = t.desc[a:b], t.bs[a:b].astype(np.int64)
        assert sc.max() == E.TOP == sc[int(t.recs["ref_row"][q]) - a] and t.recs["status"][q] == 0
        assert (rows == -1).sum() >= 1                                          # an unmatched hit
        pos = set(t.pos_of[rows[rows >= 0]].tolist())
        lo, hi = (int(t.q_lo[q]), int(t.q_hi[q])) if t.q_lo[q] >= 0 else (int(t.q_pos[q]), int(t.q_pos[q]))
        want = {p for p in (lo - 1, lo, lo + 1, hi - 1, hi, hi + 1) if 0 <= p < n} | {int(t.q_pos[q])}
        assert want <= pos, t.where(q)
        if lo > 1 or hi < n - 2:
            assert any(p < lo - 1 or p > hi + 1 for p in pos), t.where(q)       # a far row
        # a row whose verdict flips moves n_support (it has a hit), n_top_support (a hit on the maximum) and support_bits
        # (its scores do not cancel; they are the maximum and a power of two no other row has)
        low = []
        for r in set(rows.tolist()):
            mine = sc[rows == r]
            if r >= 0 and t.length[r] and r != t.desc[int(t.recs["ref_row"][q])]:
                assert (mine == E.TOP).sum() == 1 and len(mine) == 2 and mine.sum() > E.TOP, t.where(q)
                low.append(int(mine.min()))
        assert len(set(low)) == len(low) and all(x & (x - 1) == 0 for x in low)


# ---- the coverage sets of the issue ---------------------------------------------------------------------------------------------

def test_near_sweep_covers_every_distance_at_every_alignment():
    t = E.near_sweep()
    assert 8200 <= len(t.raw) <= 8400 and len(t.recs) == 128 * 129 // 2
    to_lo, to_hi = E.near_coverage(t)
    want = {(d, r) for d in range(97) for r in range(16)}
    assert want <= to_lo and want <= to_hi
    assert set((t.q_lo % 16).tolist()) == set(range(16)) and (t.q_need == 2).all()
    assert t.q_lo.min() == 1 and t.q_hi.max() == len(t.raw) - 2                 # a row outside on either side


def test_skip_path_covers_blocks_residues_and_reference_places():
    t = E.skip_path()
    up, down, from_lo, from_hi = set(), set(), set(), set()
    for q in range(len(t.recs)):
        pos, lo, hi = int(t.q_pos[q]), int(t.q_lo[q]), int(t.q_hi[q])
        u, d = E.skipped_blocks(pos, lo, hi)
        if u is not None:
            up.add((u, hi % 16))
        if d is not None:
            down.add((d, lo % 16))
        from_lo.add(pos - lo)
        from_hi.add(hi - pos)
    want = {(s, r) for s in E.SKIP_BLOCKS for r in range(16)}
    assert want <= up and want <= down
    assert set(E.END_DISTANCES) <= from_lo and set(E.END_DISTANCES) <= from_hi
    assert max(from_lo) >= 128 + 16 * 257 and max(from_hi) >= 128 + 16 * 257
    assert t.q_lo.min() == 0 and t.q_hi.max() == len(t.raw) - 1                 # a long clade at either end of the table
    ends = t.q_hi == len(t.raw) - 1
    assert (t.q_hi[ends] - t.q_pos[ends]).max() > 4000 and (t.q_pos[t.q_lo == 0]).max() > 4000


def test_high_levels_reach_the_top_of_the_sparse_table():
    t = E.high_levels()
    n = len(t.raw)
    assert n == (1 << 20) + 40
    nb = (n - 1 + 15) // 16 + 1                                                 # taxonomy.cpp: blocks per level
    assert nb.bit_length() == 17                                                # levels 0 .. 16
    spans = {(int(lo), int(hi)) for lo, hi in zip(t.q_lo, t.q_hi)}
    whole = (t.q_lo == 0) & (t.q_hi == n - 1)
    assert whole.any() and (t.recs["level_mask"][whole] == 1).all()
    assert any(lo > 0 and hi == n - 1 for lo, hi in spans) and any(lo == 0 and hi < n - 1 for lo, hi in spans)
    sizes = {(hi - lo + 1, lo % 16 == 0) for lo, hi in spans}
    for k in (4, 8, 12):
        for blocks in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            assert (16 * blocks, True) in sizes and (16 * blocks, False) in sizes, (k, blocks)
    assert {16 * ((1 << 16) + d) for d in (-1, 0, 1)} <= {s for s, _ in sizes}  # (nested: one start each)
    for lo, hi in spans:                                                        # first, middle and last row of every clade
        at = set(t.q_pos[(t.q_lo == lo) & (t.q_hi == hi)].tolist())
        assert {lo, (lo + hi) // 2, hi} <= at


def test_table_ends_cover_the_sizes_and_the_four_clades():
    tables = E.table_ends()
    assert tuple(len(t.raw) for t in tables) == E.TABLE_SIZES
    for t in tables:
        n = len(t.raw)
        spans = {(int(lo), int(hi)) for lo, hi in zip(t.q_lo, t.q_hi)}
        want = {(0, n - 1), (n - 1, n - 1), (0, 0)} | ({(n - 2, n - 1)} if n >= 2 else set())
        assert want <= spans, (n, spans)
        assert set(t.q_pos.tolist()) == set(range(n))


def test_levels_cover_needs_duplicates_prefixes_and_bad_rows():
    plain, with_bad = E.levels()
    for t in (plain, with_bad):
        lens = t.length[t.order[t.q_pos]]
        assert {1, 2, 3, 4} <= set(t.q_need[lens == 5].tolist())
        assert {63, 64} <= set(t.q_need[lens == 64].tolist())
        assert ((t.q_need > lens) & (t.q_lo == -1)).any() and ((t.q_need == lens) & (t.q_lo >= 0)).any()
        assert (t.recs["level_mask"] == 0).any() and (t.recs["level_mask"] >> np.uint64(63) == 1).any()
        exp = t.expected()
        assert not exp["n_support"][t.q_need > lens].any()
        # nested clades around one row
        row = int(np.nonzero((t.raw[:, :5] == [1, 2, 3, 4, 52]).all(axis=1) & (t.length == 5))[0][0])
        sizes = [int(t.q_hi[q] - t.q_lo[q] + 1) for need in (1, 2, 3, 4, 5)
                 for q in np.nonzero((t.q_pos == t.pos_of[row]) & (t.q_need == need))[0][:1]]
        assert sizes == sorted(sizes, reverse=True) and len(set(sizes)) == 5 and sizes[-1] == 1
        # a lineage listed twice and three times: inside one range, at its first and its last position
        sorted_lin = t.lin[t.order]
        same = (sorted_lin[1:] == sorted_lin[:-1]).all(axis=1) & (t.length[t.order][1:] > 0)
        dup_pos = set(np.nonzero(same)[0].tolist())
        assert any(p in dup_pos for p in t.q_lo.tolist()) and any(p - 1 in dup_pos for p in t.q_hi.tolist())
        assert any(p in dup_pos and p + 1 in dup_pos for p in t.q_lo.tolist())  # three in a row
        # the prefix [1, 6] in front of its extensions, the mask at each length
        p6 = [int(t.pos_of[np.nonzero((t.length == k) & (t.raw[:, :2] == [1, 6]).all(axis=1) & (t.raw[:, 2] != 61))[0][0]]) for k in (2, 3, 4, 5)]
        assert p6 == list(range(p6[0], p6[0] + 4))
        for k in (2, 3, 4, 5):
            assert ((t.q_pos == p6[3]) & (t.q_need == k) & (t.q_lo == p6[k - 2])).any()
    t = with_bad
    n_bad = int((t.length == 0).sum())
    assert n_bad == 4 and t.bad.sum() == 3 and (t.raw_len[t.bad != 0] > 0).all()
    assert (t.pos_of[t.length == 0] < n_bad).all() and (t.q_lo == n_bad).any()  # a bad row at lo - 1
    unplaced = t.recs["level_mask"] == 0
    for q in np.nonzero(unplaced)[0]:                                           # bad rows inside [0, n_tax - 1] as hits
        rows = t.desc[int(t.seg[q]):int(t.seg[q + 1])]
        assert (t.length[rows[rows >= 0]] == 0).any()
    flagged = np.nonzero(t.bad != 0)[0]
    clade_rows = np.nonzero((t.raw[:, :4] == [1, 2, 3, 4]).all(axis=1))[0]
    assert clade_rows.min() < flagged.max() and flagged.min() < clade_rows.max()


def test_segment_scan_covers_lengths_maxima_and_extremes():
    t = E.segment_scan()
    exp = t.expected()
    lens = (t.seg[1:] - t.seg[:-1]).astype(np.int64)
    assert set(lens.tolist()) == set(E.SCAN_LENGTHS)
    for n in E.SCAN_LENGTHS[1:]:
        qs = np.nonzero(lens == n)[0]
        at = set()
        for q in qs:
            sc = t.bs[int(t.seg[q]):int(t.seg[q + 1])]
            top = np.nonzero(sc == sc.max())[0]
            if len(top) == 1:
                at.add(int(top[0]))
        assert {k for k in (0, 63, 64, n - 1) if k < n} <= at, (n, at)
        assert any(k >= (n - 1) // 64 * 64 for k in at)                         # in the last partial step only
        for v in (E.INT32_MIN, E.INT32_MAX):
            assert (exp["top_score"][qs] == v).any() and ((exp["n_top"][qs] == n) & (exp["top_score"][qs] == v)).any()
    q = np.nonzero(lens == 4097)[0]
    assert (exp["bits"][q] > 1 << 32).any() and (exp["bits"][q] < -(1 << 32)).any()
    assert (exp["support_bits"][q] > 1 << 32).any() and (exp["support_bits"][q] < -(1 << 32)).any()
    big = np.abs(exp["bits"]) > 1 << 32
    assert (exp["support_bits"][big] != exp["bits"][big]).all() and (exp["support_bits"][big] != 0).all()
    tied = (exp["n_top"] > 1) & (exp["n_top"] < exp["n_hits"])
    assert tied.sum() >= 8 and ((exp["n_top_support"] < exp["n_top"]) & tied).any()
    # the maximum twice in one lane, and in several lanes of one step
    seen_lane = seen_step = False
    for q in np.nonzero(tied)[0]:
        sc = t.bs[int(t.seg[q]):int(t.seg[q + 1])]
        top = np.nonzero(sc == sc.max())[0]
        seen_lane |= len(set((top % 64).tolist())) < len(top)
        seen_step |= len(set((top // 64).tolist())) < len(top)
    assert seen_lane and seen_step


def test_hostile_offsets_are_the_documented_kinds():
    for t, limit in ((E.hostile_offsets(), None), (E.hostile_offsets_inside_allocation(), E.HOSTILE_ALLOC)):
        seg, n = t.seg.astype(object), E.HOSTILE_HITS
        assert len(t.bs) == n and (t.recs["status"] >= 2).all() and (t.recs["ref_row"] == E.U32_MAX).all()
        assert seg[-1] > n and any(a > b for a, b in zip(seg[:-1], seg[1:])) and any(a == n for a in seg[:-1])
        assert limit is None or max(seg) <= limit
        exp = t.expected()
        want = [max(0, min(b, n) - min(a, min(b, n))) for a, b in zip(seg[:-1], seg[1:])]
        assert exp["n_hits"].tolist() == want and want[-1] > 0 and 0 in want
        assert not exp["n_support"].any() and exp["n_matched"].sum() > 0
        q = len(want) - 1                                                       # the last segment: clamped, not empty
        assert exp["bits"][q] == int(t.bs[n - want[-1]:].astype(np.int64).sum())


# ---- the expected value against the plain restatement ---------------------------------------------------------------------------

def _reference_on(t, queries):
    """tests/support_reference.py on `queries` of the table, with only the lineages those queries name."""
    seg, bs, desc, recs = [0], [], [], t.recs[queries].copy()
    for k, q in enumerate(queries):
        a, b = int(t.seg[q]), int(t.seg[q + 1])
        if recs["status"][k] < 2:
            recs["ref_row"][k] = int(recs["ref_row"][k]) - a + seg[-1]
        bs.extend(t.bs[a:b].tolist()); desc.extend(t.desc[a:b].tolist()); seg.append(seg[-1] + b - a)
    desc = np.array(desc, np.int64)
    used = np.unique(desc[desc >= 0])
    remap = {int(r): i for i, r in enumerate(used)}
    small = np.array([remap.get(int(d), -1) for d in desc], np.int64)
    lineages = [[int(x) for x in t.raw[r, :t.raw_len[r]]] for r in used]
    bad = None if t.bad is None else t.bad[used]
    return ref.support(np.array(seg, np.uint64), np.array(bs, np.int32), small, lineages, bad, recs)


@pytest.mark.parametrize("t", E.ALL_TABLES, indirect=True)
def test_expected_equals_the_plain_restatement_and_keeps_the_invariants(t):
    exp = t.expected()
    E.assert_invariants(exp, t)
    queries = _sample(t, 2500 if len(t.bs) < 200000 else 150, seed=1)
    plain = _reference_on(t, queries)
    for f in ref.SUPPORT_FIELDS:
        bad = np.nonzero(plain[f] != exp[f][queries])[0]
        assert len(bad) == 0, (f, t.where(int(queries[bad[0]])), plain[f][bad[0]], exp[f][queries[bad[0]]])
    placed = t.recs["status"] < 2
    assert (exp["n_support"][placed & (t.q_lo >= 0)] >= 1).all()


def test_packed_rows_keep_word_zero():
    eng = np.arange(10, dtype=np.uint32) * 77
    for words in (4, 6):
        ones, noise = E.packed_rows(eng, words, "ones"), E.packed_rows(eng, words, "noise", 3)
        assert ones.shape == noise.shape == (10, words) and (ones[:, 0] == eng).all() and (noise[:, 0] == eng).all()
        assert (ones[:, 1:] == 0xFFFFFFFF).all() and len(np.unique(noise[:, 1:])) > 5 * words
