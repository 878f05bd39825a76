"""The minimum cover's kernels (csrc/cover_kernel.hip) on the case families of tests/min_cover_edges.py: top
groups at sorted positions up to 2^20 + 39, where the long kernel's radix selection chooses digits other than 0 in every
pass and the range minimum reads every level of the sparse table; query counts around a wave, a block and the 64 counter
words; the extremes of the score.  Verdicts, d* and counts against tests/min_cover_reference.py through the four routes of
tests/test_gpu_min_cover_edges.Table.check (host and device pointers, engine ids and desc rows under the row map).  A failure
names the family, the group, the sorted median with its four selection digits, the route and the field that differs first."""
import numpy as np
import pytest
import torch

from blutils_amd import engine
from tests import min_cover_edges as mc
from tests.test_gpu_min_cover_edges import Table, Tax

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def large():
    """the table of 2^20 + 40 rows, built once: the library's row map equals the independent sort (Tax), which puts the row of
    digits p at position p"""
    m, perm = mc.large_matrix()
    tx = Tax(matrix=m)
    assert np.array_equal(tx.pos_of, perm)
    return tx


@pytest.fixture(scope="module")
def stepped():
    """the second table of 2^20 + 40 rows (mc.stepped_lineage_of): lineages of 8 and 9 levels, two entries of lcp8 below 2"""
    m, perm = mc.stepped_matrix()
    tx = Tax(matrix=m)
    assert np.array_equal(tx.pos_of, perm)
    return tx


@pytest.fixture(scope="module")
def small():
    return Tax(mc.small_tree())


def _table(tx, groups):
    t = Table(tx)
    for g in groups:
        rows = [(r if r < 0 or g.tree == "small" else tx.row_at(r), s) for r, s in g.rows]   # (a position -> the row that holds it)
        t.query(rows, note=g.where())
    return t


def test_spread(large):
    groups = mc.spread_family()
    t = _table(large, groups)
    v, d, c = t.check(50001, narrowed=True, unresolved=False)
    assert c["n_narrowed"] == len(groups)
    t.check(80000, unresolved=False)


def test_digit(large):
    groups = mc.digit_family()
    t = _table(large, groups)
    v, d, c = t.check(50001, narrowed=True, unresolved=False)
    assert c["n_narrowed"] == len(groups) and set(d) == {6}              # the block of eight covers, the outliers go
    t.check(100000, narrowed=False, unresolved=False)


def test_bin_edge(large):
    groups = mc.bin_edge_family()
    t = _table(large, groups)
    v, d, c = t.check(50001, narrowed=True, unresolved=False)
    assert c["n_narrowed"] == len(groups) and set(d) == {6, 7}
    t.check(100000, narrowed=False, unresolved=False)


def test_range(large, stepped):
    groups = mc.range_family()
    t = _table(large, groups)
    v, d, c = t.check(75000, narrowed=True, unresolved=False)
    assert d == [mc.share(g.claims["lo"], g.claims["hi"]) for g in groups]       # (the reference's d*, said once more from the digits)
    assert c["n_narrowed"] == sum(1 for x in d if x > 0) >= 800
    groups = mc.stepped_range_family()
    t = _table(stepped, groups)
    v, d, c = t.check(75000, narrowed=True, unresolved=False)
    assert d == [mc.stepped_share(g.claims["lo"], g.claims["hi"]) for g in groups]
    assert c["n_narrowed"] == sum(1 for x in d if x > 0) >= 150


def test_queries(small):
    for count, groups in mc.queries_family().items():
        t = _table(small, groups)
        v, d, c = t.check(80000, narrowed=count >= 1, unresolved=count >= 4)
        assert c["n_queries"] == count
        t.check(50001)


def test_queries_repeated_block(small):
    """a block of 42 queries, every seventh long, 7000 times: 294 000 queries (4 594 blocks of the short kernel on the 64 counter
    words, 288 blocks of the flag scan), 42 000 long queries; the reference is computed on the block and every repetition is
    held to it"""
    block, times, milli = mc.repeated_block(), mc.REPEAT_TIMES, 80000
    seg, want_v, want_d, want_c = mc.reference(block, milli)
    assert want_c["n_narrowed"] > 0 and want_c["n_unresolved"] > 0
    n_rows, n_q = seg[-1], len(block)
    desc1 = np.array([r if r >= 0 else 0xFFFFFFFF for g in block for r, _ in g.rows], np.uint32)
    ids1 = np.where(desc1 == 0xFFFFFFFF, 0xFFFFFFFF, small.eng[np.minimum(desc1, len(small.eng) - 1)]).astype(np.uint32)
    bs = np.tile(np.array([s for g in block for _, s in g.rows], np.int32), times)
    offs = (np.arange(times, dtype=np.uint64)[:, None] * np.uint64(n_rows) + np.array(seg[:-1], np.uint64)[None, :]).reshape(-1)
    seg_all = np.concatenate([offs, np.array([times * n_rows], np.uint64)])
    want_c = {k: x * times for k, x in want_c.items()}
    want_v, want_d = np.array(want_v), np.array(want_d)

    def same(route, v, d, c):
        v, d = np.asarray(v).reshape(times, n_rows), np.asarray(d).reshape(times, n_q)
        bad = np.argwhere(d != want_d[None, :])
        assert len(bad) == 0, (route, "d* differs at repetition, query", bad[0].tolist(), block[bad[0][1]].where())
        bad = np.argwhere(v != want_v[None, :])
        assert len(bad) == 0, (route, "verdicts differ at repetition, row", bad[0].tolist())
        assert c == want_c, (route, "counts differ", c, want_c)

    t_seg = torch.tensor(seg_all.view(np.int64), device="cuda")
    t_bs = torch.tensor(bs, device="cuda")
    t_map = torch.tensor(small.eng.view(np.int32), device="cuda")
    for name, rows1, use_map in (("ids", ids1, False), ("desc", desc1, True)):
        rows = np.tile(rows1, times)
        v, d, c = engine.cover_keep_host(small.tax, seg_all, bs, rows, milli, row_map=True if use_map else None)
        same(f"host/{name}", v, d, c)
        t_keep = torch.full((len(bs),), 7, dtype=torch.int32, device="cuda")
        t_depth = torch.full((times * n_q,), 9, dtype=torch.uint8, device="cuda")
        c = engine.cover_keep_device(small.tax, t_seg, t_bs, torch.tensor(rows.view(np.int32), device="cuda"), milli, t_keep, t_depth,
                                     row_map=t_map if use_map else None)
        same(f"device/{name}", t_keep.cpu().numpy(), t_depth.cpu().numpy(), c)


def test_scores(small):
    groups = mc.scores_family()
    t = _table(small, groups)
    v, d, c = t.check(80000, narrowed=True, unresolved=False)
    assert c["n_narrowed"] >= 12
    t.check(50001, narrowed=True, unresolved=False)
    t.check(100000, narrowed=False, unresolved=False)
