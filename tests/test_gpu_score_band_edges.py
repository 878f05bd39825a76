"""The band kernel (csrc/band_kernel.hip: score_band_kernel) at its edges: blu_hits_score_band on synthetic
columns against the restatement in plain integers (tests/score_band_reference.py).  Every case runs four ways — device pointers
in place, device pointers out of place, host pointers, and a second application to the raised column — and all four must agree
with the restatement, counts included.  The device columns sit between guard words, checked after every call."""
import ctypes as C

import numpy as np
import pytest
import torch

from blutils_amd import _native as N
from blutils_amd import engine
from tests import score_band_reference as ref

pytestmark = pytest.mark.gpu

I32_MAX, I32_MIN = (1 << 31) - 1, -(1 << 31)
GUARD = 0x5A5A5A5A
PAD = 64                       # guard words either side of a device column
QUERIES_PER_BLOCK = 16         # csrc/blu_internal.h: BLU_BAND_QUERIES_PER_WAVE (4) x four waves a block
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 4097]
BANDS = [dict(m=100), dict(m=5000), dict(D=3), dict(m=1000, D=2), dict(m=100000), dict(D=(1 << 32) - 1)]


def _guarded(values):
    """a device int32 column with PAD guard words either side: (the whole buffer, the column's view)"""
    buf = torch.full((len(values) + 2 * PAD,), GUARD, dtype=torch.int32, device="cuda:0")
    col = buf[PAD:PAD + len(values)]
    col.copy_(torch.from_numpy(np.asarray(values, np.int32)))
    return buf, col


def _guards_intact(buf, n):
    g = buf.cpu().numpy()
    return (g[:PAD] == GUARD).all() and (g[PAD + n:] == GUARD).all()


def _counts(n_hits, n_queries, n_raised, n_widened):
    return {"n_hits": n_hits, "n_raised": n_raised, "n_queries": n_queries, "n_widened": n_widened}


def four_ways(seg, bs, m=None, D=None):
    """-> the raised column (numpy) after asserting that all four routes give the restatement's column and counts"""
    seg = np.asarray(seg, np.uint64)
    bs = np.asarray(bs, np.int32)
    n, nq = len(bs), len(seg) - 1
    exp, n_raised, n_widened = ref.raise_scores(seg, bs, m, D)
    exp = np.array(exp, np.int32)
    want = _counts(n, nq, n_raised, n_widened)
    seg_t = torch.from_numpy(seg.view(np.int64)).to("cuda:0")
    what = (m, D, nq, n)
    # device pointers, in place
    buf, col = _guarded(bs)
    got = engine.score_band_device(seg_t, col, m, D)
    assert _guards_intact(buf, n), what
    assert np.array_equal(col.cpu().numpy(), exp), what
    assert got == want, what
    # a second application: the raised column is unchanged and nothing counts as raised
    again = engine.score_band_device(seg_t, col, m, D)
    assert _guards_intact(buf, n) and np.array_equal(col.cpu().numpy(), exp), what
    assert again == _counts(n, nq, 0, 0), what
    # device pointers, out of place: the input is left as it was
    ibuf, icol = _guarded(bs)
    obuf, ocol = _guarded(bs)                    # (rows no segment names are not written: they start as the input's)
    got = engine.score_band_device(seg_t, icol, m, D, out=ocol)
    assert _guards_intact(ibuf, n) and _guards_intact(obuf, n), what
    assert np.array_equal(icol.cpu().numpy(), bs) and np.array_equal(ocol.cpu().numpy(), exp), what
    assert got == want, what
    # host pointers
    out, got = engine.score_band_host(seg, bs, m, D)
    assert np.array_equal(out, exp) and got == want, what
    return exp


def _near_top(rng, n, top=1000, spread=12):
    """scores within `spread` of `top`, the top itself present"""
    v = top - rng.integers(0, spread + 1, n)
    if n:
        v[int(rng.integers(0, n))] = top
    return v


def test_every_segment_length_alone():
    rng = np.random.default_rng(71)
    for n in LENGTHS:
        bs = _near_top(rng, n)
        for band in BANDS:
            four_ways([0, n], bs, **band)
    # what the lengths were chosen for: a raised row in the first, a middle and the last sweep of the longest
    out = four_ways([0, 4097], np.r_[999, np.full(2000, 5), 999, np.full(2094, 5), 1000], D=1)
    assert out[0] == 1000 and out[2001] == 1000 and (out == 5).sum() == 4094


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_all_lengths_in_one_table_with_empty_segments_between(order):
    rng = np.random.default_rng(72)
    lengths = LENGTHS if order == "ascending" else LENGTHS[::-1]
    seg, bs = [0], []
    for n in lengths:
        bs.extend(_near_top(rng, n, top=int(rng.integers(20, 3000))).tolist())
        seg += [len(bs), len(bs)]                                        # (an empty segment after each)
    seg = seg[:-1] if order == "ascending" else seg                      # the last query ends at n_hits either way
    assert seg[-1] == len(bs)
    for band in BANDS:
        four_ways(seg, bs, **band)


def test_query_counts_around_every_block_multiple():
    rng = np.random.default_rng(73)
    counts = {0, 1, 3, 4, 5}
    for k in range(1, 5):
        counts |= {k * QUERIES_PER_BLOCK - 1, k * QUERIES_PER_BLOCK, k * QUERIES_PER_BLOCK + 1}
    counts |= {k * 4 + d for k in range(1, 5) for d in (-1, 0, 1)}       # a wave's four queries
    counts |= {64 * QUERIES_PER_BLOCK + d for d in (-1, 0, 1)}           # the counter words wrap: block 64 adds to word 0 again
    for nq in sorted(counts):
        lens = rng.integers(0, 6, nq)
        if nq:
            lens[-1] = max(lens[-1], 1)                                  # the last query ends at n_hits with a row of its own
        seg = np.concatenate([[0], np.cumsum(lens)])
        bs = _near_top(rng, int(seg[-1]), spread=4)
        four_ways(seg, bs, D=2)
        four_ways(seg, bs, m=200)
    # no query at all over a column that has rows: nothing is raised
    four_ways([0], [5, 4, 3], D=9)


def test_position_of_the_maximum_and_of_the_only_in_band_row():
    for n in (256, 200, 65):
        last = n - 1
        spots = sorted({0, 63, 64, min(127, last), min(128, last), min(191, last), (last // 64) * 64, last})
        for p in spots:                                                  # the maximum
            for r in spots:                                              # the only row in the band
                if r == p:
                    continue
                bs = np.full(n, 400)
                bs[p], bs[r] = 500, 499
                out = four_ways([0, n], bs, D=1)
                assert out[r] == 500 and (out == 500).sum() == 2
    # short segments: the first and the last row, lanes 0 and 63
    for n in (2, 64):
        for p, r in ((0, n - 1), (n - 1, 0)):
            bs = np.full(n, 400)
            bs[p], bs[r] = 500, 499
            four_ways([0, n], bs, m=200)


@pytest.mark.parametrize("n", [5, 64, 65, 300])
def test_value_patterns(n):
    for band in BANDS:
        four_ways([0, n], np.full(n, 777), **band)                       # all equal: nothing to raise
        four_ways([0, n], 2000 - np.arange(n), **band)                   # strictly decreasing: BLAST's order
        four_ways([0, n], 1000 + np.arange(n), **band)                   # strictly increasing
    # INT32_MAX on top with the widest bands: t - D and b * 100000 leave 32 bits
    bs = np.array([I32_MAX - i * 1000003 for i in range(n)], np.int64)
    bs[n // 2:] = -bs[n // 2:]
    bs[-1] = I32_MIN
    for band in (dict(D=(1 << 32) - 1), dict(m=100000), dict(m=100000, D=(1 << 32) - 1), dict(m=10000), dict(D=I32_MAX)):
        out = four_ways([0, n], bs, **band)
        if band.get("m") == 100000:
            assert ((out == I32_MAX) == (bs >= 0)).all()                 # every row >= 0 is raised, negative rows are not
        elif band == dict(D=(1 << 32) - 1):
            assert (out == I32_MAX).all()                                # INT32_MIN >= INT32_MAX - (2^32 - 1)
    # a negative top: nothing is raised under percent, bits still raises
    neg = -5 - np.arange(n)
    assert np.array_equal(four_ways([0, n], neg, m=100000), neg)
    assert (four_ways([0, n], neg, D=2)[:3] == -5).all()
    assert np.array_equal(four_ways([0, n], neg, m=100000, D=2), neg)
    # INT32_MIN rows under INT32_MIN + 1
    low = np.full(n, I32_MIN, np.int64)
    low[n - 1] = I32_MIN + 1
    assert (four_ways([0, n], low, D=1) == I32_MIN + 1).all()
    assert np.array_equal(four_ways([0, n], low, m=100000), low)


def test_boundaries():
    for t, band, inside, outside in ((1000, dict(m=100), 999, 998), (370, dict(m=5000), 352, 351),
                                     (2147483647, dict(m=10000), 1932735283, 1932735282), (500, dict(D=3), 497, 496)):
        for fill in (3, 64, 65, 130):                                    # both sweeps' forms
            bs = np.full(fill, outside, np.int64)
            bs[0], bs[fill // 2], bs[-1] = inside, t, outside
            out = four_ways([0, fill], bs, **band)
            assert out[0] == t and out[-1] == outside and (out == t).sum() == 2
    # both flags: a row inside one criterion and outside the other stays
    out = four_ways([0, 4], [1000, 999, 998, 990], m=1000, D=1)          # 998 is inside 1 % and outside 1 bit
    assert out.tolist() == [1000, 1000, 998, 990]
    out = four_ways([0, 4], [1000, 999, 998, 990], m=100, D=5)           # 998 is inside 5 bits and outside 0.1 %
    assert out.tolist() == [1000, 1000, 998, 990]


def test_zero_widths_and_an_empty_mask_leave_the_column():
    rng = np.random.default_rng(74)
    lens = rng.integers(0, 200, 50)
    seg = np.concatenate([[0], np.cumsum(lens)])
    bs = _near_top(rng, int(seg[-1]))
    for band in (dict(m=0), dict(D=0), dict(m=0, D=0), dict(m=0, D=50), dict(m=5000, D=0), dict()):
        assert np.array_equal(four_ways(seg, bs, **band), bs)
    # an empty mask through the struct, and no band at all
    L = N.lib()
    for band in (N.ScoreBandC(5000, 0, 3), None):
        buf, col = _guarded(bs)
        out = torch.zeros_like(col)
        st = N.ScoreBandStats()
        seg_t = torch.from_numpy(seg.astype(np.uint64).view(np.int64)).to("cuda:0")
        for dst in (col, out):
            rc = L.blu_hits_score_band(0, col.data_ptr(), seg_t.data_ptr(), len(bs), len(seg) - 1, 1,
                                       C.byref(band) if band is not None else None, None, dst.data_ptr(), C.byref(st))
            assert rc == N.BLU_OK and np.array_equal(dst.cpu().numpy(), bs) and _guards_intact(buf, len(bs))
            assert (st.n_hits, st.n_raised, st.n_queries, st.n_widened) == (len(bs), 0, len(seg) - 1, 0)


def test_offsets_that_run_past_the_column_or_backwards():
    """The call returns, nothing outside the column is touched, and where the segments do not overlap the rows are the
    restatement's (which clamps and empties the same way)."""
    bs = 1000 - (np.arange(300) % 7)
    bs[::7] = 1000
    # an offset beyond n_hits (the last, and one in the middle), a decreasing pair
    four_ways([0, 100, 200, 300 + 5000], bs, D=3)
    four_ways([0, 100, 1 << 40, 300], bs, D=3)                           # (q1 runs to the end, q2 is empty)
    four_ways([0, 200, 100, 100, 100], bs, D=3)                          # decreasing, then empty ones: rows 200 .. 299 unnamed
    four_ways([(1 << 63), 5, 300], bs, D=3)
    # overlapping segments: only that the call returns and the guards hold
    seg = np.array([0, 250, 40, 300, 10, (1 << 64) - 1], np.uint64)
    seg_t = torch.from_numpy(seg.view(np.int64)).to("cuda:0")
    buf, col = _guarded(bs)
    engine.score_band_device(seg_t, col, None, 3)
    assert _guards_intact(buf, len(bs))
    obuf, ocol = _guarded(bs)
    engine.score_band_device(seg_t, col, 100000, None, out=ocol)
    assert _guards_intact(buf, len(bs)) and _guards_intact(obuf, len(bs))
    engine.score_band_host(seg, bs, 100000, 7)
