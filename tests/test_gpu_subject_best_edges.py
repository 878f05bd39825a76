"""The best-hit-per-subject kernels (csrc/subject_kernel.hip) at their edges: blu_hits_subject_keep and
blu_hits_subject_best on synthetic columns against the restatement (tests/subject_best_reference.py).  Every case runs the
verdicts through device pointers and through host pointers, the compaction through device pointers (in place) and through host
pointers, and a second application to the compacted table; all must agree with the restatement, counts included.  The device
buffers sit between guard words, checked after every call."""
import numpy as np
import pytest
import torch

from blutils_amd import _native as N
from blutils_amd import engine
from tests import subject_best_reference as ref

pytestmark = pytest.mark.gpu

I32_MAX, I32_MIN = (1 << 31) - 1, -(1 << 31)
GUARD = 0x5A5A5A5A
PAD = 64                       # guard elements either side of a device column
QUERIES_PER_BLOCK = 16         # csrc/blu_internal.h: BLU_SUBJECT_QUERIES_PER_WAVE (4) x four waves a block
UNMATCHED = 0xFFFFFFFF
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 5000]
MASK64 = (1 << 64) - 1


def _guarded(values, dtype):
    """a device column with PAD guard elements either side: (the whole buffer, the column's view)"""
    t = {np.int32: torch.int32, np.float64: torch.float64}[dtype]
    buf = torch.full((len(values) + 2 * PAD,), GUARD, dtype=t, device="cuda:0")
    col = buf[PAD:PAD + len(values)]
    col.copy_(torch.from_numpy(np.asarray(values).astype(dtype, copy=False)))
    return buf, col


def _intact(buf, n):
    g = buf.cpu().numpy()
    return (g[:PAD] == GUARD).all() and (g[PAD + n:] == GUARD).all()


def _i32(a):
    return np.asarray(a, np.uint32).view(np.int32)


def check(seg, bs, acc, tiled=True):
    """-> the verdicts (numpy) after asserting that every route gives the restatement's verdicts, columns and counts.  tiled:
    the segments tile the rows (the compaction is compared too)."""
    seg = np.asarray(seg, np.uint64)
    bs = np.asarray(bs, np.int64).astype(np.int32)
    acc = np.asarray(acc, np.uint32)
    n, nq = len(bs), len(seg) - 1
    exp, n_kept, n_thinned = ref.keep(seg, bs, acc)
    exp = np.array(exp, np.uint32)
    want = {"n_hits": n, "n_kept": n_kept, "n_queries": nq, "n_thinned": n_thinned}
    what = (nq, n)
    seg_t = torch.from_numpy(seg.view(np.int64)).to("cuda:0")
    # the verdicts: device pointers, host pointers
    b_buf, b_col = _guarded(bs, np.int32)
    a_buf, a_col = _guarded(_i32(acc), np.int32)
    k_buf, k_col = _guarded(np.full(n, 7), np.int32)
    got = engine.subject_keep_device(seg_t, b_col, a_col, k_col)
    assert _intact(b_buf, n) and _intact(a_buf, n) and _intact(k_buf, n), what
    assert np.array_equal(b_col.cpu().numpy(), bs) and np.array_equal(a_col.cpu().numpy(), _i32(acc)), what
    assert np.array_equal(k_col.cpu().numpy().view(np.uint32), exp), what
    assert got == want, what
    host_keep, got = engine.subject_keep_host(seg, bs, acc)
    assert np.array_equal(host_keep, exp) and got == want, what
    if not tiled:
        return exp
    # the compaction: five columns, seg_off, n_hits and the unmatched count
    aln = np.arange(n, dtype=np.int32) * 3 + 1
    tax = np.where(np.arange(n) % 5 == 2, UNMATCHED, np.arange(n) % 1000).astype(np.uint32)
    pid = np.arange(n, dtype=np.float64) / 8 + 0.125
    new_off, cols = ref.compact(seg.tolist(), exp.tolist(), bs.tolist(), aln.tolist(), tax.tolist(), acc.tolist(), pid.tolist())
    n_un = sum(1 for t in cols[2] if t == UNMATCHED)
    names = ("bitscore", "align_len", "tax_desc_row", "acc_rank", "pident")
    out, got_un, got = engine.subject_best_host(seg, bs, aln, tax, acc, pid)
    assert got == want and got_un == n_un, what
    assert out["seg_off"].tolist() == new_off, what
    for name, c in zip(names, cols):
        assert np.array_equal(out[name], np.array(c, out[name].dtype)), (name, what)
    bufs = [_guarded(bs, np.int32), _guarded(aln, np.int32), _guarded(_i32(tax), np.int32), _guarded(_i32(acc), np.int32),
            _guarded(pid, np.float64)]
    before = [c.clone() for _, c in bufs]
    seg_d = seg_t.clone()
    k, got_un, got = engine.subject_best_device(seg_d, *[c for _, c in bufs])
    assert all(_intact(b, n) for b, _ in bufs), what
    assert (k, got_un, got) == (n_kept, n_un, want), what
    if n_kept == n:                                                      # every row kept: the columns are not touched
        assert all(torch.equal(c, o) for (_, c), o in zip(bufs, before)) and torch.equal(seg_d, seg_t), what
    assert seg_d.cpu().numpy().view(np.uint64).tolist() == new_off, what
    for name, (_, c) in zip(names, bufs):
        g = c[:k].cpu().numpy()
        assert np.array_equal(g.view(out[name].dtype) if g.dtype != out[name].dtype else g, out[name]), (name, what)
    # a second application changes nothing
    k2, un2, again = engine.subject_best_device(seg_d, *[c[:k] for _, c in bufs])
    assert (k2, un2) == (k, n_un) and again == {"n_hits": k, "n_kept": k, "n_queries": nq, "n_thinned": 0}, what
    assert seg_d.cpu().numpy().view(np.uint64).tolist() == new_off and all(_intact(b, n) for b, _ in bufs), what
    return exp


def _segment(rng, n, n_subjects=None, top=1000):
    """n rows over about n / 2 subjects (so that pairs repeat) with scores that tie often"""
    k = max(1, n // 2) if n_subjects is None else n_subjects
    return (top - rng.integers(0, 4, n)).tolist(), rng.integers(0, k, n).tolist()


def _table(rng, lengths, **kw):
    seg, bs, acc = [0], [], []
    for n in lengths:
        b, a = _segment(rng, n, **kw)
        bs += b
        acc += a
        seg.append(len(bs))
    return seg, bs, acc


def test_every_segment_length_alone_and_all_in_one_table():
    rng = np.random.default_rng(101)
    for n in LENGTHS:
        check(*_table(rng, [n]))
    for lengths in (LENGTHS, LENGTHS[::-1]):                             # both paths in one call, empty segments among them
        v = check(*_table(rng, lengths))
        assert 0 < v.sum() < len(v)
    check(*_table(rng, [3, 64, 1, 17, 64, 0, 40]))                       # only short segments: no worklist, no table
    check(*_table(rng, [65, 300, 129, 1000]))                            # only long ones: the worklist is everything


def test_query_counts_around_wave_and_block_tails():
    rng = np.random.default_rng(102)
    for nq in list(range(0, 10)) + [QUERIES_PER_BLOCK - 1, QUERIES_PER_BLOCK, QUERIES_PER_BLOCK + 1, 64 * QUERIES_PER_BLOCK + 1]:
        lens = rng.integers(0, 7, nq)
        if nq > 2:
            lens[nq // 2] = 70                                           # one long query among them
        check(*_table(rng, lens.tolist(), n_subjects=3))
    check([0], [5, 4, 3], [1, 1, 1], tiled=False)                        # no query over rows: every verdict 0
    check([0], [5, 4, 3], [1, 1, 1])                                     # ... and the compaction drops every row, on both routes


def test_placement_of_duplicates():
    for n, spots in ((64, [(0, 63)]), (200, [(63, 64), (0, 199), (64, 128)]), (2, [(0, 1)]), (65, [(0, 64), (63, 64)])):
        for p, r in spots:
            for better in (p, r, None):                                  # the first better, the second better, a tie
                acc = np.arange(n) + 10
                acc[r] = acc[p]
                bs = np.full(n, 400)
                if better is not None:
                    bs[better] = 500
                v = check([0, n], bs, acc)
                loser = r if better in (p, None) else p
                assert v[loser] == 0 and v.sum() == n - 1
    # triples whose best is the first, the middle or the last, in a short and in a long segment
    for n in (9, 130):
        for best in range(3):
            rows = [1, n // 2, n - 1]
            acc = np.arange(n) + 10
            acc[rows] = 7
            bs = np.full(n, 100)
            bs[rows] = [50, 50, 50]
            bs[rows[best]] = 60
            v = check([0, n], bs, acc)
            assert [int(v[r]) for r in rows] == [int(k == best) for k in range(3)]
    # every row one subject: exactly one kept, the first maximum; all distinct: all kept
    for n in (1, 64, 65, 777):
        bs = np.full(n, 5)
        bs[n // 3:] = 9
        v = check([0, n], bs, np.full(n, 3))
        assert v.sum() == 1 and v[n // 3] == 1
        assert check([0, n], bs, np.arange(n)).all()


def test_scores_ties_and_the_sign_boundary():
    for n in (6, 64, 90):
        acc = np.zeros(n, np.int64)
        acc[1::2] = 1                                                    # two subjects interleaved
        check([0, n], np.full(n, 77), acc)                               # all tied: rows 0 and 1 win
        v = check([0, n], np.full(n, -77), acc)
        assert v[:2].tolist() == [1, 1] and v.sum() == 2
        bs = np.full(n, -1)
        bs[2], bs[3], bs[n - 2], bs[n - 1] = I32_MIN, I32_MAX, I32_MAX, I32_MIN
        v = check([0, n], bs, acc)
        assert v[3] == 1 and v[n - 2] == 1 and v.sum() == 2             # INT32_MAX wins in either order, INT32_MIN never
        bs = np.full(n, -1)
        bs[n - 2], bs[n - 1] = 0, 0                                      # 0 over -1: across the bias's sign boundary
        v = check([0, n], bs, acc)
        assert v[n - 2] == 1 and v[n - 1] == 1 and v.sum() == 2
        v = check([0, n], np.where(np.arange(n) < 2, 0, -1), acc)
        assert v[:2].tolist() == [1, 1] and v.sum() == 2
        v = check([0, n], np.full(n, I32_MIN), acc)
        assert v[:2].tolist() == [1, 1] and v.sum() == 2


def test_keys():
    rng = np.random.default_rng(103)
    for n in (8, 100):                                                   # acc_rank 0 and 0xFFFFFFFE side by side
        acc = np.where(np.arange(n) % 2 == 0, 0, 0xFFFFFFFE)
        v = check([0, n], 100 + (np.arange(n) % 5), acc)
        assert v.sum() == 2
    # two queries sharing every accession: nothing merged across queries — long ones, and short ones in one wave
    for n in (100, 20):
        bs, acc = _segment(rng, n)
        bs2 = (np.array(bs) + rng.integers(-2, 3, n)).tolist()
        v = check([0, n, 2 * n], bs + bs2, acc + acc)
        one = check([0, n], bs, acc)
        two = check([0, n], bs2, acc)
        assert np.array_equal(v, np.concatenate([one, two]))
    # a short and a long query sharing them
    bs, acc = _segment(rng, 30, n_subjects=10)
    bl, al = _segment(rng, 300, n_subjects=10)
    check([0, 30, 330], bs + bl, acc + al)


def _home(q, acc, cap):
    """the home slot of the pair (q, acc) in a table of `cap` slots"""
    x = (((q << 32) | acc) * 0x9E3779B97F4A7C15) & MASK64
    return (x ^ (x >> 32)) & (cap - 1)


def _capacity(long_rows):
    """the smallest power of two >= 2 R (and >= 2)"""
    c = 2
    while c < 2 * long_rows:
        c <<= 1
    return c


def _subjects_at(q, cap, slots, count):
    out, a = [], 0
    while len(out) < count:
        if _home(q, a, cap) in slots:
            out.append(a)
        a += 1
    return out


def test_hash_table_load_chains_and_wrap():
    rng = np.random.default_rng(104)
    # all distinct at the design load: R = 256 rows, 256 keys in 512 slots
    assert _capacity(256) == 512
    assert check([0, 256], 1000 - rng.integers(0, 3, 256), rng.permutation(256)).all()
    # 40 subjects with one home slot, each three times: a probe chain of 40; then the chain placed over the table's end
    n = 120
    cap = _capacity(n)
    assert cap == 256
    for slots in ({77}, {cap - 2, cap - 1}, {cap - 1}):
        subj = _subjects_at(0, cap, slots, 40)
        acc = np.array(subj * 3)[rng.permutation(n)]
        bs = 500 + rng.integers(0, 3, n)
        v = check([0, n], bs, acc)
        assert v.sum() == 40
    # the same chain in the second of two long queries (its key holds the query) beside short ones
    subj = _subjects_at(2, _capacity(70 + n), {_capacity(70 + n) - 1}, 40)
    acc = np.array(subj * 3)[rng.permutation(n)]
    b0, a0 = _segment(rng, 70)
    b1, a1 = _segment(rng, 9)
    v = check([0, 70, 79, 79 + n], b0 + b1 + (500 + rng.integers(0, 3, n)).tolist(), a0 + a1 + acc.tolist())
    assert v[79:].sum() == 40


def test_offsets_that_run_past_the_columns_or_backwards():
    rng = np.random.default_rng(105)
    bs, acc = _segment(rng, 300, n_subjects=40)
    check([0, 100, 200, 300 + 5000], bs, acc)                            # the last offset beyond n_hits: clamped
    check([0, 100, 1 << 40, 300], bs, acc, tiled=False)                  # q1 runs to the end, q2 is empty
    check([0, 100, 300, 200], bs, acc, tiled=False)                      # a decreasing pair at the end: an empty segment
    check([0, 30, 10, 10, 10], bs, acc, tiled=False)                     # rows 30 .. 299 unnamed: dropped
    check([(1 << 63), 5, 300], bs, acc, tiled=False)
    # no query at all: n_queries = 0 with and without rows
    check([0], [], [], tiled=False)
    check([0], bs, acc, tiled=False)
    # overlapping long segments whose rows sum to more than n_hits are refused, nothing outside the columns is touched
    seg = np.array([0, 250, 40, 300, 10, MASK64], np.uint64)
    seg_t = torch.from_numpy(seg.view(np.int64)).to("cuda:0")
    b_buf, b_col = _guarded(bs, np.int32)
    a_buf, a_col = _guarded(acc, np.int32)
    k_buf, k_col = _guarded(np.zeros(300), np.int32)
    with pytest.raises(N.BluError):
        engine.subject_keep_device(seg_t, b_col, a_col, k_col)
    assert "overlap" in N.last_error()
    assert _intact(b_buf, 300) and _intact(a_buf, 300) and _intact(k_buf, 300)


def test_a_few_million_rows():
    """4.2 M rows, 675 000 queries, two long ones in each repetition of the block: the scan and the gathers span thousands of blocks.  The expected
    verdicts come from the block the table repeats (a subject shared by two repetitions is two pairs: the query differs)."""
    rng = np.random.default_rng(106)
    lens = rng.integers(1, 12, 3000).tolist()
    lens[100], lens[2000] = 700, 66
    seg, bs, acc = _table(rng, lens)
    v, n_kept, n_thinned = ref.keep(seg, bs, acc)
    reps = 4_200_000 // len(bs) + 1
    n = len(bs) * reps
    seg_all = np.concatenate([[0], (np.array(seg[1:])[None, :] + (np.arange(reps) * len(bs))[:, None]).ravel()]).astype(np.uint64)
    bs_all, acc_all = np.tile(np.array(bs, np.int32), reps), np.tile(np.array(acc, np.uint32), reps)
    exp = np.tile(np.array(v, np.uint32), reps).astype(bool)
    want = {"n_hits": n, "n_kept": n_kept * reps, "n_queries": 3000 * reps, "n_thinned": n_thinned * reps}
    assert n >= 4_000_000 and 0 < n_kept < len(bs)
    seg_t = torch.from_numpy(seg_all.view(np.int64)).to("cuda:0")
    cols = [torch.from_numpy(bs_all).to("cuda:0"), torch.arange(n, dtype=torch.int32, device="cuda:0"),
            torch.from_numpy((np.arange(n) % 977).astype(np.int32)).to("cuda:0"), torch.from_numpy(acc_all.view(np.int32)).to("cuda:0"),
            torch.arange(n, dtype=torch.float64, device="cuda:0")]
    keep = torch.empty(n, dtype=torch.int32, device="cuda:0")
    assert engine.subject_keep_device(seg_t, cols[0], cols[3], keep) == want
    assert np.array_equal(keep.cpu().numpy().astype(bool), exp)
    k, n_un, got = engine.subject_best_device(seg_t, *cols)
    assert (k, n_un, got) == (n_kept * reps, 0, want)
    rows = np.flatnonzero(exp)
    assert np.array_equal(cols[0][:k].cpu().numpy(), bs_all[rows]) and np.array_equal(cols[1][:k].cpu().numpy(), rows.astype(np.int32))
    assert np.array_equal(cols[2][:k].cpu().numpy(), (rows % 977).astype(np.int32))
    assert np.array_equal(cols[3][:k].cpu().numpy().view(np.uint32), acc_all[rows])
    assert np.array_equal(cols[4][:k].cpu().numpy(), rows.astype(np.float64))
    before = np.concatenate([[0], np.cumsum(exp)])
    assert np.array_equal(seg_t.cpu().numpy().view(np.uint64), before[seg_all.astype(np.int64)].astype(np.uint64))
