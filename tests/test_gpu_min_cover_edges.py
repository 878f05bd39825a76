"""Edge cases of the minimum cover's kernels (csrc/cover_kernel.hip) on tables built by hand: the verdicts, d*
and the counts against tests/min_cover_reference.py, which counts prefix tuples in a dict and knows no sorted position, no
median and no range minimum.  Every table goes through the host-pointer and the device-pointer route, with engine row ids
(row_map NULL) and with desc rows under a row map.  The sorted order the engine ids are made of is numpy's
(tests/support_edges.sort_rows), checked against the library's row map."""
import numpy as np
import pytest
import torch

from blutils_amd import engine, synth
from tests import min_cover_reference as ref
from tests import support_edges as se

pytestmark = pytest.mark.gpu

UNMATCHED = 0xFFFFFFFF
TOP = 1000


class _RowLineages:
    """row -> its lineage as the reference takes it, read from the matrix when asked for"""

    def __init__(self, lin, length):
        self.lin, self.length = lin, length

    def __getitem__(self, t):
        return tuple(int(x) for x in self.lin[t, :self.length[t]])


class Tax:
    """lineages (lists of node ids; bad rows flagged), or their [n, depth] matrix padded with -1 -> the library's handle, the
    independent engine row ids, and each row's lineage as the reference takes it"""

    def __init__(self, lineages=None, bad=(), matrix=None):
        if matrix is None:
            self.lineages = [list(l) for l in lineages]
            raw, raw_len = se.to_matrix(self.lineages)
        else:                                                            # (a table too large to go through lists)
            raw, raw_len = matrix, (matrix >= 0).sum(axis=1).astype(np.int64)
        n = len(raw)
        self.bad = np.zeros(n, np.uint8)
        self.bad[list(bad)] = 1
        lin = raw.copy()
        lin[self.bad != 0] = -1
        length = np.where(self.bad != 0, 0, raw_len)
        order = se.sort_rows(lin)
        self.pos_of = np.empty(n, np.int64)
        self.pos_of[order] = np.arange(n)
        self.order = order
        self.eng = (self.pos_of | (length << se.ROW_BITS)).astype(np.uint32)
        lin_off = np.concatenate([[0], np.cumsum(raw_len)]).astype(np.uint64)
        node = raw[raw >= 0].astype(np.uint32)
        rank = np.full(len(node), synth.RANK_NAMES.index("clade"), np.uint16)
        self.tax = engine.Taxonomy(lin_off, node, rank, synth.RANK_NAMES, taxon="bacteria", device=0, bad=self.bad)
        fwd = self.tax.row_map()[0]
        assert np.array_equal(fwd, self.eng), "the row map differs from the independent sort"
        self.ref_lineage = _RowLineages(lin, length)
        self.eng_dev = None

    def row_at(self, pos):
        return int(self.order[pos])


class Table:
    """segments of (desc row | -1 unmatched | ('id', raw engine id) | ('desc', raw desc row), score)"""

    def __init__(self, tx):
        self.tx, self.seg, self.bs, self.desc, self.ids, self.lin, self.notes = tx, [0], [], [], [], [], []

    def query(self, rows, note=None):
        """`note`: what a failure at this query is to say about it"""
        self.notes.append(note)
        for r, b in rows:
            self.bs.append(int(b))
            if isinstance(r, tuple):                                     # a corrupt word: no lineage, whichever route carries it
                self.desc.append(r[1] if r[0] == "desc" else None)
                self.ids.append(r[1] if r[0] == "id" else None)
                self.lin.append(None)
            elif r < 0:
                self.desc.append(UNMATCHED); self.ids.append(UNMATCHED); self.lin.append(None)
            else:
                self.desc.append(int(r)); self.ids.append(int(self.tx.eng[r])); self.lin.append(self.tx.ref_lineage[r])
        self.seg.append(len(self.bs))
        return len(self.seg) - 2

    def check(self, milli, seg=None, narrowed=None, unresolved=None):
        """all four routes against the reference; -> (verdicts, depths, counts)"""
        seg = self.seg if seg is None else seg
        want_v, want_d, want_c = ref.keep(seg, self.bs, self.lin, milli)
        routes = []
        if all(x is not None for x in self.ids):
            routes.append(("ids", np.array(self.ids, np.uint32), None))
        if all(x is not None for x in self.desc):
            routes.append(("desc", np.array(self.desc, np.uint32), True))
        assert routes
        bs = np.array(self.bs, np.int32)
        for name, rows, use_map in routes:
            v, d, c = engine.cover_keep_host(self.tx.tax, seg, bs, rows, milli, row_map=use_map)
            self._same(f"host/{name}", v, d, c, want_v, want_d, want_c)
            t_seg = torch.tensor(np.array(seg, np.uint64).view(np.int64), device="cuda")
            t_bs, t_rows = torch.tensor(bs, device="cuda"), torch.tensor(rows.view(np.int32), device="cuda")
            t_keep = torch.full((len(bs),), 7, dtype=torch.int32, device="cuda")
            t_depth = torch.full((len(seg) - 1,), 9, dtype=torch.uint8, device="cuda")
            if use_map and self.tx.eng_dev is None:
                self.tx.eng_dev = torch.tensor(self.tx.eng.view(np.int32), device="cuda")
            t_map = self.tx.eng_dev if use_map else None
            c = engine.cover_keep_device(self.tx.tax, t_seg, t_bs, t_rows, milli, t_keep, t_depth, row_map=t_map)
            self._same(f"device/{name}", t_keep.cpu().numpy(), t_depth.cpu().numpy(), c, want_v, want_d, want_c)
        if narrowed is not None:
            assert (want_c["n_narrowed"] > 0) == narrowed, want_c
        if unresolved is not None:
            assert (want_c["n_unresolved"] > 0) == unresolved, want_c
        return want_v, want_d, want_c

    def _same(self, route, v, d, c, want_v, want_d, want_c):
        v, d = [int(x) for x in v], [int(x) for x in d]
        note = lambda q: self.notes[q] if q < len(self.notes) and self.notes[q] else f"query {q}"
        bad_q = [q for q in range(len(d)) if d[q] != want_d[q]]
        assert not bad_q, (route, "d* differs at queries", bad_q[:5], [d[q] for q in bad_q[:5]], [want_d[q] for q in bad_q[:5]],
                           note(bad_q[0]) if bad_q else None)
        bad_i = [i for i in range(len(v)) if v[i] != want_v[i]]
        assert not bad_i, (route, "verdicts differ at rows", bad_i[:10],
                           [note(q) for q in range(len(d)) if bad_i and self.seg[q] <= bad_i[0] < self.seg[q + 1]][:1])
        assert c == want_c, (route, "counts differ", c, want_c)


def _tree(n_phyla=3, n_fam=3, n_gen=3, n_sp=3):
    """a four-level tree, the rows in an order that is not the sorted one, plus the inner nodes as rows of their own"""
    lins = [[p, 10 + f, 20 + g, 30 + s] for p in range(n_phyla) for f in range(n_fam) for g in range(n_gen) for s in range(n_sp)]
    lins += [[p] for p in range(n_phyla)] + [[p, 10 + f] for p in range(n_phyla) for f in range(n_fam)]
    perm = np.random.default_rng(3).permutation(len(lins))
    return [lins[i] for i in perm]


@pytest.fixture(scope="module")
def tree():
    return Tax(_tree())


def _row(tx, lineage):
    return tx.lineages.index(list(lineage))


def _group(tx, rng, n, outliers, genus=(1, 11, 21)):
    """n top rows: the species of one genus, `outliers` of them replaced by rows of another phylum, at the given places"""
    rows = [_row(tx, list(genus) + [30 + int(rng.integers(0, 3))]) for _ in range(n)]
    for at in outliers:
        rows[at] = _row(tx, [2, 10 + int(rng.integers(0, 3)), 20, 30])
    return rows


@pytest.mark.parametrize("shape", ["whole", "single", "band"])
def test_segment_lengths_and_top_groups(tree, shape):
    rng = np.random.default_rng(11)
    t = Table(tree)
    for length in (0, 1, 2, 63, 64, 65, 128, 129, 1000):
        if shape == "whole":
            n_top, first = length, 0
        elif shape == "single":
            n_top, first = min(length, 1), length // 2
        else:
            n_top, first = length // 2, length // 4
        group = _group(tree, rng, n_top, [k for k in (0, n_top // 2, n_top - 1) if 0 <= k < n_top and n_top >= 8][:max(0, n_top // 8)])
        rows = [(int(rng.integers(0, len(tree.lineages))), TOP - 1 - int(rng.integers(0, 50))) for _ in range(length)]
        for k, r in enumerate(group):
            rows[first + k] = (r, TOP)
        t.query(rows)
    t.check(80000, narrowed=shape != "single", unresolved=False)
    t.check(100000, narrowed=False)
    t.check(50001)


@pytest.mark.parametrize("pad", [0, 70], ids=["short", "long"])
def test_outlier_places_even_and_odd_duplicates_and_prefixes(tree, pad):
    rng = np.random.default_rng(12)
    t = Table(tree)
    under = lambda: [(int(rng.integers(0, len(tree.lineages))), TOP - 5) for _ in range(pad)]
    names = []
    for n in (8, 9, 40, 41):
        for where in ("first", "last", "median"):
            # the outlier is the segment's first row, its last, or its row n // 2: the lane a median taken by index, not by
            # sorted position, would choose (by position the outlier of another phylum always sorts to an end of the group)
            group = _group(tree, rng, n, [{"first": 0, "last": n - 1, "median": n // 2}[where]])
            t.query([(r, TOP) for r in group] + under())
            names.append((n, where))
        # n equal rows; and two positions only, the minority dropped
        t.query([(_row(tree, [1, 11, 21, 31]), TOP)] * n + under())
        t.query([(_row(tree, [1, 11, 21, 31]), TOP)] * (n - 1) + [(_row(tree, [0, 10, 20, 30]), TOP)] + under())
        # a lineage that is a prefix of the others: as the median (the inner node [1, 11] among its species: it sorts first of
        # its clade, so half of the group is put before it) and as an outlier
        fam, sp = _row(tree, [1, 11]), _row(tree, [1, 11, 21, 30])
        before = _row(tree, [1, 10, 22, 32])
        t.query([(before, TOP)] * (n // 2) + [(fam, TOP)] + [(sp, TOP)] * (n - n // 2 - 1) + under())
        t.query([(fam, TOP)] + [(sp, TOP)] * (n - 1) + under())
        t.query([(_row(tree, [1]), TOP)] * (n - 2) + [(sp, TOP)] * 2 + under())
    v, d, c = t.check(80000, narrowed=True, unresolved=False)
    t.check(66667, narrowed=True)
    t.check(50001, narrowed=True)
    t.check(100000, narrowed=False)


def test_depths_of_one_and_of_sixty_four():
    deep = [[100 + j for j in range(64)], [100 + j for j in range(63)] + [999], [100] + [500 + j for j in range(63)], [7], [8], [100]]
    tx = Tax(deep)
    t = Table(tx)
    q64 = t.query([(0, TOP)] * 4 + [(3, TOP)])                           # d* = 64: four equal rows of 64 levels and one other
    q63 = t.query([(0, TOP)] * 2 + [(1, TOP)] * 2 + [(3, TOP)])          # d* = 63
    q1 = t.query([(0, TOP), (1, TOP), (2, TOP), (5, TOP), (4, TOP)])     # d* = 1: node 100 covers four
    q0 = t.query([(3, TOP), (4, TOP), (0, TOP)])                         # d* = 0: nothing in common, nothing dropped
    q1b = t.query([(3, TOP)] * 3 + [(4, TOP)])                           # lineages of one level: d* = 1
    v, d, c = t.check(75000, narrowed=True, unresolved=False)
    assert [d[q] for q in (q64, q63, q1, q0, q1b)] == [64, 63, 1, 0, 1]
    assert c["n_narrowed"] == 4
    # the same in long segments
    t2 = Table(tx)
    for q in range(5):
        s0, s1 = t.seg[q], t.seg[q + 1]
        t2.query([(t.desc[i], TOP) for i in range(s0, s1)] + [(int(i % 6), TOP - 1 - i) for i in range(80)])
    v, d2, c2 = t2.check(75000, narrowed=True)
    assert d2 == d


@pytest.mark.parametrize("pad", [0, 90], ids=["short", "long"])
def test_rows_without_a_lineage_in_the_top_group_and_under_it(pad):
    lins = _tree() + [[1, 11, 77], []]
    tx = Tax(lins, bad=[len(lins) - 2])
    bad_row, empty_row = len(lins) - 2, len(lins) - 1
    rng = np.random.default_rng(13)
    t = Table(tx)
    under = lambda: [(int(rng.integers(0, len(lins) - 2)), TOP - 9) for _ in range(pad)]
    in_top, below = [], []
    for r in (-1, bad_row, empty_row):
        group = [(x, TOP) for x in _group(tx, rng, 9, [0])]
        in_top.append(t.query(group[:4] + [(r, TOP)] + group[4:] + under()))          # in the top group: the query is left alone
        below.append(t.query(group + [(r, TOP - 1)] + under()))                       # under it: ignored, the outlier goes
    v, d, c = t.check(80000, narrowed=True, unresolved=True)
    assert c["n_unresolved"] == 3 and c["n_narrowed"] == 3
    assert all(d[q] == ref.NONE_U8 for q in in_top) and all(d[q] == 3 for q in below)      # (the genus: three levels)
    assert all(v[i] == 1 for q in in_top for i in range(t.seg[q], t.seg[q + 1]))


def test_four_queries_of_one_wave_with_different_outcomes(tree):
    rng = np.random.default_rng(14)
    t = Table(tree)
    for rep in range(3):                                                 # (queries 0 .. 3, 4 .. 7, 8 .. 11: three waves)
        t.query([(x, TOP) for x in _group(tree, rng, 10, [3])])                       # narrowed
        t.query([(x, TOP) for x in _group(tree, rng, 10, [])] + [(-1, TOP)])          # unresolved
        t.query([] if rep == 0 else [(5, TOP), (6, TOP - 1)])                         # empty / one top row
        t.query([(x, TOP) for x in _group(tree, rng, 64 if rep == 1 else 7, [])] + ([(0, 3)] * 60 if rep == 2 else []))   # kept whole; long once
    v, d, c = t.check(80000, narrowed=True, unresolved=True)
    assert (c["n_narrowed"], c["n_unresolved"]) == (3, 3)
    assert d[0] == 3 and d[1] == ref.NONE_U8 and d[2] == ref.NONE_U8 and d[3] in (3, 4)


@pytest.mark.parametrize("n_tax", [17, 18, 32, 33, 2, 1])
def test_table_sizes_around_a_block_of_sixteen(n_tax):
    """(n_tax - 1) mod 16 in {0, 1, 15}: the last lcp8 entry ends a block, starts one, or sits alone before the padding"""
    lins = [[i // 8, 10 + i // 2, 100 + i] for i in range(n_tax)]
    tx = Tax(lins)
    t = Table(tx)
    last, first = tx.row_at(n_tax - 1), tx.row_at(0)
    t.query([(last, TOP)] * 3 + [(first, TOP)])                          # the range [0, n_tax - 1): every entry of lcp8
    t.query([(last, TOP)] * 2 + [(tx.row_at(max(n_tax - 2, 0)), TOP)] * 2 + [(first, TOP)])
    t.query([(tx.row_at(p % n_tax), TOP) for p in range(0, 3 * n_tax, 3)][:60])
    t.check(75000, narrowed=n_tax > 1)
    t.check(60000)


def _bits(i, width=14):
    return [(i >> (width - 1 - k)) & 1 for k in range(width)]


@pytest.fixture(scope="module")
def binary_table():
    """2^13 + 37 rows, row i = the 14 bits of i, most significant first: the sorted order is the numeric one and the rows at
    positions lo < hi share the leading bits lo and hi share, which is min lcp8[lo .. hi).  lcp8 dips at every block edge (15 ->
    16 shares 9 bits, 16 -> 17 shares 13), so an entry too many or too few at either end of a range changes the minimum."""
    n = (1 << 13) + 37
    tx = Tax([_bits(i) for i in np.random.default_rng(4).permutation(n)])
    assert all(tx.lineages[tx.row_at(p)] == _bits(p) for p in (0, 1, 4097, n - 1))
    return tx, n


@pytest.mark.parametrize("pad", [0, 70], ids=["short", "long"])
def test_range_minimum_distances(binary_table, pad):
    tx, n = binary_table
    dists = [1, 15, 16, 17] + [x for k in range(5, 13) for x in ((1 << k) - 1, 1 << k, (1 << k) + 1)]
    t = Table(tx)
    want = []
    starts = lambda d: [b * 16 + o for o in (0, 1, 15) for b in (3, 100)] + [n - 1 - d]      # the last: hi is the table's last row
    for d in dists:
        for lo in starts(d):
            hi = lo + d
            if lo < 0 or hi >= n:
                continue
            # T = lo, hi, hi and a far row (the top bit flipped): need 3 of 4 at 75 % -> d* = the bits lo and hi share, and
            # far row goes unless lo and hi differ in the top bit themselves; the median by position is hi either way
            far = (1 << 13) + hi % 37 if hi < (1 << 13) else hi - (1 << 13)
            t.query([(tx.row_at(far), TOP), (tx.row_at(hi), TOP), (tx.row_at(lo), TOP), (tx.row_at(hi), TOP)]
                    + [(tx.row_at((lo * 7 + j) % n), TOP - 1) for j in range(pad)])
            want.append(next(k for k in range(15) if k == 14 or _bits(lo)[k] != _bits(hi)[k]))
    v, d, c = t.check(75000, narrowed=True, unresolved=False)
    assert d == want                                                     # (the reference's d*, said once more from the bits)
    assert len(want) >= 150 and c["n_narrowed"] >= 100


def test_hostile_offsets(tree):
    rng = np.random.default_rng(15)
    t = Table(tree)
    for n in (10, 70, 12, 9, 80):
        t.query([(x, TOP) for x in _group(tree, rng, n, [1])])
    n_hits = len(t.bs)
    good = list(t.seg)
    assert n_hits == 181
    for seg in ([0, 10, 80, 1 << 40, 181, n_hits + 7],                   # beyond n_hits, decreasing
                [0, 10, 80, n_hits + 7, 181, 5],
                [n_hits + 1, 0, 80, 80, 5, 0],                           # a first offset beyond the columns; rows no segment names
                [(1 << 64) - 1, 10, 80, 92, 101, (1 << 63)],
                [0, 0, 0, 0, 0, 0]):
        v, d, c = t.check(80000, seg=seg)
        named = set()
        for q in range(5):
            s1 = min(seg[q + 1], n_hits)
            named.update(range(min(seg[q], s1), s1))
        assert all(v[i] == 0 for i in range(n_hits) if i not in named)
    v, d, c = t.check(80000, seg=good, narrowed=True)
    assert c["n_narrowed"] == 5


@pytest.mark.parametrize("pad", [0, 70], ids=["short", "long"])
def test_row_ids_that_name_no_taxonomy_row(tree, pad):
    rng = np.random.default_rng(16)
    n_tax = len(tree.lineages)
    under = lambda: [(int(rng.integers(0, n_tax)), TOP - 9) for _ in range(pad)]
    words = {"id": [n_tax | (4 << se.ROW_BITS), se.POS_MASK | (4 << se.ROW_BITS), 5 | (65 << se.ROW_BITS), 5 | (127 << se.ROW_BITS), 0x7FFFFFFF],
             "desc": [n_tax, n_tax + 1, 0x7FFFFFFF, 0xFFFFFFFE]}
    for kind, bad_words in words.items():
        t = Table(tree)
        for w in bad_words:
            group = [(x, TOP) for x in _group(tree, rng, 9, [0])]
            t.query(group[:5] + [((kind, w), TOP)] + group[5:] + under())             # in the top group: unresolved, untouched
            t.query(group + [((kind, w), TOP - 1)] + under())                         # under it: ignored
        v, d, c = t.check(80000, narrowed=True, unresolved=True)
        assert c["n_unresolved"] == len(bad_words) == c["n_narrowed"]


def test_apply_compacts_as_the_reference_says(tree):
    """blu_hits_cover_apply on both routes: the five columns and the offsets of the reference's verdicts, the unmatched rows
    recounted; every row kept leaves the columns untouched."""
    from tests import subject_best_reference as sb
    rng = np.random.default_rng(17)
    t = Table(tree)
    for n in (10, 70, 1, 12, 0, 80):
        t.query([(x, TOP) for x in _group(tree, rng, n, [1] if n > 2 else [])] + [(-1, TOP - 3)] * (n % 3))
    n_hits = len(t.bs)
    aln, acc, pid = np.arange(n_hits, dtype=np.int32) + 5, np.arange(n_hits, dtype=np.uint32)[::-1].copy(), np.arange(n_hits) / 8.0
    want_v, _, want_c = ref.keep(t.seg, t.bs, t.lin, 80000)
    off, cols = sb.compact(t.seg, want_v, t.bs, aln, t.desc, acc, pid)
    assert want_c["n_kept"] < n_hits
    out, n_un, c = engine.cover_apply_host(tree.tax, t.seg, t.bs, aln, np.array(t.desc, np.uint32), acc, pid, 80000, row_map=True)
    dev = [torch.tensor(np.array(x), device="cuda") for x in (np.array(t.seg, np.int64), np.array(t.bs, np.int32), aln,
                                                               np.array(t.desc, np.uint32).view(np.int32), acc.view(np.int32), pid)]
    k, n_un_d, c_d = engine.cover_apply_device(tree.tax, *dev, 80000, row_map=torch.tensor(tree.eng.view(np.int32), device="cuda"))
    assert c == c_d == want_c and k == want_c["n_kept"]
    assert n_un == n_un_d == sum(1 for x in cols[2] if x == UNMATCHED) > 0
    for name, col, d_col in zip(("bitscore", "align_len", "tax_row", "acc_rank", "pident"), cols, dev[1:]):
        assert out[name].tolist() == [x for x in col], name
        got = d_col[:k].cpu().numpy()
        assert (got.view(np.uint32) if got.dtype == np.int32 and name in ("tax_row", "acc_rank") else got).tolist() == [x for x in col], name
    assert out["seg_off"].tolist() == off == dev[0].cpu().tolist()
    # at 100 % nothing moves
    out, n_un, c = engine.cover_apply_host(tree.tax, t.seg, t.bs, aln, np.array(t.desc, np.uint32), acc, pid, 100000, row_map=True)
    assert c["n_kept"] == n_hits and out["bitscore"].tolist() == t.bs and out["seg_off"].tolist() == t.seg
    # no query over three rows, engine row ids and no map: no segment names a row, so both routes drop them all
    bs3, ids3 = t.bs[:3], np.array(t.ids[:3], np.uint32)
    want_v, _, want_c = ref.keep([0], bs3, t.lin[:3], 80000)
    off, cols = sb.compact([0], want_v, bs3, aln[:3], ids3, acc[:3], pid[:3])
    out, n_un, c = engine.cover_apply_host(tree.tax, [0], bs3, aln[:3], ids3, acc[:3], pid[:3], 80000)
    dev = [torch.tensor(np.array(x), device="cuda") for x in (np.zeros(1, np.int64), np.array(bs3, np.int32), aln[:3], ids3.view(np.int32),
                                                               acc[:3].view(np.int32), pid[:3])]
    k, n_un_d, c_d = engine.cover_apply_device(tree.tax, *dev, 80000)
    assert c == c_d == want_c and k == want_c["n_kept"] == 0 and n_un == n_un_d == 0
    assert out["seg_off"].tolist() == off == dev[0].cpu().tolist() == [0]
    assert all(out[name].tolist() == col == [] for name, col in zip(("bitscore", "align_len", "tax_row", "acc_rank", "pident"), cols))
