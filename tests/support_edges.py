"""Edge cases of the support kernel's clade range search and segment scan (csrc/support_kernel.hip), with
an expected value that shares none of the kernel's method.

Three independent pieces:

- `expected`: the eight fields of every query, vectorised numpy on a padded [n_tax, depth] lineage matrix.  A hit supports
  when it is matched and its first L + 1 nodes equal the reference row's; no sorted position, no lcp8 / rmq, no row map.
- `sort_rows`: the lexicographic order of the lineages by numpy (a prefix sorts first, equal lineages by row index), so a
  case can name "the row at sorted position lo - 1"; `clade_range` narrows [lo, hi] column by column in that order.
- the case families (`near_sweep`, `skip_path`, `high_levels`, `table_ends`, `levels`, `segment_scan`, `hostile_offsets`):
  hand-built records, each edge query holding the reference hit, the rows at lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, an
  unmatched hit and a far row.  Every probe row is there twice, once on the segment's maximum (tied with the reference) and
  once on a power of two of its own, so a single row whose verdict flips changes n_support, n_top_support and support_bits.

tests/test_support_edges.py (no GPU) checks that every family lies where it claims; tests/test_gpu_support_edges.py runs them."""
import functools

import numpy as np

from blutils_amd import engine
from tests import support_reference as ref

ROW_BITS = 25
POS_MASK = (1 << ROW_BITS) - 1
UNMATCHED = 0xFFFFFFFF
U32_MAX = 0xFFFFFFFF
TOP = 1 << 20                                        # the score of the reference hit and of one copy of every probe row
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1

SKIP_BLOCKS = (0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 255, 256, 257)
END_DISTANCES = (0, 63, 64, 65, 79, 80, 81)
TABLE_SIZES = (1, 2, 15, 16, 17, 18, 31, 32, 33, 64, 65, 66, 80, 81, 82)
SCAN_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 4097)
LARGE_ROWS = (1 << 20) + 40


# ---- lineages as a matrix, the independent sort, the independent expected value -------------------------------------------------

def to_matrix(lineages):
    """(matrix [n, depth] int32 padded with -1, lengths)."""
    depth = max(1, max((len(l) for l in lineages), default=1))
    m = np.full((len(lineages), depth), -1, np.int32)
    for t, l in enumerate(lineages):
        m[t, :len(l)] = l
    return m, np.array([len(l) for l in lineages], np.int64)


def sort_rows(lin):
    """Sorted position -> row: numpy's lexicographic order of the padded rows (-1 sorts in front of every node id, so a prefix
    comes first); lexsort is stable, so equal lineages stay in row order."""
    return np.lexsort(tuple(lin[:, j] for j in range(lin.shape[1] - 1, -1, -1)))


def clade_range(sorted_lin, prefix):
    """[lo, hi] of the sorted rows that start with `prefix`, or None: one binary search per level on the sorted matrix."""
    lo, hi = 0, len(sorted_lin)
    for j, v in enumerate(prefix):
        col = sorted_lin[lo:hi, j]
        a, b = np.searchsorted(col, v, "left"), np.searchsorted(col, v, "right")
        lo, hi = lo + int(a), lo + int(b)
        if lo >= hi:
            return None
    return lo, hi - 1


def clade_range_brute(lin, length, pos_of, row, need):
    """The same by "which rows share the prefix": (lo, hi, number of members), or None."""
    if need > length[row]:
        return None
    member = (length >= need) & (lin[:, :need] == lin[row, :need]).all(axis=1)
    p = pos_of[member]
    return int(p.min()), int(p.max()), int(member.sum())


def _seg_sum(x, first, lens):
    cs = np.concatenate([[0], np.cumsum(x.astype(np.int64))])
    return cs[first + lens] - cs[first]


def expected(lin, length, seg_off, bitscore, desc_row, records):
    """The eight fields of every query (support_reference.DTYPE: int64 throughout).  lin: [n_tax, depth] padded with -1, rows
    that did not parse all -1; length: levels per row (0 = bad / empty); desc_row: row per hit, -1 = unmatched.  Offsets are
    clamped as support_counts documents: s1 = min(s1, n_hits), s0 = min(s0, s1)."""
    n_hits, nq, depth = len(bitscore), len(seg_off) - 1, lin.shape[1]
    seg = np.minimum(np.asarray(seg_off, np.uint64), np.uint64(n_hits)).astype(np.int64)
    s1 = seg[1:]
    s0 = np.minimum(seg[:-1], s1)
    lens = s1 - s0
    first = np.cumsum(lens) - lens
    qid = np.repeat(np.arange(nq), lens)
    hit = s0[qid] + (np.arange(int(lens.sum())) - first[qid])
    bs = np.asarray(bitscore)[hit].astype(np.int64)
    desc_row = np.asarray(desc_row, np.int64)
    d = desc_row[hit]
    named = (d >= 0) & (d < len(lin))
    dz = np.where(named, d, 0)
    dlen = np.where(named, length[dz], 0)
    matched = named & (dlen > 0)
    status = records["status"].astype(np.int64)
    need = np.array([int(m).bit_length() for m in records["level_mask"]], np.int64)
    rdesc = np.full(nq, -1, np.int64)
    placed = status < 2
    rdesc[placed] = desc_row[records["ref_row"][placed].astype(np.int64)]
    assert (rdesc[placed] >= 0).all(), "a record with a taxon needs a matched reference row"
    rz = np.maximum(rdesc, 0)
    has_clade = placed & (need <= length[rz])
    nd = need[qid]
    same = ((lin[dz] == lin[rz[qid]]) | (np.arange(depth)[None, :] >= nd[:, None])).all(axis=1)
    sup = matched & has_clade[qid] & (dlen >= nd) & same
    out = np.zeros(nq, ref.DTYPE)
    full = lens > 0
    top = np.zeros(nq, np.int64)
    if full.any():
        top[full] = np.maximum.reduceat(bs, first[full])
    on_top = bs == top[qid]
    out["n_hits"] = lens
    out["n_matched"] = _seg_sum(matched, first, lens)
    out["n_top"] = _seg_sum(on_top, first, lens)
    out["n_top_support"] = _seg_sum(on_top & sup, first, lens)
    out["n_support"] = _seg_sum(sup, first, lens)
    out["top_score"] = top
    out["bits"] = _seg_sum(bs, first, lens)
    out["support_bits"] = _seg_sum(np.where(sup, bs, 0), first, lens)
    return out


# ---- a table: taxonomy + hits + records, and what each query is about -----------------------------------------------------------

class Table:
    """family / name; raw [n_tax, depth] and raw_len as stated (what the product is given), bad; lin / length as they count
    (bad rows empty); order, pos_of (the independent sort), eng (row -> engine row id, from that sort); seg, bs, desc, recs;
    per query: q_pos (sorted position of the reference row, -1 without one), q_need, q_lo, q_hi (-1 / -1: no clade), q_note."""

    def lineages(self):
        return [[int(x) for x in self.raw[t, :self.raw_len[t]]] for t in range(len(self.raw))]

    def lin_arrays(self):
        lin_off = np.concatenate([[0], np.cumsum(self.raw_len)]).astype(np.uint64)
        return lin_off, self.raw[self.raw >= 0].astype(np.uint32)

    def eng_rows(self):
        return np.where(self.desc < 0, UNMATCHED, self.eng[np.maximum(self.desc, 0)]).astype(np.uint32)

    def expected(self):
        return expected(self.lin, self.length, self.seg, self.bs, self.desc, self.recs)

    def where(self, q):
        """For a failure message: family, table, query, reference position, lo, hi."""
        return (f"family {self.family} table {self.name} query {q} ({self.q_note[q]}): reference at sorted position "
                f"{self.q_pos[q]}, need {self.q_need[q]}, lo {self.q_lo[q]}, hi {self.q_hi[q]}")


class Builder:
    def __init__(self, family, name, raw, raw_len, bad=None, seed=0):
        t = self.t = Table()
        t.family, t.name, t.raw, t.raw_len = family, name, raw, np.asarray(raw_len, np.int64)
        t.bad = None if bad is None else np.asarray(bad, np.uint8)
        is_bad = np.zeros(len(raw), bool) if bad is None else t.bad != 0
        t.length = np.where(is_bad, 0, t.raw_len)
        t.lin = raw.copy()
        t.lin[is_bad] = -1
        t.order = sort_rows(t.lin)
        t.pos_of = np.empty(len(raw), np.int64)
        t.pos_of[t.order] = np.arange(len(raw))
        t.eng = (t.pos_of | (t.length << ROW_BITS)).astype(np.uint32)
        self.sorted_lin = t.lin[t.order]
        self.rng = np.random.default_rng(seed)
        self.seg, self.bs, self.desc, self.recs = [0], [], [], []
        self.q_pos, self.q_need, self.q_lo, self.q_hi, self.q_note = [], [], [], [], []

    def mask_of(self, need):
        return 0 if need == 0 else (1 << (need - 1)) | int(self.rng.integers(0, 1 << min(need - 1, 62)))

    def segment(self, rows, scores, status, ref_at=None, need=0, note="", mask=None):
        """One query: `rows` (desc rows, -1 unmatched) and `scores`; a record of `status` whose reference hit is the segment's
        `ref_at`-th (None: no reference row); the mask's top bit is need - 1 (need 0: mask 0)."""
        t = self.t
        rec = np.zeros(1, engine.RESULT_DTYPE)
        rec["status"], rec["ref_row"] = status, U32_MAX
        rec["level_mask"] = self.mask_of(need) if mask is None else mask
        pos, lo, hi = -1, -1, -1
        if ref_at is not None:
            rec["ref_row"] = self.seg[-1] + ref_at
            r = int(rows[ref_at])
            pos = int(t.pos_of[r])
            if need == 0:
                lo, hi = 0, len(t.raw) - 1
            elif need <= t.length[r]:
                lo, hi = clade_range(self.sorted_lin, t.lin[r, :need])
        self.seg.append(self.seg[-1] + len(rows))
        self.bs.extend(int(s) for s in scores)
        self.desc.extend(int(r) for r in rows)
        self.recs.append(rec)
        self.q_pos.append(pos); self.q_need.append(need); self.q_lo.append(lo); self.q_hi.append(hi); self.q_note.append(note)

    def edge_query(self, r_row, need, note="", extra=()):
        """The reference hit, both copies of the rows at lo - 1 ... hi + 1 and of a far row (and of `extra` rows), two
        unmatched hits; in a random order.  Status 0: the maximum is tied."""
        t, n = self.t, len(self.t.raw)
        pos = int(t.pos_of[r_row])
        if need == 0:
            lo, hi = 0, n - 1
        elif need <= t.length[r_row]:
            lo, hi = clade_range(self.sorted_lin, t.lin[r_row, :need])
        else:
            lo = hi = pos                                                       # no clade: the rows around the reference row
        probes = []
        for p in (lo - 1, lo, lo + 1, hi - 1, hi, hi + 1):
            if 0 <= p < n and p not in probes:
                probes.append(p)
        far = [p for p in (0, n - 1, (pos + n // 2) % n) if p < lo - 1 or p > hi + 1]
        if far:                                                                 # (none where the clade and its neighbours are the table)
            probes.append(far[-1])
        rows = [r_row] + ([int(t.order[p]) for p in probes] + [int(x) for x in extra]) * 2 + [-1, -1]
        k = len(probes) + len(extra)
        scores = [TOP] + [TOP] * k + [1 << j for j in range(k)] + [TOP, 1 << k]
        perm = self.rng.permutation(len(rows))
        self.segment(np.array(rows)[perm], np.array(scores)[perm], 0, int(np.nonzero(perm == 0)[0][0]), need, note)

    def finish(self):
        t = self.t
        t.seg = np.array(self.seg, np.uint64)
        t.bs = np.array(self.bs, np.int32)
        t.desc = np.array(self.desc, np.int64)
        t.recs = np.concatenate(self.recs) if self.recs else np.zeros(0, engine.RESULT_DTYPE)
        t.q_pos, t.q_need = np.array(self.q_pos, np.int64), np.array(self.q_need, np.int64)
        t.q_lo, t.q_hi, t.q_note = np.array(self.q_lo, np.int64), np.array(self.q_hi, np.int64), self.q_note
        return t


def _shuffled(lineages, seed):
    """The rows in an order that is not the sorted one, so the row map is not the identity."""
    perm = np.random.default_rng(seed).permutation(len(lineages))
    return [lineages[i] for i in perm]


# ---- family 1: near sweep -------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def near_sweep():
    """Sibling clades of 1 ... 128 rows under one parent, a single row in front and behind: the clade starts are triangular
    numbers + 1 and hit every residue mod 16.  Every row of every clade is the reference once, at the clade's level."""
    L = [[1, 5, 7]]
    for c in range(1, 129):
        L += [[1, 10 + c, 1000 * c + i] for i in range(c)]
    L += [[1, 5000, 7]]
    m, ln = to_matrix(_shuffled(L, 1))
    b = Builder(1, "near_sweep", m, ln, seed=11)
    for r in range(len(m)):
        if 10 < m[r, 1] < 5000:
            b.edge_query(r, 2, f"clade of {m[r, 1] - 10} rows")
    return b.finish()


def near_coverage(t):
    """{(pos - lo, pos mod 16)}, {(hi - pos, pos mod 16)} over the table's queries."""
    return (set(zip((t.q_pos - t.q_lo).tolist(), (t.q_pos % 16).tolist())),
            set(zip((t.q_hi - t.q_pos).tolist(), (t.q_pos % 16).tolist())))


# ---- family 2: the skip path ----------------------------------------------------------------------------------------------------

def skipped_blocks(pos, lo, hi):
    """(towards hi, towards lo): the whole 16-entry blocks of lcp8 that hold between the end of the first 64-entry probe,
    re-aligned, and the boundary; None where the first probe already meets the boundary.  lcp8[lo .. hi - 1] hold,
    lcp8[hi] and lcp8[lo - 1] do not."""
    up = (hi >> 4) - ((pos + 64) >> 4) if pos + 64 <= hi else None
    down = ((pos - 64 + 15) >> 4) - ((lo + 15) >> 4) if pos - 64 >= lo else None
    return up, down


@functools.lru_cache(None)
def skip_path():
    """Sixteen clades of about 4 400 rows: clade k starts at a position = k mod 16 and ends at one = 5k + 3 mod 16; the first
    starts at 0 and the last ends at n_tax - 1.  In each the reference sits where 0 ... 257 whole blocks are skipped towards hi,
    the same towards lo, at the first and the last row and 63 ... 81 rows from either end."""
    L, spans = [], []
    for k in range(16):
        j = 0
        while len(L) % 16 != k:
            L.append([1, 100 * (k + 1) - 50 + j, 7])
            j += 1
        lo = len(L)
        size = 4400
        while (lo + size - 1) % 16 != (5 * k + 3) % 16:
            size += 1
        L += [[1, 100 * (k + 1), 10 + i] for i in range(size)]
        spans.append((lo, lo + size - 1))
    perm = np.random.default_rng(2).permutation(len(L))
    m, ln = to_matrix([L[i] for i in perm])
    b = Builder(2, "skip_path", m, ln, seed=12)
    assert np.array_equal(perm[b.t.order], np.arange(len(L)))                   # L is in sorted order: `spans` are positions
    for k, (lo, hi) in enumerate(spans):
        want = []
        for s in SKIP_BLOCKS:
            off = (7 * s + k) % 16
            if s == 0:
                off %= hi % 16 + 1
            want.append((16 * ((hi >> 4) - s) - 64 + off, f"{s} blocks skipped towards hi"))
            off = (7 * s + k) % 16
            if s == 0:
                off %= (16 - lo % 16) % 16 + 1
            want.append((64 + 16 * (((lo + 15) >> 4) + s) - off, f"{s} blocks skipped towards lo"))
        for dist in END_DISTANCES:
            want.append((lo + dist, f"{dist} rows from lo"))
            want.append((hi - dist, f"{dist} rows from hi"))
        for p, note in want:
            assert lo <= p <= hi
            b.edge_query(int(b.t.order[p]), 2, f"clade {k}: {note}")
    return b.finish()


# ---- family 3: high rmq levels --------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def high_levels(n_rows=LARGE_ROWS):
    """One table of 2^20 + 40 rows (rmq_nb = 65 540: 17 levels), six levels deep, every row under node 1:

        [0, 4] (starts at 0) | X = [5, n - 20]: 65 537 blocks, unaligned start | [n - 19, n - 1] (ends at n_tax - 1)
        inside X: Y = [16, n - 25]: 65 536 blocks, aligned start;  inside Y: Z = [21, n - 36]: 65 535 blocks, unaligned
        inside Z: clades of 2^k - 1, 2^k and 2^k + 1 blocks for k = 4, 8, 12 at an aligned and an unaligned start each, single
        rows in between, one clade of what is left.

    The three 2^16-block clades fill the table, so they can only nest: each has the one start given here.  The reference is the
    first, the middle and the last row of each clade, and of the whole table under level_mask = 1."""
    n = n_rows
    big = n - 40                                                                # 2^20 (or 2^17) rows: 2^16 (2^13) blocks
    kk = (4, 8, 12) if big >= 1 << 20 else (4, 8)
    m = np.full((n, 6), -1, np.int32)
    m[:, 0] = 1
    leaf = np.arange(n, dtype=np.int32) + 100
    clades = [(1, 0, n - 1, "whole table")]

    def put(lo, hi, prefix, name):
        """Rows lo .. hi get `prefix`; (need, lo, hi, name) is recorded."""
        for j, v in enumerate(prefix):
            m[lo:hi + 1, 1 + j] = v
        clades.append((1 + len(prefix), lo, hi, name))

    put(0, 4, [10], "starts at 0")
    put(n - 19, n - 1, [30], "ends at n_tax - 1")
    put(5, n - 20, [20], "X: 2^k + 1 blocks, unaligned")
    assert n - 20 - 5 + 1 == big + 16
    put(5, 15, [20, 10], "in front of Y")
    put(n - 24, n - 20, [20, 30], "behind Y")
    put(16, n - 25, [20, 20], "Y: 2^k blocks, aligned")
    assert n - 25 - 16 + 1 == big
    put(16, 20, [20, 20, 10], "in front of Z")
    put(n - 35, n - 25, [20, 20, 30], "behind Z")
    put(21, n - 36, [20, 20, 20], "Z: 2^k - 1 blocks, unaligned")
    assert n - 36 - 21 + 1 == big - 16
    cur, d = 21, 10
    for k in kk:
        for delta in (-1, 0, 1):
            for start in (0, 5 + 2 * delta):                                    # aligned, unaligned (3, 5, 7 mod 16)
                while cur % 16 != start:
                    put(cur, cur, [20, 20, 20, d], "single row")
                    clades.pop()
                    cur, d = cur + 1, d + 1
                size = 16 * ((1 << k) + delta)
                put(cur, cur + size - 1, [20, 20, 20, d], f"{(1 << k) + delta} blocks at {start} mod 16")
                cur, d = cur + size, d + 1
    assert cur < n - 36 - 1000
    put(cur, n - 36, [20, 20, 20, d], "the rest of Z")
    depth = (m >= 0).sum(axis=1)
    m[np.arange(n), depth] = leaf                                               # a leaf of its own behind every prefix
    ln = depth + 1
    perm = np.random.default_rng(3).permutation(n)
    b = Builder(3, f"high_levels_{n}", m[perm], ln[perm], seed=13)
    assert np.array_equal(perm[b.t.order], np.arange(n))                        # built in sorted order
    for need, lo, hi, name in clades:
        for p, at in ((lo, "first"), ((lo + hi) // 2, "middle"), (hi, "last")):
            b.edge_query(int(b.t.order[p]), need, f"{name}: reference at its {at} row")
    return b.finish()


# ---- family 4: table ends and sizes ---------------------------------------------------------------------------------------------

def _ends_lineages(n):
    if n == 1:
        return [[1, 2, 3]]
    if n == 2:
        return [[1, 6, 7], [1, 6, 8]]
    return [[1, 2, 3]] + [[1, 4, 10 + i] for i in range(n - 3)] + [[1, 6, 7], [1, 6, 8]]


@functools.lru_cache(None)
def table_ends():
    """One table per n_tax: the first row alone, a middle clade, the last two rows under one node.  Every row is the reference
    at need 1 (the whole table), 2 and 3 (the row alone)."""
    out = []
    for n in TABLE_SIZES:
        m, ln = to_matrix(_shuffled(_ends_lineages(n), 40 + n))
        b = Builder(4, f"n_tax_{n}", m, ln, seed=14 + n)
        for r in range(n):
            for need in (1, 2, 3):
                b.edge_query(r, need, f"row {r} need {need}")
        out.append(b.finish())
    return out


# ---- family 5: levels -----------------------------------------------------------------------------------------------------------

def _levels_lineages():
    deep = list(range(100, 164))                                                # 64 levels
    L = [[1, 2, 3, 4, 50 + i] for i in range(5)]                                # nested: need 1 ... 4 around [1, 2, 3, 4, *]
    L += [[1, 2, 3, 5, 60 + i] for i in range(20)]
    L += [[1, 2, 4, 5, 70 + i] for i in range(70)]
    L += [[1, 3, 4, 5, 80 + i] for i in range(150)]
    L += [[1, 6], [1, 6, 60], [1, 6, 60, 600], [1, 6, 60, 600, 6000], [1, 6, 61]]      # a prefix in front of its extensions
    L += [[1, 7, 70]] * 2 + [[1, 7, 71]] * 3 + [[1, 7, 72]] + [[1, 8, 80]] * 3  # listed twice / three times, at clade boundaries
    L += [deep, deep, deep[:63] + [999], deep[:62] + [998, 5], deep[:62] + [998, 6], deep[:40]]
    L += [[2, 9, 90], [2, 9]]
    return L


@functools.lru_cache(None)
def levels():
    """Two tables over the same lineages: plain, and with rows that did not parse (`bad`).  Bad rows count as empty, sort in
    front of everything and match nothing: one of them states the lineage of the first clade, so in row order it sits between
    that clade's rows, and in sorted order the bad rows are what lies at lo - 1 of the first clade.  (Nothing can sort behind
    hi as a bad row; the rows behind every hi are real.)  Every row is the reference at every need up to its length + 1
    (need > len: no clade) -- for the 64-level rows at 1, 2, 40, 41, 62, 63, 64."""
    out = []
    for with_bad in (False, True):
        L = _levels_lineages()
        bad = None
        if with_bad:
            L = L + [[1, 2, 3, 4, 50], [1, 2, 3, 4, 54], [2, 9, 90], []]        # stated lineages of rows flagged bad (and one empty)
            bad_rows = list(range(len(L) - 4, len(L) - 1))
        perm = np.random.default_rng(5 + with_bad).permutation(len(L))
        m, ln = to_matrix([L[i] for i in perm])
        if with_bad:
            bad = np.zeros(len(L), np.uint8)
            bad[np.nonzero(np.isin(perm, bad_rows))[0]] = 1
        b = Builder(5, "levels_bad" if with_bad else "levels", m, ln, bad, seed=15 + with_bad)
        t = b.t
        bad_idx = np.nonzero(t.length == 0)[0]
        for r in range(len(m)):
            n = int(t.length[r])
            if n == 0:
                continue
            needs = range(1, n + 2) if n < 40 else (1, 2, 40, 41, 62, 63, 64)
            for need in needs:
                if need <= 64:
                    b.edge_query(r, need, f"row {r} of {n} levels, need {need}", extra=bad_idx[:2])
        for r in (0, len(m) // 2):                                              # mask 0 with a taxon: every matched hit
            if t.length[r]:
                b.edge_query(r, 0, "unplaced", extra=bad_idx)
        out.append(b.finish())
    return out


# ---- family 6: the segment scan -------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def segment_scan():
    """Segments of the edge lengths over a small taxonomy, about half of each segment's hits inside the clade: a unique maximum
    at index 0, 63, 64, n - 1 and in the last partial 64-hit step; the maximum tied across lanes and steps (and twice in one
    lane); a lane whose first hit is its largest next to one whose last is; INT32_MIN / INT32_MAX everywhere and mixed."""
    L = [[1, 2, 10 + i] for i in range(40)] + [[1, 3, 50 + i] for i in range(40)] + [[4, 5]]
    m, ln = to_matrix(_shuffled(L, 6))
    b = Builder(6, "segment_scan", m, ln, seed=16)
    rng, t = b.rng, b.t
    inside = np.nonzero(m[:, 1] == 2)[0]

    def rows_for(n):
        rows = rng.integers(0, len(m), n)
        rows = np.where(rng.random(n) < 0.3, rng.choice(inside, n), rows)
        return np.where(rng.random(n) < 0.1, -1, rows)

    def add(n, scores, ref_at, status, note):
        rows = rows_for(n)
        if ref_at is not None:
            rows[ref_at] = rng.choice(inside)
        b.segment(rows, scores, status, ref_at, 2 if ref_at is not None else 0, f"{n} hits, {note}")

    for n in SCAN_LENGTHS:
        if n == 0:
            for st in (2, 16):
                b.segment([], [], st, None, 0, "empty segment")
            continue
        base = lambda: rng.integers(-50, 51, n)
        for k in sorted({0, 63, 64, n - 1, (n - 1) // 64 * 64, (n - 1) // 64 * 64 + (n - 1) % 64 // 2}):
            if k < n:
                s = base()
                s[k] = 1000
                add(n, s, k, 1, f"unique maximum at {k}")
        tied = sorted({0, n // 2, n - 1} | {k for k in (3, 67, 131, 64 * 5 + 3, 17, 64 + 40, 4096) if k < n})
        s = base()
        s[tied] = 1000
        add(n, s, tied[len(tied) // 2], 0, f"maximum tied at {tied}")
        add(n, s, None, 16, f"maximum tied at {tied}, no taxon")
        if n >= 129:
            s = np.full(n, -7)
            s[[0, 64, 128]] = [30, 20, 10]                                      # lane 0: its first hit is its largest
            s[[1, 65]] = [10, 20]                                               # lane 1: its last hit is
            s[129 if n > 129 else 65] = 30
            add(n, s, 0, 0, "descending lane 0, ascending lane 1")
            s = np.full(n, -7)
            s[[1, 65]] = [10, 20]
            s[128] = 5                                                          # lane 0's last hit is its largest, not the wave's
            add(n, s, 65, 1, "a lane whose last hit is its largest below the maximum")
        for name, s in (("INT32_MIN", np.full(n, INT32_MIN)), ("INT32_MAX", np.full(n, INT32_MAX)),
                        ("INT32_MIN and INT32_MAX", np.where(rng.random(n) < 0.5, INT32_MIN, INT32_MAX))):
            s = s.astype(np.int64)
            if name.endswith("and INT32_MAX"):
                s[n - 1] = INT32_MAX
            ref_at = int(np.nonzero(s == s.max())[0][-1])
            add(n, s, ref_at, 0 if (s == s.max()).sum() > 1 else 1, f"every score {name}")
    return b.finish()


# ---- family 7: hostile offsets --------------------------------------------------------------------------------------------------

HOSTILE_HITS = 300
HOSTILE_ALLOC = 1024


def _hostile(name, offsets, seed):
    L = [[1, 2, 10 + i] for i in range(20)]
    m, ln = to_matrix(L)
    b = Builder(7, name, m, ln, seed=seed)
    t = b.finish()
    rng = np.random.default_rng(seed)
    t.seg = np.array(offsets, np.uint64)
    nq = len(offsets) - 1
    t.bs = rng.integers(-1000, 1000, HOSTILE_HITS).astype(np.int32)
    t.desc = np.where(rng.random(HOSTILE_HITS) < 0.2, -1, rng.integers(0, len(L), HOSTILE_HITS)).astype(np.int64)
    t.recs = np.zeros(nq, engine.RESULT_DTYPE)
    t.recs["status"] = rng.choice([2, 16, 17, 18, 19, 20], nq)                  # no taxon: no reference row is involved
    t.recs["ref_row"] = U32_MAX
    t.q_pos = t.q_need = t.q_lo = t.q_hi = np.full(nq, -1, np.int64)
    t.q_note = [f"offsets {int(offsets[q])} .. {int(offsets[q + 1])} of {HOSTILE_HITS} hits" for q in range(nq)]
    return t


@functools.lru_cache(None)
def hostile_offsets():
    """status >= 2 records over offsets that the kernel clamps: a pair with s0 > s1, a segment that starts at n_hits, offsets
    past n_hits (by a little, by 2^40), the last offset past n_hits in front of a segment that still holds hits."""
    return _hostile("hostile", [0, 50, 40, 120, 300, 300, 1000, 700, 1 << 40, 250, 5000], 17)


@functools.lru_cache(None)
def hostile_offsets_inside_allocation():
    """The same kinds with every offset below HOSTILE_ALLOC: run on columns that are the first HOSTILE_HITS elements of
    HOSTILE_ALLOC-element buffers, what lies behind n_hits is real memory that must not be counted."""
    return _hostile("hostile_inside_allocation", [0, 50, 40, 120, 300, 300, 1000, 700, 250, 900], 18)


# ---- family 8: strides ----------------------------------------------------------------------------------------------------------

def packed_rows(eng_rows, words, fill, seed=0):
    """[n, words] uint32 side records: word 0 the engine row id, every other word 0xFFFFFFFF (fill "ones") or noise."""
    n = len(eng_rows)
    if fill == "ones":
        out = np.full((n, words), 0xFFFFFFFF, np.uint32)
    else:
        out = np.random.default_rng(seed).integers(0, 1 << 32, (n, words), dtype=np.uint64).astype(np.uint32)
    out[:, 0] = eng_rows
    return out


SMALL_TABLES = ("near_sweep", "skip_path") + tuple(f"n_tax_{n}" for n in TABLE_SIZES) + ("levels", "levels_bad")   # families 1, 2, 4, 5
ALL_TABLES = SMALL_TABLES + ("segment_scan", "high_levels")


def table(name):
    """A table by name, built on first use."""
    if name in ("levels", "levels_bad"):
        return levels()[name == "levels_bad"]
    if name.startswith("n_tax_"):
        return table_ends()[TABLE_SIZES.index(int(name[6:]))]
    return {"near_sweep": near_sweep, "skip_path": skip_path, "segment_scan": segment_scan, "high_levels": high_levels}[name]()


def small_tables():
    """Every table of families 1, 2, 4 and 5."""
    return [table(name) for name in SMALL_TABLES]


# ---- invariants of DESIGN.md §15.1 ----------------------------------------------------------------------------------------------

def assert_invariants(fields, t):
    f = {k: np.asarray(fields[k]).astype(np.int64) for k in ref.SUPPORT_FIELDS}
    recs = t.recs
    assert (f["n_support"] <= f["n_matched"]).all() and (f["n_matched"] <= f["n_hits"]).all()
    assert (f["n_top_support"] <= f["n_top"]).all() and (f["n_top"] <= f["n_hits"]).all()
    placed = (recs["status"] < 2) & (recs["level_mask"] != 0) & (t.q_lo >= 0)   # (q_lo < 0: need > len, no clade)
    assert (f["n_top_support"][placed] >= 1).all()
    assert (f["n_top"][recs["status"] == 1] == 1).all()
    none = (recs["status"] >= 2) | ((recs["status"] < 2) & (t.q_lo < 0))
    assert not f["n_top_support"][none].any() and not f["n_support"][none].any() and not f["support_bits"][none].any()
    empty = f["n_hits"] == 0
    for k in ref.SUPPORT_FIELDS:
        assert not f[k][empty].any()
