"""Taxonomies, a restatement and cases for the shared-level lookups of the consensus kernels.

How many leading levels do the sorted taxonomy rows [lo, hi] of a top group share?  consensus_kernel.hip answers in five ways,
depending on where the group lies in the table: the reference row's run-length bytes, those bytes and then the range-minimum
tables, the wide-node chains (three depth classes), the range-minimum tables where the chains do not reach (an overflow block,
no wide tables), and the branch-free `shared_levels()` of the long kernel and the worklist path.  This module builds small
taxonomies in which every one of those answers is asked for at its edges, restates the answer from the lineages alone
(`Table.shared`), says which way the stream kernel must take (`Table.path_of`) and which shape of `shared_levels()` a span has
(`Table.shapes_of`), and lays the cases out as hit tables.  Test infrastructure only: deterministic, no GPU, no product code.

Every table is emitted in sorted order (node ids are handed out in depth-first order of first appearance), so a sorted position
is also a row of the input arrays; the tests still go through `Taxonomy.row_map()`.
"""
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from blutils_amd import synth

BACKBONE = ["d", "k", "p", "c", "o", "f", "g", "s"]
RANK_NAMES = BACKBONE + ["clade", "strain"]
ZERO_CUTS = {"domain": 0, "kingdom": 0, "phylum": 0, "class": 0, "order": 0, "family": 0, "genus": 0, "species": 0}

# what the issue's description of the engine fixes (blu_internal.h holds the same numbers; they are restated, not imported)
WIDE_MIN = 128          # rows from which a node is wide
RUN_MAX = 127           # a run-length byte saturates here
ROW_LEVELS = 20         # levels whose run lengths sit in the row
BLOCK = 64              # sorted positions per wide-node block entry
BLOCK_CHANGES = 2       # changes of the deepest wide node one entry holds
CHAIN_FIRST, CHAIN = 12, 16
MAX_WIDE_LEVELS, MAX_WIDE_NODES = 32, 65534
LCP_BLOCK = 16          # entries per block of the range-minimum tables

ROW_BYTES, ROW_BYTES_RMQ = "row bytes", "row bytes -> rmq"
CHAIN_0, CHAIN_12, CHAIN_16 = "chain 0-11", "chain 12-15", "chain 16-31"
OVERFLOW_RMQ, NO_TABLES_RMQ, NO_WIDE_NODE = "overflow -> rmq", "no wide tables -> rmq", "no wide node around lo"
PATHS = (ROW_BYTES, ROW_BYTES_RMQ, CHAIN_0, CHAIN_12, CHAIN_16, OVERFLOW_RMQ, NO_TABLES_RMQ, NO_WIDE_NODE)
# the classes answered by a chain lookup (`via == 1` on the host): "no wide node" reads row 0 of the chain table, which is all zeros
CHAIN_LOOKUPS = (CHAIN_0, CHAIN_12, CHAIN_16, NO_WIDE_NODE)
SHAPES = ("one block", "head at 0", "empty tail", "no middle", "middle k=0", "middle k=1", "middle k=2", "middle k>=3", "last block")

WIDTHS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 126, 127, 128, 129, 130, 191, 192, 193, 255, 256, 257, 400, 700, 1000)
FORMS = (0, 200, 600)   # lower-scoring rows around the top rows: stream kernel, long pass, worklist / long kernel
EDGE_DISTANCES = (0, 1, 126, 127, 128)


class Table:
    """A taxonomy in sorted order with everything the restatement needs: `nodes` [n, depth] (-1 beyond a row's length),
    `length` [n], `lcp` [n - 1] (levels shared by rows i and i + 1) and, per level, the run of rows around each row."""

    def __init__(self, name, nodes, length, ranks=None):
        self.name = name
        nodes = np.asarray(nodes, np.int64)
        length = np.asarray(length, np.int64)
        n, depth = nodes.shape
        self.n, self.depth, self.nodes, self.length = n, depth, nodes, length
        lv = np.arange(depth)
        has = lv[None, :] < length[:, None]
        assert (nodes[has] >= 0).all() and (nodes[~has] == -1).all()
        # sorted order: lexicographic by node id, a prefix before its extensions (ties keep the input order)
        for a in range(0, n - 1, 65536):
            b = min(a + 65536, n - 1)
            x, y = nodes[a:b], nodes[a + 1:b + 1]
            ne = x != y
            first = np.where(ne.any(1), ne.argmax(1), depth)
            k = np.minimum(first, depth - 1)
            r = np.arange(len(x))
            assert ((first == depth) | (x[r, k] < y[r, k])).all(), f"{name}: rows are not in sorted order"
        if n > 1:
            eq = (nodes[:-1] == nodes[1:]) & has[:-1] & has[1:]
            self.lcp = np.where(eq.all(1), depth, (~eq).argmax(1)).astype(np.int64)
        else:
            self.lcp = np.zeros(0, np.int64)
        if ranks is None:   # the backbone for the first eight levels, clade below, strain last (only rows of the full depth have it)
            ranks = np.where(lv < 8, np.minimum(lv, 7), 8)[None, :].repeat(n, 0)
            full = (length == depth) & (depth > 8)
            ranks[full, depth - 1] = 9
        off = np.concatenate([[0], np.cumsum(length)]).astype(np.uint64)
        self.tax = synth.SynthTaxonomy(list(RANK_NAMES), off, nodes[has].astype(np.uint32), ranks[has].astype(np.uint16),
                                       (100 + np.arange(n)).astype(np.int64), np.zeros((9, n), np.int32), np.zeros((9, n), np.int32), n, 0, False)
        # runs: at level j a node is a maximal stretch of rows that have level j and share levels 0 .. j
        idx = np.arange(n)
        hasT = has.T                                              # [depth, n]
        lcp_prev = np.concatenate([[0], self.lcp])                # levels shared with the previous row
        lcp_next = np.concatenate([self.lcp, [0]])
        starts = hasT & (lcp_prev[None, :] <= lv[:, None])
        ends = hasT & (lcp_next[None, :] <= lv[:, None])
        self.run_start = np.maximum.accumulate(np.where(starts, idx[None, :], -1), axis=1).astype(np.int32)
        self.run_end = (np.minimum.accumulate(np.where(ends, idx[None, :], n)[:, ::-1], axis=1)[:, ::-1] + 1).astype(np.int32)   # exclusive
        self.has = hasT
        wide = hasT & (self.run_end - self.run_start >= WIDE_MIN)
        self.wide_level = wide.sum(0) - 1                         # deepest wide node around each position (-1: none): its ancestors are wide too
        self.n_wide = int((starts & wide).sum())
        self.wide_levels = int(self.wide_level.max()) + 1 if n else 0
        self.wide_tables = self.n_wide <= MAX_WIDE_NODES and self.wide_levels <= MAX_WIDE_LEVELS
        wl = np.maximum(self.wide_level, 0)
        ident = np.where(self.wide_level >= 0, (wl + 1) * (n + 1) + self.run_start[wl, idx], 0)
        change = np.zeros(n, bool)
        change[1:] = ident[1:] != ident[:-1]
        change[::BLOCK] = False                                   # a block's first row is its entry's first node, not a change
        self.block_changes = np.bincount(idx[change] // BLOCK, minlength=n // BLOCK + 1)
        self.change = change
        self.node_edges = np.nonzero(np.concatenate([[False], ident[1:] != ident[:-1]]))[0]

    # ---- the plain restatement ------------------------------------------------------------------------------------
    def shared(self, lo, hi):
        """Leading levels shared by every sorted row of [lo, hi]: the minimum of the adjacent common-prefix lengths."""
        return int(self.lcp[lo:hi].min()) if lo < hi else int(self.length[lo])

    # ---- which way the stream kernel takes ------------------------------------------------------------------------
    def path_of(self, lo, ref, hi, minlen=None):
        assert 0 <= lo <= ref <= hi < self.n
        dl, dh = ref - lo, hi - ref
        if minlen is None:
            minlen = int(min(self.length[lo], self.length[ref], self.length[hi]))
        if dl <= RUN_MAX and dh <= RUN_MAX:
            if lo == hi:
                return ROW_BYTES
            top = min(ROW_LEVELS, int(self.length[ref]))
            reach = (ref - self.run_start[:top, ref] >= dl) & (self.run_end[:top, ref] - 1 - ref >= dh)
            return ROW_BYTES_RMQ if int(reach.sum()) >= ROW_LEVELS and minlen > ROW_LEVELS else ROW_BYTES
        if not self.wide_tables:
            return NO_TABLES_RMQ
        if self.block_changes[lo // BLOCK] > BLOCK_CHANGES:
            return OVERFLOW_RMQ
        w = int(self.wide_level[lo])
        if w < 0:
            return NO_WIDE_NODE
        holds = self.run_end[: w + 1, lo] > hi                    # the chain of the deepest wide node around lo: one end per level
        if self.wide_levels > CHAIN_FIRST and int(holds[:CHAIN_FIRST].sum()) == CHAIN_FIRST:
            if self.wide_levels > CHAIN and int(holds[:CHAIN].sum()) == CHAIN:
                return CHAIN_16
            return CHAIN_12
        return CHAIN_0

    def block_slot(self, lo):
        """Where `lo` lies in its block's entry: (changes of the deepest wide node at or before it: 0, 1, 2; lo is the very row
        of a change).  The entry holds three nodes and the two offsets at which they change: both compares have an edge."""
        b = lo - lo % BLOCK
        return int(self.change[b:lo + 1].sum()), bool(self.change[lo])

    # ---- which shape of the branch-free shared_levels() -----------------------------------------------------------
    def shapes_of(self, lo, hi):
        assert lo < hi
        b0, b1 = (lo + LCP_BLOCK - 1) // LCP_BLOCK, hi // LCP_BLOCK
        out = []
        if b0 > b1:
            out.append("one block")
        else:
            if lo % LCP_BLOCK == 0:
                out.append("head at 0")
            if hi % LCP_BLOCK == 0:
                out.append("empty tail")
            if b0 == b1:
                out.append("no middle")
            else:
                k = (b1 - b0).bit_length() - 1
                out.append(f"middle k={k}" if k < 3 else "middle k>=3")
        if b1 == (self.n - 1) // LCP_BLOCK:
            out.append("last block")
        return tuple(out)


# ---- builders ------------------------------------------------------------------------------------------------------
def _from_paths(name, rows, depth):
    """rows: label tuples in depth-first order, a prefix before its extensions.  A node is (level, label); ids in order of
    first appearance, so the order given is the sorted order."""
    ids = {}
    nodes = np.full((len(rows), depth), -1, np.int64)
    for r, path in enumerate(rows):
        assert 0 < len(path) <= depth
        for j, label in enumerate(path):
            nodes[r, j] = ids.setdefault((j, label), len(ids))
    return Table(name, nodes, [len(p) for p in rows])


def _own(tag, depth, frm, prefix=()):
    """`prefix`, then nodes of the row's own from level `frm` down to `depth`."""
    return tuple(prefix) + tuple(("own", tag, j) for j in range(frm, depth))


def _outside(tag, k, depth):
    """k rows outside every trunk, in families of 50 under roots of their own: no wide node around them."""
    return [_own((tag, i), depth, 1, prefix=[("fam", tag, i // 50)]) for i in range(k)]


def chain(L, spacing, depth, short_rows, extra):
    """Nested trunk nodes: level j holds 128 + spacing * (L - 1 - j) rows, each inside the one above.  A row leaves the trunk at
    its deepest level into nodes of its own; with `short_rows` every seventh row ends there instead (the row is the node).
    `extra` rows outside every trunk, half in front, half behind."""
    assert depth > L
    trunk = [("trunk", j) for j in range(L)]
    at = [[] for _ in range(L)]                                    # rows by the level at which they leave the trunk
    r = 0
    for j in range(L - 1, -1, -1):
        for _ in range(WIDE_MIN if j == L - 1 else spacing):
            at[j].append(tuple(trunk[: j + 1]) if short_rows and r % 7 == 3 else _own(r, depth, j + 1, prefix=trunk[: j + 1]))
            r += 1
    rows = _outside("front", extra // 2, depth)
    rows += [tuple(p) for j in range(L) for p in at[j] if len(p) == j + 1]                 # the short rows: prefixes first
    rows += [p for j in range(L - 1, -1, -1) for p in at[j] if len(p) != j + 1]
    rows += _outside("back", extra - extra // 2, depth)
    return _from_paths(f"chain({L},{spacing},{depth},{int(short_rows)},{extra})", rows, depth)


def runs(level, size):
    """Three sibling nodes at `level`, exactly `size` rows each, side by side under one trunk; inside a sibling the rows split
    once more at the next level (64 rows, then the rest), so levels below `level` agree for some spans and not for others."""
    depth = max(22, level + 3)
    trunk = [("trunk", j) for j in range(level)]
    rows = _outside("front", 5, depth)
    for s in range(3):
        for r in range(size):
            rows.append(_own((s, r), depth, level + 2, prefix=trunk + [("sib", s), ("sub", s, r // 64)]))
    if level > 0:
        rows += [_own(("in", i), depth, level, prefix=trunk) for i in range(3)]           # rows of the trunk beside the siblings
    rows += _outside("back", 5, depth)
    return _from_paths(f"runs({level},{size})", rows, depth)


def block_changes():
    """64-row blocks with 0, 1, 2 and 3 changes of the deepest wide node, at block offsets 1 and 63 (and 32 in the block of
    three): R (level 0) > P (level 1) > A, B, C (level 2).  A = [0, 193), B = [193, 321), rows of P alone [321, 383),
    C = [383, 513), P alone [513, 544), R alone [544, 575), then 100 rows with no wide node (the change at 575 is to none)
    and a wide root Q at [675, 815)."""
    depth = 22
    R, P = ("R",), ("P",)
    rows = []

    def add(k, prefix):
        for _ in range(k):
            rows.append(_own(len(rows), depth, len(prefix), prefix=prefix))
    add(193, [R, P, ("A",)])
    add(128, [R, P, ("B",)])
    add(62, [R, P])
    add(130, [R, P, ("C",)])
    add(31, [R, P])
    add(31, [R])
    rows += _outside("none", 100, depth)
    add(140, [("Q",)])
    t = _from_paths("block_changes()", rows, depth)
    assert list(t.block_changes[:11]) == [0, 0, 0, 1, 0, 2, 0, 0, 3, 0, 1], t.block_changes
    return t


def limit(n_wide):
    """32-level nested chains over 159 rows each (spacing 1), one shorter chain and one plain wide node last: exactly `n_wide`
    wide nodes, depth 33.  65 534 is the most the wide tables hold; with 65 535 there are none.  Built in numpy."""
    depth, L = 33, 32
    full, rest = divmod(n_wide - 1, L)
    lens = [WIDE_MIN + L - 1] * full + ([WIDE_MIN + rest - 1] if rest else []) + [200]
    tops = [L] * full + ([rest] if rest else []) + [1]            # trunk levels of each chain
    start = np.concatenate([[0], np.cumsum(lens)])
    n = int(start[-1])
    c = np.repeat(np.arange(len(lens)), lens)
    i = np.arange(n) - start[c]
    top = np.asarray(tops)[c]
    tj = np.clip(top - 1 - (i - (WIDE_MIN - 1)), 0, top - 1)      # deepest trunk level of the row: the first 128 rows hold them all
    lv = np.arange(depth)
    nodes = np.where(lv[None, :] <= tj[:, None], 1 + c[:, None] * 64 + lv[None, :], (1 << 27) + np.arange(n)[:, None] * 64 + lv[None, :])
    t = Table(f"limit({n_wide})", nodes, np.full(n, depth))
    assert t.n_wide == n_wide, (t.n_wide, n_wide)
    return t


CHAINS = ((12, 70, 20, False, 62), (13, 20, 21, False, 17), (16, 64, 20, False, 63), (16, 30, 21, False, 9), (17, 9, 21, False, 150), (17, 21, 64, True, 140),
          (17, 70, 64, False, 32), (32, 3, 64, False, 200), (32, 20, 64, True, 20), (33, 5, 64, False, 130))
RUNS = tuple((level, size) for level in (0, 1, 18, 19, 20, 21) for size in (126, 127, 128, 129, 130))
LIMITS = (65534, 65535)
SMALL = tuple(("chain",) + a for a in CHAINS) + tuple(("runs",) + a for a in RUNS) + (("block_changes",),)
INSTANCES = SMALL + tuple(("limit", k) for k in LIMITS)


def instance_id(inst):
    return inst[0] + "(" + ",".join(str(int(a)) for a in inst[1:]) + ")"


@functools.lru_cache(maxsize=None)
def table(inst) -> Table:
    return {"chain": chain, "runs": runs, "block_changes": block_changes, "limit": limit}[inst[0]](*inst[1:])


# ---- cases ---------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    lo: int
    ref: int                      # the row meant to be the reference row (it is, wherever the group's lineages have one length)
    hi: int
    extra: Optional[int] = None   # a fourth row strictly inside

    @property
    def rows(self) -> Tuple[int, ...]:
        return (self.lo, self.ref, self.hi) + (() if self.extra is None else (self.extra,))


def _anchors(t: Table, cap=48):
    a = {0, 1, 15, 16, 17, 63, 64, 65, t.n - 1, t.n - 2, t.n - 16, t.n - 17, t.n - 18}
    edges = list(t.node_edges)
    if len(edges) > cap:
        edges = edges[: cap // 2] + edges[-cap // 2:]
    for e in edges:
        a.update((int(e) - 1, int(e), int(e) + 1))
    over = np.nonzero(t.block_changes > BLOCK_CHANGES)[0][:4]
    a.update(int(b) * BLOCK + o for b in over for o in (0, 31, 63))
    return sorted(p for p in a if 0 <= p < t.n)


def _run_anchors(t: Table, cap=16):
    """Rows at the edge distances from either end of the runs of about a wide node's size, wide or not."""
    big = t.has & (t.run_end - t.run_start >= WIDE_MIN - 8)
    ends = sorted(set(t.run_start[big].tolist()) | set((t.run_end[big] - 1).tolist()))
    if len(ends) > cap:
        ends = ends[: cap // 2] + ends[-cap // 2:]
    a = {e + s * d for e in ends for d in EDGE_DISTANCES for s in (1, -1)}
    return sorted(p for p in a if 0 <= p < t.n)


@functools.lru_cache(maxsize=None)
def cases(inst, per_bucket=2, limit_to=600):
    """Spans at the block, node and table edges with the reference row at either end, in the middle and 127 / 128 rows from an
    end, and reference rows with both distances out of {0, 1, 126, 127, 128}; of the candidates that fall into one bucket —
    (path class, slot of lo in its block's entry, both distances, shared depth) for the second kind, (path class, slot, shape,
    place of the reference row) for the first — the first one or two are kept, so that no class rests on one table's one case."""
    t = table(inst)
    anchors = _anchors(t)
    kept, buckets, seen = [], {}, set()

    def offer(lo, ref, hi, key_extra):
        if not (0 <= lo <= ref <= hi < t.n) or (lo, ref, hi) in seen:
            return
        seen.add((lo, ref, hi))
        path = t.path_of(lo, ref, hi)
        key = (path, t.block_slot(lo) if path in CHAIN_LOOKUPS else None) + key_extra
        if buckets.get(key, 0) < (per_bucket if len(key_extra) == 2 else 1):
            buckets[key] = buckets.get(key, 0) + 1
            extra = None
            if hi - lo >= 2 and len(kept) % 3 == 0:
                extra = lo + 1 + (7 * len(kept)) % (hi - lo - 1)
            kept.append(Case(lo, ref, hi, extra))

    for a in sorted(set(anchors) | set(_run_anchors(t))):
        for dl in EDGE_DISTANCES:
            for dh in EDGE_DISTANCES:
                lo, hi = a - dl, a + dh
                if 0 <= lo and hi < t.n:
                    offer(lo, a, hi, (dl, dh, t.shared(lo, hi)))
    n_edge = len(kept)
    for a in anchors:
        for w in WIDTHS + (31, 32, 33, 47, 48):
            for lo, hi in ((a, a + w), (a - w, a)):
                for k, ref in enumerate((lo, hi, (lo + hi) // 2, lo + 127, lo + 128, hi - 127, hi - 128)):
                    if lo < hi:
                        offer(lo, min(max(ref, lo), hi), hi, (t.shapes_of(lo, hi), k))
    if len(kept) > limit_to > n_edge:      # thin the second kind evenly, never by class: the coverage test counts what is left
        rest = kept[n_edge:]
        kept = kept[:n_edge] + [rest[i] for i in np.linspace(0, len(rest) - 1, limit_to - n_edge).astype(int)]
    return tuple(kept)


def reference_hit(lengths, align_len, acc_rank, strategy):
    """The engine's rule for a top group of equal identities: stable sort by (lineage length, identity, align_len, acc_rank);
    cautious takes the first, relaxed the last.  Index into the group, which is in file order."""
    keys = [(int(l), int(a), int(c)) for l, a, c in zip(lengths, align_len, acc_rank)]
    order = sorted(range(len(keys)), key=keys.__getitem__)   # (sorted() is stable)
    return order[0] if strategy == "cautious" else order[-1]


def build_hits(t: Table, case_list, strategy, inv, forms=FORMS, interleave=False, seed=11):
    """One query per (case, form): the case's rows with bit-score 900, identity 100, spread among `form` lower-scoring rows of
    random taxa.  The row meant as the reference gets the align_len that wins under `strategy`; where lineage lengths differ
    the rule decides, and `ref_pos` / `ref_row` say what it decided.  inv: sorted position -> input row (Taxonomy.row_map()[1]).
    Returns (hits, meta): hits as the parity tests pass them around (+ pident_milli), meta with one entry per query."""
    specs = [(ci, f) for ci in range(len(case_list)) for f in forms] if interleave else [(ci, f) for f in forms for ci in range(len(case_list))]
    g = np.array([len(case_list[ci].rows) for ci, _ in specs], np.int64)
    lens = g + np.array([f for _, f in specs], np.int64)
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nh = int(seg[-1])
    rng = np.random.default_rng(seed)
    bs = rng.integers(100, 800, nh).astype(np.int32)
    pos = rng.integers(0, t.n, nh)
    pm = rng.integers(70000, 100001, nh).astype(np.uint32)
    aln = rng.integers(380, 480, nh).astype(np.int32)
    acc = rng.integers(0, 50, nh).astype(np.int32)
    win = 399 if strategy == "cautious" else 401
    meta = {"case": np.array([ci for ci, _ in specs]), "form": np.array([f for _, f in specs]),
            "ref_row": np.zeros(len(specs), np.int64), "ref_pos": np.zeros(len(specs), np.int64), "minlen": np.zeros(len(specs), np.int64)}
    for q, (ci, _) in enumerate(specs):
        rows = case_list[ci].rows
        k = len(rows)
        turn = ci % k                                              # file order differs from case to case
        order = [(turn + i) % k for i in range(k)]
        step = int(lens[q]) // k
        at = int(seg[q]) + (ci % step) + step * np.arange(k)
        a = np.array([win if i == 1 else 400 for i in order], np.int32)
        c = 1000 + np.arange(k, dtype=np.int32)
        p = np.array([rows[i] for i in order])
        bs[at], pos[at], pm[at], aln[at], acc[at] = 900, p, 100000, a, c
        r = reference_hit(t.length[p], a, c, strategy)
        meta["ref_row"][q], meta["ref_pos"][q], meta["minlen"][q] = at[r], p[r], t.length[p].min()
    hits = {"seg_off": seg, "bitscore": bs, "tax_row": np.asarray(inv)[pos].astype(np.int32), "pident": pm.astype(np.float64) / 1000.0,
            "align_len": aln, "acc_rank": acc, "pident_milli": pm}
    return hits, meta


def expected(t: Table, case_list, meta):
    """Per query, from the restatement alone: (shared, root_disagree, agree, bean_index)."""
    out = []
    for q, ci in enumerate(meta["case"]):
        c = case_list[ci]
        s, m = t.shared(c.lo, c.hi), int(meta["minlen"][q])
        out.append((s, s == 0, s >= m, (m if s >= m else s) - 1))
    return out
