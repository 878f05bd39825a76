"""Boundary tables for the conformance matrix (tests/test_gpu_conformance.py); numpy + the CPU oracle, no GPU.

A table is a synthetic taxonomy plus a hit table whose segment lengths reach every path of the consensus kernels (empty,
single-row, every streamed width, the long pass, the worklist kernel) and whose top groups carry identities right at a
level's cutoff: for most queries a level j of the first top row is picked, its cutoff c is taken from the ORACLE's
interpolation of that row's ranks, and every row of the top group gets one value of the boundary set

    kthr(c) - 1, kthr(c), kthr(c) + 1          (milli-percent; kthr(c) = smallest k with k / 1000.0 >= c)
    nextafter(c, -inf), c, nextafter(c, +inf)  (f64 only)

so that the reference row and the group maximum both carry it.  `>=` (filter) and `>` (skip_while) only part at
identity == cutoff, and an off-by-one in the engine's integer thresholds only shows one milli-percent below, at or above
them.  The other queries keep the generator's random identities, so integer-keyed and f64 wave tasks sit side by side.

`grid=True` gives the on-grid variant of the same table (the f64 kinds fold onto their milli-percent counterparts), for
the layouts that carry milli-percent identities."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np

from blutils_amd import synth
from oracle import oracle as orc

KINDS = ("kthr-1", "kthr", "kthr+1", "c-ulp", "c", "c+ulp")
MILLI_KINDS = KINDS[:3]
KTHR_NEVER = (1 << 17) - 1          # the engine's 17-bit identity range: [0, 131 071)

# segment length -> queries of it per 3000 (every kernel path: streamed widths 4..32 lanes, the long pass, the worklist)
# (few enough segments past 512 rows that a table's worklist queue can stay short: the device path's "skip the worklist
# kernel" bit is then set for its repeated calls)
LENGTHS = {0: 40, 1: 300, 3: 300, 10: 500, 17: 400, 33: 400, 64: 300, 65: 300, 129: 150, 257: 80, 513: 12, 700: 8,
           1100: 3, 1300: 3, 1500: 3}
TOP_GROUPS = ("geo", "zymo", "all")


def kthr(c):
    """Smallest k in [0, KTHR_NEVER) with fl(k / 1000) >= c (KTHR_NEVER if none), elementwise."""
    c = np.atleast_1d(np.asarray(c, dtype=np.float64))
    k = np.clip(np.ceil(np.nan_to_num(c, nan=KTHR_NEVER) * 1000.0), 0, KTHR_NEVER).astype(np.int64)
    for _ in range(2):      # ceil(c * 1000) is at most one off the smallest passing k on either side
        down = (k > 0) & ((k - 1) / 1000.0 >= c)
        k = np.where(down, k - 1, k)
        up = (k < KTHR_NEVER) & (k / 1000.0 < c)
        k = np.where(up, k + 1, k)
    return np.where(np.isnan(c), KTHR_NEVER, k)


def kthr_equal(c):
    """The engine's "equals" bit: fl(kthr(c) / 1000) == c (then `>` needs one milli-percent more than `>=`)."""
    k = kthr(c)
    return (k < KTHR_NEVER) & (k / 1000.0 == np.atleast_1d(c))


@dataclass
class BoundaryTable:
    tax: synth.SynthTaxonomy
    hits: Dict[str, np.ndarray]     # seg_off bitscore tax_row (desc rows) pident align_len acc_rank (+ pident_milli if grid)
    kind: np.ndarray                # int8 per query: index into KINDS, -1 = random identities
    level: np.ndarray               # int16 per query: the level j of the first top row whose cutoff was approached
    cutoff: np.ndarray              # f64 per query: that cutoff (oracle)
    taxon: str
    custom: Optional[dict]
    grid: bool
    _expected: dict = field(default_factory=dict, repr=False)

    @property
    def n_queries(self) -> int:
        return len(self.hits["seg_off"]) - 1

    def expected(self, strategy: str) -> np.ndarray:
        """The columnar oracle's records (cached)."""
        if strategy not in self._expected:
            h = self.hits
            self._expected[strategy] = orc.columnar_run(
                self.tax.lin_off, self.tax.lin_node, self.tax.lin_rank, self.tax.rank_names, h["seg_off"], h["bitscore"],
                h["tax_row"], h["pident"], h["align_len"], h["acc_rank"], taxon=self.taxon, strategy=strategy,
                custom=self.custom, threads=8)
        return self._expected[strategy]

    def counts(self, strategies=("relaxed", "cautious")) -> Dict[str, Dict[str, int]]:
        """Per boundary kind: queries carrying it, and over the strategies how many oracle records take (pass) or leave
        out (fail) the chosen level in their level mask (records without a consensus count as neither)."""
        out = {k: {"queries": int((self.kind == i).sum()), "pass": 0, "fail": 0} for i, k in enumerate(KINDS)}
        q = np.nonzero(self.kind >= 0)[0]
        for s in strategies:
            rec = self.expected(s)[q]
            ok = rec["status"] <= 1
            bit = ((rec["level_mask"] >> self.level[q].astype(np.uint64)) & np.uint64(1)).astype(bool)
            for i, k in enumerate(KINDS):
                m = ok & (self.kind[q] == i)
                out[k]["pass"] += int((m & bit).sum())
                out[k]["fail"] += int((m & ~bit).sum())
        return out

    def with_segments(self, seg_off: np.ndarray) -> "BoundaryTable":
        """The same rows cut into other queries (same query and row counts): boundary bookkeeping does not carry over."""
        assert len(seg_off) == len(self.hits["seg_off"]) and seg_off[-1] == self.hits["seg_off"][-1]
        nq = self.n_queries
        return BoundaryTable(self.tax, dict(self.hits, seg_off=np.ascontiguousarray(seg_off, dtype=np.int64)), np.full(nq, -1, np.int8),
                             np.zeros(nq, np.int16), np.zeros(nq), self.taxon, self.custom, self.grid)


def even_segments(seg_off: np.ndarray) -> np.ndarray:
    """Another offset table over the same rows and query count: every query of (nearly) the same length, none long
    enough for the worklist kernel."""
    nq, nh = len(seg_off) - 1, int(seg_off[-1])
    lens = np.full(nq, nh // nq, dtype=np.int64)
    lens[: nh % nq] += 1
    assert lens.max() <= 512
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def long_segments(seg_off: np.ndarray, seed: int, lo: int = 1100, hi: int = 1500) -> np.ndarray:
    """Another offset table over the same rows and query count: segments of lo..hi rows (the worklist kernel), the
    remaining queries empty, in shuffled order."""
    rng = np.random.default_rng(seed)
    nq, nh = len(seg_off) - 1, int(seg_off[-1])
    lens = []
    left = nh
    while left > 0 and len(lens) < nq:
        n = min(left, int(rng.integers(lo, hi + 1)))
        lens.append(n)
        left -= n
    if left:
        lens[-1] += left
    lens = np.array(lens + [0] * (nq - len(lens)), dtype=np.int64)
    lens = lens[rng.permutation(nq)]
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def build(seed: int, taxon: str, custom: Optional[dict] = None, deep: bool = True, n_taxa: int = 4000,
          scale: float = 1.0, grid: bool = False, p_boundary: float = 0.8, p_one_taxon: float = 0.5) -> BoundaryTable:
    """One boundary table.  scale multiplies the query counts of LENGTHS (about 3000 queries and 150 k rows at 1.0).
    p_one_taxon: share of boundary queries whose top group is put on one taxon (agreement down to its last level, so the
    level's cutoff alone decides); the others keep the generator's top groups (disagreement and other reference rows)."""
    rng = np.random.default_rng(seed)
    tax = synth.make_taxonomy(n_taxa, seed, deep=deep)
    parts, lens = [], []
    sub = 0
    for L, n in LENGTHS.items():
        n = max(1, int(round(n * scale))) if L >= 1000 else int(round(n * scale))
        for g, m in zip(TOP_GROUPS, (n - 2 * (n // 3), n // 3, n // 3)):
            if m == 0:
                continue
            sub += 1
            lens += [L] * m
            if L:
                parts.append(synth.make_hits(tax, m, seed * 1000 + sub, L, p_unmatched=0.003, top_group=g).numpy())
    keys = ("bitscore", "tax_row", "pident", "align_len", "acc_rank")
    cols = {k: np.concatenate([p[k] for p in parts]) for k in keys}
    lens = np.array(lens, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    order = rng.permutation(len(lens))                        # lengths and top-group kinds interleaved across wave tasks
    lens, starts = lens[order], starts[order]
    take = np.concatenate([np.arange(s, s + l) for s, l in zip(starts, lens)])
    hits = {k: cols[k][take].copy() for k in keys}
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    hits = {"seg_off": seg, **hits}

    nq = len(lens)
    kind = np.full(nq, -1, np.int8)
    level = np.zeros(nq, np.int16)
    cutoff = np.zeros(nq)
    cuts_of: Dict[tuple, np.ndarray] = {}
    tr, pid, bs = hits["tax_row"], hits["pident"], hits["bitscore"]
    draws = rng.random((nq, 4))
    for q in range(nq):
        a, b = int(seg[q]), int(seg[q + 1])
        if a == b or draws[q, 0] >= p_boundary:
            continue
        top = a + np.nonzero(bs[a:b] == bs[a:b].max())[0]
        t0 = int(tr[top[0]])
        if t0 < 0:
            continue
        if draws[q, 1] < p_one_taxon:
            tr[top] = t0
        shape = tuple(tax.lin_rank[int(tax.lin_off[t0]):int(tax.lin_off[t0 + 1])])
        if shape not in cuts_of:
            cuts_of[shape] = orc.interpolate([tax.rank_names[r] for r in shape], taxon, custom)[0]
        cuts = cuts_of[shape]
        j = int(draws[q, 2] * len(cuts))
        c = float(cuts[j])
        k = int(draws[q, 3] * len(KINDS))
        if grid:
            k %= 3
        kt = int(kthr(c)[0])
        v = {0: max(kt - 1, 0) / 1000.0, 1: kt / 1000.0, 2: (kt + 1) / 1000.0,
             3: np.nextafter(c, -np.inf), 4: c, 5: np.nextafter(c, np.inf)}[k]
        pid[top] = v
        kind[q], level[q], cutoff[q] = k, j, c
    if grid:
        pm = np.round(pid * 1000.0).astype(np.uint32)
        assert (pm / 1000.0 == pid).all()
        hits["pident_milli"] = pm
    return BoundaryTable(tax, hits, kind, level, cutoff, taxon, custom, grid)
