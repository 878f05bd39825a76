"""Edge cases of the report, sample-table and count-table kernels (csrc/report_kernel.hip: report_paths, sample_cells,
count_cells), with an expected value that shares none of the kernels' method.

Three independent pieces:

- `expected`: plain Python integers and dicts over (lineages, records, per-query rows of (sample, count)): `cells[(node tuple,
  sample)]`, `direct[node tuple]` for every path reached (zeros included), `unclassified[s]`, `unplaced[s]`, `total`.  No
  hashing, no numpy sums.
- restatements of what a case needs in order to aim: `fmix64` (mix_key), the two LDS hashes, the table sizes of the three
  entry points on the first attempt and on the retry, the constants.  The GPU module holds `table_slots` to them on every call.
- the case families (`global_chains`, `lds_chains`, `lane_mapping`, and the small builders of the refusals, shapes and the
  reserved node id).  A first-level key is (0xFFFFFFFF << 32) | node and node ids pass through the taxonomy unchanged, so a
  case picks node ids by search for a home slot; a lone first-level path sits in its home slot, so second-level keys
  (slot << 32) | node and cell keys (slot << 32) | sample are aimed the same way.  Only chains of keys with one common home
  plus isolated keys are used: their occupied span and longest probe do not depend on the insertion order.

A case names desc rows in `ref_row` and is run with `tax_row` = the engine row of every desc row followed by `extra_rows`.
tests/test_report_table_edges.py (no GPU) recomputes every claim made here; tests/test_gpu_report_table_edges.py runs the cases."""
import functools

import numpy as np

from blutils_amd import engine

U32_MAX = 0xFFFFFFFF
U64_MAX = (1 << 64) - 1
NONE = 0xFFFFFFFF                  # REPORT_NONE: the parent of a first-level path
CELL_UNCLASSIFIED, CELL_UNPLACED = 0xFFFFFFFE, 0xFFFFFFFD
UNMATCHED = 0xFFFFFFFF
ROW_BITS = 25
PROBE_FIRST = 128                  # REPORT_PROBE_FIRST
LDS_PROBE = 8
LDS_SLOTS = 2048                   # LDS_SLOTS and CELL_LDS_SLOTS
MIN_SLOTS = 1024
COUNT_Q = 32                       # consecutive queries of one wave of count_cells
COUNT_BLOCK = 128                  # ... of one block
WALK_BLOCK = 1024                  # consecutive queries of one block of report_paths / sample_cells
ENTRIES = ("report", "sample", "count")


# ---- restatements: hashes ---------------------------------------------------------------------------------------------------------

def fmix64(k):
    """murmur3's finaliser on a Python integer (mix_key keeps the low 32 bits of it)"""
    k ^= k >> 33
    k = k * 0xff51afd7ed558ccd & U64_MAX
    k ^= k >> 33
    k = k * 0xc4ceb9fe1a85ec53 & U64_MAX
    k ^= k >> 33
    return k


def home(key, slots):
    """home slot of a key in a global table of `slots` slots"""
    return fmix64(key) & U32_MAX & (slots - 1)


def lds_path_home(path):
    """home of a leaf path id in the block's table of report_paths"""
    return (path * 2654435761 & U32_MAX) >> 21


def lds_cell_home(key):
    """home of a cell key in the block's table of sample_cells / count_cells"""
    return (key * 0x9E3779B97F4A7C15 & U64_MAX) >> 53


def _fmix64_np(k):
    k = k.copy()
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xff51afd7ed558ccd)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xc4ceb9fe1a85ec53)
    k ^= k >> np.uint64(33)
    return k


def _home_np(keys, slots):
    return (_fmix64_np(keys) & np.uint64(U32_MAX) & np.uint64(slots - 1)).astype(np.int64)


def _lds_cell_home_np(keys):
    return ((keys * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(53)).astype(np.int64)


def search(hi, fn, accept, n, start=1, limit=1 << 24, distinct=False):
    """the first n low words v >= start for which fn(keys (hi << 32) | v) -> a home that `accept` (a set, or one home) holds;
    distinct: every home once.  -> (values, homes); fewer than n when `limit` values hold no more."""
    accept = {accept} if isinstance(accept, int) else set(accept)
    ok = np.zeros(LDS_SLOTS if max(accept) < LDS_SLOTS else max(accept) + 1, bool)
    ok[list(accept)] = True
    out, homes, seen = [], [], set()
    step = 1 << 16
    for lo in range(start, limit, step):
        v = np.arange(lo, min(lo + step, limit, U32_MAX), dtype=np.uint64)
        h = fn((np.uint64(hi) << np.uint64(32)) | v)
        for i in np.nonzero(ok[np.minimum(h, len(ok) - 1)] & (h < len(ok)))[0].tolist():
            if distinct and int(h[i]) in seen:
                continue
            seen.add(int(h[i]))
            out.append(int(v[i]))
            homes.append(int(h[i]))
            if len(out) == n:
                return out, homes
    return out, homes


def isolated(hi, slots, taken, n, start=1):
    """n low words whose keys (hi << 32) | v have homes outside `taken` and apart from each other; `taken` grows by them"""
    out = []
    v = start
    while len(out) < n:
        h = home((hi << 32) | v, slots)
        if h not in taken:
            taken.add(h)
            out.append(v)
        v += 1
    return out


# ---- restatements: table sizes ----------------------------------------------------------------------------------------------------

def next_pow2(x):
    c = 1
    while c < x:
        c <<= 1
    return c


def _slots(x):
    return max(next_pow2(2 * x), MIN_SLOTS)


def path_guess(nq, depth, n_tax):
    return min(nq * max(depth, 1), 2 * n_tax + 4096)


def bounds(recs, row_len=None):
    """(P, B): the sum of popcount(level_mask) over the records with a taxon, and the same times the length of each one's row"""
    P = B = 0
    for q in range(len(recs)):
        if int(recs["status"][q]) < 2:
            pc = bin(int(recs["level_mask"][q])).count("1")
            P += pc
            if row_len is not None:
                B += pc * int(row_len[q])
    return P, B


def first_sizes(entry, nq, depth, n_tax, n_samples=1, cell_bound=0):
    """(cap, ccap) of the first attempt (ccap None for the report)"""
    guess = path_guess(nq, depth, n_tax)
    cap = _slots(guess)
    if entry == "report":
        return cap, None
    if entry == "sample":
        return cap, _slots(min(nq * max(depth, 1), guess + nq))
    return cap, _slots(min(cell_bound, guess * max(n_samples, 1)))


def retry_sizes(entry, P, B=0):
    if entry == "report":
        return _slots(P), None
    if entry == "sample":
        return _slots(P), _slots(P)
    return _slots(P), _slots(B)


# ---- the expected value -----------------------------------------------------------------------------------------------------------

def selected(lineage, mask):
    """the node tuple a record's mask selects from its lineage"""
    return tuple(int(node) for j, node in enumerate(lineage) if (mask >> j) & 1)


def expected(lineages, recs, desc, rows, n_samples):
    """rows[q]: the (sample, count) pairs of query q.  -> {"cells", "direct", "unclassified", "unplaced", "total"}"""
    cells, direct = {}, {}
    unc, unp = [0] * n_samples, [0] * n_samples
    for q in range(len(recs)):
        if int(recs["status"][q]) >= 2:
            for s, w in rows[q]:
                unc[s] += w
            continue
        p = selected(lineages[int(desc[q])], int(recs["level_mask"][q]))
        if not p:
            for s, w in rows[q]:
                unp[s] += w
            continue
        prefixes = [p[:k] for k in range(1, len(p) + 1)]
        for x in prefixes:
            direct.setdefault(x, 0)
        for s, w in rows[q]:
            if w:
                for x in prefixes:
                    cells[(x, s)] = cells.get((x, s), 0) + w
                direct[p] += w
    return {"cells": cells, "direct": direct, "unclassified": unc, "unplaced": unp,
            "total": sum(unc) + sum(unp) + sum(direct.values())}


def decode_paths(paths):
    """the `paths` array of a result -> node tuple of every entry (parents come first, every path once)"""
    full = []
    for i in range(len(paths)):
        par = int(paths["parent"][i])
        assert par == NONE or par < i, f"path {i}: parent {par} does not come first"
        full.append((full[par] if par != NONE else ()) + (int(paths["node"][i]),))
    assert len(set(full)) == len(full), "a path is listed twice"
    return full


def decode(result, entry):
    """a result dict of blutils_amd.report -> the shape `expected` returns (a report: one sample, no cells)"""
    full = decode_paths(result["paths"])
    out = {"direct": {p: int(v) for p, v in zip(full, result["paths"]["direct"].tolist())},
           "clade": {p: int(v) for p, v in zip(full, result["paths"]["clade"].tolist())}}
    if entry == "report":
        out.update(unclassified=[int(result["unclassified"])], unplaced=[int(result["unplaced"])], total=int(result["total"]))
        return out
    C = result["cells"]
    keys = list(zip(C["path"].tolist(), C["sample"].tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys), "cells not sorted by (path, sample), or one twice"
    out["cells"] = {(full[p], s): int(v) for (p, s), v in zip(keys, C["clade"].tolist())}
    out["unclassified"] = [int(x) for x in result["unclassified"].tolist()]
    out["unplaced"] = [int(x) for x in result["unplaced"].tolist()]
    return out


def first_difference(got, want):
    """the smallest key on which two dicts differ, with both values; None when they are equal"""
    for k in sorted(set(got) | set(want)):
        if got.get(k) != want.get(k):
            return k, got.get(k), want.get(k)
    return None


def compare(got, want, entry):
    """None, or a sentence on the first thing in which a decoded result differs from the expected value"""
    if entry == "report":
        clade = {}
        for (p, _), v in want["cells"].items():
            clade[p] = clade.get(p, 0) + v
        for name, g, w in (("direct", got["direct"], want["direct"]), ("clade", got["clade"], {p: clade.get(p, 0) for p in want["direct"]})):
            d = first_difference(g, w)
            if d:
                return f"{name} of path {d[0]}: {d[1]} for {d[2]}"
        for k in ("unclassified", "unplaced"):
            if got[k][0] != sum(want[k]):
                return f"{k}: {got[k][0]} for {sum(want[k])}"
        return None if got["total"] == want["total"] else f"total: {got['total']} for {want['total']}"
    d = first_difference(got["cells"], want["cells"])
    if d:
        return f"cell (path {d[0][0]}, sample {d[0][1]}): {d[1]} for {d[2]}"
    d = first_difference(got["direct"], want["direct"])
    if d:
        return f"direct of path {d[0]}: {d[1]} for {d[2]}"
    clade = {p: 0 for p in want["direct"]}
    for (p, _), v in want["cells"].items():
        clade[p] += v
    d = first_difference(got["clade"], clade)
    if d:
        return f"clade of path {d[0]}: {d[1]} for {d[2]}"
    for k in ("unclassified", "unplaced"):
        if got[k] != want[k]:
            s = next(i for i in range(max(len(got[k]), len(want[k]))) if got[k][i:i + 1] != want[k][i:i + 1])
            return f"{k} of sample {s}: {got[k][s:s + 1]} for {want[k][s:s + 1]}"
    return None


# ---- a case -----------------------------------------------------------------------------------------------------------------------

def records(n):
    recs = np.zeros(n, engine.RESULT_DTYPE)
    recs["ref_row"] = U32_MAX
    return recs


class Case:
    """family / name; lineages (desc rows); recs with ref_row = desc row (or an index into extra_rows behind them); weights
    (uint32 per query, None = 1) and sample_of for the first two entry points; csr = (row_ptr, sample, count) for the third, None:
    one non-zero per query, (sample_of, weight); attempts[entry]: what an aimed case claims, None elsewhere; claims: what the
    builder aimed at, for tests/test_report_table_edges.py."""

    def __init__(self, family, name, lineages, recs, sample_of=None, n_samples=1, weights=None, csr=None, attempts=None,
                 entries=ENTRIES, extra_rows=(), claims=None):
        self.family, self.name, self.lineages, self.recs = family, name, lineages, recs
        nq = len(recs)
        self.sample_of = np.zeros(nq, np.uint32) if sample_of is None else np.asarray(sample_of, np.uint32)
        self.n_samples, self.weights, self.csr = n_samples, None if weights is None else np.asarray(weights, np.uint32), csr
        self.attempts = attempts or {}
        self.entries, self.extra_rows, self.claims = entries, list(extra_rows), claims or {}
        self.desc = recs["ref_row"].astype(np.int64)

    @property
    def depth(self):
        return max((len(l) for l in self.lineages), default=0)

    def weight(self, q):
        return 1 if self.weights is None else int(self.weights[q])

    def count_rows(self):
        """the CSR arrays of the third entry point"""
        if self.csr is not None:
            return self.csr
        nq = len(self.recs)
        w = np.ones(nq, np.uint32) if self.weights is None else self.weights
        return np.arange(nq + 1, dtype=np.uint64), self.sample_of.copy(), w.copy()

    def rows(self, entry):
        nq = len(self.recs)
        if entry == "report":
            return [[(0, self.weight(q))] for q in range(nq)]
        if entry == "sample":
            return [[(int(self.sample_of[q]), self.weight(q))] for q in range(nq)]
        ptr, s, c = self.count_rows()
        s, c = s.tolist(), c.tolist()
        return [list(zip(s[int(ptr[q]):int(ptr[q + 1])], c[int(ptr[q]):int(ptr[q + 1])])) for q in range(nq)]

    @functools.lru_cache(None)
    def expected(self, entry):
        return expected(self.lineages, self.recs, self.desc, self.rows(entry), 1 if entry == "report" else self.n_samples)

    def sizes(self, entry, attempts):
        """(cap, ccap) the host code computes for the attempt that succeeded"""
        row_len = None
        if entry == "count":
            row_len = np.diff(self.count_rows()[0].astype(np.int64))
        P, B = bounds(self.recs, row_len)
        if attempts == 1:
            return first_sizes(entry, len(self.recs), self.depth, len(self.lineages), self.n_samples, B)
        return retry_sizes(entry, P, B)

    def table_slots(self, entry, attempts):
        cap, ccap = self.sizes(entry, attempts)
        return cap if entry == "report" else ccap

    def where(self, entry, route):
        return f"family {self.family} case {self.name} entry {entry} route {route}"


def _weights(nq, seed):
    return ((np.arange(nq, dtype=np.uint64) * np.uint64(7919) + np.uint64(seed)) % np.uint64(1000) + np.uint64(1)).astype(np.uint32)


def _span(h, n, slots):
    return {(h + i) % slots for i in range(n)}


def _first_level(node):
    return (NONE << 32) | node


# ---- family 1: chains in the global tables ----------------------------------------------------------------------------------------

CHAIN_LENGTHS = (2, 127, 128, 129)
ACROSS_LENGTHS = (2, 126, 127, 128)          # one more slot of the span is the parent's: the longest probe is n + 1
CHAIN_KINDS = ("first", "first_at_cap-1", "first_at_cap-2", "second", "second_across_parent", "cells", "cells_at_ccap-1")


def _tail(lineages, desc, status, mask, others):
    """queries every chain case ends with: the isolated paths, five without a taxon, five with a taxon and no level"""
    for r in others:
        desc.append(r); status.append(0); mask.append(1)
    for st in (2, 3, 16, 17, 2):
        desc.append(-1); status.append(st); mask.append(0b11)
    for k in range(5):
        desc.append(others[k % len(others)]); status.append(k % 2); mask.append(0 if k < 4 else 1 << 7)   # (bit 7: beyond every lineage)


def _case_of(family, name, lineages, desc, status, mask, sample_of, n_samples, attempts, claims, seed):
    nq = len(desc)
    recs = records(nq)
    recs["status"] = status
    recs["level_mask"] = np.array(mask, np.uint64)
    recs["ref_row"] = np.where(np.array(desc) < 0, U32_MAX, np.array(desc)).astype(np.uint32)
    return Case(family, name, lineages, recs, sample_of, n_samples, _weights(nq, seed), attempts=attempts, claims=claims)


@functools.lru_cache(None)
def global_chain(kind, n):
    """One case of 1 024 / 1 024 slots on every entry point.  The chain's keys share one home and nothing else has its home in
    the slots they take, so they take `span` whatever the order and the longest probe is `probe`: at most 128 is one attempt, 129
    starts again from the bound."""
    S = MIN_SLOTS
    lineages, desc, status, mask = [], [], [], []
    claims = {"kind": kind, "slots": S}
    if kind.startswith("first"):
        target = {"first": 500, "first_at_cap-1": S - 1, "first_at_cap-2": S - 2}[kind]
        chain, _ = search(NONE, lambda k: _home_np(k, S), target, n)
        span = _span(target, n, S)
        taken = set(span)
        others = isolated(NONE, S, taken, 6, start=max(chain) + 1)
        lineages = [[v] for v in chain] + [[v] for v in others]
        for i in range(n):
            for _ in range(2):
                desc.append(i); status.append(0); mask.append(1)
        _tail(lineages, desc, status, mask, list(range(n, n + 6)))
        nq = len(desc)
        sample_of = np.arange(nq) % 3
        probe = n
        claims.update(table="path", home=target, span=span, probe=probe, chain_keys=[_first_level(v) for v in chain],
                      other_keys=[_first_level(v) for v in others])
        attempts = dict.fromkeys(ENTRIES, 2 if probe > PROBE_FIRST else 1)
        return _case_of(1, f"{kind}_{n}", lineages, desc, status, mask, sample_of, 3, attempts, claims, n)
    if kind.startswith("second"):
        taken = set()
        parent = isolated(NONE, S, taken, 1, start=7)[0]
        a = home(_first_level(parent), S)
        target = (a - 1) % S if kind == "second_across_parent" else (a + 300) % S
        chain, _ = search(a, lambda k: _home_np(k, S), target, n)
        probe = n + 1 if kind == "second_across_parent" else n
        span = _span(target, probe, S)
        assert (a in span) == (kind == "second_across_parent")
        taken |= span
        others = isolated(NONE, S, taken, 6, start=1000)
        lineages = [[parent, v] for v in chain] + [[v] for v in others]
        for i in range(n):
            desc.append(i); status.append(0); mask.append(0b11)
        for i in (0, n - 1):
            desc.append(i); status.append(1); mask.append(0b01)
        _tail(lineages, desc, status, mask, list(range(n, n + 6)))
        nq = len(desc)
        claims.update(table="path", home=target, span=span, probe=probe, parent_slot=a, chain_keys=[(a << 32) | v for v in chain],
                      other_keys=[_first_level(v) for v in others] + [_first_level(parent)])
        attempts = dict.fromkeys(ENTRIES, 2 if probe > PROBE_FIRST else 1)
        return _case_of(1, f"{kind}_{n}", lineages, desc, status, mask, np.arange(nq) % 3, 3, attempts, claims, n)
    # cells of one lone path: the path table holds seven isolated keys, the cell table the chain
    ptaken = set()
    nodes = isolated(NONE, S, ptaken, 7, start=11)
    slots = [home(_first_level(v), S) for v in nodes]
    target = S - 1 if kind == "cells_at_ccap-1" else 640
    chain, _ = search(slots[0], lambda k: _home_np(k, S), target, n)
    span = _span(target, n, S)
    ctaken = set(span)
    lineages = [[v] for v in nodes]
    sample_of = []
    for s in chain:
        desc.append(0); status.append(0); mask.append(1); sample_of.append(s)
    other_cells = []
    for r in range(1, 7):
        s = isolated(slots[r], S, ctaken, 1, start=r)[0]
        other_cells.append((slots[r] << 32) | s)
        desc.append(r); status.append(r % 2); mask.append(1); sample_of.append(s)
    for k, st in enumerate((2, 3, 16, 17, 2)):
        desc.append(-1); status.append(st); mask.append(1); sample_of.append(chain[k % n])
    for k in range(5):
        desc.append(k % 7); status.append(k % 2); mask.append(0 if k < 4 else 1 << 7); sample_of.append(chain[-1 - k % n])
    claims.update(table="cell", home=target, span=span, probe=n, chain_keys=[(slots[0] << 32) | s for s in chain],
                  other_keys=other_cells, path_keys=[_first_level(v) for v in nodes])
    attempts = {"report": 1, "sample": 2 if n > PROBE_FIRST else 1, "count": 2 if n > PROBE_FIRST else 1}
    return _case_of(1, f"{kind}_{n}", lineages, desc, status, mask, sample_of, max(sample_of) + 1, attempts, claims, n)


def global_chains(kind):
    return [global_chain(kind, n) for n in (ACROSS_LENGTHS if kind == "second_across_parent" else CHAIN_LENGTHS)]


# ---- family 2: chains in the blocks' LDS tables -----------------------------------------------------------------------------------

LDS_PATH_CASES = ((8, 1000), (9, 1000), (40, 1000), (9, 2047), (40, 2046))
LDS_PATH_TAX, LDS_PATH_QUERIES, LDS_PATH_SLOTS = 14400, 32900, 131072
LDS_CELL_CASES = tuple((n, t, hi) for hi in ("path", "unclassified", "unplaced") for n, t in ((8, 77), (9, 77), (40, 77), (9, 2047), (40, 2046)))


@functools.lru_cache(None)
def lds_path_chain(n, target):
    """report_paths: n leaf paths whose ids (their home slots in a path table of 131 072 slots, the smallest that has 40 slots
    under one LDS home) share the LDS home `target`, all in the first block of 1 024 queries, every second query on the first of
    them.  14 400 one-level rows and 32 900 queries give that table; the queries behind the block have no taxon."""
    S = LDS_PATH_SLOTS
    assert first_sizes("report", LDS_PATH_QUERIES, 1, LDS_PATH_TAX)[0] == S
    wanted = [s for s in range(S) if lds_path_home(s) == target]
    chain, slots = search(NONE, lambda k: _home_np(k, S), wanted, n, distinct=True, limit=1 << 22)
    found = len(chain)
    lineages = [[v] for v in chain] + [[20_000_000 + i] for i in range(LDS_PATH_TAX - found)]
    nq = LDS_PATH_QUERIES
    recs = records(nq)
    recs["status"] = 2
    q = np.arange(WALK_BLOCK)
    recs["status"][:WALK_BLOCK] = q % 2
    recs["level_mask"][:WALK_BLOCK] = 1
    recs["ref_row"][:WALK_BLOCK] = np.where(q % 2 == 0, 0, 1 + (q // 2) % max(found - 1, 1))
    recs["status"][WALK_BLOCK + 5::11] = 1                              # with a taxon and no level: unplaced
    recs["ref_row"][WALK_BLOCK + 5::11] = 3
    recs["level_mask"][WALK_BLOCK + 5::11] = 0
    claims = {"found": found, "lds_home": target, "path_ids": slots, "chain_keys": [_first_level(v) for v in chain], "slots": S}
    return Case(2, f"lds_paths_{n}_at_{target}", lineages, recs, np.arange(nq) % 3, 3, _weights(nq, n), claims=claims)


@functools.lru_cache(None)
def lds_cell_chain(n, target, hi):
    """sample_cells / count_cells: n cell keys of one path (or of the unclassified / the unplaced row) with the LDS home
    `target`, in one block of either kernel (2 n queries <= 128), every second query on the first of them."""
    S = MIN_SLOTS
    taken = set()
    nodes = isolated(NONE, S, taken, 3, start=21)
    slot = home(_first_level(nodes[0]), S)
    word = {"path": slot, "unclassified": CELL_UNCLASSIFIED, "unplaced": CELL_UNPLACED}[hi]
    chain, _ = search(word, _lds_cell_home_np, target, n, limit=1 << 22)
    found = len(chain)
    lineages = [[v] for v in nodes]
    nq = 2 * found + 6
    recs = records(nq)
    sample_of = np.zeros(nq, np.uint32)
    for q in range(2 * found):
        sample_of[q] = chain[0] if q % 2 == 0 else chain[(q // 2) % found]
    if hi == "path":
        recs["ref_row"][:2 * found] = 0
        recs["level_mask"][:2 * found] = 1
    elif hi == "unclassified":
        recs["status"][:2 * found] = 2 + np.arange(2 * found) % 3
    else:
        recs["ref_row"][:2 * found] = np.arange(2 * found) % 3
        recs["status"][:2 * found] = np.arange(2 * found) % 2
        recs["level_mask"][:2 * found] = 0
    recs["ref_row"][2 * found:] = np.arange(6) % 3                      # classified queries beside them
    recs["level_mask"][2 * found:] = 1
    sample_of[2 * found:] = [chain[k % found] for k in range(6)]
    claims = {"found": found, "lds_home": target, "chain_keys": [(word << 32) | s for s in chain], "slots": S}
    return Case(2, f"lds_cells_{hi}_{n}_at_{target}", lineages, recs, sample_of, max(chain) + 1, _weights(nq, n), claims=claims)


@functools.lru_cache(None)
def long_fixed_rows():
    """count_cells: a row without a taxon and a row with a taxon and no level of 5 000 distinct samples each (more than the
    2 048 LDS slots of their block), beside classified rows of three non-zeros; the last block is partial."""
    lineages = [[7, 20 + i // 4, 5000 + i] for i in range(16)]
    nq, ns = COUNT_BLOCK + 37, 5003
    recs = records(nq)
    recs["ref_row"] = np.arange(nq) % 16
    recs["level_mask"] = 0b111
    recs["status"] = np.arange(nq) % 2
    recs["status"][3], recs["ref_row"][3] = 2, U32_MAX
    recs["level_mask"][70] = 0
    lengths = np.full(nq, 3)
    lengths[[3, 70]] = 5000
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    rng = np.random.default_rng(5)
    sample = rng.integers(0, ns, int(row_ptr[-1])).astype(np.uint32)
    for q in (3, 70):
        sample[int(row_ptr[q]):int(row_ptr[q + 1])] = rng.permutation(ns)[:5000]
    count = rng.integers(1, 1 << 20, len(sample)).astype(np.uint32)
    return Case(2, "long_fixed_rows", lineages, recs, None, ns, None, csr=(row_ptr, sample, count), entries=("count",))


@functools.lru_cache(None)
def crowded_block():
    """sample_cells: one block of 1 024 queries in which 700 queries have three levels of their own under one root (2 101
    cells, more than the 2 048 LDS slots) and the other 324, without a taxon or without a level, a sample each of their own."""
    n = 700
    lineages = [[7, 1000 + i, 50_000 + i, 90_000 + i] for i in range(n)]
    nq = WALK_BLOCK
    recs = records(nq)
    kind = np.arange(nq) * 324 // nq != (np.arange(nq) + 1) * 324 // nq      # 324 of the 1 024, spread evenly
    assert kind.sum() == 324
    recs["level_mask"] = 0b1111
    recs["ref_row"][~kind] = np.arange(n)
    fixed = np.nonzero(kind)[0]
    recs["status"][fixed[::2]] = 2
    recs["ref_row"][fixed[1::2]] = np.arange(len(fixed[1::2])) % n
    recs["level_mask"][fixed[1::2]] = 0
    sample_of = np.zeros(nq, np.uint32)
    sample_of[fixed] = 1 + np.arange(324)
    return Case(2, "crowded_block", lineages, recs, sample_of, 325, _weights(nq, 3))


# ---- family 3: the lane mapping of count_cells ------------------------------------------------------------------------------------

ROW_KINDS = ("0", "1", "per-1", "per", "per+1", "2per", "2per+1", "3x64+1")
MASK_KINDS = ("low", "high", "short")
PRIMES = [p for p in range(2, 1500) if all(p % d for d in range(2, int(p ** 0.5) + 1))]


def row_length(kind, L):
    per = 64 // L
    return {"0": 0, "1": 1, "per-1": per - 1, "per": per, "per+1": per + 1, "2per": 2 * per, "2per+1": 2 * per + 1, "3x64+1": 193}[kind]


def distinct_counts(n, zero_every=5):
    """n counts: the powers of two below 2^32, then primes that are none; every `zero_every`-th entry of a row of three or
    more is 0 instead"""
    vals = [1 << i for i in range(32)] + [p for p in PRIMES if p & (p - 1)]
    return [0 if n >= 3 and i % zero_every == 2 else vals[i] for i in range(n)]


@functools.lru_cache(None)
def lane_mapping():
    """549 queries: every L = 1 ... 64 levels against every row kind (512), placed so that each of the 32 places of a wave's run
    holds each row kind, then 37 more (bit 63 alone, queries without a taxon or a level with long rows, and seeded repeats) that
    leave the fifth block partial.  Rows 0 ... 2 have 64 levels, row 2 + L has the first L of another."""
    deep = [[1000 * (i + 1) + j for j in range(64)] for i in range(3)]
    lineages = deep + [[9000 + j for j in range(L)] for L in range(1, 65)]
    plan = []                                                            # (L, row kind, mask kind) per query
    seen = [0] * len(ROW_KINDS)
    for q in range(512):
        k = (q % COUNT_Q + q // COUNT_Q) % len(ROW_KINDS)
        seen[k] += 1
        L = seen[k]
        plan.append((L, ROW_KINDS[k], MASK_KINDS[(L + k) % 3]))
    rng = np.random.default_rng(9)
    plan.append((1, "3x64+1", "bit63"))
    plan += [(1, "3x64+1", "no_taxon"), (1, "2per+1", "no_level"), (1, "per+1", "no_taxon"), (1, "3x64+1", "no_level")]
    while len(plan) < 549:
        plan.append((int(rng.integers(1, 65)), ROW_KINDS[int(rng.integers(2, 8))], MASK_KINDS[int(rng.integers(0, 3))]))
    nq, ns = len(plan), 256
    recs = records(nq)
    row_ptr, sample, count = [0], [], []
    for q, (L, rk, mk) in enumerate(plan):
        recs["status"][q] = q % 2
        if mk == "low":
            recs["ref_row"][q], recs["level_mask"][q] = q % 3, (1 << L) - 1
        elif mk == "high":
            recs["ref_row"][q], recs["level_mask"][q] = q % 3, ((1 << L) - 1) << (64 - L)
        elif mk == "short":
            recs["ref_row"][q], recs["level_mask"][q] = 2 + L, U64_MAX
        elif mk == "bit63":
            recs["ref_row"][q], recs["level_mask"][q] = 1, 1 << 63
        elif mk == "no_taxon":
            recs["status"][q] = 2 + q % 3
        else:
            recs["ref_row"][q], recs["level_mask"][q] = 2 + 5, 0b11 << 5    # (bits beyond the five levels of that row)
        n = row_length(rk, L)
        sample += [(7 * q + i) % ns for i in range(n)]
        count += distinct_counts(n)
        row_ptr.append(row_ptr[-1] + n)
    csr = (np.array(row_ptr, np.uint64), np.array(sample, np.uint32), np.array(count, np.uint32))
    return Case(3, "lane_mapping", lineages, recs, None, ns, None, csr=csr, entries=("count",), claims={"plan": plan})


# ---- families 4 to 6: small cases built by hand -----------------------------------------------------------------------------------

def small(family, name, lineages, desc, status, mask, sample_of=None, n_samples=1, weights=None, csr=None, entries=ENTRIES,
          extra_rows=()):
    """a case from per-query lists; desc -1: no reference row"""
    nq = len(desc)
    recs = records(nq)
    if nq:
        recs["status"] = status
        recs["level_mask"] = np.array(mask, np.uint64)
        recs["ref_row"] = np.where(np.array(desc) < 0, U32_MAX, np.array(desc)).astype(np.uint32)
    return Case(family, name, lineages, recs, sample_of, n_samples, weights, csr=csr, entries=entries, extra_rows=extra_rows)


REFUSAL_QUERIES = 200
REFUSAL_LINEAGES = [[1, 2, 3], [1, 2, 4]]
BAD_RECORDS = ("unmatched_row", "row_out_of_range", "ref_row_past_n_rows")
BAD_PLACES = (0, 100, REFUSAL_QUERIES - 1, 95)                               # first, middle, last, the last of a wave's run


def refusal_case(how=None, bad=None, status=0):
    """200 good queries over two lineages; query `bad` names, by `how`, no taxonomy row.  extra_rows: an unmatched hit and an
    engine row id whose position (2 + 5) no table of two rows has."""
    nq = REFUSAL_QUERIES
    desc = [q % 2 for q in range(nq)]
    st = [0 if q % 5 else 2 for q in range(nq)]
    desc = [-1 if s == 2 else d for d, s in zip(desc, st)]
    if how is not None:
        desc[bad] = {"unmatched_row": 2, "row_out_of_range": 3, "ref_row_past_n_rows": 4 + 5}[how]
        st[bad] = status
    c = small(4, f"{how}_at_{bad}_status_{status}", REFUSAL_LINEAGES, desc, st, [0b111] * nq, [q % 4 for q in range(nq)], 4,
              extra_rows=(UNMATCHED, 7 | 3 << ROW_BITS))
    if how is not None and status >= 2:
        c.desc[bad] = -1
    return c
