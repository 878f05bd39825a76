"""The shared-level lookups at their table edges, on the host (tests/shared_level_edges.py).

Three things are pinned before any GPU is involved: the library's host tables (`blu_taxonomy_shared_levels`: the adjacent-row
scan, and the wide-node chains or the range-minimum tables) agree with the plain restatement on every table for every `lo` and
23 span widths, and take the chains exactly where the classifier says so; the case list reaches every path class of the
stream kernel and every shape of `shared_levels()` at least eight times; and the columnar oracle's record of every case is what
the restatement says (bean index, root disagreement, agreement)."""
import collections
import ctypes as C

import numpy as np
import pytest

from blutils_amd import _native as N
from blutils_amd import engine
from tests import helpers as H
from tests import shared_level_edges as E

MIN_CASES = 8


def _taxonomy(t, device=-1):
    x = t.tax
    return engine.Taxonomy(x.lin_off, x.lin_node, x.lin_rank, x.rank_names, taxon="custom", custom=E.ZERO_CUTS, device=device)


def _host_answers(handle, pairs):
    L = N.lib()
    scan, tab, via = C.c_uint32(), C.c_uint32(), C.c_int32()
    for lo, hi in pairs:
        assert L.blu_taxonomy_shared_levels(handle, int(lo), int(hi), C.byref(scan), C.byref(tab), C.byref(via)) == N.BLU_OK
        yield lo, hi, scan.value, tab.value, via.value


def _check_pairs(t, handle, pairs):
    n_chain = 0
    for lo, hi, scan, tab, via in _host_answers(handle, pairs):
        s = t.shared(lo, hi)
        path = t.path_of(lo, lo, hi)
        assert scan == tab == s, (t.name, lo, hi, scan, tab, s, path)
        assert (via == 1) == (path in E.CHAIN_LOOKUPS), (t.name, lo, hi, via, path)
        n_chain += via
    return n_chain


def test_the_instances_are_what_the_issue_asks_for():
    ls = {a[0] for a in E.CHAINS}
    assert {12, 13, 16, 17, 32, 33} <= ls
    assert any(a[1] >= 64 for a in E.CHAINS) and any(18 <= a[1] <= 22 for a in E.CHAINS) and any(a[1] <= 9 for a in E.CHAINS)
    assert {a[2] for a in E.CHAINS} == {20, 21, 64}
    assert any(a[3] for a in E.CHAINS) and any(a[4] for a in E.CHAINS)
    ns = {E.table(("chain",) + a).n % 64 for a in E.CHAINS}
    assert {0, 1, 63} <= ns, ns
    for inst in E.SMALL:
        assert E.table(inst).n <= 2000, inst
    assert not E.table(("chain", 33, 5, 64, False, 130)).wide_tables
    for level, size in E.RUNS:
        t = E.table(("runs", level, size))
        sib = np.nonzero(t.lcp == level)[0] + 1                  # the rows at which a sibling (or the trunk's rest) starts,
        sib = sib[sib > 5]                                       # behind the five rows in front and the first sibling's start
        assert list(sib[:3]) == [5 + size, 5 + 2 * size, 5 + 3 * size], (level, size, sib)


@pytest.mark.parametrize("inst", E.SMALL, ids=E.instance_id)
def test_host_tables_against_the_restatement_exhaustively(inst):
    t = E.table(inst)
    tx = _taxonomy(t)
    inv = tx.row_map()[1]
    assert (inv == np.arange(t.n)).all()                         # the table is emitted in sorted order
    pairs = ((lo, lo + w) for lo in range(t.n) for w in E.WIDTHS if lo + w < t.n)
    n_chain = _check_pairs(t, tx.handle, pairs)
    assert (n_chain > 0) == (t.wide_tables and t.n > E.WIDE_MIN)
    tx.close()


@pytest.mark.parametrize("n_wide", E.LIMITS)
def test_host_tables_at_the_wide_node_limit(n_wide):
    """65 534 wide nodes are the most the 16-bit block entries name; with 65 535 the library builds no wide tables."""
    t = E.table(("limit", n_wide))
    assert t.n_wide == n_wide and t.wide_levels == 32 and t.wide_tables == (n_wide == 65534)
    tx = _taxonomy(t)
    rng = np.random.default_rng(n_wide)
    lo = rng.integers(0, t.n, 19000)
    hi = np.minimum(lo + rng.choice(np.array(E.WIDTHS), len(lo)), t.n - 1)
    last = t.n - 200                                             # the last node: reached through the highest chain id
    lo2 = rng.integers(last, t.n, 1000)
    hi2 = np.minimum(lo2 + rng.choice(np.array([0, 1, 127, 128, 129, 150, 199]), len(lo2)), t.n - 1)
    pairs = list(zip(np.concatenate([lo, lo2]).tolist(), np.concatenate([hi, hi2]).tolist()))
    assert len(pairs) == 20000 and sum(1 for a, b in pairs if a >= last and b - a >= 128) >= 50
    n_chain = _check_pairs(t, tx.handle, pairs)
    assert (n_chain > 0) == (n_wide == 65534), n_chain
    tx.close()


def test_every_path_and_shape_class_holds_eight_cases(capsys):
    """Counted under both strategies (the reference row, and with it the path, is the rule's where lineage lengths differ)."""
    for strategy in ("cautious", "relaxed"):
        paths, shapes, slots = collections.Counter(), collections.Counter(), collections.Counter()
        for inst in E.INSTANCES:
            t, cs = E.table(inst), E.cases(inst)
            assert len(cs) > 0, inst
            _, meta = E.build_hits(t, cs, strategy, np.arange(t.n), forms=(0,))
            for q, c in enumerate(cs):
                path = t.path_of(c.lo, int(meta["ref_pos"][q]), c.hi, int(meta["minlen"][q]))
                paths[path] += 1
                if path in E.CHAIN_LOOKUPS:
                    slots[t.block_slot(c.lo)] += 1
                if c.lo < c.hi:
                    shapes.update(t.shapes_of(c.lo, c.hi))
        with capsys.disabled():
            print(f"\nshared-level cases, {strategy}: " + ", ".join(f"{k}: {paths[k]}" for k in E.PATHS))
            print("shared_levels() shapes: " + ", ".join(f"{k}: {shapes[k]}" for k in E.SHAPES))
            print("block entry slots of the chain lookups (changes before lo, lo on a change): " + ", ".join(f"{k}: {slots[k]}" for k in sorted(slots)))
        for k in E.PATHS:
            assert paths[k] >= MIN_CASES, (strategy, k, paths[k])
        for k in ((0, False), (1, False), (1, True), (2, False), (2, True)):   # both compares of the entry reader, on and beside their edge
            assert slots[k] >= MIN_CASES, (strategy, k, slots[k])
        for k in E.SHAPES:
            assert shapes[k] >= MIN_CASES, (strategy, k, shapes[k])
        assert set(paths) == set(E.PATHS) and set(shapes) == set(E.SHAPES)


def test_each_builder_reaches_the_classes_it_is_there_for():
    def classes(inst):
        t, cs = E.table(inst), E.cases(inst)
        _, meta = E.build_hits(t, cs, "cautious", np.arange(t.n), forms=(0,))
        return {t.path_of(c.lo, int(meta["ref_pos"][q]), c.hi, int(meta["minlen"][q])) for q, c in enumerate(cs)}
    assert E.CHAIN_12 not in classes(("chain", 12, 70, 20, False, 62)) and E.CHAIN_0 in classes(("chain", 12, 70, 20, False, 62))
    assert E.CHAIN_12 in classes(("chain", 13, 20, 21, False, 17))
    assert E.CHAIN_12 in classes(("chain", 16, 64, 20, False, 63)) and E.CHAIN_16 not in classes(("chain", 16, 64, 20, False, 63))
    for inst in (("chain", 17, 70, 64, False, 32), ("chain", 32, 20, 64, True, 20), ("limit", 65534)):
        assert E.CHAIN_16 in classes(inst), inst
    assert E.OVERFLOW_RMQ in classes(("chain", 17, 9, 21, False, 150)) and E.OVERFLOW_RMQ in classes(("chain", 32, 3, 64, False, 200))
    assert E.OVERFLOW_RMQ not in classes(("chain", 17, 70, 64, False, 32))
    for inst in (("chain", 33, 5, 64, False, 130), ("limit", 65535)):
        assert E.NO_TABLES_RMQ in classes(inst) and not (classes(inst) & set(E.CHAIN_LOOKUPS)), inst
    assert E.NO_WIDE_NODE in classes(("chain", 17, 9, 21, False, 150)) and E.NO_WIDE_NODE in classes(("block_changes",))
    assert E.OVERFLOW_RMQ in classes(("block_changes",))
    for inst in (("chain", 32, 3, 64, False, 200), ("runs", 20, 128), ("runs", 21, 127)):
        assert E.ROW_BYTES_RMQ in classes(inst), inst
    # runs(): from some reference row, every pair of distances out of {0, 1, 126, 127, 128}
    for level, size in E.RUNS:
        have = {(c.ref - c.lo, c.hi - c.ref) for c in E.cases(("runs", level, size))}
        assert {(a, b) for a in E.EDGE_DISTANCES for b in E.EDGE_DISTANCES} <= have, (level, size)


@pytest.mark.parametrize("inst", E.INSTANCES, ids=E.instance_id)
def test_the_oracle_says_what_the_restatement_says(inst):
    t, cs = E.table(inst), E.cases(inst)
    forms = (0,) if inst[0] == "limit" else (0, 200)
    for strategy in ("cautious", "relaxed"):
        hits, meta = E.build_hits(t, cs, strategy, np.arange(t.n), forms=forms)
        rec = H.columnar(t.tax, hits, "custom", strategy, E.ZERO_CUTS)
        for q, (s, root, agree, bean) in enumerate(E.expected(t, cs, meta)):
            where = (t.name, strategy, cs[meta["case"][q]], int(meta["form"][q]), s)
            if root:
                assert rec["status"][q] == N.ST_ERR_ROOT, where
                assert rec["ref_row"][q] == meta["ref_row"][q], where
                continue
            assert rec["status"][q] == N.ST_MULTI and rec["ref_row"][q] == meta["ref_row"][q], where
            assert bool(rec["flags"][q] & N.FLAG_AGREE) == agree, where
            assert rec["bean_index"][q] == bean, where
            if not agree and bean < 8:   # the first bean_index + 1 levels that pass their cutoff; the backbone's cutoffs are all zero
                assert rec["level_mask"][q] == np.uint64((1 << (bean + 1)) - 1), where
