"""The per-wave top-row list of the ring stream kernel at its capacity edges, against the columnar oracle.

A wave task (64 consecutive queries, 50 hits each, segments back to back: a ring task) collects its top rows in an LDS
list of LIST_CAP* entries (consensus_kernel.hip).  The tables here are made of 64-query blocks whose top-row TOTALS sit
one below, at and one above each build's old and new capacity, and at twice the new one, with the heavy queries (the ones
that fill the list) at the start, in the middle or at the end of the block.  The table holds one whole round of 64-query
tasks for every build of the kernel (16 waves per CU at most), so the blocks of that round are wave tasks as they stand;
what follows the last whole round is cut into smaller pieces and is checked all the same.

Milli-percent column layout only: top groups holding identities of 131 071 milli-percent and above (not BLAST output) with
a custom cutoff table whose values lie up there as well — those queries take the f64 level tests, which read their
cutoffs from global memory in the milli-percent builds (they keep no LDS cutoff table)."""
import numpy as np
import pytest

from blutils_amd import engine, synth
from tests import helpers as H

pytestmark = pytest.mark.gpu

HITS = 50
WAVE = 64
# list capacities per build, before and after the ring builds took the LDS of the cutoff table and of the duplicate row
# offsets: milli-percent layouts 208 -> 248, f64 layouts 232 -> 240 (the builds without the ring: 208 / 232 as before)
CAPS_OLD_NEW = ((208, 248), (232, 240))
TOTALS = tuple(sorted({c + d for old, new in CAPS_OLD_NEW for c in (old, new) for d in (-1, 0, 1)} | {2 * new for _, new in CAPS_OLD_NEW}))
POSITIONS = ("first", "middle", "last")
CASES = tuple((total, pos) for total in TOTALS for pos in POSITIONS)
LAYOUTS = ("packed", "milli", "f64", "packed64")
STRATEGIES = ("relaxed", "cautious")
# cutoffs above 131.071 %: identities up there are told apart by the f64 tests only
CUSTOM_HIGH = {"domain": 50, "kingdom": 60, "phylum": 120, "class": 132, "order": 135, "family": 140, "genus": 150, "species": 200}
HIGH_MILLI = np.array([131071, 131072, 131999, 132000, 132001, 135000, 139999, 140000, 150000, 150001, 199999, 200000, 250000],
                      dtype=np.int64)


def block_sizes(total: int, pos: str) -> np.ndarray:
    """Top-group sizes of the 64 queries of a block, `total` rows in all: one row each, half of the rest dealt out evenly,
    the other half given to as few queries as possible (up to all 50 hits tied: the heavy queries), from the start, around
    the middle or from the end of the block."""
    assert 2 * WAVE <= total <= WAVE * HITS // 2
    sizes = np.ones(WAVE, dtype=np.int64)
    even = (total - WAVE) // 2
    sizes += even // WAVE
    sizes[(np.arange(even % WAVE) * 5 + 3) % WAVE] += 1          # (5 and 64 are coprime: distinct queries)
    extra = total - int(sizes.sum())
    order = {"first": np.arange(WAVE), "last": np.arange(WAVE)[::-1],
             "middle": np.concatenate([np.arange(WAVE // 2 - 4, WAVE), np.arange(0, WAVE // 2 - 4)])}[pos]
    for q in order:
        add = min(extra, HITS - int(sizes[q]))
        sizes[q] += add
        extra -= add
        if extra == 0:
            break
    assert int(sizes.sum()) == total
    return sizes


def capacity_table(tax, n_queries: int, seed: int):
    """The generator's 50-hit table with the bit-scores rewritten: block b of 64 queries gets the top-group sizes of
    CASES[b % len(CASES)], each group a window of its segment at a position of its own (it may wrap around the end)."""
    assert n_queries % WAVE == 0
    h = synth.make_hits(tax, n_queries, seed, HITS, device="cpu", p_unmatched=0.001).numpy()
    rng = np.random.default_rng(seed)
    n_blocks = n_queries // WAVE
    per_case = np.stack([block_sizes(total, pos) for total, pos in CASES])          # [case, query of the block]
    gsz = per_case[np.arange(n_blocks) % len(CASES)].reshape(-1)                    # per query
    off = rng.integers(0, HITS, n_queries)
    top = 200 + rng.integers(0, 1801, n_queries)
    j = np.tile(np.arange(HITS), n_queries)
    is_top = ((j + np.repeat(off, HITS)) % HITS) < np.repeat(gsz, HITS)
    below = np.repeat(top, HITS) - 1 - rng.integers(0, 16, n_queries * HITS)
    h["bitscore"] = np.where(is_top, np.repeat(top, HITS), below).astype(np.int32)
    totals = is_top.reshape(n_blocks, WAVE * HITS).sum(axis=1)
    assert np.array_equal(totals, np.array([CASES[b % len(CASES)][0] for b in range(n_blocks)]))
    h["pident_milli"] = np.rint(h["pident"] * 1000.0).astype(np.int64).astype(np.uint32)
    assert np.array_equal(h["pident_milli"].astype(np.float64) / 1000.0, h["pident"])
    return h, is_top


def one_round_of_tasks() -> int:
    """Queries of one whole round of 64-query tasks of the widest build (16 waves per CU), plus every case once more."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return (cus * 16 + len(CASES)) * WAVE


def device_buffers(t, h, layout):
    import torch
    cols = {"seg_off": torch.from_numpy(h["seg_off"]).cuda(), "bitscore": torch.from_numpy(h["bitscore"]).cuda(),
            "tax_row": torch.from_numpy(t.engine_rows(h["tax_row"]).view(np.int32)).cuda(),
            "align_len": torch.from_numpy(h["align_len"]).cuda(), "acc_rank": torch.from_numpy(h["acc_rank"]).cuda()}
    if layout in ("f64", "packed64"):
        cols["pident"] = torch.from_numpy(h["pident"]).cuda()
    else:
        cols["pident_milli"] = torch.from_numpy(h["pident_milli"].view(np.int32)).cuda()
    if layout in ("packed", "packed64"):
        rec = engine.pack_hits_device(t, cols, wide=layout == "packed64")
        torch.cuda.synchronize()
        return {"seg_off": cols["seg_off"], "bitscore": cols["bitscore"], layout: rec}
    return cols


def run_ring(t, h, layout, strategy):
    import torch
    bufs = device_buffers(t, h, layout)
    out = torch.empty(32 * (len(h["seg_off"]) - 1), dtype=torch.uint8, device="cuda")
    out.fill_(0xA5)
    engine.run_consensus_device(t, bufs, out, strategy=strategy)
    torch.cuda.synchronize()
    name, _, block = engine.last_launch()
    assert "stream" in name and block in (768, 704), (name, block)      # the build with the ring (12 or 11 waves per block)
    return engine.records_from_tensor(out)


def test_block_sizes_cover_the_edges():
    assert {207, 208, 209, 247, 248, 249, 496} <= set(TOTALS)
    for total, pos in CASES:
        s = block_sizes(total, pos)
        assert s.min() >= 1 and s.max() <= HITS
        heavy = int(np.argmax(s))                       # the first query with all (or most) of its hits tied
        assert s[heavy] >= 40 and {"first": heavy == 0, "last": np.argmax(s[::-1]) == 0, "middle": heavy == WAVE // 2 - 4}[pos]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_tasks_at_the_list_capacity_edges(layout, monkeypatch):
    monkeypatch.setenv("BLU_STREAM_KIND", "ring")
    tax = synth.make_taxonomy(3000, 77)
    h, _ = capacity_table(tax, one_round_of_tasks(), 9100)
    t = engine.Taxonomy(tax.lin_off, tax.lin_node, tax.lin_rank, tax.rank_names, taxon="custom", custom=H.CUSTOM_16S, device=0)
    for strategy in STRATEGIES:
        exp = H.columnar(tax, h, "custom", strategy, H.CUSTOM_16S, threads=16)
        got = run_ring(t, h, layout, strategy)
        assert got.tobytes() == exp.tobytes(), (layout, strategy, _first_difference(got, exp))
    t.close()


def test_identities_past_the_key_read_their_cutoffs_from_global_memory(monkeypatch):
    monkeypatch.setenv("BLU_STREAM_KIND", "ring")
    tax = synth.make_taxonomy(3000, 78)
    h, is_top = capacity_table(tax, one_round_of_tasks(), 9200)
    rng = np.random.default_rng(9201)
    n_queries = len(h["seg_off"]) - 1
    # two queries in five: every top row gets an identity of 131.071 % or more (one value per query, or one per row)
    kind = rng.integers(0, 5, n_queries)
    per_query = np.repeat(rng.choice(HIGH_MILLI, n_queries), HITS)
    per_row = rng.choice(HIGH_MILLI, n_queries * HITS)
    pm = h["pident_milli"].astype(np.int64)
    pm = np.where(is_top & (np.repeat(kind, HITS) == 0), per_query, pm)
    pm = np.where(is_top & (np.repeat(kind, HITS) == 1), per_row, pm)
    h["pident_milli"] = pm.astype(np.uint32)
    h["pident"] = pm.astype(np.float64) / 1000.0
    assert int((pm >= 131071).sum()) > n_queries // 2
    t = engine.Taxonomy(tax.lin_off, tax.lin_node, tax.lin_rank, tax.rank_names, taxon="custom", custom=CUSTOM_HIGH, device=0)
    for strategy in STRATEGIES:
        exp = H.columnar(tax, h, "custom", strategy, CUSTOM_HIGH, threads=16)
        got = run_ring(t, h, "milli", strategy)
        assert got.tobytes() == exp.tobytes(), (strategy, _first_difference(got, exp))
        # the f64 column of the same values: the builds that keep the LDS table
        got = run_ring(t, h, "f64", strategy)
        assert got.tobytes() == exp.tobytes(), ("f64", strategy, _first_difference(got, exp))
    t.close()


def _first_difference(got, exp):
    a = np.frombuffer(got.tobytes(), dtype=np.uint8).reshape(-1, 32)
    b = np.frombuffer(exp.tobytes(), dtype=np.uint8).reshape(-1, 32)
    bad = np.nonzero((a != b).any(axis=1))[0]
    if len(bad) == 0:
        return None
    q = int(bad[0])
    return {"queries": len(bad), "first": q, "block": q // WAVE, "case": CASES[(q // WAVE) % len(CASES)], "got": got[q], "exp": exp[q]}
