"""GPU parity tests proper: the HIP path (through the C ABI) against the oracle.

Bit-exact on every field of the 32-byte record against the columnar oracle, and on the rendered
reference fields (identifier, ranks, taxonomy string, flags, f64 percIdentity/bitScore — tolerance 0:
the engine copies, never recomputes, the floats) against the string-faithful oracle."""
import gzip
import json
import os

import numpy as np
import pytest

from blutils_amd import _native as N
from blutils_amd import engine, synth
from oracle import oracle as orc
from tests import helpers as H
from tests.golden_recipe import table_from_taxa

pytestmark = pytest.mark.gpu


def _engine_tax(tax, taxon, custom=None, bad=None):
    return engine.Taxonomy(tax.lin_off, tax.lin_node, tax.lin_rank, tax.rank_names, taxon=taxon, custom=custom,
                           device=0, taxid=tax.taxid, bad=bad)


def _run_host(t, hits, strategy):
    # hits["tax_row"] holds desc row indices (what the oracle reads); the engine takes its own row ids
    return engine.run_consensus_host(t, hits["seg_off"], hits["bitscore"], t.engine_rows(hits["tax_row"]), hits["pident"],
                                     hits["align_len"], hits["acc_rank"], strategy=strategy)


_assert_records_equal = H.assert_records_equal


def _engine_renderer(t, tax, hits):
    return H.Renderer(tax, hits, lambda c: t.rank_name(c), lambda c: t.rank_name(c, serde=True),
                      lambda row, lvl: bool(t.row_cutoffs(row)[1][lvl]))


@pytest.mark.parametrize("strategy", ["relaxed", "cautious"])
@pytest.mark.parametrize("taxon,custom", [("bacteria", None), ("custom", H.CUSTOM_16S)])
def test_c1_against_both_oracles(strategy, taxon, custom):
    """BASELINE config #1: 1k queries x 10 hits, 2k-taxid taxonomy, assets custom cutoffs."""
    tax = synth.make_taxonomy(2000, synth.SEEDS["C1"])
    hits = synth.make_hits(tax, 1000, synth.SEEDS["C1"], 10, p_unmatched=0.002).numpy()
    t = _engine_tax(tax, taxon, custom)
    got = _run_host(t, hits, strategy)
    _assert_records_equal(got, H.columnar(tax, hits, taxon, strategy, custom))
    faithful = orc.run(H.oracle_table(tax, hits), taxon=taxon, strategy=strategy, custom=custom, threads=4).results()
    r = _engine_renderer(t, tax, hits)
    for q in range(len(got)):
        H.assert_matches_faithful(r.render(got[q]), faithful[q], q)


@pytest.mark.parametrize("strategy", ["relaxed", "cautious"])
def test_c2_100k_by_50(strategy):
    """BASELINE config #2: 100k queries x 50 hits, 50k-node taxonomy; device-pointer path."""
    import torch
    tax = synth.make_taxonomy(50000, synth.SEEDS["C2"])
    dh = synth.make_hits(tax, 100000, synth.SEEDS["C2"], 50, device="cuda")
    t = _engine_tax(tax, "custom", H.CUSTOM_16S)
    out = torch.zeros(32 * dh.n_queries, dtype=torch.uint8, device="cuda")
    hits = dh.numpy()
    dev_hits = dh.as_dict()
    dev_hits["tax_row"] = t.engine_rows(dev_hits["tax_row"]).contiguous()
    engine.run_consensus_device(t, dev_hits, out, strategy=strategy)
    torch.cuda.synchronize()
    got = engine.records_from_tensor(out)
    # the generator is counter-based integer arithmetic: the CPU copy of the same seed is the same table
    cpu = synth.make_hits(tax, 100000, synth.SEEDS["C2"], 50, device="cpu").numpy()
    for k in hits:
        np.testing.assert_array_equal(hits[k], cpu[k], err_msg=k)
    _assert_records_equal(got, H.columnar(tax, hits, "custom", strategy, H.CUSTOM_16S, threads=8))
    st = got["status"]
    assert (st == 0).sum() > 30000 and (st == 1).sum() > 20000 and (st >= 16).sum() > 0


@pytest.mark.parametrize("strategy", ["relaxed", "cautious"])
def test_c5_zipf_deep(strategy):
    """Scaled-down config #5: Zipf hit counts 1..5000, deep lineages (chunked path + long segments)."""
    tax = synth.make_taxonomy(30000, synth.SEEDS["C5"], deep=True)
    hits = synth.make_hits(tax, 20000, synth.SEEDS["C5"], None, zipf=(1.1, 1, 5000)).numpy()
    assert np.diff(hits["seg_off"]).max() > 2000
    t = _engine_tax(tax, "fungi")
    got = _run_host(t, hits, strategy)
    _assert_records_equal(got, H.columnar(tax, hits, "fungi", strategy, threads=8))


def test_large_top_groups_and_ties():
    """Whole segments tie on bit-score (top group = segment, up to 700 rows) and on every sort key."""
    tax = synth.make_taxonomy(3000, 21, deep=True)
    hits = synth.make_hits(tax, 3000, 22, None, zipf=(0.8, 1, 700)).numpy()
    hits["bitscore"][:] = 500
    hits["pident"][:] = np.round(hits["pident"] / 5) * 5       # few distinct values -> deep tie-breaks
    hits["align_len"][:] = 400 + hits["align_len"] % 2
    t = _engine_tax(tax, "bacteria")
    for strategy in ("relaxed", "cautious"):
        _assert_records_equal(_run_host(t, hits, strategy), H.columnar(tax, hits, "bacteria", strategy, threads=8))


def test_error_statuses_and_edge_segments():
    """Reference panic sites -> statuses; empty segments; single-row segments; segment of exactly 64 and 65."""
    tax = synth.make_taxonomy(500, 5)
    bad = (np.arange(tax.n) % 37 == 0).astype(np.uint8)
    lens = np.array([0, 1, 64, 65, 0, 2, 128, 129, 63, 1, 0], dtype=np.int64)
    reps = 40
    lens = np.tile(lens, reps)
    base = synth.make_hits(tax, int((lens > 0).sum()), 6, 200, p_unmatched=0.01).numpy()
    seg = np.zeros(len(lens) + 1, dtype=np.int64)
    seg[1:] = np.cumsum(lens)
    # carve ragged segments out of the 200-hit queries
    take = np.concatenate([np.arange(l) + 200 * i for i, l in enumerate(lens[lens > 0])])
    hits = {k: (base[k][take] if k != "seg_off" else seg) for k in base}
    t = _engine_tax(tax, "bacteria", bad=bad)
    for strategy in ("relaxed", "cautious"):
        got = _run_host(t, hits, strategy)
        _assert_records_equal(got, H.columnar(tax, hits, "bacteria", strategy, bad=bad))
        assert (got["status"][lens == 0] == N.ST_NO_HITS).all()
        assert {16, 17, 18, 19}.issubset(set(got["status"].tolist())), set(got["status"].tolist())
    # NaN perc_identity in a top group is outside the restated domain: flagged, never silently used
    h2 = {k: v.copy() for k, v in hits.items()}
    h2["pident"][:] = np.nan
    got = _run_host(t, h2, "relaxed")
    assert set(got["status"].tolist()) <= {N.ST_NO_HITS, 16, 17, N.ST_ERR_BAD_PIDENT}


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_adversarial_ties_and_prefix_lineages(seed):
    """Tiny tables built to collide on every sort key (see helpers.adversarial_case): the engine against both
    oracles, both strategies, built-in and custom backbones, bad lineages included."""
    tax, hits = H.adversarial_case(seed, n_q=5000)
    bad = (np.arange(tax.n) % 17 == 3).astype(np.uint8)
    for taxon, custom in (("bacteria", None), ("custom", H.CUSTOM_16S), ("fungi", None)):
        t = _engine_tax(tax, taxon, custom, bad=bad)
        for strategy in ("relaxed", "cautious"):
            got = _run_host(t, hits, strategy)
            _assert_records_equal(got, H.columnar(tax, hits, taxon, strategy, custom, bad=bad))
    faithful = orc.run(H.oracle_table(tax, hits, bad), taxon="fungi", strategy="cautious", threads=4).results()
    r = _engine_renderer(t, tax, hits)
    for q in range(len(got)):
        H.assert_matches_faithful(r.render(got[q]), faithful[q], q)


def test_milli_percent_layout_gives_identical_records():
    """perc_identity as milli-percent u32 (20 B/hit) is a lossless re-encoding of 3-decimal values: every record is
    bit-identical to the f64 layout's, on the short path, the worklist path and the device-pointer path."""
    import torch
    tax = synth.make_taxonomy(30000, synth.SEEDS["C5"], deep=True)
    dh = synth.make_hits(tax, 30000, synth.SEEDS["C5"], None, zipf=(1.1, 1, 3000), device="cuda")
    t = _engine_tax(tax, "bacteria")
    rows = t.engine_rows(dh.tax_row).contiguous()
    outs = []
    for layout in ("f64", "milli"):
        hd = dh.as_dict(layout)
        hd["tax_row"] = rows
        out = torch.zeros(32 * dh.n_queries, dtype=torch.uint8, device="cuda")
        engine.run_consensus_device(t, hd, out, strategy="relaxed")
        torch.cuda.synchronize()
        outs.append(engine.records_from_tensor(out))
    assert outs[0].tobytes() == outs[1].tobytes()
    h = dh.numpy()
    assert np.array_equal(h["pident"], dh.pident_milli.cpu().numpy() / 1000.0)
    _assert_records_equal(outs[1], H.columnar(tax, h, "bacteria", "relaxed", threads=8))
    # host-pointer path, cautious, C1-like table
    tax1 = synth.make_taxonomy(2000, synth.SEEDS["C1"])
    d1 = synth.make_hits(tax1, 1000, synth.SEEDS["C1"], 10)
    h1 = d1.numpy()
    t1 = _engine_tax(tax1, "custom", H.CUSTOM_16S)
    a = engine.run_consensus_host(t1, h1["seg_off"], h1["bitscore"], t1.engine_rows(h1["tax_row"]), h1["pident"], h1["align_len"], h1["acc_rank"], "cautious")
    b = engine.run_consensus_host(t1, h1["seg_off"], h1["bitscore"], t1.engine_rows(h1["tax_row"]), None, h1["align_len"], h1["acc_rank"], "cautious",
                                  pident_milli=d1.pident_milli.numpy())
    assert a.tobytes() == b.tobytes()


def _intern_lineages(lineages):
    """lineage strings -> CSR over interned canonical (rank, identifier) pairs."""
    ranks, rank_id, nodes = [], {}, {}
    off, node, rk = [0], [], []
    for lin in lineages:
        for el in lin.split(";"):
            r, ident = el.split("__")
            if r not in rank_id:
                rank_id[r] = len(ranks)
                ranks.append(r)
            node.append(nodes.setdefault((orc.rank_display(r), ident), len(nodes)))
            rk.append(rank_id[r])
        off.append(len(node))
    inv = {v: k for k, v in nodes.items()}
    return (np.array(off, np.uint64), np.array(node, np.uint32), np.array(rk, np.uint16), ranks, inv)


@pytest.mark.parametrize("strategy,reverse", [("relaxed", False), ("cautious", False), ("relaxed", True), ("cautious", True)])
def test_golden_vectors_through_the_gpu(golden_dir, strategy, reverse):
    """The reference's golden output (zymo mock, 253 distinct results = 2283 queries) and the docs worked
    example, re-synthesised by the §8c recipe (align_lengths ascending in each bean's listed accession order, so that the
    golden's own accession order is what the 4-key sort must produce; hit rows in the recipe's file order and reversed),
    interned, and run through the HIP path."""
    with gzip.open(os.path.join(golden_dir, "zymo_mock_distilled.json.gz"), "rt") as f:
        zymo = json.load(f)
    doc = json.load(open(os.path.join(golden_dir, "docs_worked_example.json")))
    taxa = [c["taxon"] for c in zymo["cases"]] + [r["taxon"] for r in doc["results"]]
    tab = table_from_taxa(taxa, reverse_file_order=reverse)
    off, node, rk, ranks, inv = _intern_lineages(tab.lineages)
    t = engine.Taxonomy(off, node, rk, ranks, taxon="bacteria", device=0)
    acc_sorted = sorted(range(len(tab.accessions)), key=lambda i: tab.accessions[i].encode())
    acc_rank = np.zeros(len(tab.accessions), dtype=np.uint32)
    acc_rank[acc_sorted] = np.arange(len(acc_sorted), dtype=np.uint32)
    got = engine.run_consensus_host(t, tab.seg_off, tab.bit_score.astype(np.int32), t.engine_rows(tab.tax_row.astype(np.uint32)),
                                    tab.pident, tab.align_len.astype(np.int32), acc_rank[tab.acc_idx], strategy=strategy)
    faithful = orc.run(tab, taxon="bacteria", strategy=strategy).results()
    for q, (exp, rec) in enumerate(zip(taxa, got)):
        assert int(rec["status"]) == (1 if exp["singleMatch"] else 0)
        ident = inv[int(rec["identifier_node"])][1]
        row = int(rec["ref_row"])
        trow = int(tab.tax_row[row])
        lin = tab.lineages[trow].split(";")
        taxonomy = ";".join(lin[j] for j in range(len(lin)) if (int(rec["level_mask"]) >> j) & 1)
        # golden fields the recipe can reproduce
        assert ident == exp["identifier"] and taxonomy == exp["taxonomy"], (q, ident, exp["identifier"])
        assert t.rank_name(int(rec["reached_rank"]), serde=True) == exp["reachedRank"]
        assert float(tab.pident[row]) == exp["percIdentity"] and float(tab.bit_score[row]) == exp["bitScore"]
        # every field against the golden-pinned oracle on the same table
        mal = int(rec["max_allowed_level"])
        if mal == 0xFF:
            mar = None
        else:
            _, isdef, codes = t.row_cutoffs(trow)
            mar = t.rank_name(codes[mal], serde=bool(isdef[mal]))
        o = faithful[q]["taxon"]
        assert mar == o["maxAllowedRank"] and bool(rec["flags"] & 1) == o["mutated"], (q, mar, o["maxAllowedRank"])
        # the reference row the engine picked is the one the faithful oracle's sort picked: its accession leads (Cautious) or
        # ends (Relaxed) the sorted list the beans were folded from
        assert o["percIdentity"] == float(tab.pident[row]) and tab.accessions[int(tab.acc_idx[row])] in {a for b in o["consensusBeans"] for a in b["accessions"]}
        if q >= len(zymo["cases"]) and strategy == doc["strategy"]:
            assert mar == exp["maxAllowedRank"] and bool(rec["flags"] & 1) == exp["mutated"]   # docs example: all fields


def test_run_is_replayable_as_a_hip_graph():
    """The two kernels of a run leave the worklist counters as they found them, so a captured run can be replayed on
    new contents of the same buffers (and plain runs can follow graph replays on the same handle)."""
    import torch
    tax = synth.make_taxonomy(30000, synth.SEEDS["C5"], deep=True)
    t = _engine_tax(tax, "bacteria")
    tables = [synth.make_hits(tax, 20000, seed, None, zipf=(1.1, 1, 800), device="cuda") for seed in (5, 6, 7)]
    nh = max(h.n_hits for h in tables)
    static = {k: torch.zeros(nh if k != "seg_off" else 20001, dtype=dt, device="cuda")
              for k, dt in (("seg_off", torch.int64), ("bitscore", torch.int32), ("tax_row", torch.int32),
                            ("pident_milli", torch.int32), ("align_len", torch.int32), ("acc_rank", torch.int32))}
    out = torch.zeros(32 * 20000, dtype=torch.uint8, device="cuda")

    def load(h):
        d = h.as_dict("milli")
        d["tax_row"] = t.engine_rows(h.tax_row).contiguous()
        for k in static:
            static[k].zero_()
            static[k][: d[k].numel()].copy_(d[k])
        static["seg_off"][d["seg_off"].numel() - 1:] = int(d["seg_off"][-1])
        return d

    load(tables[0])
    views = dict(static)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        engine.run_consensus_device(t, views, out, strategy="relaxed")     # warm-up (allocates the workspace)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        engine.run_consensus_device(t, views, out, strategy="relaxed")
    for h in tables + [tables[0]]:
        load(h)
        torch.cuda.synchronize()
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = engine.records_from_tensor(out)[: h.n_queries]
        _assert_records_equal(got, H.columnar(tax, h.numpy(), "bacteria", "relaxed", threads=8))
    # a plain run after the replays
    d = tables[1].as_dict("milli")
    d["tax_row"] = t.engine_rows(tables[1].tax_row).contiguous()
    out2 = torch.zeros(32 * 20000, dtype=torch.uint8, device="cuda")
    engine.run_consensus_device(t, d, out2, strategy="relaxed")
    torch.cuda.synchronize()
    _assert_records_equal(engine.records_from_tensor(out2), H.columnar(tax, tables[1].numpy(), "bacteria", "relaxed", threads=8))


def test_hostile_offsets_and_row_ids_do_not_disturb_valid_queries():
    """The C ABI takes offsets and row ids as data: a non-ascending or out-of-range offset table and garbage row ids
    must neither fault nor change the records of the queries whose own segment is intact."""
    rng = np.random.default_rng(17)
    tax = synth.make_taxonomy(5000, synth.SEEDS["C2"])
    hits = synth.make_hits(tax, 3000, synth.SEEDS["C2"], 20).numpy()
    t = _engine_tax(tax, "bacteria")
    rows = t.engine_rows(hits["tax_row"])
    clean = engine.run_consensus_host(t, hits["seg_off"], hits["bitscore"], rows, hits["pident"], hits["align_len"],
                                      hits["acc_rank"], "relaxed")
    nq, nh = 3000, len(rows)
    # 1. offsets: some entries swapped, some far past the table, some huge
    seg = hits["seg_off"].copy()
    touched = np.zeros(nq, bool)
    for q in rng.choice(np.arange(1, nq - 1), 60, replace=False):
        kind = int(rng.integers(0, 3))
        seg[q] = [seg[q + 1] + 7, nh + 1000, 2 ** 40][kind] if kind else max(int(seg[q - 1]) - 3, 0)
        touched[q - 1] = touched[q] = True
    L = N.lib()
    out = np.zeros(nq, dtype=engine.RESULT_DTYPE)
    cols = [np.ascontiguousarray(hits["bitscore"], np.int32), np.ascontiguousarray(rows, np.uint32),
            np.ascontiguousarray(hits["pident"], np.float64), np.ascontiguousarray(hits["align_len"], np.int32),
            np.ascontiguousarray(hits["acc_rank"]).view(np.uint32)]
    segc = np.ascontiguousarray(seg, np.uint64)
    h = N.Hits(cols[0].ctypes.data, cols[1].ctypes.data, cols[2].ctypes.data, cols[3].ctypes.data, cols[4].ctypes.data,
               segc.ctypes.data, nh, nq, 0, 0, None)
    import ctypes as C
    params = N.RunParams(N.STRATEGY["relaxed"], 0, None)
    assert L.blu_consensus_run(t.handle, C.byref(h), C.byref(params), out.ctypes.data) == N.BLU_OK
    ok = ~touched
    assert out[ok].tobytes() == clean[ok].tobytes()
    assert set(np.unique(out["status"])) <= {0, 1, 2, 16, 17, 18, 19, 20}
    # 2. row ids: random bit patterns in 5 % of the rows (wrong length bits, positions past the table, the unmatched marker)
    bad_rows = rows.copy()
    idx = rng.choice(nh, nh // 20, replace=False)
    bad_rows[idx] = rng.integers(0, 2 ** 32, len(idx), dtype=np.uint64).astype(np.uint32)
    out2 = engine.run_consensus_host(t, hits["seg_off"], hits["bitscore"], bad_rows, hits["pident"], hits["align_len"],
                                     hits["acc_rank"], "relaxed")
    qid = np.searchsorted(hits["seg_off"], idx, side="right") - 1
    intact = np.ones(nq, bool)
    intact[qid] = False
    assert intact.sum() > 300 and out2[intact].tobytes() == clean[intact].tobytes()
    assert set(np.unique(out2["status"])) <= {0, 1, 2, 16, 17, 18, 19, 20}


def test_sharded_run_over_several_handles_equals_the_single_run():
    """blu_consensus_run_multi: contiguous query ranges balanced by hit count, one handle and host thread per range,
    records in query order with table-wide reference rows (two and three handles on the one GPU of the test box)."""
    tax = synth.make_taxonomy(30000, synth.SEEDS["C5"], deep=True)
    dh = synth.make_hits(tax, 20000, synth.SEEDS["C5"], None, zipf=(1.1, 1, 2000), device="cuda")
    h = dh.numpy()
    handles = [_engine_tax(tax, "bacteria") for _ in range(3)]
    rows = handles[0].engine_rows(h["tax_row"])
    single = engine.run_consensus_host(handles[0], h["seg_off"], h["bitscore"], rows, h["pident"], h["align_len"], h["acc_rank"], "cautious")
    _assert_records_equal(single, H.columnar(tax, h, "bacteria", "cautious", threads=8))
    for n in (2, 3):
        multi = engine.run_consensus_multi(handles[:n], h["seg_off"], h["bitscore"], rows, h["pident"], h["align_len"], h["acc_rank"], "cautious")
        assert multi.tobytes() == single.tobytes()
    milli = engine.run_consensus_multi(handles, h["seg_off"], h["bitscore"], rows, None, h["align_len"], h["acc_rank"], "cautious",
                                       pident_milli=dh.pident_milli.cpu().numpy())
    assert milli.tobytes() == single.tobytes()
    with pytest.raises(N.BluError):   # one handle twice: its scratch is per handle
        engine.run_consensus_multi([handles[0], handles[0]], h["seg_off"], h["bitscore"], rows, h["pident"], h["align_len"], h["acc_rank"])


def test_maximum_depth_lineages_and_wide_groups():
    """64-level lineages (BLU_MAX_DEPTH, level-mask bit 63) that agree for 10..63 levels — beyond the 20 levels whose
    run lengths sit in the reference row — and groups spanning more than 255 sorted rows: both take the range-minimum
    path of the stream kernel; segments over 64 rows take the worklist kernel.  Against both oracles."""
    rng = np.random.default_rng(21)
    backbone = ["d", "k", "p", "c", "o", "f", "g", "s"]
    rank_names = backbone + ["clade", "strain"]
    n_tax = 1500
    off, node, rank = [0], [], []
    for t in range(n_tax):
        depth = 64 if t % 3 else int(rng.integers(9, 64))
        split = int(rng.integers(10, 64))                       # first level at which this taxon leaves the common trunk
        fam = t % 5                                             # five trunks: long common prefixes, wide sorted spans
        for j in range(depth):
            if j < 8:
                r = backbone[j]
            else:
                r = "strain" if j == depth - 1 else "clade"
            ident = f"t{fam}_{j}" if j < split else f"x{t}_{j}"
            if j == 0:
                ident = "root"
            node.append((r, ident))
            rank.append(rank_names.index(r))
        off.append(len(node))
    interned = {}
    node = [interned.setdefault((orc.rank_display(r), i), len(interned)) for r, i in node]
    tax = synth.SynthTaxonomy(rank_names, np.array(off, np.uint64), np.array(node, np.uint32), np.array(rank, np.uint16),
                              (100 + np.arange(n_tax)).astype(np.int64), np.zeros((9, n_tax), np.int32), np.zeros((9, n_tax), np.int32),
                              n_tax, 21, False)
    n_q = 1500
    lens = np.where(rng.random(n_q) < 0.1, rng.integers(65, 200, n_q), rng.integers(1, 30, n_q))
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nh = int(seg[-1])
    qid = np.repeat(np.arange(n_q), lens)
    same_trunk = (qid % 2 == 0)
    rows = np.where(same_trunk, (rng.integers(0, n_tax // 5, nh) * 5 + qid % 5) % n_tax, rng.integers(0, n_tax, nh)).astype(np.int32)
    pident = (rng.integers(80000, 100001, nh) / 1000).astype(np.float64)
    whole = qid % 10 == 0                                     # one 64-level taxon per query, identity 100: every level passes
    rows[whole] = (1 + 3 * (qid[whole] % 400)).astype(np.int32)
    pident[whole] = 100.0
    hits = {"seg_off": seg, "bitscore": rng.choice([900, 900, 899], nh).astype(np.int32), "tax_row": rows,
            "pident": pident,
            "align_len": rng.integers(380, 480, nh).astype(np.int32), "acc_rank": rng.integers(0, 50, nh).astype(np.int32)}
    for taxon, custom in (("bacteria", None), ("custom", H.CUSTOM_16S)):
        t = _engine_tax(tax, taxon, custom)
        assert t.max_depth == 64
        for strategy in ("relaxed", "cautious"):
            got = _run_host(t, hits, strategy)
            _assert_records_equal(got, H.columnar(tax, hits, taxon, strategy, custom))
    assert (got["level_mask"] >> np.uint64(63)).any()               # the deepest level is reached by somebody
    assert ((got["status"] == 0) & (got["bean_index"] >= 20)).any() # agreement deeper than the row's run lengths
    faithful = orc.run(H.oracle_table(tax, hits), taxon="custom", strategy="cautious", custom=H.CUSTOM_16S, threads=4).results()
    r = _engine_renderer(t, tax, hits)
    for q in range(len(got)):
        H.assert_matches_faithful(r.render(got[q]), faithful[q], q)


def test_host_table_staged_in_chunks(monkeypatch):
    """A host table larger than the device budget goes over PCIe in chunks of whole queries, double-buffered on two
    streams (BLU_STAGE_ROWS forces the cut here): same records, reference rows still table-wide; a single query longer
    than the chunk gets a chunk of its own."""
    tax = synth.make_taxonomy(30000, synth.SEEDS["C5"], deep=True)
    dh = synth.make_hits(tax, 20000, synth.SEEDS["C5"], None, zipf=(1.1, 1, 3000), device="cuda")
    h = dh.numpy()
    t = _engine_tax(tax, "bacteria")
    rows = t.engine_rows(h["tax_row"])
    whole = engine.run_consensus_host(t, h["seg_off"], h["bitscore"], rows, h["pident"], h["align_len"], h["acc_rank"], "relaxed")
    for stage_rows in (100000, 7919, 1000):
        monkeypatch.setenv("BLU_STAGE_ROWS", str(stage_rows))
        cut = engine.run_consensus_host(t, h["seg_off"], h["bitscore"], rows, h["pident"], h["align_len"], h["acc_rank"], "relaxed")
        assert cut.tobytes() == whole.tobytes(), stage_rows
        cut = engine.run_consensus_host(t, h["seg_off"], h["bitscore"], rows, None, h["align_len"], h["acc_rank"], "relaxed",
                                        pident_milli=dh.pident_milli.cpu().numpy())
        assert cut.tobytes() == whole.tobytes(), stage_rows
    # a chunked table needs an ascending offset table
    seg = h["seg_off"].copy()
    seg[5], seg[6] = seg[6], seg[5]
    if seg[5] != seg[6]:
        with pytest.raises(N.BluError):
            engine.run_consensus_host(t, seg, h["bitscore"], rows, h["pident"], h["align_len"], h["acc_rank"], "relaxed")
    monkeypatch.delenv("BLU_STAGE_ROWS")


@pytest.mark.parametrize("hits", [4, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025])
def test_lanes_per_query_paths(hits):
    """The stream kernel gives a query 4, 8, 16 or 32 lanes depending on the task's longest streamed segment (<= 16 / 32 /
    64 / 128 rows), takes 129..512-row segments in its long pass (256-row slots) and leaves longer ones to the worklist
    kernel (1024 rows per round trip): uniform tables on both sides of each boundary, and one ragged table mixing them,
    against the oracle."""
    tax = synth.make_taxonomy(4000, synth.SEEDS["C2"])
    t = _engine_tax(tax, "custom", H.CUSTOM_16S)
    h = synth.make_hits(tax, 3000 if hits <= 64 else (700 if hits <= 257 else 300), 100 + hits, hits, p_unmatched=0.003).numpy()
    for strategy in ("relaxed", "cautious"):
        _assert_records_equal(_run_host(t, h, strategy), H.columnar(tax, h, "custom", strategy, H.CUSTOM_16S))
    # ragged: runs of 64 queries each capped at 16 / 32 / 64 / 128 / 256 / 300 rows, carved out of a 300-hit table
    base = synth.make_hits(tax, 64 * 30, 200 + hits, 300).numpy()
    rng = np.random.default_rng(hits)
    caps = np.repeat(rng.choice([16, 32, 64, 128, 256, 300], 30), 64)
    lens = np.minimum(rng.integers(1, 301, 64 * 30), caps)
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    take = np.concatenate([np.arange(l) + 300 * i for i, l in enumerate(lens)])
    ragged = {k: (base[k][take] if k != "seg_off" else seg) for k in base}
    _assert_records_equal(_run_host(t, ragged, "relaxed"), H.columnar(tax, ragged, "custom", "relaxed", H.CUSTOM_16S))


def test_packed_layout_gives_identical_records():
    """ABI v3: the four non-bit-score values of a hit as one 16-byte record next to the bit-score column.  Records must be
    bit-identical to the column layouts on the streamed widths, the long pass, the worklist kernel, through host and
    device pointers, and through the chunked / sharded host paths."""
    import torch
    tax = synth.make_taxonomy(30000, synth.SEEDS["C5"], deep=True)
    dh = synth.make_hits(tax, 30000, synth.SEEDS["C5"], None, zipf=(1.1, 1, 3000), device="cuda")
    t = _engine_tax(tax, "bacteria")
    dh.tax_row = t.engine_rows(dh.tax_row).contiguous()
    outs = []
    # "packed" without the handle: side records put together by hand, no shape hint (the engine then reads the shape from
    # the row); with it: blu_hits_pack / blu_hits_pack64 on the device, hints included
    for layout, tx in (("milli", None), ("packed", None), ("packed", t), ("packed64", t)):
        out = torch.zeros(32 * dh.n_queries, dtype=torch.uint8, device="cuda")
        engine.run_consensus_device(t, dh.as_dict(layout, tax=tx), out, strategy="cautious")
        torch.cuda.synchronize()
        outs.append(engine.records_from_tensor(out))
    for o in outs[1:]:
        assert outs[0].tobytes() == o.tobytes()
    # a hint that names another shape (or none that exists) costs a round trip, never a result
    hinted = dh.as_dict("packed", tax=t)
    rec = hinted["packed"].view(-1, 4)
    wrong = rec.clone()
    wrong[:, 1] = (rec[:, 1] & 0x1FFFF) | (((rec[:, 1] >> 17) * 7 + 3) % 32768 << 17)
    out = torch.zeros(32 * dh.n_queries, dtype=torch.uint8, device="cuda")
    engine.run_consensus_device(t, {"seg_off": hinted["seg_off"], "bitscore": hinted["bitscore"], "packed": wrong.reshape(-1).contiguous()}, out,
                                strategy="cautious")
    torch.cuda.synchronize()
    assert engine.records_from_tensor(out).tobytes() == outs[0].tobytes()
    # fixed lengths around every width, host pointers
    for hits_per_query in (7, 20, 30, 50, 100, 200, 400, 600):
        tax2 = synth.make_taxonomy(3000, 77)
        d2 = synth.make_hits(tax2, 900, 300 + hits_per_query, hits_per_query, p_unmatched=0.003)
        h2 = d2.numpy()
        t2 = _engine_tax(tax2, "custom", H.CUSTOM_16S)
        rows = t2.engine_rows(h2["tax_row"])
        milli = d2.pident_milli.numpy()
        a = engine.run_consensus_host(t2, h2["seg_off"], h2["bitscore"], rows, None, h2["align_len"], h2["acc_rank"], "relaxed", pident_milli=milli)
        b = engine.run_consensus_host(t2, h2["seg_off"], h2["bitscore"], rows, None, h2["align_len"], h2["acc_rank"], "relaxed", pident_milli=milli,
                                      packed=True)
        assert a.tobytes() == b.tobytes(), hits_per_query
        c = engine.run_consensus_host(t2, h2["seg_off"], h2["bitscore"], rows, h2["pident"], h2["align_len"], h2["acc_rank"], "relaxed", packed="wide")
        assert a.tobytes() == c.tobytes(), hits_per_query
        _assert_records_equal(b, H.columnar(tax2, h2, "custom", "relaxed", H.CUSTOM_16S))


@pytest.mark.parametrize("group", [3, 6, 14, 30, 50])
def test_many_ties_take_rounds_not_the_worklist(group):
    """Top groups of `group` rows per query (identical database sequences tie on bit-score): the 64 queries of a wave
    task no longer fit its LDS list at once, so phase 1 / 2a run in rounds.  Same records as the oracle."""
    tax = synth.make_taxonomy(5000, 31)
    dh = synth.make_hits(tax, 2500, 32 + group, 50)
    h = dh.numpy()
    bs = h["bitscore"].reshape(-1, 50).copy()
    bs[:, :group] = bs.max(axis=1, keepdims=True)
    h["bitscore"] = bs.reshape(-1)
    t = _engine_tax(tax, "custom", H.CUSTOM_16S)
    rows = t.engine_rows(h["tax_row"])
    for strategy in ("relaxed", "cautious"):
        exp = H.columnar(tax, h, "custom", strategy, H.CUSTOM_16S)
        got = _run_host(t, h, strategy)
        _assert_records_equal(got, exp)
        pk = engine.run_consensus_host(t, h["seg_off"], h["bitscore"], rows, None, h["align_len"], h["acc_rank"], strategy,
                                       pident_milli=dh.pident_milli.numpy(), packed=True)
        assert pk.tobytes() == exp.tobytes()


@pytest.mark.parametrize("hits", [10, 50, 300, 700])
def test_extreme_column_values(hits):
    """Values no BLAST run writes but the ABI's types admit: bit-scores at INT32_MIN / INT32_MAX (the kernel's own
    "no row" filler is INT32_MIN), negative and maximal alignment lengths, accession ranks up to 2^32 - 1, perc_identity
    of -inf / -0.0 / subnormal / 1e308 / +inf (f64 layout) and milli-percent values up to 2^32 - 1 (packed layout):
    every width of the stream kernel, its long pass and the worklist kernel against the oracle."""
    tax = synth.make_taxonomy(3000, 91)
    t = _engine_tax(tax, "custom", H.CUSTOM_16S)
    dh = synth.make_hits(tax, 600, 900 + hits, hits, p_unmatched=0.002)
    h = dh.numpy()
    rng = np.random.default_rng(hits)
    n = len(h["bitscore"])
    i32 = np.iinfo(np.int32)
    h["bitscore"] = rng.choice(np.array([i32.min, i32.min + 1, -1, 0, 1, i32.max - 1, i32.max], dtype=np.int32), n)
    h["align_len"] = rng.choice(np.array([i32.min, -7, 0, 400, i32.max], dtype=np.int32), n)
    h["acc_rank"] = rng.choice(np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], dtype=np.uint32), n).view(np.int32)
    rows = t.engine_rows(h["tax_row"])
    # f64 layouts: the five columns, and the 24-byte side records of blu_hits_pack64
    h["pident"] = rng.choice(np.array([-np.inf, -1.0, -0.0, 0.0, 5e-324, 66.667, 97.0, 100.0, 1e308, np.inf]), n)
    for strategy in ("relaxed", "cautious"):
        exp = H.columnar(tax, h, "custom", strategy, H.CUSTOM_16S)
        _assert_records_equal(_run_host(t, h, strategy), exp)
        got = engine.run_consensus_host(t, h["seg_off"], h["bitscore"], rows, h["pident"], h["align_len"], h["acc_rank"], strategy, packed="wide")
        _assert_records_equal(got, exp)
    # milli-percent column: any u32 is a milli-percent value; the oracle reads the double k / 1000.  The 16-byte side
    # records hold values below BLU_PACKED_PIDENT_LIMIT (131.071 %): blu_hits_pack refuses the rest, up to that limit they
    # give the column's records.
    milli = rng.choice(np.array([0, 1, 66667, 96999, 97000, 100000, 100001, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], dtype=np.uint32), n)
    h["pident"] = milli.astype(np.float64) / 1000.0
    for strategy in ("relaxed", "cautious"):
        exp = H.columnar(tax, h, "custom", strategy, H.CUSTOM_16S)
        got = engine.run_consensus_host(t, h["seg_off"], h["bitscore"], rows, None, h["align_len"], h["acc_rank"], strategy,
                                        pident_milli=milli)
        _assert_records_equal(got, exp)
        with pytest.raises(N.BluError, match="milli-percent"):
            engine.run_consensus_host(t, h["seg_off"], h["bitscore"], rows, None, h["align_len"], h["acc_rank"], strategy,
                                      pident_milli=milli, packed=True)
    small = rng.choice(np.array([0, 1, 66667, 96999, 97000, 100000, 100001, 131069, 131070], dtype=np.uint32), n)
    h["pident"] = small.astype(np.float64) / 1000.0
    for strategy in ("relaxed", "cautious"):
        exp = H.columnar(tax, h, "custom", strategy, H.CUSTOM_16S)
        got = engine.run_consensus_host(t, h["seg_off"], h["bitscore"], rows, None, h["align_len"], h["acc_rank"], strategy,
                                        pident_milli=small, packed=True)
        _assert_records_equal(got, exp)
        got = engine.run_consensus_host(t, h["seg_off"], h["bitscore"], rows, h["pident"], h["align_len"], h["acc_rank"], strategy, packed=True)
        _assert_records_equal(got, exp)                                      # (an f64 column of exact milli-percent values packs as well)


def test_more_distinct_cutoffs_than_the_lds_table_holds():
    """Interpolated cutoffs (linnaean_ranks.rs:289-366) depend on how many non-default levels sit between two backbone
    ranks; 1..60 stacked clades between domain and species give > 512 distinct values, more than the stream kernel
    keeps in LDS, so the cutoff tests read the global table instead.  Same records as the oracle."""
    from types import SimpleNamespace
    names = ["d", "clade", "s"]
    lin_node, lin_rank, lin_off = [], [], [0]
    for n in range(1, 61):
        for sp in range(3):
            lin_node += [1] + [100 + j for j in range(n)] + [5000 + 3 * n + sp]
            lin_rank += [0] + [1] * n + [2]
            lin_off.append(len(lin_node))
    n_tax = len(lin_off) - 1
    tax = SimpleNamespace(rank_names=names, lin_off=np.array(lin_off, dtype=np.uint64), lin_node=np.array(lin_node, dtype=np.uint32),
                          lin_rank=np.array(lin_rank, dtype=np.uint16), taxid=np.arange(1, n_tax + 1, dtype=np.int64), n=n_tax)
    custom = {"domain": 50, "species": 99}
    t = _engine_tax(tax, "custom", custom)
    distinct = set()
    for row in range(0, n_tax, 3):
        distinct.update(np.asarray(t.row_cutoffs(row)[0]).view(np.uint64).tolist())
    assert len(distinct) > 512
    rng = np.random.default_rng(12)
    Q = 3000
    lens = rng.integers(1, 41, Q)
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nrow = int(seg[-1])
    centre = np.repeat(rng.integers(0, n_tax, Q), lens)
    rows = np.clip(centre + rng.integers(-4, 5, nrow), 0, n_tax - 1).astype(np.int32)
    top = np.repeat(rng.integers(100, 900, Q), lens)
    h = {"seg_off": seg, "bitscore": (top - rng.integers(0, 2, nrow) * rng.integers(1, 50, nrow)).astype(np.int32), "tax_row": rows,
         "pident": np.round(rng.uniform(50.0, 100.0, nrow), 3), "align_len": rng.integers(380, 480, nrow).astype(np.int32),
         "acc_rank": rng.integers(0, 1000, nrow).astype(np.int32)}
    for strategy in ("relaxed", "cautious"):
        exp = H.columnar(tax, h, "custom", strategy, custom)
        _assert_records_equal(_run_host(t, h, strategy), exp)
        assert (exp["status"] <= 1).sum() > Q // 2


@pytest.mark.parametrize("hits", [10, 50, 300, 700, 1500])
def test_sparse_nan_perc_identity(hits):
    """NaN perc_identity on a few rows (f64 layout): a query whose top group holds one gets BLU_ST_ERR_BAD_PIDENT at
    the group's first NaN row in file order — after the parse errors, which win — and every other query is
    untouched; stream kernel widths, long pass and worklist kernel against the oracle."""
    tax = synth.make_taxonomy(3000, 17)
    bad = (np.arange(tax.n) % 41 == 0).astype(np.uint8)
    t = _engine_tax(tax, "custom", H.CUSTOM_16S, bad=bad)
    h = synth.make_hits(tax, 800 if hits <= 300 else 300, 1700 + hits, hits, p_unmatched=0.002).numpy()
    rng = np.random.default_rng(hits)
    bs = h["bitscore"].reshape(-1, hits).copy()
    bs[:, : max(2, hits // 8)] = bs.max(axis=1, keepdims=True)          # top groups wide enough to catch a NaN
    h["bitscore"] = bs.reshape(-1)
    h["pident"][rng.random(len(h["pident"])) < 0.02] = np.nan
    for strategy in ("relaxed", "cautious"):
        exp = H.columnar(tax, h, "custom", strategy, H.CUSTOM_16S, bad=bad)
        _assert_records_equal(_run_host(t, h, strategy), exp)
        st = set(exp["status"].tolist())
        assert N.ST_ERR_BAD_PIDENT in st and (0 in st or hits >= 300)


def test_degenerate_tables():
    """No rows at all (every query empty), a single query, a single row, zero queries: host and device pointers."""
    import torch
    tax = synth.make_taxonomy(200, 3)
    t = _engine_tax(tax, "bacteria")
    z32, zf = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64)
    # zero queries: nothing to do, nothing touched
    got = engine.run_consensus_host(t, np.zeros(1, dtype=np.int64), z32, z32, zf, z32, z32, "relaxed")
    assert len(got) == 0
    # 1000 queries, no rows
    seg = np.zeros(1001, dtype=np.int64)
    got = engine.run_consensus_host(t, seg, z32, z32, zf, z32, z32, "relaxed")
    assert (got["status"] == N.ST_NO_HITS).all() and (got["ref_row"] == 0xFFFFFFFF).all()
    out = torch.full((32 * 1000,), 7, dtype=torch.uint8, device="cuda")
    dev = {"seg_off": torch.zeros(1001, dtype=torch.int64, device="cuda"), "bitscore": torch.zeros(0, dtype=torch.int32, device="cuda"),
           "packed": torch.zeros(0, dtype=torch.int32, device="cuda")}
    engine.run_consensus_device(t, dev, out, strategy="cautious")
    torch.cuda.synchronize()
    assert engine.records_from_tensor(out).tobytes() == got.tobytes()
    # one query of one row / of 3000 rows
    for rows_n in (1, 3000):
        h = synth.make_hits(tax, 1, 40 + rows_n, rows_n, p_unmatched=0.0).numpy()
        for strategy in ("relaxed", "cautious"):
            _assert_records_equal(_run_host(t, h, strategy), H.columnar(tax, h, "bacteria", strategy))


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled", "peak_in_the_middle"])
def test_worklist_kernel_score_orders(order):
    """Long segments (1100..5000 rows: several 1024-row round trips of the worklist kernel, plus some under 1024 rows that
    stay in registers between its two passes) whose scores rise along the file, fall (BLAST's own order), are shuffled,
    or peak in the middle, with plateaus of equal scores; unmatched taxids, unparseable lineages and NaN identities
    sit in rows that are NOT in the top group and must not matter.  f64 and packed layouts against the oracle."""
    tax = synth.make_taxonomy(3000, 23)
    bad = (np.arange(tax.n) % 29 == 0).astype(np.uint8)
    t = _engine_tax(tax, "custom", H.CUSTOM_16S, bad=bad)
    rng = np.random.default_rng(len(order))
    lens = np.concatenate([rng.integers(1100, 5001, 100), rng.integers(513, 1025, 20)])
    rng.shuffle(lens)
    base = synth.make_hits(tax, len(lens), 77, 5000, p_unmatched=0.01).numpy()
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    take = np.concatenate([np.arange(l) + 5000 * i for i, l in enumerate(lens)])
    h = {k: (base[k][take] if k != "seg_off" else seg) for k in base}
    bs = np.empty(int(seg[-1]), dtype=np.int32)
    for i, l in enumerate(lens):
        steps = np.sort(rng.integers(0, 60, l)) * 7 + 100            # plateaus: several rows share every score
        if order == "descending":
            steps = steps[::-1]
        elif order == "shuffled":
            rng.shuffle(steps)
        elif order == "peak_in_the_middle":
            steps = np.concatenate([steps[::2], steps[1::2][::-1]])
        bs[seg[i]:seg[i + 1]] = steps
    h["bitscore"] = bs
    h["pident"][rng.random(len(bs)) < 0.01] = np.nan
    rows = t.engine_rows(h["tax_row"])
    for strategy in ("relaxed", "cautious"):
        exp = H.columnar(tax, h, "custom", strategy, H.CUSTOM_16S, bad=bad, threads=8)
        _assert_records_equal(_run_host(t, h, strategy), exp)
    assert len(set(exp["status"].tolist())) >= 3
    # packed layout (no NaN there: milli-percent values)
    milli = np.where(np.isnan(h["pident"]), 0, np.round(np.nan_to_num(h["pident"]) * 1000)).astype(np.uint32)
    h["pident"] = milli.astype(np.float64) / 1000.0
    for strategy in ("relaxed", "cautious"):
        exp = H.columnar(tax, h, "custom", strategy, H.CUSTOM_16S, bad=bad, threads=8)
        got = engine.run_consensus_host(t, h["seg_off"], h["bitscore"], rows, None, h["align_len"], h["acc_rank"], strategy,
                                        pident_milli=milli, packed=True)
        _assert_records_equal(got, exp)


@pytest.mark.parametrize("hits_per_query", [4, 10, 20, 50, 100])
def test_dense_top_groups_in_short_segments(hits_per_query):
    """Many hits tie on the top score in segments the stream kernel's ring path takes (identical database sequences): a
    step whose top rows would not fit an empty list is reduced by the lanes that scanned it (dense step), the others go
    through the list in rounds.  Whole-segment ties, half-segment ties and a mix, few distinct values on every sort key
    (so the stable-sort tie rule decides), unmatched rows in the groups; both strategies, milli-percent and packed layouts."""
    rng = np.random.default_rng(100 + hits_per_query)
    tax = synth.make_taxonomy(3000, 31)
    t = _engine_tax(tax, "custom", H.CUSTOM_16S)
    nq = 1500
    h = synth.make_hits(tax, nq, 500 + hits_per_query, hits_per_query, p_unmatched=0.002).numpy()
    bs = h["bitscore"].reshape(nq, hits_per_query)
    kind = rng.integers(0, 3, nq)                                   # 0: every row tied, 1: the first half tied, 2: as generated
    top = bs.max(axis=1)
    bs[kind == 0, :] = top[kind == 0, None]
    half = max(1, hits_per_query // 2)
    bs[kind == 1, :half] = top[kind == 1, None]
    h["pident"][:] = np.round(h["pident"] / 4) * 4                   # few distinct values: deep tie-breaks
    h["align_len"][:] = 400 + h["align_len"] % 2
    h["acc_rank"][:] = h["acc_rank"] % 3
    rows = t.engine_rows(h["tax_row"])
    pm = np.round(h["pident"] * 1000).astype(np.uint32)
    for strategy in ("relaxed", "cautious"):
        exp = H.columnar(tax, h, "custom", strategy, H.CUSTOM_16S, threads=8)
        for packed in (False, True):
            got = engine.run_consensus_host(t, h["seg_off"], h["bitscore"], rows, None, h["align_len"], h["acc_rank"], strategy=strategy,
                                            pident_milli=pm, packed=packed)
            _assert_records_equal(got, exp)
    assert (exp["status"] == 0).sum() > 500


@pytest.mark.parametrize("kind", ["ring", "noring"])
def test_both_builds_of_the_stream_kernel_give_the_same_records(kind, monkeypatch):
    """The stream kernel exists with the bit-score ring (168 VGPRs, 12 waves per CU) and without it (128 VGPRs, 16 waves);
    blu_classify_tasks picks one per table.  Whichever runs, the records are the oracle's: each build is forced
    (BLU_STREAM_KIND) onto a uniform 50-hit table, a tie-heavy one, a ragged one and a Zipf one — i.e. also onto the tables
    the classification would have given to the other build — in the packed, milli-percent and f64 layouts."""
    monkeypatch.setenv("BLU_STREAM_KIND", kind)
    tax = synth.make_taxonomy(5000, 77)
    t = _engine_tax(tax, "custom", H.CUSTOM_16S)
    tables = [synth.make_hits(tax, 4000, 78, 50, p_unmatched=0.002).numpy(),
              synth.make_hits(tax, 3000, 79, 50, top_group="zymo").numpy(),
              synth.make_hits(tax, 2500, 80, None, zipf=(1.1, 1, 3000)).numpy()]
    base = synth.make_hits(tax, 64 * 20, 81, 300).numpy()
    rng = np.random.default_rng(82)
    lens = np.minimum(rng.integers(1, 301, 64 * 20), np.repeat(rng.choice([16, 32, 64, 128, 256, 300], 20), 64))
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    take = np.concatenate([np.arange(l) + 300 * i for i, l in enumerate(lens)])
    tables.append({k: (base[k][take] if k != "seg_off" else seg) for k in base})
    for h in tables:
        rows = t.engine_rows(h["tax_row"])
        pm = np.round(h["pident"] * 1000).astype(np.uint32)
        h = dict(h, pident=pm / 1000.0)
        for strategy in ("relaxed", "cautious"):
            exp = H.columnar(tax, h, "custom", strategy, H.CUSTOM_16S, threads=8)
            _assert_records_equal(engine.run_consensus_host(t, h["seg_off"], h["bitscore"], rows, h["pident"], h["align_len"], h["acc_rank"], strategy=strategy), exp)
            for packed in (False, True):
                got = engine.run_consensus_host(t, h["seg_off"], h["bitscore"], rows, None, h["align_len"], h["acc_rank"], strategy=strategy,
                                                pident_milli=pm, packed=packed)
                _assert_records_equal(got, exp)


@pytest.mark.parametrize("top_group", ["all", "zymo"])
def test_flat_pass_with_a_list_that_fills_up(top_group, monkeypatch):
    """The flat pass of the kernel without the ring (units of 8 rows dealt to the lanes, two sub-passes, lane descriptors +
    gather) on tables that push it through its corners: mixed segment lengths of 1..600 rows whose top groups are whole
    segments ("all": the list fills up inside a step, queries come again in the next round, top groups larger than the list
    end on the worklist, segments over 512 rows go there directly) or follow the reference's real histogram ("zymo")."""
    monkeypatch.setenv("BLU_STREAM_KIND", "noring")
    tax = synth.make_taxonomy(3000, 91)
    t = _engine_tax(tax, "custom", H.CUSTOM_16S)
    h = synth.make_hits(tax, 2200, 92, None, zipf=(0.7, 1, 600), top_group=top_group, p_unmatched=0.001).numpy()
    rows = t.engine_rows(h["tax_row"])
    pm = np.round(h["pident"] * 1000).astype(np.uint32)
    h = dict(h, pident=pm / 1000.0)
    lens = np.diff(h["seg_off"].astype(np.int64))
    assert (lens > 512).any() and ((lens > 256) & (lens <= 512)).any() and (lens <= 8).any()
    for strategy in ("relaxed", "cautious"):
        exp = H.columnar(tax, h, "custom", strategy, H.CUSTOM_16S, threads=8)
        for packed in (False, True):
            got = engine.run_consensus_host(t, h["seg_off"], h["bitscore"], rows, None, h["align_len"], h["acc_rank"], strategy=strategy,
                                            pident_milli=pm, packed=packed)
            _assert_records_equal(got, exp)
        _assert_records_equal(engine.run_consensus_host(t, h["seg_off"], h["bitscore"], rows, h["pident"], h["align_len"], h["acc_rank"], strategy=strategy), exp)


@pytest.mark.parametrize("kind", ["ring", "noring"])
def test_reported_levels_beyond_the_node_ids_kept_in_registers(kind, monkeypatch):
    """Phase 2c keeps the node ids of the first 12 levels of the reference row in registers (packed relaxed ring build) or
    none at all (the other builds) and reads a deeper reported level's id back from the row: deep lineages on a uniform
    50-hit table, every layout, both strategies, both builds of the stream kernel, against the oracle — with reported levels
    on both sides of the 12."""
    monkeypatch.setenv("BLU_STREAM_KIND", kind)
    tax = synth.make_taxonomy(6000, 93, deep=True)
    t = _engine_tax(tax, "custom", H.CUSTOM_16S)
    h = synth.make_hits(tax, 3000, 94, 50, p_unmatched=0.001).numpy()
    rows = t.engine_rows(h["tax_row"])
    pm = np.round(h["pident"] * 1000).astype(np.uint32)
    h = dict(h, pident=pm / 1000.0)
    for strategy in ("relaxed", "cautious"):
        exp = H.columnar(tax, h, "custom", strategy, H.CUSTOM_16S, threads=8)
        ok = exp["status"] <= 1
        last = np.array([int(m).bit_length() - 1 for m in exp["level_mask"][ok]])
        assert (last >= 12).sum() > 50 and (last < 12).sum() > 50, (int((last >= 12).sum()), int((last < 12).sum()))
        _assert_records_equal(engine.run_consensus_host(t, h["seg_off"], h["bitscore"], rows, h["pident"], h["align_len"], h["acc_rank"], strategy=strategy), exp)
        for packed in (False, True, "wide"):
            got = engine.run_consensus_host(t, h["seg_off"], h["bitscore"], rows, None if packed != "wide" else h["pident"], h["align_len"], h["acc_rank"],
                                            strategy=strategy, pident_milli=pm if packed != "wide" else None, packed=packed)
            _assert_records_equal(got, exp)


def test_a_queue_that_turns_up_after_an_empty_one_is_still_worked_off():
    """The call after a run that left the worklist empty launches no worklist kernel (a kernel boundary is a tenth of a C4
    slice).  If the same buffers then hold a table WITH long segments, the stream kernel's last block drains the queue
    itself: same records as the oracle, on that call and on the ones after it (which launch the worklist kernel again)."""
    import torch
    tax = synth.make_taxonomy(4000, 17)
    t = _engine_tax(tax, "custom", H.CUSTOM_16S)
    nq = 6000
    a = synth.make_hits(tax, nq, 5, 50, device="cuda")                         # no segment over 512 rows: empty queue
    # table B in the same number of rows: 40 queries of 1500 / 700 rows, the others share what is left
    rng = np.random.default_rng(2)
    lens = np.full(nq, 1, dtype=np.int64)
    big = rng.choice(nq, 40, replace=False)
    lens[big] = rng.choice([700, 1500], 40)
    rest = a.n_hits - int(lens.sum())
    small = np.setdiff1d(np.arange(nq), big)
    lens[small] += rng.multinomial(rest, np.ones(len(small)) / len(small))
    assert int(lens.sum()) == a.n_hits and lens.max() <= 1500 + 200
    seg_b = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    dev = a.as_dict("milli")
    dev["tax_row"] = t.engine_rows(dev["tax_row"]).contiguous()
    desc_rows = a.numpy()["tax_row"]
    out = torch.zeros(32 * nq, dtype=torch.uint8, device="cuda")
    h = a.numpy()
    h["pident"] = a.pident_milli.cpu().numpy().astype(np.float64) / 1000.0
    exp_a = H.columnar(tax, h, "custom", "relaxed", H.CUSTOM_16S)
    for _ in range(3):                                                           # classify, then the remembered kind, no worklist kernel
        engine.run_consensus_device(t, dev, out, strategy="relaxed")
        torch.cuda.synchronize()
        _assert_records_equal(engine.records_from_tensor(out), exp_a)
    dev["seg_off"].copy_(torch.from_numpy(seg_b).to("cuda"))                     # same buffers, another table
    hb = dict(h, seg_off=seg_b.astype(np.uint64))
    hb["tax_row"] = desc_rows
    exp_b = H.columnar(tax, hb, "custom", "relaxed", H.CUSTOM_16S)
    assert int((np.diff(seg_b) > 512).sum()) == 40
    for _ in range(3):
        out.zero_()
        engine.run_consensus_device(t, dev, out, strategy="relaxed")
        torch.cuda.synchronize()
        _assert_records_equal(engine.records_from_tensor(out), exp_b)


@pytest.mark.parametrize("hits", [10, 50])
def test_f64_identities_exact_milli_in_some_tasks_only(hits):
    """f64 layouts (five columns, 24-byte side records): a wave task whose top-row identities are all exact milli-percent
    values is ordered on the integers, any other one on the doubles — blocks of 64 queries of either kind side by side, and
    tasks with a single inexact value (one more decimal, a value one ulp off a milli-percent value, 131.07 and up)."""
    tax = synth.make_taxonomy(3000, 5)
    t = _engine_tax(tax, "custom", H.CUSTOM_16S)
    dh = synth.make_hits(tax, 64 * 24, 700 + hits, hits, p_unmatched=0.001)
    h = dh.numpy()
    rng = np.random.default_rng(hits)
    pid = h["pident"].copy()
    seg = h["seg_off"].astype(np.int64)
    for task in range(24):
        a, b = int(seg[64 * task]), int(seg[64 * (task + 1)])
        kind = task % 4
        if kind == 1:                                   # every value off the milli-percent grid
            pid[a:b] = pid[a:b] + 0.0001234
        elif kind == 2:                                 # one value of the task one ulp above a milli-percent value
            i = a + int(rng.integers(0, b - a))
            pid[i] = np.nextafter(pid[i], 200.0)
        elif kind == 3:                                 # values the 17-bit key cannot hold
            pid[a:b:7] = rng.choice(np.array([131.07, 131.071, 250.0]), len(pid[a:b:7]))
    h["pident"] = pid
    rows = t.engine_rows(h["tax_row"])
    for strategy in ("relaxed", "cautious"):
        exp = H.columnar(tax, h, "custom", strategy, H.CUSTOM_16S)
        _assert_records_equal(_run_host(t, h, strategy), exp)
        got = engine.run_consensus_host(t, h["seg_off"], h["bitscore"], rows, h["pident"], h["align_len"], h["acc_rank"], strategy, packed="wide")
        _assert_records_equal(got, exp)


def test_hits_pack_on_the_device_writes_the_host_packs_words():
    """blu_hits_pack / blu_hits_pack64 with device pointers (the kernels of pack_kernel.hip) against the host loop."""
    import torch
    tax = synth.make_taxonomy(4000, 29)
    t = _engine_tax(tax, "bacteria")
    dh = synth.make_hits(tax, 3000, 41, 20, device="cuda", p_unmatched=0.01)
    dh.tax_row = t.engine_rows(dh.tax_row).contiguous()
    h = {k: v.cpu().numpy() for k, v in dh.as_dict("milli").items()}
    for layout, wide in (("packed", False), ("packed64", True)):
        dev = dh.as_dict(layout, tax=t)[layout].cpu().numpy().view(np.uint32).reshape(-1, 6 if wide else 4)
        host = engine.pack_records(t, h["tax_row"], None if wide else h["pident_milli"], h["align_len"], h["acc_rank"],
                                   pident=dh.pident.cpu().numpy() if wide else None, wide=wide)
        assert np.array_equal(dev, host), layout
    bad = dh.as_dict("milli")
    bad["pident_milli"] = bad["pident_milli"].clone()
    bad["pident_milli"][17] = 131071
    with pytest.raises(N.BluError, match="milli-percent"):
        engine.pack_hits_device(t, bad)
