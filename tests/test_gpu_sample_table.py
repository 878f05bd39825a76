"""Per-sample taxon table counted on the GPU: `build-consensus --sample-table` against the restatement
(tests/sample_table_reference.py) applied to the reference's own pooled document and to the document the same run wrote,
and blu_consensus_sample_table against a numpy aggregate of the records it was given."""
import gzip
import json
import os

import numpy as np
import pytest
import torch

from blutils_amd import _native as N
from blutils_amd import cli, engine, pipeline, report, synth, tabular
from tests import report_reference as rref
from tests import sample_table_reference as ref

pytestmark = pytest.mark.gpu


def _golden_inputs(tmp_path, taxa, names):
    """tests/golden_recipe.py's reconstruction: one row per bean occurrence, one query per golden taxon (as
    tests/test_gpu_report.py writes it)."""
    lineages, rows = {}, []
    for name, t in zip(names, taxa):
        for bean in t["consensusBeans"]:
            taxid = lineages.setdefault(bean["taxonomy"], 1000 + len(lineages))
            for k in range(int(bean["occurrences"])):
                a = bean["accessions"][min(k, len(bean["accessions"]) - 1)]
                rows.append(f"{name}\t{a}\t{taxid}\t{t['percIdentity']:.3f}\t{400 + k}\t0\t0\t1\t400\t1\t400\t1e-50\t{int(t['bitScore'])}")
    (tmp_path / "b.tsv").write_text("\n".join(rows) + "\n")
    (tmp_path / "t.json").write_text(json.dumps({"blutilsVersion": "7.1.3", "sourceDatabase": "golden", "taxonomies": [
        {"taxid": v, "rank": "", "numericLineage": k, "textLineage": k, "accessions": []} for k, v in lineages.items()]}))
    return str(tmp_path / "b.tsv"), str(tmp_path / "t.json")


def _label(q):
    """many samples, both label forms"""
    s = q // 97
    return f"S{s}.{q}" + (f"_size_{q % 7}" if q % 2 else "") if s % 3 else f"q{q};size={q % 5};sample=X{s % 11}"


def _synth_inputs(tmp_path, n_tax=400, n_q=3000, seed=5, p_unmatched=0.002):
    tax = synth.make_taxonomy(n_tax, seed)
    hits = synth.make_hits(tax, n_q, seed, 6, p_unmatched=p_unmatched).numpy()
    db = {"blutilsVersion": "8.3.1", "sourceDatabase": "synthetic", "taxonomies": [
        {"taxid": int(tax.taxid[t]), "rank": "species", "numericLineage": num, "textLineage": text, "accessions": []}
        for t, (num, text) in enumerate(zip(tax.lineage_strings(text=False), tax.lineage_strings(text=True)))]}
    (tmp_path / "t.json").write_text(json.dumps(db))
    seg, acc = hits["seg_off"], hits["acc_rank"].view(np.uint32)
    rows = []
    for q in range(n_q):
        name = _label(q)
        for i in range(int(seg[q]), int(seg[q + 1])):
            t = int(hits["tax_row"][i])
            taxid = int(tax.taxid[t]) if t >= 0 else 999999999
            rows.append(f'{name}\tNR_{int(acc[i]):010d}.1\t{taxid}\t{hits["pident"][i]:.3f}\t{int(hits["align_len"][i])}'
                        f'\t3\t1\t1\t400\t5\t404\t1e-120\t{int(hits["bitscore"][i])}')
    (tmp_path / "b.tsv").write_text("\n".join(rows) + "\n")
    return str(tmp_path / "b.tsv"), str(tmp_path / "t.json")


def _run(tmp_path, bt, tj, taxon="bacteria", strategy="relaxed", use_taxid=False, custom=None, weight="one", lenient=True,
         fmt="json", headers=None):
    doc, rep, tab = str(tmp_path / f"doc.{fmt}"), str(tmp_path / "report.tsv"), str(tmp_path / "table.tsv")
    for p in (rep, tab):
        if os.path.exists(p):
            os.remove(p)
    pipeline.build_consensus_identities_with_tables(bt, tj, taxon, strategy, use_taxid, custom, headers=headers, out_format=fmt,
                                                    lenient=lenient, out_path=doc, report_path=rep, sample_table_path=tab,
                                                    report_weight=weight)
    results = tabular.load_content(doc, fmt)["results"] if fmt != "jsonl" else \
        [json.loads(l) for l in open(doc).read().splitlines()[1:]]
    return results, open(rep).read(), open(tab).read()


def _zymo(golden_dir):
    with gzip.open(os.path.join(golden_dir, "zymo_mock_distilled.json.gz"), "rt") as f:
        cases = json.load(f)["cases"]
    with gzip.open(os.path.join(golden_dir, "zymo_mock_queries.json.gz"), "rt") as f:
        rows = json.load(f)["results"]
    return cases, rows


@pytest.mark.parametrize("host_columns", [False, True])
def test_zymo_reference_document_pinned(tmp_path, golden_dir, monkeypatch, host_columns):
    if host_columns:
        monkeypatch.setenv("BLU_PIPELINE_HOST_COLUMNS", "1")
    cases, rows = _zymo(golden_dir)
    theirs = [{"query": q, "taxon": None if i is None else cases[i]["taxon"]} for q, i in rows]
    cls = [(q, i) for q, i in rows if i is not None]
    bt, tj = _golden_inputs(tmp_path, [cases[i]["taxon"] for _, i in cls], [q for q, _ in cls])
    headers = [q for q, i in rows if i is None]
    for strategy in ("relaxed", "cautious"):
        for weight in ("one", "size"):
            results, rep, tab = _run(tmp_path, bt, tj, strategy=strategy, weight=weight, lenient=False, headers=headers)
            assert len(results) == 3626
            assert tab == ref.table(theirs, weight)           # the reference's own document, not only this run's
            assert tab == ref.table(results, weight)
            assert rep == rref.report(results, weight)
    lines = [l.split("\t") for l in ref.table(theirs, "one").splitlines()]
    assert lines[1][3:] == ["1343", "0", "0", "116", "349", "116", "97", "246", "115", "304"]


@pytest.mark.parametrize("host_columns", [False, True])
def test_synthetic_tables_strategies_taxid_cutoffs_and_panics(tmp_path, golden_dir, monkeypatch, host_columns):
    if host_columns:
        monkeypatch.setenv("BLU_PIPELINE_HOST_COLUMNS", "1")
    bt, tj = _synth_inputs(tmp_path)
    vals = json.load(open(os.path.join(golden_dir, "custom_taxon_cutoffs_bacteria_16S.json")))["values"]
    headers = [f"Hdr.{i}_size_{i + 2}" for i in range(3)] + ["y;sample=S1"]
    seen_null = 0
    for strategy in ("relaxed", "cautious"):
        for use_taxid in (False, True):
            for taxon, custom in (("bacteria", None), ("custom", vals)):
                for weight in ("one", "size"):
                    results, rep, tab = _run(tmp_path, bt, tj, taxon, strategy, use_taxid, custom, weight=weight,
                                             fmt="jsonl" if use_taxid else "json", headers=headers)
                    assert tab == ref.table(results, weight)
                    assert rep == rref.report(results, weight)
                    # the total column is the report's clade column, line for line
                    assert [l.split("\t")[3] for l in tab.splitlines()[1:]] == [l.split("\t")[1] for l in rep.splitlines()[1:]]
                    seen_null += sum(r["taxon"] is None for r in results)
    assert seen_null > 0
    assert len(tab.splitlines()[0].split("\t")) - 4 > 30
    # strict mode: the reference panics on these tables; no file is left behind
    for p in ("s.json", "r.tsv", "t.tsv"):
        assert not (tmp_path / p).exists()
    with pytest.raises(N.BluError) as e:
        pipeline.build_consensus_identities_with_tables(bt, tj, "bacteria", "relaxed", out_path=str(tmp_path / "s.json"),
                                                        report_path=str(tmp_path / "r.tsv"),
                                                        sample_table_path=str(tmp_path / "t.tsv"))
    assert e.value.code == pipeline.BLU_ERR_REFERENCE_PANIC
    for p in ("s.json", "r.tsv", "t.tsv"):
        assert not (tmp_path / p).exists()


def test_cli_flag_leaves_the_document_as_it_is_and_a_name_without_sample_fails(tmp_path, golden_dir):
    cases, rows = _zymo(golden_dir)
    cls = [(q, i) for q, i in rows if i is not None]
    bt, tj = _golden_inputs(tmp_path, [cases[i]["taxon"] for _, i in cls], [q for q, _ in cls])
    a, b, tab = tmp_path / "a.json", tmp_path / "b.json", tmp_path / "t.tsv"
    base = ["blastn", "build-consensus", bt, "-t", tj, "--taxon", "bacteria", "--strategy", "cautious"]
    assert cli.main(base + ["--blutils-out-file", str(a)]) == 0
    assert cli.main(base + ["--blutils-out-file", str(b), "--sample-table", str(tab), "--report-weight", "size"]) == 0
    da, db = json.load(open(a)), json.load(open(b))
    rid_a, rid_b = da["results"][0]["runId"], db["results"][0]["runId"]
    assert a.read_text().replace(rid_a, "R") == b.read_text().replace(rid_b, "R")
    assert tab.read_text() == ref.table(db["results"], "size")
    # one query that names no sample: the call fails naming it, and writes nothing
    text = open(bt).read().replace(cls[1234][0] + "\t", "orphan_1234\t")
    (tmp_path / "bad.tsv").write_text(text)
    out, rep, t2 = tmp_path / "o.json", tmp_path / "r2.tsv", tmp_path / "t2.tsv"
    with pytest.raises(N.BluError, match="orphan_1234") as e:
        cli.main(["blastn", "build-consensus", str(tmp_path / "bad.tsv"), "-t", tj, "--taxon", "bacteria", "--strategy",
                  "cautious", "--blutils-out-file", str(out), "--report", str(rep), "--sample-table", str(t2)])
    assert e.value.code == N.BLU_ERR_INVALID_ARG
    assert not out.exists() and not rep.exists() and not t2.exists()


# ---- engine level: blu_consensus_sample_table --------------------------------------------------------------------------

U32_MAX = (1 << 32) - 1


def _cells(paths_of, recs, sample, weights):
    """{(node tuple, sample): clade}, unclassified[s], unplaced[s] in Python integers; paths_of(desc rows, masks) ->
    node tuples."""
    w = np.ones(len(recs), np.uint64) if weights is None else weights.astype(np.uint64)
    ns = int(sample.max()) + 1 if len(sample) else 0
    cls = recs["status"] < 2
    unc = np.zeros(ns, np.uint64)
    np.add.at(unc, sample[~cls], w[~cls])
    desc, mask = paths_of(cls)
    key = np.stack([desc.astype(np.uint64), mask, sample[cls].astype(np.uint64)], axis=1)
    uniq, inv = np.unique(key, axis=0, return_inverse=True)
    sums = np.zeros(len(uniq), np.uint64)
    np.add.at(sums, inv.ravel(), w[cls])
    unp = [0] * ns
    cells = {}
    node_cache = {}
    for (d, m, s), v in zip(uniq.tolist(), sums.tolist()):
        p = node_cache.get((d, m))
        if p is None:
            p = node_cache[(d, m)] = paths_of.nodes(d, m)
        if not p:
            unp[s] += v
            continue
        for k in range(1, len(p) + 1):
            if v:
                cells[(p[:k], s)] = cells.get((p[:k], s), 0) + v
    return cells, [int(x) for x in unc], unp


def _as_cells(tab):
    P, C = tab["paths"], tab["cells"]
    full = []
    for i in range(len(P)):
        par = int(P["parent"][i])
        assert par == report.NO_PARENT or par < i
        full.append((full[par] if par != report.NO_PARENT else ()) + (int(P["node"][i]),))
    assert len(set(full)) == len(full)
    keys = list(zip(C["path"].tolist(), C["sample"].tolist()))
    assert keys == sorted(keys)                                     # sorted by (path, sample)
    assert (C["clade"] > 0).all()
    out = {(full[p], s): int(c) for (p, s), c in zip(keys, C["clade"].tolist())}
    per_path = np.zeros(len(full), dtype=object)
    for (p, _), c in zip(keys, C["clade"].tolist()):
        per_path[p] += int(c)
    assert [int(x) for x in per_path] == [int(x) for x in P["clade"]]   # a path's clade: the sum of its cells
    return out, full


class _EnginePaths:
    def __init__(self, tax, t, recs, rows):
        self.tax, self.recs = tax, recs
        _, inv = t.row_map()
        self.desc_all = inv[(rows & ((1 << 25) - 1)).astype(np.int64)].astype(np.int64)
        self.lens = (tax.lin_off[1:] - tax.lin_off[:-1]).astype(np.int64)

    def __call__(self, cls):
        d = self.desc_all[cls]
        m = self.recs["level_mask"][cls] & ((np.uint64(1) << self.lens[d].astype(np.uint64)) - np.uint64(1))
        return d, m

    def nodes(self, d, m):
        o = int(self.tax.lin_off[d])
        return tuple(int(self.tax.lin_node[o + j]) for j in range(int(self.lens[d])) if (m >> j) & 1)


def _engine_run(n_tax, n_q, seed, few=0, hpq=3):
    tax = synth.make_taxonomy(n_tax, seed)
    t = engine.Taxonomy(tax.lin_off, tax.lin_node, tax.lin_rank, tax.rank_names, taxon="bacteria", device=0)
    dh = synth.make_hits(tax, n_q, seed, hpq, device="cuda:0", p_unmatched=0.001)
    rows = t.engine_rows(dh.tax_row)
    if few:
        pick = torch.tensor(t.row_map()[0][np.linspace(0, n_tax - 1, few).astype(np.int64)].astype(np.int64), device="cuda:0")
        matched = rows != -1
        rows = torch.where(matched, pick[(dh.bitscore.to(torch.int64) % few)].to(torch.int32), rows)
    dh.tax_row = rows.contiguous()
    out = torch.zeros(32 * n_q, dtype=torch.uint8, device="cuda:0")
    engine.run_consensus_device(t, dh.as_dict(), out, strategy="relaxed")
    torch.cuda.synchronize()
    return tax, t, dh, out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def test_engine_device_and_host_pointers_agree_with_numpy():
    tax, t, dh, out = _engine_run(3000, 200_000, 11)
    recs = engine.records_from_tensor(out)
    rows_all = dh.tax_row.cpu().numpy().view(np.uint32)
    rows = np.where(recs["status"] < 2, rows_all[np.minimum(recs["ref_row"], len(rows_all) - 1)], 0)
    rng = np.random.default_rng(3)
    sample = np.sort(rng.integers(0, 37, dh.n_queries)).astype(np.uint32)
    weights = (np.arange(dh.n_queries, dtype=np.uint64) * 2654435761 % 7).astype(np.uint32)
    for w in (None, weights):
        dev = report.consensus_sample_table(t, dh.tax_row, out, dh.n_hits, _dev(sample), 40,
                                            weights=None if w is None else _dev(w))
        host = report.consensus_sample_table(t, rows_all, recs, dh.n_hits, sample, 40, weights=w)
        a, fa = _as_cells(dev)
        b, fb = _as_cells(host)
        assert a == b and sorted(fa) == sorted(fb)
        for k in ("unclassified", "unplaced"):
            assert (dev[k] == host[k]).all()
        cells, unc, unp = _cells(_EnginePaths(tax, t, recs, rows), recs, sample, w)
        assert a == cells
        assert dev["unclassified"][:37].tolist() == unc and dev["unplaced"][:37].tolist() == unp
        assert dev["unclassified"][37:].tolist() == [0, 0, 0]
        # the paths are the report's, with its numbers
        rep = report.consensus_report(t, dh.tax_row, out, dh.n_hits, weights=None if w is None else _dev(w))
        got = {p: (int(dev["paths"]["direct"][i]), int(dev["paths"]["clade"][i])) for i, p in enumerate(fa)}
        full = []
        for i in range(len(rep["paths"])):
            par = int(rep["paths"]["parent"][i])
            full.append((full[par] if par != report.NO_PARENT else ()) + (int(rep["paths"]["node"][i]),))
        assert got == {p: (int(rep["paths"]["direct"][i]), int(rep["paths"]["clade"][i])) for i, p in enumerate(full)}
    packed64 = engine.pack_hits_device(t, dh.as_dict(), wide=True)
    rp = report.consensus_sample_table(t, packed64, out, dh.n_hits, _dev(sample), 40, packed="packed64")
    assert _as_cells(rp)[0] == _as_cells(report.consensus_sample_table(t, dh.tax_row, out, dh.n_hits, _dev(sample), 40))[0]


@pytest.mark.parametrize("order", ["contiguous", "random"])
def test_engine_ten_million_queries(order):
    tax, t, dh, out = _engine_run(20_000, 10_000_000, 23, few=10, hpq=2)
    recs = engine.records_from_tensor(out)
    rows_all = dh.tax_row.cpu().numpy().view(np.uint32)
    rows = np.where(recs["status"] < 2, rows_all[np.minimum(recs["ref_row"], len(rows_all) - 1)], 0)
    n = dh.n_queries
    if order == "contiguous":
        sample = (np.arange(n, dtype=np.uint64) * 100 // n).astype(np.uint32)
    else:
        sample = np.random.default_rng(9).integers(0, 100, n).astype(np.uint32)
    tab = report.consensus_sample_table(t, dh.tax_row, out, dh.n_hits, _dev(sample), 100)
    cells, unc, unp = _cells(_EnginePaths(tax, t, recs, rows), recs, sample, None)
    assert _as_cells(tab)[0] == cells
    assert tab["unclassified"].tolist() == unc and tab["unplaced"].tolist() == unp
    first = sum(int(c) for c, par in zip(tab["paths"]["clade"], tab["paths"]["parent"]) if par == report.NO_PARENT)
    assert first + sum(unc) + sum(unp) == n


def _hand_taxonomy(lineages):
    lens = np.array([len(l) for l in lineages], np.uint64)
    lin_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    lin_node = np.concatenate([np.asarray(l, np.uint32) for l in lineages])
    lin_rank = np.full(len(lin_node), synth.RANK_NAMES.index("clade"), np.uint16)
    t = engine.Taxonomy(lin_off, lin_node, lin_rank, synth.RANK_NAMES, taxon="bacteria", device=0)
    return t, t.row_map()[0].copy()


def _records(n):
    recs = np.zeros(n, engine.RESULT_DTYPE)
    recs["ref_row"] = U32_MAX
    return recs


class _HandPaths:
    def __init__(self, lineages, recs):
        self.lineages, self.recs = lineages, recs
        self.lens = np.array([len(l) for l in lineages], np.uint64)

    def __call__(self, cls):
        d = self.recs["ref_row"][cls].astype(np.int64)
        ln = self.lens[d]
        full = np.uint64(U32_MAX) << np.uint64(32) | np.uint64(U32_MAX)
        low = np.where(ln >= 64, full, (np.uint64(1) << np.minimum(ln, 63)) - np.uint64(1))
        return d, self.recs["level_mask"][cls] & low

    def nodes(self, d, m):
        return tuple(int(node) for j, node in enumerate(self.lineages[d]) if (m >> j) & 1)


def _check_hand(lineages, t, fwd, recs, sample, n_samples, weights):
    dev = report.consensus_sample_table(t, _dev(fwd), torch.from_numpy(recs.view(np.uint8)).to("cuda:0"), len(fwd),
                                        _dev(sample), n_samples, weights=None if weights is None else _dev(weights))
    host = report.consensus_sample_table(t, fwd, recs, len(fwd), sample, n_samples, weights=weights)
    for k in ("attempts", "table_slots"):
        assert dev[k] == host[k]
    cells, unc, unp = _cells(_HandPaths(lineages, recs), recs, sample, weights)
    for tab in (dev, host):
        assert _as_cells(tab)[0] == cells
        assert tab["unclassified"][:len(unc)].tolist() == unc and tab["unplaced"][:len(unp)].tolist() == unp
    return dev, cells


def test_engine_rebuilds_the_tables_from_the_bound():
    rng = np.random.default_rng(40)
    lineages = [[1] + [100 * (i + 1) + j for j in range(39)] for i in range(6)]
    t, fwd = _hand_taxonomy(lineages)
    nq = 100_000
    recs = _records(nq)
    recs["status"] = rng.choice([0, 1, 2, 3], nq, p=[0.6, 0.3, 0.05, 0.05])
    recs["ref_row"] = np.where(recs["status"] < 2, rng.integers(0, len(lineages), nq), U32_MAX)
    levels = (rng.random((nq, 40)) < 0.2).astype(np.uint64) << np.arange(40, dtype=np.uint64)
    recs["level_mask"] = np.bitwise_or.reduce(levels, axis=1)
    sample = rng.integers(0, 50, nq).astype(np.uint32)
    weights = rng.integers(1, 6, nq).astype(np.uint32)
    tab, cells = _check_hand(lineages, t, fwd, recs, sample, 50, weights)
    assert tab["attempts"] == 2


def test_engine_cells_past_2_to_the_32_and_2_to_the_53():
    n_leaf = 256
    lineages = [[7, 20 + i // 64, 5000 + i] for i in range(n_leaf)]
    t, fwd = _hand_taxonomy(lineages)
    hot = (1 << 21) + 2048
    spread = 4 * 1024
    nq = hot + spread
    recs = _records(nq)
    recs["level_mask"] = 0b111
    recs["ref_row"][:hot] = 0
    recs["ref_row"][hot:] = np.arange(spread) % n_leaf
    sample = np.zeros(nq, np.uint32)
    sample[hot:] = np.arange(spread) % 3 + 2
    weights = np.full(nq, U32_MAX, np.uint32)
    tab, cells = _check_hand(lineages, t, fwd, recs, sample, 5, weights)
    assert cells[((7, 20, 5000), 0)] > 1 << 53 and cells[((7,), 0)] > 1 << 53
    assert any((1 << 32) < v < (1 << 40) for v in cells.values())


def test_engine_64_level_lineages():
    rng = np.random.default_rng(64)
    lineages = [[1] + [1000 * (i + 1) + j for j in range(63)] for i in range(3)]
    lineages += [[1] + [9000 + 100 * i + j for j in range(n - 1)] for i, n in enumerate((10, 33, 63))]
    t, fwd = _hand_taxonomy(lineages)
    nq = 20_000
    recs = _records(nq)
    recs["status"] = rng.choice([0, 1, 2, 3, 16], nq, p=[0.5, 0.3, 0.1, 0.05, 0.05])
    cls = recs["status"] < 2
    recs["ref_row"][cls] = rng.integers(0, len(lineages), int(cls.sum()))
    recs["level_mask"] = rng.integers(0, 1 << 64, nq, dtype=np.uint64, endpoint=False)
    recs["level_mask"][::7] = np.uint64((1 << 64) - 1)
    recs["level_mask"][::13] = 0
    sample = (np.arange(nq) // 700).astype(np.uint32)
    weights = rng.integers(0, 1 << 32, nq, dtype=np.uint64).astype(np.uint32)
    tab, cells = _check_hand(lineages, t, fwd, recs, sample, int(sample.max()) + 1, weights)
    assert any(len(p) == 64 for p, _ in cells)
    assert sum(tab["unplaced"]) > 0 and sum(tab["unclassified"]) > 0


def test_engine_bad_sample_id_is_an_error_naming_the_query():
    lineages = [[1, 2, 3], [1, 2, 4]]
    t, fwd = _hand_taxonomy(lineages)
    recs = _records(3000)
    recs["ref_row"] = np.arange(3000) % 2
    recs["level_mask"] = 0b111
    sample = (np.arange(3000) % 4).astype(np.uint32)
    bad = 2047
    sample[bad] = 4
    for side in ("device", "host"):
        args = (_dev(fwd), torch.from_numpy(recs.view(np.uint8)).to("cuda:0"), _dev(sample)) if side == "device" else \
            (fwd, recs, sample)
        with pytest.raises(N.BluError, match=f"query {bad} ") as e:
            report.consensus_sample_table(t, args[0], args[1], len(fwd), args[2], 4)
        assert e.value.code == N.BLU_ERR_INVALID_ARG
