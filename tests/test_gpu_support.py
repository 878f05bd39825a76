"""Per-query assignment support counted on the GPU: blu_consensus_support against the restatement
(tests/support_reference.py) applied to the engine's own records, on synthetic and hand-built tables, in every layout and
through both pointer routes; `build-consensus --support-table` against the renderer applied to the document the run wrote,
the ingest's columns and the engine's records on them."""
import gzip
import json
import os
import stat
import sys

import numpy as np
import pytest
import torch

from blutils_amd import _native as N
from blutils_amd import cli, engine, pipeline, synth, tabular
from oracle import oracle as orc
from tests import support_reference as ref

pytestmark = pytest.mark.gpu

U32_MAX = (1 << 32) - 1
POS_MASK = (1 << 25) - 1


def _assert_fields(got, exp, what=""):
    assert len(got) == len(exp)
    for f in ref.SUPPORT_FIELDS:
        bad = np.nonzero(got[f].astype(np.int64) != exp[f])[0]
        assert len(bad) == 0, (what, f, bad[:5], got[bad[:5]], exp[bad[:5]])


def _assert_invariants(fields, recs):
    f = {k: fields[k].astype(np.int64) for k in ref.SUPPORT_FIELDS}
    assert (f["n_support"] <= f["n_matched"]).all() and (f["n_matched"] <= f["n_hits"]).all()
    assert (f["n_top_support"] <= f["n_top"]).all() and (f["n_top"] <= f["n_hits"]).all()
    placed = (recs["status"] < 2) & (recs["level_mask"] != 0)
    assert (f["n_top_support"][placed] >= 1).all()
    assert (f["n_top"][recs["status"] == 1] == 1).all()
    none = recs["status"] >= 2
    assert not f["n_top_support"][none].any() and not f["n_support"][none].any() and not f["support_bits"][none].any()
    empty = f["n_hits"] == 0
    for k in ref.SUPPORT_FIELDS:
        assert not f[k][empty].any()


# ---- kernel level: synthetic tables, every layout, both pointer routes ------------------------------------------------------

@pytest.mark.parametrize("strategy", ["relaxed", "cautious"])
def test_synthetic_tables_all_layouts_device_and_host(strategy):
    tax = synth.make_taxonomy(3000, 17)
    t = engine.Taxonomy(tax.lin_off, tax.lin_node, tax.lin_rank, tax.rank_names, taxon="bacteria", device=0)
    dh = synth.make_hits(tax, 6000, 17, None, zipf=(1.3, 1, 90), device="cuda:0", p_unmatched=0.02)
    desc = dh.tax_row.cpu().numpy().astype(np.int64)
    dh.tax_row = t.engine_rows(dh.tax_row).contiguous()
    lineages = ref.lineages_of(tax.lin_off, tax.lin_node)
    seg = dh.seg_off.cpu().numpy().astype(np.uint64)
    bs = dh.bitscore.cpu().numpy()
    exp = None
    for layout in ("f64", "milli", "packed", "packed64"):
        hits = dh.as_dict(layout, tax=t)
        out = torch.zeros(32 * dh.n_queries, dtype=torch.uint8, device="cuda:0")
        engine.run_consensus_device(t, hits, out, strategy=strategy)
        torch.cuda.synchronize()
        recs = engine.records_from_tensor(out)
        if exp is None:
            exp = ref.support(seg, bs, desc, lineages, None, recs)
            assert (recs["status"] < 2).sum() > 1000 and (exp["n_support"] < exp["n_matched"]).any()
        got = engine.support_device(t, hits, out)
        _assert_fields(got, exp, (layout, "device"))
        _assert_invariants(got, recs)
        if layout in ("packed", "packed64"):
            host = engine.support_host(t, seg, bs, None, recs, **{layout: hits[layout].cpu().numpy().view(np.uint32)})
        else:
            host = engine.support_host(t, seg, bs, dh.tax_row.cpu().numpy(), recs)
        assert host.tobytes() == got.tobytes(), layout


# ---- kernel level: hand-built tables -------------------------------------------------------------------------------------------

def _hand_taxonomy(lineages, bad=None):
    lens = np.array([len(l) for l in lineages], np.uint64)
    lin_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    lin_node = np.concatenate([np.asarray(l, np.uint32) for l in lineages])
    lin_rank = np.full(len(lin_node), synth.RANK_NAMES.index("clade"), np.uint16)
    t = engine.Taxonomy(lin_off, lin_node, lin_rank, synth.RANK_NAMES, taxon="bacteria", device=0, bad=bad)
    return t, t.row_map()[0].copy()


def _edge_lineages():
    """Every row under node 1 (a level-0 assignment is the whole table); by node order the first and the last row are known."""
    L = [[1, 2, 20]]                                                        # sorted first; a clade of one row at levels 1, 2
    L += [[1, 3, 30, 300 + i] for i in range(200)]                          # a wide node: 200 rows under [1, 3, 30]
    L += [[1, 3, 31, 600 + i] for i in range(70)]                           # (270 rows under [1, 3])
    L += [[1, 4, 40 + g, 4000 + 100 * g + s] for g in range(45) for s in range(100)]   # 4 500 rows under [1, 4]
    L += [[1, 6], [1, 6, 60], [1, 6, 60, 600], [1, 6, 60, 600], [1, 6, 61, 601]]       # prefixes of each other, one lineage twice
    L += [[1, 9, 90, 900]]                                                  # sorted last
    return L


def _edge_table(lineages, fwd, bad, rng, ref_rows):
    """Segments of the edge lengths for every reference row and every level of it, plus records without a clade.  The reference
    hit ties with the segment's maximum (status 0) or beats it (status 1), so the top-group invariants hold."""
    n_tax = len(lineages)
    lengths = [1, 63, 64, 65, 512, 513, 3000]
    seg, bs, desc, recs = [0], [], [], []
    ok_rows = np.array([t for t in range(n_tax) if not (bad is not None and bad[t])], np.int64)

    def add(n, status, r_row=None, mask=0, tie=False, scores=None):
        rows = rng.choice(ok_rows, n) if n else np.zeros(0, np.int64)
        rows = np.where(rng.random(n) < 0.4, rng.integers(0, n_tax, n), rows)       # (bad rows too)
        if r_row is not None and n > 1:                                             # some of the reference row's neighbours
            near = np.clip(r_row + rng.integers(-3, 4, n), 0, n_tax - 1)
            rows = np.where(rng.random(n) < 0.3, near, rows)
        rows = np.where(rng.random(n) < 0.1, -1, rows)
        sc = np.full(n, 77, np.int64) if tie else rng.choice(scores if scores is not None else [-40, -1, 0, 0, 5, 5, 900], n)
        rec = np.zeros(1, engine.RESULT_DTYPE)
        rec["status"], rec["level_mask"], rec["ref_row"] = status, mask, U32_MAX
        if status < 2:
            k = int(rng.integers(0, n))
            rows[k] = r_row
            sc[k] = sc.max() + (1 if status == 1 else 0)
            rec["ref_row"] = seg[-1] + k
        seg.append(seg[-1] + n)
        bs.extend(sc.tolist()); desc.extend(rows.tolist()); recs.append(rec)

    for r_row in ref_rows:
        for level in range(len(lineages[r_row])):
            for n in lengths:
                # the string may skip levels below its last one: any lower bits, the highest is what counts
                mask = (1 << level) | int(rng.integers(0, 1 << level)) if level else 1
                add(n, int(rng.integers(0, 2)), r_row, mask)
        add(64, 0, r_row, 0)                                                        # unplaced
        add(200, 0, r_row, (1 << len(lineages[r_row])) - 1, tie=True)               # every hit ties
        add(130, 1, r_row, 1, scores=[-9, -8, -8])                                  # negative scores only
    add(0, 2)                                                                       # empty segments
    add(0, 2)
    for st in (16, 17, 18, 19, 20):
        add(65, st)
    add(700, 16, tie=True)
    add(5, 2)
    seg = np.array(seg, np.uint64)
    desc = np.array(desc, np.int64)
    eng = np.where(desc < 0, N.BLU_UNMATCHED_TAXID, fwd[np.maximum(desc, 0)]).astype(np.uint32)
    return seg, np.array(bs, np.int32), desc, eng, np.concatenate(recs)


def _both_routes(t, seg, bs, eng, recs):
    hits = {"seg_off": torch.from_numpy(seg.view(np.int64)).to("cuda:0"), "bitscore": torch.from_numpy(bs).to("cuda:0"),
            "tax_row": torch.from_numpy(eng.view(np.int32)).to("cuda:0")}
    dev = engine.support_device(t, hits, torch.from_numpy(recs.view(np.uint8)).to("cuda:0"))
    host = engine.support_host(t, seg, bs, eng, recs)
    assert dev.tobytes() == host.tobytes()
    return dev


@pytest.mark.parametrize("with_bad", [False, True])
def test_hand_built_edges(with_bad):
    rng = np.random.default_rng(5 + with_bad)
    lineages = _edge_lineages()
    n_tax = len(lineages)
    bad = None
    if with_bad:
        bad = np.zeros(n_tax, np.uint8)
        bad[[7, 250, 1000, n_tax - 2]] = 1                                          # (n_tax - 2: [1, 6, 61, 601])
    t, fwd = _hand_taxonomy(lineages, bad)
    pos = fwd & POS_MASK
    first, last = 0, n_tax - 1
    if not with_bad:
        assert pos[first] == 0 and pos[last] == n_tax - 1                           # R at sorted position 0 and n_tax - 1
    dup = n_tax - 4                                                                 # [1, 6, 60, 600], listed twice
    assert lineages[dup] == lineages[dup + 1]
    ref_rows = [first, last, 1, 150, 200, 230, 271 + 37, 271 + 4499, n_tax - 6, n_tax - 5, dup, dup + 1]
    assert not with_bad or not bad[ref_rows].any()
    seg, bs, desc, eng, recs = _edge_table(lineages, fwd, bad, rng, ref_rows)
    got = _both_routes(t, seg, bs, eng, recs)
    exp = ref.support(seg, bs, desc, lineages, bad, recs)
    _assert_fields(got, exp)
    _assert_invariants(got, recs)
    # what the table was built to hold: a clade of one row, a wide one, thousands of rows, the whole table
    lens = (seg[1:] - seg[:-1]).astype(np.int64)
    assert set(lens.tolist()) >= {0, 1, 63, 64, 65, 512, 513, 3000}
    assert (exp["n_support"][lens == 3000] > 1500).any() and (exp["n_support"][lens == 3000] < 400).any()
    assert (exp["top_score"] < 0).any() and (exp["n_top"] == 200).any()
    whole = (recs["status"] < 2) & (recs["level_mask"] == 1)
    assert (exp["n_support"][whole] == exp["n_matched"][whole]).all()
    if with_bad:
        assert any(bad[d] for d in desc if d >= 0)


def test_one_taxon_table():
    t, fwd = _hand_taxonomy([[7, 8]])
    seg = np.array([0, 3, 3, 70], np.uint64)
    desc = np.array([0, -1, 0] + [0, -1] * 33 + [0], np.int64)
    bs = np.array([9, 9, 4] + [3] * 67, np.int32)
    eng = np.where(desc < 0, N.BLU_UNMATCHED_TAXID, fwd[0]).astype(np.uint32)
    recs = np.zeros(3, engine.RESULT_DTYPE)
    recs["status"] = [0, 2, 1]
    recs["ref_row"] = [0, U32_MAX, 3]
    recs["level_mask"] = [0b11, 0, 0b01]
    bs[3] = 5
    got = _both_routes(t, seg, bs, eng, recs)
    _assert_fields(got, ref.support(seg, bs, desc, [[7, 8]], None, recs))
    assert got["n_support"].tolist() == [2, 0, 34] and got["n_top"].tolist() == [2, 0, 1]


@pytest.mark.parametrize("how", ["unmatched_row", "row_out_of_range"])
def test_a_record_whose_reference_row_names_no_taxonomy_row(how):
    t, fwd = _hand_taxonomy([[1, 2, 3], [1, 2, 4]])
    eng = np.concatenate([np.tile(fwd, 1500), [N.BLU_UNMATCHED_TAXID]]).astype(np.uint32)
    nq = 3000
    seg = np.arange(nq + 1, dtype=np.uint64)
    seg[-1] = len(eng)
    bs = np.ones(len(eng), np.int32)
    recs = np.zeros(nq, engine.RESULT_DTYPE)
    recs["ref_row"] = np.arange(nq)
    recs["level_mask"] = 0b111
    bad = 2047
    recs["ref_row"][bad] = len(eng) - 1 if how == "unmatched_row" else len(eng) + 5
    for side in ("device", "host"):
        with pytest.raises(N.BluError, match=f"record {bad} ") as e:
            if side == "host":
                engine.support_host(t, seg, bs, eng, recs)
            else:
                engine.support_device(t, {"seg_off": torch.from_numpy(seg.view(np.int64)).to("cuda:0"),
                                          "bitscore": torch.from_numpy(bs).to("cuda:0"),
                                          "tax_row": torch.from_numpy(eng.view(np.int32)).to("cuda:0")},
                                      torch.from_numpy(recs.view(np.uint8)).to("cuda:0"))
        assert e.value.code == N.BLU_ERR_INVALID_ARG
    recs["status"][bad] = 2
    _both_routes(t, seg, bs, eng, recs)


# ---- pipeline level: build-consensus --support-table ---------------------------------------------------------------------------

def _synth_inputs(tmp_path, n_tax=400, n_q=1500, seed=5, p_unmatched=0.002, sample_names=False):
    tax = synth.make_taxonomy(n_tax, seed)
    hits = synth.make_hits(tax, n_q, seed, 6, p_unmatched=p_unmatched).numpy()
    db = {"blutilsVersion": "8.3.1", "sourceDatabase": "synthetic", "taxonomies": [
        {"taxid": int(tax.taxid[t]), "rank": "species", "numericLineage": num, "textLineage": text, "accessions": []}
        for t, (num, text) in enumerate(zip(tax.lineage_strings(text=False), tax.lineage_strings(text=True)))]}
    (tmp_path / "t.json").write_text(json.dumps(db))
    seg, acc = hits["seg_off"], hits["acc_rank"].view(np.uint32)
    rows = []
    for q in range(n_q):
        name = (f"smp{q % 3}.{q}" if sample_names else f"q{q:06d}") + (f";size={q % 9 + 1}" if sample_names else "")
        for i in range(int(seg[q]), int(seg[q + 1])):
            t = int(hits["tax_row"][i])
            taxid = int(tax.taxid[t]) if t >= 0 else 999999999
            rows.append(f'{name}\tNR_{int(acc[i]):010d}.1\t{taxid}\t{hits["pident"][i]:.3f}\t{int(hits["align_len"][i])}'
                        f'\t3\t1\t1\t400\t5\t404\t1e-120\t{int(hits["bitscore"][i])}')
    (tmp_path / "b.tsv").write_text("\n".join(rows) + "\n")
    return str(tmp_path / "b.tsv"), str(tmp_path / "t.json")


def _golden_inputs(tmp_path, taxa, names):
    """tests/golden_recipe.py's reconstruction: one row per bean occurrence, one query per golden taxon."""
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


def _db_arrays(tj, use_taxid):
    """The taxonomies file as the C ABI's arrays, row = its position in the file: nodes interned on (Display(rank),
    identifier), `bad` where an element does not split into exactly two parts (blast_result.rs:38-120)."""
    entries = json.load(open(tj))["taxonomies"]
    rank_names, rank_at, nodes = [], {}, {}
    lin_off, lin_node, lin_rank, bad, strings = [0], [], [], [], []
    for e in entries:
        s = e["numericLineage" if use_taxid else "textLineage"]
        strings.append(s)
        parts = [el.split("__") for el in s.split(";")]
        is_bad = any(len(p) != 2 for p in parts)
        bad.append(1 if is_bad else 0)
        if not is_bad:
            for rk, ident in parts:
                if rk not in rank_at:
                    rank_at[rk] = len(rank_names)
                    rank_names.append(rk)
                lin_rank.append(rank_at[rk])
                lin_node.append(nodes.setdefault((orc.rank_display(rk), ident), len(nodes)))
        lin_off.append(len(lin_node))
    return (np.array(lin_off, np.uint64), np.array(lin_node, np.uint32), np.array(lin_rank, np.uint16), rank_names or ["d"],
            np.array(bad, np.uint8), strings)


def _results(doc, fmt):
    if fmt == "jsonl":
        return [json.loads(l) for l in open(doc).read().splitlines()[1:]]
    return tabular.load_content(doc, fmt)["results"]


def _expected(bt, tj, results, taxon, strategy, use_taxid, custom, hit_filter):
    """The renderer on the document, the ingest's columns and the engine's records on those columns; and, from the document
    alone: the database lineage of every supporting hit holds the elements of the result's taxonomy, in order."""
    cols = pipeline.ingest_columns(bt, tj, bool(use_taxid), device=0, hit_filter=hit_filter)
    lin_off, lin_node, lin_rank, rank_names, bad, strings = _db_arrays(tj, use_taxid)
    t = engine.Taxonomy(lin_off, lin_node, lin_rank, rank_names, taxon=taxon, custom=custom, device=0, bad=bad)
    desc = cols["tax_desc_row"]
    recs = engine.run_consensus_host(t, cols["seg_off"], cols["bitscore"], t.engine_rows(desc), cols["pident"], cols["align_len"],
                                     cols["acc_rank"], strategy=strategy)
    lineages = ref.lineages_of(lin_off, lin_node)
    fields = ref.support(cols["seg_off"], cols["bitscore"], desc, lineages, bad, recs)
    _assert_invariants(fields, recs)
    _, sup = ref.supporting(cols["seg_off"], cols["bitscore"], desc, lineages, bad, recs)
    by_name = {r["query"]: r for r in results}
    checked = 0
    for q, name in enumerate(cols["query_names"]):
        r = by_name[name.decode()]
        if r.get("taxon") is None:
            assert not sup[int(cols["seg_off"][q]):int(cols["seg_off"][q + 1])].any()
            continue
        want = [e for e in r["taxon"]["taxonomy"].split(";") if e]
        for i in range(int(cols["seg_off"][q]), int(cols["seg_off"][q + 1])):
            if sup[i]:
                it = iter(f"{orc.rank_display(e.split('__')[0])}__{e.split('__')[1]}" for e in strings[int(desc[i])].split(";"))
                assert all(w in it for w in want), (name, want, strings[int(desc[i])])
                checked += 1
    assert checked or not len(desc)
    return ref.render(results, cols["query_names"], fields)


def _check(tmp_path, bt, tj, taxon="bacteria", strategy="relaxed", use_taxid=False, custom=None, lenient=True, fmt="json",
           headers=None, hit_filter=None, report=False, sample_table=False):
    doc, plain, sup = str(tmp_path / f"doc.{fmt}"), str(tmp_path / f"plain.{fmt}"), str(tmp_path / "support.tsv")
    rep, tab = str(tmp_path / "report.tsv"), str(tmp_path / "table.tsv")
    for p in (sup, rep, tab):
        if os.path.exists(p):
            os.remove(p)
    kw = dict(headers=headers, out_format=fmt, lenient=lenient, hit_filter=hit_filter,
              report_path=rep if report else None, sample_table_path=tab if sample_table else None)
    pipeline.build_consensus_identities_with_tables(bt, tj, taxon, strategy, use_taxid, custom, out_path=doc,
                                                    support_table_path=sup, **kw)
    results = _results(doc, fmt)
    text = open(sup).read()
    assert text == _expected(bt, tj, results, taxon, strategy, use_taxid, custom, hit_filter)
    assert os.path.exists(rep) == report and os.path.exists(tab) == sample_table
    # the document is what the run without the flag writes, apart from the fresh run id
    extra = {}
    if report or sample_table:
        extra = dict(report_path=str(tmp_path / "r2.tsv") if report else None, sample_table_path=str(tmp_path / "t2.tsv") if sample_table else None)
        pipeline.build_consensus_identities_with_tables(bt, tj, taxon, strategy, use_taxid, custom, out_path=plain, headers=headers,
                                                        out_format=fmt, lenient=lenient, hit_filter=hit_filter, **extra)
        if report:
            assert open(rep).read() == open(tmp_path / "r2.tsv").read()
        if sample_table:
            assert open(tab).read() == open(tmp_path / "t2.tsv").read()
    else:
        pipeline.build_consensus_identities(bt, tj, taxon, strategy, use_taxid, custom, out_path=plain, headers=headers,
                                            out_format=fmt, lenient=lenient, hit_filter=hit_filter)
    a, b = open(doc).read(), open(plain).read()
    if results:
        a, b = a.replace(results[0]["runId"], "R"), b.replace(_results(plain, fmt)[0]["runId"], "R")
    assert a == b
    return results, text


MODES = [{}, {"BLU_PIPELINE_HOST_COLUMNS": "1"}, {"BLU_INGEST": "cpu"}]


@pytest.mark.parametrize("env", MODES, ids=["device", "host_columns", "cpu_ingest"])
def test_docs_example_and_zymo_golden(tmp_path, golden_dir, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    doc = json.load(open(os.path.join(golden_dir, "docs_worked_example.json")))
    bt, tj = _golden_inputs(tmp_path, [r["taxon"] for r in doc["results"]], [r["query"] for r in doc["results"]])
    _, text = _check(tmp_path, bt, tj, lenient=False)
    assert len(text.splitlines()) == 2
    with gzip.open(os.path.join(golden_dir, "zymo_mock_distilled.json.gz"), "rt") as f:
        cases = json.load(f)["cases"]
    bt, tj = _golden_inputs(tmp_path, [c["taxon"] for c in cases], [f"case{i:04d}" for i in range(len(cases))])
    for strategy in ("relaxed", "cautious"):
        results, text = _check(tmp_path, bt, tj, strategy=strategy)
        assert len(results) == len(cases) and len(text.splitlines()) == len(cases) + 1
    assert all(int(l.split("\t")[3]) > 0 for l in text.splitlines()[1:])


@pytest.mark.parametrize("env", MODES, ids=["device", "host_columns", "cpu_ingest"])
def test_synthetic_tables_strategies_taxid_headers_and_panics(tmp_path, golden_dir, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    bt, tj = _synth_inputs(tmp_path)
    vals = json.load(open(os.path.join(golden_dir, "custom_taxon_cutoffs_bacteria_16S.json")))["values"]
    headers = [f"fasta_only_{i}" for i in range(3)]
    seen_null = 0
    for strategy in ("relaxed", "cautious"):
        for use_taxid in (False, True):
            taxon, custom = ("custom", vals) if use_taxid else ("bacteria", None)
            results, text = _check(tmp_path, bt, tj, taxon, strategy, use_taxid, custom, fmt="jsonl" if use_taxid else "json",
                                   headers=headers)
            seen_null += sum(r["taxon"] is None for r in results)
            lines = {l.split("\t")[0]: l for l in text.splitlines()[1:]}
            for h in headers:
                assert lines[h] == f"{h}\t-\tunclassified\t0\t0\t0\t0\t0\t0\t0\t0\t0.0000"
    assert seen_null > len(headers) * 4                   # lenient panics: unclassified lines with their counts
    # strict mode: the reference panics on these tables; the call fails and leaves no support file behind
    sup = tmp_path / "strict.tsv"
    with pytest.raises(N.BluError) as e:
        pipeline.build_consensus_identities_with_tables(bt, tj, "bacteria", "relaxed", out_path=str(tmp_path / "s.json"),
                                                        support_table_path=str(sup))
    assert e.value.code == pipeline.BLU_ERR_REFERENCE_PANIC
    assert not sup.exists()


@pytest.mark.parametrize("env", MODES, ids=["device", "host_columns", "cpu_ingest"])
def test_with_report_sample_table_and_a_hit_filter_together(tmp_path, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    bt, tj = _synth_inputs(tmp_path, sample_names=True)
    flt = {"min_perc_identity": 90.0, "min_bit_score": 300.0}
    full = pipeline.ingest_columns(bt, tj, device=0)
    kept = pipeline.ingest_columns(bt, tj, device=0, hit_filter=flt)
    assert 0 < kept["n_kept"] < len(full["bitscore"])
    _, text = _check(tmp_path, bt, tj, hit_filter=flt, report=True, sample_table=True)
    assert sum(int(l.split("\t")[3]) for l in text.splitlines()[1:]) == kept["n_kept"]     # the kept lines only
    _check(tmp_path, bt, tj, report=True)
    _check(tmp_path, bt, tj, hit_filter=flt)


def test_cli_build_consensus_and_run_with_consensus(tmp_path, golden_dir, capsys):
    with gzip.open(os.path.join(golden_dir, "zymo_mock_distilled.json.gz"), "rt") as f:
        cases = json.load(f)["cases"]
    names = [f"case{i:04d}" for i in range(len(cases))]
    bt, tj = _golden_inputs(tmp_path, [c["taxon"] for c in cases], names)
    a, b, sup = tmp_path / "a.json", tmp_path / "b.json", tmp_path / "s.tsv"
    base = ["blastn", "build-consensus", bt, "-t", tj, "--taxon", "bacteria", "--strategy", "relaxed"]
    assert cli.main(base + ["--blutils-out-file", str(a)]) == 0
    assert cli.main(base + ["--blutils-out-file", str(b), "--support-table", str(sup)]) == 0
    da, db = json.load(open(a)), json.load(open(b))
    assert a.read_text().replace(da["results"][0]["runId"], "R") == b.read_text().replace(db["results"][0]["runId"], "R")
    assert sup.read_text() == _expected(bt, tj, db["results"], "bacteria", "relaxed", False, None, None)
    # run-with-consensus: a stand-in `blastn` replays the table; one FASTA header has no hits
    fa = tmp_path / "queries.fa"
    fa.write_text("".join(f">{n} read\nACGTACGTAC\n" for n in names) + ">fasta_only\nAC\n")
    os.mkdir(tmp_path / "db")
    (tmp_path / "db" / "ref16s.nsq").write_text("")
    exe = tmp_path / "blastn"
    exe.write_text(f"#!{sys.executable}\nimport sys\n"
                   f"want = {{l[1:].split()[0] for l in sys.stdin.read().split(chr(10)) if l.startswith('>')}}\n"
                   f"sys.stdout.write(''.join(l for l in open({bt!r}) if l.split(chr(9))[0] in want))\n")
    exe.chmod(exe.stat().st_mode | stat.S_IEXEC)
    sup2 = tmp_path / "s2.tsv"
    argv = ["blastn", "run-with-consensus", str(fa), "-d", str(tmp_path / "db" / "ref16s"), "-t", tj, "--blast-out-file",
            str(tmp_path / "work" / "hits.tsv"), "--blutils-out-file", str(tmp_path / "res" / "c.json"), "--taxon", "bacteria",
            "--strategy", "relaxed", "--threads", "2", "--blastn", str(exe), "--support-table", str(sup2)]
    assert cli.main(argv) == 0
    doc = json.load(open(tmp_path / "res" / "c.json"))
    text = sup2.read_text()
    assert text == _expected(str(tmp_path / "work" / "hits.out"), tj, doc["results"], "bacteria", "relaxed", False, None, None)
    assert "fasta_only\t-\tunclassified\t0\t0\t0\t0\t0\t0\t0\t0\t0.0000\n" in text
    assert [l.split("\t")[0] for l in text.splitlines()[1:]] == [r["query"] for r in doc["results"]]
    capsys.readouterr()
