"""The document at the edges of the code between the engine's records and the text (tests/document_edges.py):
every case on the three routes of the use-case — the columns the GPU ingest left on the device (`top_rows_kernel`, the packed
or f64 side of `device_run_consensus`), the same columns downloaded (BLU_PIPELINE_HOST_COLUMNS=1: `top_rows_from_columns`) and
the host parser's (BLU_INGEST=cpu) — as `json` and as `jsonl`.  On each route every rendered query's `taxon` object equals the
faithful oracle's field for field, `null` stands exactly where the oracle has no consensus, and the three routes' documents
are the same bytes once `runId` is masked.  Strict mode fails exactly when the table holds a query the reference panics on.
A taxonomies document that lists a taxid twice is read by the host parser on every route (pipeline_ingest.cpp: load_hits), so
for those cases the first route asserts `cpu`."""
import json
import re

import pytest

from blutils_amd import _native as N
from blutils_amd import pipeline
from oracle import oracle as orc
from tests import document_edges as E

pytestmark = pytest.mark.gpu

PARAMS, IDS = E.case_params()
ROUTES = {"device": {"BLU_INGEST": "gpu"}, "host_columns": {"BLU_INGEST": "gpu", "BLU_PIPELINE_HOST_COLUMNS": "1"}, "cpu": {"BLU_INGEST": "cpu"}}
PACKED_BLOCKS, F64_BLOCKS = (768, 1024), (704, 768)        # consensus_kernel.hip: BLOCK_A / BLOCK_N and BLOCK_F / BLOCK_A


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    return str(tmp_path_factory.mktemp("document_edges"))


def mask(raw):
    return re.sub(r'"runId": ?"[0-9a-f-]+"', '"runId":"x"', raw)


def records(raw, fmt):
    if fmt == "json":
        doc = json.loads(raw)
        assert doc["config"] is None
        return doc["results"]
    lines = raw.splitlines()
    assert lines[0] == "null"
    return [json.loads(l) for l in lines[1:]]


def check_document(case, strategy, route, fmt, recs, exp):
    where = f"family={case.family} case={case.name} strategy={strategy} route={route} format={fmt}"
    want_names = sorted([q.name for q in case.queries] + list(case.headers), key=str.encode)
    assert [r["query"] for r in recs] == want_names, where
    assert len({r["runId"] for r in recs}) == 1, where
    n_rendered = 0
    for r in recs:
        at = f"{where} query={r['query']}"
        if r["query"] in case.headers:
            assert r["taxon"] is None, f"{at}: a header without hits has a taxon"
            continue
        o = exp[r["query"]]
        if o["status"] != orc.ST_CONSENSUS:
            assert r["taxon"] is None, f"{at}: taxon where the oracle has status {o['status']} ({o.get('panic')})"
            continue
        assert r["taxon"] is not None, f"{at}: null where the oracle has a consensus"
        diff = E.first_difference(r["taxon"], o["taxon"])
        assert diff is None, f"{at}: first difference at {diff[0]}: got {diff[1]!r}, the oracle has {diff[2]!r}"
        n_rendered += 1
    return n_rendered


@pytest.mark.parametrize("case, strategy", PARAMS, ids=IDS)
def test_document_equals_the_oracle_on_every_route(directory, monkeypatch, case, strategy):
    bt, tj = E.write(case, directory)
    exp = E.expected(case, strategy, directory)
    headers = list(case.headers) or None
    panics = any(o["status"] >= orc.ST_PANIC_PARSE for o in exp.values())
    docs = {}
    for route, env in ROUTES.items():
        for k in ("BLU_INGEST", "BLU_PIPELINE_HOST_COLUMNS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for fmt in ("json", "jsonl"):
            raw, stats = pipeline.build_consensus_identities(bt, tj, "bacteria", strategy, headers=headers, out_format=fmt, lenient=True, parse=False)
            want_path = "cpu" if route == "cpu" or case.dup else "gpu"
            assert pipeline.last_ingest_path() == want_path, (case.id, route, fmt)
            assert stats["n_queries"] == len(case.queries)
            if route == "device" and case.route:
                from blutils_amd import engine
                _, _, block = engine.last_launch()
                assert block in (PACKED_BLOCKS if case.route == "packed" else F64_BLOCKS), (case.id, block)
            n = check_document(case, strategy, route, fmt, records(raw, fmt), exp)
            assert n == sum(q.claim["kind"] == E.RENDERED for q in case.queries)
            docs[route, fmt] = mask(raw)
        if panics:                  # strict mode mirrors the reference: a query on which it panics fails the call
            with pytest.raises(N.BluError) as e:
                pipeline.build_consensus_identities(bt, tj, "bacteria", strategy, headers=headers, parse=False)
            assert e.value.code == pipeline.BLU_ERR_REFERENCE_PANIC, (case.id, route)
        else:
            raw, _ = pipeline.build_consensus_identities(bt, tj, "bacteria", strategy, headers=headers, parse=False)
            assert mask(raw) == docs[route, "json"], (case.id, route, "strict")
    for fmt in ("json", "jsonl"):
        for route in ROUTES:
            assert docs[route, fmt] == docs["device", fmt], f"family={case.family} case={case.name} format={fmt}: route {route} and the device route differ"


def test_the_identity_routes_take_different_layouts(directory, monkeypatch):
    """The same 300-query table with one value changed: exact milli-percent below 131.071 stays on the packed records, a fourth
    decimal or 131.071 itself leaves them (engine_dev.hip: pack_side_records).  The launch geometry tells the layouts apart: the
    packed and the f64 builds of the stream kernel differ in block size for one table shape."""
    from blutils_amd import engine
    monkeypatch.setenv("BLU_INGEST", "gpu")
    monkeypatch.delenv("BLU_PIPELINE_HOST_COLUMNS", raising=False)
    block = {}
    for case in (c for c in E.cases() if c.family == "routes"):
        bt, tj = E.write(case, directory)
        pipeline.build_consensus_identities(bt, tj, "bacteria", "relaxed", lenient=True, parse=False)
        assert pipeline.last_ingest_path() == "gpu"
        block[case.name] = engine.last_launch()[2]
    print("[identity routes] block sizes", block)
    assert block["exact"] == block["below_limit"] and block["four_decimals"] == block["at_limit"], block
    assert block["exact"] != block["at_limit"], block
    assert block["exact"] in PACKED_BLOCKS and block["at_limit"] in F64_BLOCKS, block
