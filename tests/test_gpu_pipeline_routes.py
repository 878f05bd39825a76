"""The use-case's routes give one answer (blutils_amd/csrc/pipeline.cpp: Run).  One request — headers without hits, the
report, the per-sample table and the support table — must leave the same document and the same three table files, byte for
byte, (a) as returned text and as a file written through out_path, and (b) with the engine and the table passes on the columns
the GPU ingest left on the device and on host columns (BLU_PIPELINE_HOST_COLUMNS=1).  Every output format, at the sizes where
the code changes path: no query at all (the two headers alone; without them, an empty `results`), three, and 4097 results,
which cross one 4096-record render block — head, block and tail pieces, the writer's buffer pool — and whose out_path run
replaces an existing regular file.
The >= 65536-item parallel sort is test_gpu_pipeline.test_large_unsorted_table_streams_to_a_file_in_query_order's."""
import json

import numpy as np
import pytest

from blutils_amd import blast, pipeline

pytestmark = pytest.mark.gpu

TAXA = 60
HEADERS = ["s1.9000001", "s2.9000002"]          # FASTA ids without a hit
FILES = ("doc", "report", "table", "support")


def write_inputs(d):
    """{n_queries: table path}, the taxonomies file.  Queries `s<k % 3>.<k>` in shuffled order, three hits each, about half
    of the top groups tied."""
    tj = d / "t.json"
    tj.write_text(json.dumps({"blutilsVersion": "8.3.1", "sourceDatabase": "synthetic", "taxonomies": [
        {"taxid": 1000 + t, "rank": "species", "numericLineage": f"d__2;f__{t // 12};g__{t // 3};s__{1000 + t}",
         "textLineage": f"d__bacteria;f__fam{t // 12};g__gen{t // 3};s__sp{t}", "accessions": []} for t in range(TAXA)]}))
    tables = {}
    for nq in (0, 3, 4095):
        rng = np.random.default_rng(nq + 1)
        perm = rng.permutation(nq)
        sub = (np.repeat(rng.integers(0, TAXA, nq), 3) + rng.integers(0, 3, 3 * nq)) % TAXA
        pid = rng.integers(80000, 100001, 3 * nq)
        bs = np.repeat(rng.integers(200, 2000, nq), 3) - rng.integers(0, 2, 3 * nq)
        tables[nq] = d / f"b{nq}.tsv"
        tables[nq].write_text("".join(
            f"s{perm[i // 3] % 3}.{perm[i // 3]}\tNR_{sub[i]:06d}.1\t{1000 + sub[i]}\t{pid[i] // 1000}.{pid[i] % 1000:03d}\t400\t3\t1\t1\t400\t5\t404"
            f"\t1e-120\t{bs[i]}\n" for i in range(3 * nq)))
    return {k: str(v) for k, v in tables.items()}, str(tj)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return write_inputs(tmp_path_factory.mktemp("routes"))


@pytest.mark.parametrize("nq, headers", [(0, HEADERS), (0, None), (3, HEADERS), (4095, HEADERS)], ids=["0+2", "0+0", "3+2", "4095+2"])
@pytest.mark.parametrize("fmt", ["json", "json-compact", "jsonl", "yaml"])
def test_text_and_file_device_and_host_columns_give_the_same_bytes(tmp_path, monkeypatch, inputs, fmt, nq, headers):
    tables, tj = inputs
    monkeypatch.setenv("BLU_INGEST", "gpu")
    cfg = blast.BlastBuilder.default("/db/ref16s", "bacteria")          # (one run id for every document)
    got = {}
    for route in ("device", "host_columns"):
        if route == "host_columns":
            monkeypatch.setenv("BLU_PIPELINE_HOST_COLUMNS", "1")
        else:
            monkeypatch.delenv("BLU_PIPELINE_HOST_COLUMNS", raising=False)
        for to_file in (False, True):
            paths = {k: tmp_path / f"{route}{int(to_file)}.{k}" for k in FILES}
            if to_file and nq == 4095:
                paths["doc"].write_text("an older result\n" * 1000)     # (a regular file: replaced)
            text, stats = pipeline.build_consensus_identities_with_tables(
                tables[nq], tj, "bacteria", "relaxed", headers=headers, out_format=fmt, lenient=True, parse=False, config=cfg,
                out_path=str(paths["doc"]) if to_file else None, report_path=str(paths["report"]),
                sample_table_path=str(paths["table"]), support_table_path=str(paths["support"]))
            assert stats["n_queries"] == nq and (nq == 0 or pipeline.last_ingest_path() == "gpu")
            files = {k: paths[k].read_bytes() for k in FILES[1:]}
            files["doc"] = paths["doc"].read_bytes() if to_file else text.encode()
            got[route, to_file] = files
    first = got["device", False]
    n_results = nq + len(headers or ())
    assert first["support"].count(b"\n") == n_results + 1 and len(first["doc"]) > 0
    if n_results == 0:
        assert {"json": b'"results": []', "json-compact": b'"results":[]', "jsonl": b"", "yaml": b"results: []"}[fmt] in first["doc"]
    for key, files in got.items():
        for k in FILES:
            assert files[k] == first[k], (key, k)
