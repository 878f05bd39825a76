#!/usr/bin/env python3
"""Distil the query names of the reference's golden output into a small committed fixture (data only).

Source (read-only, build container only):
  /root/reference/test/mock/output/zymo-mock/blutils.consensus.json — nine SRA runs pooled in one document, every query
  named `<run>.<n>_size_<m>` (the reference's QC pipeline: vsearch --relabel `<run>.`, `;size=` rewritten to `_size_`).

For each of its 3626 results, in document order: the query name and the index of its `taxon` among the cases of
zymo_mock_distilled.json.gz (make_golden.py), or null for "taxon": null.  With the two fixtures the reference's own
`results` list is rebuilt exactly, which the per-sample table is pinned to.

Run:  python tests/golden/make_sample_golden.py      (needs /root/reference; after make_golden.py)
"""
import gzip
import json
import os

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    src = os.path.join(REF, "test/mock/output/zymo-mock/blutils.consensus.json")
    d = json.load(open(src))
    with gzip.open(os.path.join(HERE, "zymo_mock_distilled.json.gz"), "rt") as f:
        cases = json.load(f)["cases"]
    index = {json.dumps(c["taxon"], sort_keys=True): i for i, c in enumerate(cases)}
    rows = []
    for r in d["results"]:
        t = r.get("taxon")
        rows.append([r["query"], index[json.dumps(t, sort_keys=True)] if t else None])
    out = {"source": "test/mock/output/zymo-mock/blutils.consensus.json",
           "fields": ["query", "case index in zymo_mock_distilled.json.gz, null for a null taxon"],
           "results": rows}
    with gzip.GzipFile(os.path.join(HERE, "zymo_mock_queries.json.gz"), "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())


if __name__ == "__main__":
    main()
