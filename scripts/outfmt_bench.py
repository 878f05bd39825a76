#!/usr/bin/env python3
"""What the column-layout builds of the GPU parse kernels cost:

    python scripts/outfmt_bench.py [--queries 2000000] [--hits 50] [--taxa 300000] [--reps 5] [--json profiles/outfmt_bench.json]
        [--parent-lib OLD/libblu_consensus.so]

The table is scripts/taxon_filter_bench.py's (scripts/tools/gen_blast.c, 100 M lines by default) and a copy of it written as
`6 std staxid` — the taxid moved behind the bit-score, so every line keeps its bytes — both read from a warm page cache.  One
process parses both with the GPU ingest (blu_ingest_columns_selected / _laid_out on the device), alternating inside every repetition, under
BLU_INGEST_TRACE=1, and takes the `parse` lap of the ingest trace: the parse kernel alone, the device drained before and after.

  reference   the original under no layout: parse_rows, the baseline
  laid_out    the copy under blast_outfmt="6 std staxid": parse_rows_layout

--parent-lib: a process of its own then parses the original with the library of the parent commit, the same way (`parent`):
the default path launches the same kernels in both, so `reference` must sit inside the parent's spread.

Both must give the same columns (compared by their sums).  Prints one line per run and a JSON summary (median, min and max
per variant, the added milliseconds and the ratio; the trace prints whole milliseconds); --json also writes it to a file.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAID_OUT = "6 std staxid"
# the reference's columns 1 .. 13 in the order `6 std staxid` writes them
AWK = r"""BEGIN { FS = OFS = "\t" } { print $1, $2, $4, $5, $6, $7, $8, $9, $10, $11, $12, $13, $3 }"""


def parse_lap(fn):
    """fn() with the process's stderr in a file: its result and the seconds of the `[ingest-gpu] parse` line"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode("utf-8", "replace")
    m = re.search(r"^\[ingest-gpu\] parse\s+([0-9.]+) s$", text, re.M)
    if not m:
        sys.stderr.write(text)
        raise SystemExit("no `parse` lap in the ingest trace: did the GPU parser decline the table?")
    return out, float(m.group(1))


def columns_digest(pipeline, path, taxonomies, device, spec):
    """The ingest's columns of `path` (under the layout `spec`, or none) summed in place — no copy of 100 M rows through numpy —
    and released: what the two variants must agree on."""
    import ctypes as C

    import numpy as np
    L = pipeline._bind()
    c, st = pipeline.IngestColumns(), pipeline.HitSelectionStats()
    if spec is None:
        rc = L.blu_ingest_columns_selected(path.encode(), taxonomies.encode(), 0, device, None, C.byref(c), C.byref(st))
    else:
        lay = pipeline.table_layout(spec)
        rc = L.blu_ingest_columns_laid_out(path.encode(), taxonomies.encode(), 0, device, C.byref(lay), None, C.byref(c), C.byref(st))
    if rc != 0:
        raise SystemExit(f"ingest failed with blu_error {rc}")
    try:
        nh, nq = int(c.n_hits), int(c.n_queries)
        view = lambda p, n: np.ctypeslib.as_array(p, shape=(n,))
        digest = {"n_hits": nh, "n_queries": nq, "n_accessions": int(c.n_accessions)}
        for name, n in (("seg_off", nq + 1), ("bitscore", nh), ("align_len", nh), ("tax_desc_row", nh), ("acc_rank", nh)):
            digest[name] = int(view(getattr(c, name), n).sum(dtype=np.int64))
        digest["pident"] = float(view(c.pident, nh).sum())
        return digest
    finally:
        L.blu_ingest_columns_free(C.byref(c))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=2000000)
    ap.add_argument("--hits", type=int, default=50)
    ap.add_argument("--taxa", type=int, default=300000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--dir", default="/tmp/blu_taxon_filter")
    ap.add_argument("--json", help="also write the summary here")
    ap.add_argument("--parent-lib", help="libblu_consensus.so built from the parent commit: its `parse` lap on the original, in a process of its own")
    ap.add_argument("--only-reference", action="store_true", help="the original under no layout alone (what --parent-lib runs)")
    args = ap.parse_args()
    os.makedirs(args.dir, exist_ok=True)
    gen = os.path.join(args.dir, "gen_blast")
    subprocess.run(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "scripts", "tools", "gen_blast.c")], check=True)
    tj, cache = os.path.join(args.dir, "tax.blutils.json"), os.path.join(args.dir, "tax.blucache")
    bt = os.path.join(args.dir, f"blast.{args.queries}x{args.hits}.tsv")
    laid = os.path.join(args.dir, f"blast.{args.queries}x{args.hits}.std_staxid.tsv")
    taxa = -(-args.taxa // 96) * 96
    subprocess.run([gen, "db", tj, str(taxa + 96)], check=True)
    if not os.path.exists(bt):
        subprocess.run([gen, "table", bt, str(args.queries), str(args.hits), str(taxa), "1", "clustered"], check=True)
    print("table written", flush=True)
    if not os.path.exists(laid) or os.path.getsize(laid) != os.path.getsize(bt):
        with open(bt, "rb") as src, open(laid, "wb") as dst:
            subprocess.run(["awk", AWK], stdin=src, stdout=dst, check=True)
    assert os.path.getsize(laid) == os.path.getsize(bt)        # the same bytes per line
    print("relaid copy written", flush=True)
    os.environ["BLU_INGEST"] = "gpu"
    os.environ["BLU_INGEST_TRACE"] = "1"
    from blutils_amd import pipeline
    pipeline.build_db_cache(tj, cache, False)
    for path in (bt, laid):                                     # warm page cache
        with open(path, "rb") as f:
            while f.read(1 << 26):
                pass
    size = os.path.getsize(bt)
    print(f"table: {args.queries} queries x {args.hits} hits = {size / 1e9:.2f} GB of text, twice", flush=True)
    variants = [("reference", bt, None), ("laid_out", laid, LAID_OUT)]
    if args.only_reference:
        variants = variants[:1]
    laps = {name: [] for name, _, _ in variants}
    sums = {}
    for rep in range(args.reps + 1):                            # (repetition 0 warms the device up and is not counted)
        for name, path, spec in variants:
            got, lap = parse_lap(lambda: columns_digest(pipeline, path, cache, args.device, spec))
            assert pipeline.last_ingest_path() == "gpu", name
            sums[name] = got
            if rep:
                laps[name].append(lap)
            print(f"rep {rep} {name:10s} parse {lap * 1e3:.1f} ms  rows {got['n_hits']}  queries {got['n_queries']}", flush=True)
    med = {k: statistics.median(v) for k, v in laps.items()}
    if args.only_reference:
        print(json.dumps({"parse_ms": [round(x * 1e3, 2) for x in laps["reference"]], "digest": sums["reference"]}))
        return
    assert sums["reference"] == sums["laid_out"], sums
    summary = {"text_gb": size / 1e9, "lines": args.queries * args.hits, "reps": args.reps, "laid_out_spec": LAID_OUT,
               "parse_ms": {k: {"median": round(med[k] * 1e3, 2), "min": round(min(v) * 1e3, 2), "max": round(max(v) * 1e3, 2),
                                "all": [round(x * 1e3, 2) for x in v]} for k, v in laps.items()},
               "laid_out_added_ms": round((med["laid_out"] - med["reference"]) * 1e3, 2),
               "laid_out_over_reference": round(med["laid_out"] / med["reference"], 3),
               "gb_per_s": {k: round(size / 1e9 / med[k], 1) for k in med}, "rows": sums["reference"]["n_hits"]}
    if args.parent_lib:
        argv = [sys.executable, os.path.abspath(__file__), "--only-reference", "--queries", str(args.queries), "--hits", str(args.hits),
                "--taxa", str(args.taxa), "--reps", str(args.reps), "--device", str(args.device), "--dir", args.dir]
        p = subprocess.run(argv, env=dict(os.environ, BLU_CONSENSUS_LIB=os.path.abspath(args.parent_lib)), capture_output=True, text=True)
        if p.returncode != 0:
            print(p.stdout[-2000:], p.stderr[-4000:])
            raise SystemExit(1)
        parent = json.loads(p.stdout.strip().splitlines()[-1])
        assert parent["digest"] == sums["reference"], parent
        v = parent["parse_ms"]
        summary["parse_ms"]["parent"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}
        summary["reference_minus_parent_ms"] = round(summary["parse_ms"]["reference"]["median"] - statistics.median(v), 2)
        summary["reference_within_parent_spread"] = min(v) <= summary["parse_ms"]["reference"]["median"] <= max(v)
    print(json.dumps(summary))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
