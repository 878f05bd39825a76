#!/usr/bin/env python3
"""What the query-cover builds of the GPU layout parse kernels cost:

    python scripts/query_cover_bench.py [--queries 2000000] [--hits 50] [--taxa 300000] [--reps 5]
        [--json profiles/query_cover_bench.json] [--parent-lib OLD/libblu_consensus.so]

The table is scripts/taxon_filter_bench.py's (scripts/tools/gen_blast.c, 100 M lines by default) written twice more: as
`6 std staxid qlen` (qlen so that the exact coverage of a line is 100, 90, 70 or 40 percent in turn) and as `6 std staxid qcovhsp`
(the same four as BLAST's integer).  All read from a warm page cache.  One process parses them with the GPU ingest, alternating
inside every repetition, under BLU_INGEST_TRACE=1, and takes the `parse` lap of the ingest trace — with a filter the lap named
`parse (filtered)`: the parse kernel alone, the device drained before and after.

  filtered_qlen / filtered_qcovhsp   the copy under a hit filter that keeps every line: parse_rows_layout_filtered, the baseline
  all_qlen / all_qcovhsp             the same filter and a cover of 0 percent (keeps everything): parse_rows_layout_qcov
  half_qlen / half_qcovhsp           the same filter and a cover of 80 percent (keeps half): parse_rows_layout_qcov

--parent-lib: a process of its own then parses the original table with the library of the parent commit (`parent`) — the
default path launches the same kernel in both, so `reference` (this tree on the original) must sit inside the parent's spread.

Prints one line per run and a JSON summary (median, min and max per variant; the trace prints whole milliseconds); --json also
writes it to a file.
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPECS = {"qlen": "6 std staxid qlen", "qcovhsp": "6 std staxid qcovhsp"}
# the reference's columns in the order `6 std staxid X` writes them; the coverage of line NR is 100, 90, 70, 40 percent in turn
AWK = {"qlen": r"""BEGIN { FS = OFS = "\t" } { s = $9 - $8; if (s < 0) s = -s; s += 1; k = NR % 4; q = k == 0 ? s : k == 1 ? int(s * 10 / 9) + 1 : k == 2 ? int(s * 10 / 7) + 1 : int(s * 10 / 4) + 1;
print $1, $2, $4, $5, $6, $7, $8, $9, $10, $11, $12, $13, $3, q }""",
       "qcovhsp": r"""BEGIN { FS = OFS = "\t"; split("100 90 70 40", c, " ") } { print $1, $2, $4, $5, $6, $7, $8, $9, $10, $11, $12, $13, $3, c[NR % 4 + 1] }"""}
KEEP_ALL = {"min_perc_identity": 0.0}


def parse_lap(fn, filtered):
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
    m = re.search(r"^\[ingest-gpu\] parse \(filtered\)\s+([0-9.]+) s$" if filtered else r"^\[ingest-gpu\] parse\s+([0-9.]+) s$", text, re.M)
    if not m:
        sys.stderr.write(text)
        raise SystemExit("no `parse` lap in the ingest trace: did the GPU parser decline the table?")
    return out, float(m.group(1))


def ingest(pipeline, path, taxonomies, device, spec, hit_filter, cover):
    """the ingest's counts of `path`, the columns released at once"""
    L = pipeline._bind()
    c, sel = pipeline.IngestColumns(), pipeline._Selection(hit_filter, None, None, False)
    st = sel.stats()
    if cover is not None:
        cv = pipeline._Cover(cover, spec)
        rc = L.blu_ingest_columns_covered(path.encode(), taxonomies.encode(), 0, device, C.byref(cv.layout), C.byref(cv.c), C.byref(sel.c), C.byref(c), C.byref(st))
    elif spec is not None:
        lay = pipeline.table_layout(spec)
        rc = L.blu_ingest_columns_laid_out(path.encode(), taxonomies.encode(), 0, device, C.byref(lay), C.byref(sel.c), C.byref(c), C.byref(st))
    else:
        rc = L.blu_ingest_columns_selected(path.encode(), taxonomies.encode(), 0, device, C.byref(sel.c), C.byref(c), C.byref(st))
    if rc != 0:
        raise SystemExit(f"ingest failed with blu_error {rc}")
    out = {"n_hits": int(c.n_hits), "n_queries": int(c.n_queries), "n_kept": int(st.hit_filter.n_kept)}
    if cover is not None:
        out["n_below"] = int(cv.st.n_below)
    L.blu_ingest_columns_free(C.byref(c))
    return out


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
    taxa = -(-args.taxa // 96) * 96
    subprocess.run([gen, "db", tj, str(taxa + 96)], check=True)
    if not os.path.exists(bt):
        subprocess.run([gen, "table", bt, str(args.queries), str(args.hits), str(taxa), "1", "clustered"], check=True)
    print("table written", flush=True)
    copies = {}
    for name in SPECS:
        copies[name] = os.path.join(args.dir, f"blast.{args.queries}x{args.hits}.{name}.tsv")
        if not args.only_reference and not os.path.exists(copies[name]):
            with open(bt, "rb") as src, open(copies[name], "wb") as dst:
                subprocess.run(["awk", AWK[name]], stdin=src, stdout=dst, check=True)
            print(f"copy written: {SPECS[name]}", flush=True)
    print("copies written", flush=True)
    os.environ["BLU_INGEST"] = "gpu"
    os.environ["BLU_INGEST_TRACE"] = "1"
    from blutils_amd import pipeline
    pipeline.build_db_cache(tj, cache, False)
    paths = [bt] if args.only_reference else [bt] + list(copies.values())
    for path in paths:                                          # warm page cache
        with open(path, "rb") as f:
            while f.read(1 << 26):
                pass
    size = os.path.getsize(bt)
    print(f"table: {args.queries} queries x {args.hits} hits = {size / 1e9:.2f} GB of text", flush=True)
    variants = [("reference", bt, None, None, None)]
    if not args.only_reference:
        for name, spec in SPECS.items():
            variants += [(f"filtered_{name}", copies[name], spec, KEEP_ALL, None), (f"all_{name}", copies[name], spec, KEEP_ALL, {"percent": "0", "source": name}),
                         (f"half_{name}", copies[name], spec, KEEP_ALL, {"percent": "80", "source": name})]
    laps = {v[0]: [] for v in variants}
    counts = {}
    for rep in range(args.reps + 1):                            # (repetition 0 warms the device up and is not counted)
        for name, path, spec, flt, cover in variants:
            got, lap = parse_lap(lambda: ingest(pipeline, path, cache, args.device, spec, flt, cover), flt is not None or cover is not None)
            assert pipeline.last_ingest_path() == "gpu", name
            counts[name] = got
            if rep:
                laps[name].append(lap)
            print(f"rep {rep} {name:18s} parse {lap * 1e3:.1f} ms  {got}", flush=True)
    if args.only_reference:
        print(json.dumps({"parse_ms": [round(x * 1e3, 2) for x in laps["reference"]], "counts": counts["reference"]}))
        return
    lines = args.queries * args.hits
    for name in SPECS:                                          # keeps everything; keeps the 100 and 90 percent lines: half
        assert counts[f"all_{name}"]["n_below"] == 0 and counts[f"all_{name}"]["n_hits"] == counts[f"filtered_{name}"]["n_hits"], counts
        assert counts[f"half_{name}"]["n_below"] == lines // 2, counts
    stat = lambda v: {"median": round(statistics.median(v) * 1e3, 2), "min": round(min(v) * 1e3, 2), "max": round(max(v) * 1e3, 2),
                      "all": [round(x * 1e3, 2) for x in v]}
    summary = {"text_gb": size / 1e9, "lines": lines, "reps": args.reps, "specs": SPECS, "parse_ms": {k: stat(v) for k, v in laps.items()}, "counts": counts}
    for name in SPECS:
        base = summary["parse_ms"][f"filtered_{name}"]["median"]
        summary[f"added_ms_{name}"] = {k: round(summary["parse_ms"][f"{k}_{name}"]["median"] - base, 2) for k in ("all", "half")}
    if args.parent_lib:
        argv = [sys.executable, os.path.abspath(__file__), "--only-reference", "--queries", str(args.queries), "--hits", str(args.hits),
                "--taxa", str(args.taxa), "--reps", str(args.reps), "--device", str(args.device), "--dir", args.dir]
        p = subprocess.run(argv, env=dict(os.environ, BLU_CONSENSUS_LIB=os.path.abspath(args.parent_lib)), capture_output=True, text=True)
        if p.returncode != 0:
            print(p.stdout[-2000:], p.stderr[-4000:])
            raise SystemExit(1)
        parent = json.loads(p.stdout.strip().splitlines()[-1])
        assert parent["counts"] == counts["reference"], parent
        v = parent["parse_ms"]
        summary["parse_ms"]["parent"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}
        summary["reference_within_parent_spread"] = min(v) <= summary["parse_ms"]["reference"]["median"] <= max(v)
    print(json.dumps(summary))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
