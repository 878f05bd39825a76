#!/usr/bin/env python3
"""What the hit filters of build-consensus cost and what they replace:

    python scripts/hit_filter_bench.py [--queries 2000000] [--hits 50] [--taxa 300000] [--reps 3]
        [--parent-lib OLD/libblu_consensus.so] [--json profiles/hit_filter_bench.json]

The table is scripts/e2e_bench.py's (scripts/tools/gen_blast.c: perc_identity uniform in 80 .. 100, e-value 1e-120), read
from a warm page cache; every run is a FRESH process (HIP start-up inside the wall time) of
build_consensus_identities(..., out_path=...), JSONL out; the variants alternate inside every repetition:

  parent      the unfiltered use-case with --parent-lib (the library of the commit before the filters), if given
  unfiltered  the same with this tree's library: must sit inside the spread of `parent`
  keep_all    --min-perc-identity 0 --min-align-length 0 --max-e-value 1e-5 --min-bit-score 0: every line kept — the cost of
              reading column 11 and evaluating the predicate
  keep_half   --min-perc-identity 90 --max-e-value 1e-20: about half the lines kept — plus the scan and the scatter
  awk         the route without the feature: awk writes the filtered copy (same predicate as keep_half), then the
              unfiltered run on the copy; wall time of both steps

Prints one line per run and a JSON summary (median and min/max per variant, added milliseconds and GB/s of text for the two
filters, the awk ratio); --json also writes it to a file.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEEP_ALL = {"min_perc_identity": 0.0, "min_align_length": 0, "max_e_value": 1e-5, "min_bit_score": 0.0}
KEEP_HALF = {"min_perc_identity": 90.0, "max_e_value": 1e-20}
AWK_HALF = "$4 >= 90 && $12 <= 1e-20"


def run_once(table, cache, outp, hit_filter, lib):
    code = ("import sys, json, time; sys.path.insert(0, %r); from blutils_amd import pipeline; t0 = time.perf_counter(); "
            "_, st = pipeline.build_consensus_identities(%r, %r, 'bacteria', 'relaxed', out_format='jsonl', lenient=True, parse=False, "
            "out_path=%r%s); st['wall_s'] = time.perf_counter() - t0; st['path'] = pipeline.last_ingest_path(); print(json.dumps(st))"
            % (ROOT, table, cache, outp, ", hit_filter=%r" % (hit_filter,) if hit_filter else ""))
    env = dict(os.environ)
    if lib:
        env["BLU_CONSENSUS_LIB"] = lib
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        print(p.stdout[-2000:], p.stderr[-4000:])
        raise SystemExit(1)
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=2000000)
    ap.add_argument("--hits", type=int, default=50)
    ap.add_argument("--taxa", type=int, default=300000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--awk-reps", type=int, default=1, help="the awk route is slow: repeated this often only")
    ap.add_argument("--parent-lib", help="libblu_consensus.so built from the parent commit (same ABI)")
    ap.add_argument("--dir", default="/tmp/blu_hit_filter")
    ap.add_argument("--pause", type=float, default=0.5, help="seconds between processes")
    ap.add_argument("--json", help="also write the summary here")
    args = ap.parse_args()
    os.makedirs(args.dir, exist_ok=True)
    gen = os.path.join(args.dir, "gen_blast")
    subprocess.run(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "scripts", "tools", "gen_blast.c")], check=True)
    tj, cache = os.path.join(args.dir, "tax.blutils.json"), os.path.join(args.dir, "tax.blucache")
    bt = os.path.join(args.dir, f"blast.{args.queries}x{args.hits}.tsv")
    subprocess.run([gen, "db", tj, str(args.taxa)], check=True)
    if not os.path.exists(bt):
        subprocess.run([gen, "table", bt, str(args.queries), str(args.hits), str(args.taxa), "1", "clustered"], check=True)
    from blutils_amd import pipeline
    pipeline.build_db_cache(tj, cache, False)
    size = os.path.getsize(bt)
    with open(bt, "rb") as f:                       # warm page cache
        while f.read(1 << 26):
            pass
    print(f"table: {args.queries} queries x {args.hits} hits = {size / 1e9:.2f} GB of text", flush=True)
    outp, copy = os.path.join(args.dir, "consensus.jsonl"), os.path.join(args.dir, "filtered_copy.tsv")
    variants = [("unfiltered", None, None), ("keep_all", KEEP_ALL, None), ("keep_half", KEEP_HALF, None)]
    if args.parent_lib:
        variants.insert(0, ("parent", None, os.path.abspath(args.parent_lib)))
    walls = {name: [] for name, _, _ in variants}
    walls["awk"], awk_step, facts = [], [], {}
    for rep in range(args.reps):
        for name, flt, lib in variants:
            time.sleep(args.pause)                  # (the driver is still tearing the previous process's device memory down)
            st = run_once(bt, cache, outp, flt, lib)
            walls[name].append(st["wall_s"])
            facts[name] = {k: st.get(k) for k in ("n_hits", "n_queries", "n_lines", "n_kept", "path", "t_load_hits_s")}
            print(f"rep {rep} {name:10s} wall {st['wall_s']:.3f} s  ingest {st['t_load_hits_s']:.3f} s  rows {st['n_hits']}  parser {st['path']}", flush=True)
        if rep < args.awk_reps:
            t0 = time.perf_counter()
            with open(copy, "wb") as f:
                subprocess.run(["awk", "-F", "\t", AWK_HALF, bt], stdout=f, check=True)
            t_awk = time.perf_counter() - t0
            time.sleep(args.pause)
            st = run_once(copy, cache, outp, None, None)
            awk_step.append(t_awk)
            walls["awk"].append(t_awk + st["wall_s"])
            facts["awk"] = {"n_hits": st["n_hits"], "n_queries": st["n_queries"], "copy_gb": os.path.getsize(copy) / 1e9}
            print(f"rep {rep} awk        awk {t_awk:.2f} s + run {st['wall_s']:.3f} s  rows {st['n_hits']}", flush=True)
    for p in (outp, copy):
        if os.path.exists(p):
            os.remove(p)
    med = {k: statistics.median(v) for k, v in walls.items() if v}
    summary = {"text_gb": size / 1e9, "lines": args.queries * args.hits, "reps": args.reps,
               "wall_s": {k: {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4), "all": [round(x, 4) for x in v]}
                          for k, v in walls.items() if v},
               "facts": facts}
    for k in ("keep_all", "keep_half"):
        added = med[k] - med["unfiltered"]
        summary[k + "_added_ms"] = round(added * 1e3, 1)
        summary[k + "_added_gb_per_s"] = round(size / 1e9 / added, 1) if added > 0 else None
    if "parent" in med:
        summary["unfiltered_minus_parent_ms"] = round((med["unfiltered"] - med["parent"]) * 1e3, 1)
        summary["parent_spread_ms"] = round((max(walls["parent"]) - min(walls["parent"])) * 1e3, 1)
    if walls["awk"]:
        summary["awk_step_s"] = round(statistics.median(awk_step), 2)
        summary["awk_route_over_keep_half"] = round(med["awk"] / med["keep_half"], 1)
    assert facts["keep_all"]["n_kept"] == facts["keep_all"]["n_lines"] == facts["unfiltered"]["n_hits"]
    if "awk" in facts:
        assert facts["awk"]["n_hits"] == facts["keep_half"]["n_kept"] == facts["keep_half"]["n_hits"]     # the same lines either way
    print(json.dumps(summary))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
