#!/usr/bin/env python3
"""The unfiltered use-case with this tree's library against another build of the same ABI (the parent commit's, as a rule):

    python scripts/use_case_ab.py --parent-lib OLD/libblu_consensus.so [--reps 12] [--json FILE]

scripts/taxon_filter_bench.py's table (100 M lines) and its fresh-process run, the two libraries alternating and their order
swapped every repetition: in a fixed order the process that runs second is the slower one whichever library it loads.  Prints
one line per run and a JSON summary (median, min and max of the wall time and of the ingest, per library and per position)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", required=True)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--json")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import taxon_filter_bench as T
d = "/tmp/blu_taxon_filter"
os.makedirs(d, exist_ok=True)
gen = os.path.join(d, "gen_blast")
subprocess.run(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "scripts", "tools", "gen_blast.c")], check=True)
tj, cache, bt = os.path.join(d, "tax.blutils.json"), os.path.join(d, "tax.blucache"), os.path.join(d, "blast.2000000x50.tsv")
taxa = -(-300000 // 96) * 96
subprocess.run([gen, "db", tj, str(taxa + 96)], check=True)
if not os.path.exists(bt):
    subprocess.run([gen, "table", bt, "2000000", "50", str(taxa), "1", "clustered"], check=True)
from blutils_amd import pipeline
pipeline.build_db_cache(tj, cache, False)
with open(bt, "rb") as f:
    while f.read(1 << 26):
        pass
print("table ready", flush=True)
parent = os.path.abspath(args.parent_lib)
outp = os.path.join(d, "consensus.jsonl")
walls = {"parent": [], "head": []}
ingest = {"parent": [], "head": []}
by_pos = {("parent", 0): [], ("parent", 1): [], ("head", 0): [], ("head", 1): []}
T.run_once(bt, cache, outp, None, None)          # one uncounted process first
for rep in range(args.reps):
    order = ("parent", "head") if rep % 2 == 0 else ("head", "parent")
    for pos, name in enumerate(order):
        time.sleep(0.5)
        st = T.run_once(bt, cache, outp, None, parent if name == "parent" else None)
        walls[name].append(st["wall_s"]); ingest[name].append(st["t_load_hits_s"]); by_pos[(name, pos)].append(st["wall_s"])
        print(f"rep {rep} pos {pos} {name:6s} wall {st['wall_s']:.3f} s ingest {st['t_load_hits_s']:.3f} s", flush=True)
r = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "all": [round(x, 4) for x in v]}
out = {"lines": 100000000, "reps": args.reps, "wall_s": {k: r(v) for k, v in walls.items()}, "ingest_s": {k: r(v) for k, v in ingest.items()},
       "wall_s_by_position": {f"{k[0]}_{'first' if k[1] == 0 else 'second'}": r(v) for k, v in by_pos.items()}}
print(json.dumps(out))
if args.json:
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
