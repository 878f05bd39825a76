#!/usr/bin/env python3
"""What the taxon filters of build-consensus cost:

    python scripts/taxon_filter_bench.py [--queries 2000000] [--hits 50] [--taxa 300000] [--reps 3]
        [--parent-lib OLD/libblu_consensus.so] [--json profiles/taxon_filter_bench.json]

The table is scripts/e2e_bench.py's (scripts/tools/gen_blast.c: every subject under `d__bacteria`, 96 species to a family
`f__fam<k>`), read from a warm page cache; the database lists one family more than the table names, so that a list can name
a taxon no line holds.  Every run is a FRESH process (HIP start-up inside the wall time) of
build_consensus_identities(..., out_path=...), JSONL out; the variants alternate inside every repetition:

  parent        the unfiltered use-case with --parent-lib (the library of the commit before the filters), if given
  unfiltered    the same with this tree's library: must sit inside the spread of `parent`
  exclude_none  --exclude-taxon f__fam<last>: a family of the database that no line of the table names — the cost of the code
                table, its upload, the verdict and the keep words (every line kept: no compaction)
  exclude_half  --exclude-taxon f__fam1* f__fam3* f__fam4* f__fam5*: about half the families — plus the per-wave counts, the
                scan and the scatter; less work after the parse
  only_domain   --only-taxon d__bacteria: the one domain this table has, so nothing is dropped — the only-list verdict alone

Prints one line per run and a JSON summary (median and min/max per variant, added milliseconds over `unfiltered` for the
three filters, `unfiltered` against `parent` with the parent's spread); --json also writes it to a file.
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

EXCLUDE_HALF = ["f__fam1*", "f__fam3*", "f__fam4*", "f__fam5*"]
ONLY_DOMAIN = ["d__bacteria"]


def run_once(table, cache, outp, taxon_filter, lib):
    code = ("import sys, json, time; sys.path.insert(0, %r); from blutils_amd import pipeline; t0 = time.perf_counter(); "
            "_, st = pipeline.build_consensus_identities(%r, %r, 'bacteria', 'relaxed', out_format='jsonl', lenient=True, parse=False, "
            "out_path=%r%s); st['wall_s'] = time.perf_counter() - t0; st['path'] = pipeline.last_ingest_path(); print(json.dumps(st))"
            % (ROOT, table, cache, outp, ", taxon_filter=%r" % (taxon_filter,) if taxon_filter else ""))
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
    ap.add_argument("--parent-lib", help="libblu_consensus.so built from the parent commit (same ABI)")
    ap.add_argument("--dir", default="/tmp/blu_taxon_filter")
    ap.add_argument("--pause", type=float, default=0.5, help="seconds between processes")
    ap.add_argument("--json", help="also write the summary here")
    args = ap.parse_args()
    os.makedirs(args.dir, exist_ok=True)
    gen = os.path.join(args.dir, "gen_blast")
    subprocess.run(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "scripts", "tools", "gen_blast.c")], check=True)
    tj, cache = os.path.join(args.dir, "tax.blutils.json"), os.path.join(args.dir, "tax.blucache")
    bt = os.path.join(args.dir, f"blast.{args.queries}x{args.hits}.tsv")
    taxa = -(-args.taxa // 96) * 96                 # whole families in the table's range, then one family more in the database
    subprocess.run([gen, "db", tj, str(taxa + 96)], check=True)
    if not os.path.exists(bt):
        subprocess.run([gen, "table", bt, str(args.queries), str(args.hits), str(taxa), "1", "clustered"], check=True)
    from blutils_amd import pipeline
    pipeline.build_db_cache(tj, cache, False)
    size = os.path.getsize(bt)
    with open(bt, "rb") as f:                       # warm page cache
        while f.read(1 << 26):
            pass
    print(f"table: {args.queries} queries x {args.hits} hits = {size / 1e9:.2f} GB of text", flush=True)
    outp = os.path.join(args.dir, "consensus.jsonl")
    exclude_none = [f"f__fam{taxa // 96}"]
    variants = [("unfiltered", None, None), ("exclude_none", {"exclude": exclude_none}, None),
                ("exclude_half", {"exclude": EXCLUDE_HALF}, None), ("only_domain", {"only": ONLY_DOMAIN}, None)]
    if args.parent_lib:
        variants.insert(0, ("parent", None, os.path.abspath(args.parent_lib)))
    walls = {name: [] for name, _, _ in variants}
    facts = {}
    for rep in range(args.reps):
        for name, flt, lib in variants:
            time.sleep(args.pause)                  # (the driver is still tearing the previous process's device memory down)
            st = run_once(bt, cache, outp, flt, lib)
            walls[name].append(st["wall_s"])
            facts[name] = {k: st.get(k) for k in ("n_hits", "n_queries", "n_lines", "n_kept", "path", "t_load_db_s", "t_load_hits_s")}
            if "taxon_filter" in st:
                facts[name].update({k: st["taxon_filter"][k] for k in ("n_excluded", "n_not_only", "excluded_by")})
            print(f"rep {rep} {name:12s} wall {st['wall_s']:.3f} s  db {st['t_load_db_s']:.3f} s  ingest {st['t_load_hits_s']:.3f} s  "
                  f"rows {st['n_hits']}  parser {st['path']}", flush=True)
    if os.path.exists(outp):
        os.remove(outp)
    med = {k: statistics.median(v) for k, v in walls.items() if v}
    summary = {"text_gb": size / 1e9, "lines": args.queries * args.hits, "reps": args.reps,
               "wall_s": {k: {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4), "all": [round(x, 4) for x in v]}
                          for k, v in walls.items() if v},
               "facts": facts}
    for k in ("exclude_none", "exclude_half", "only_domain"):
        summary[k + "_added_ms"] = round((med[k] - med["unfiltered"]) * 1e3, 1)
    if "parent" in med:
        summary["unfiltered_minus_parent_ms"] = round((med["unfiltered"] - med["parent"]) * 1e3, 1)
        summary["parent_spread_ms"] = round((max(walls["parent"]) - min(walls["parent"])) * 1e3, 1)
        summary["unfiltered_within_parent_spread"] = min(walls["parent"]) <= med["unfiltered"] <= max(walls["parent"]) or med["unfiltered"] <= med["parent"]
    n = facts["unfiltered"]["n_hits"]
    assert facts["exclude_none"]["n_kept"] == facts["exclude_none"]["n_lines"] == n and facts["exclude_none"]["n_excluded"] == 0
    assert facts["only_domain"]["n_kept"] == n and facts["only_domain"]["n_not_only"] == 0
    assert 0.4 * n < facts["exclude_half"]["n_kept"] < 0.6 * n and all(facts["exclude_half"]["excluded_by"])
    print(json.dumps(summary))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
