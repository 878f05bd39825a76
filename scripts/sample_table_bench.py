#!/usr/bin/env python3
"""Per-sample table timings -> profiles/sample_table_bench.json:

    python scripts/sample_table_bench.py [--out profiles/sample_table_bench.json] [--queries 10000000] [--taxa 2400000]
        [--e2e-queries 2000000] [--reps 3]

1. blu_consensus_sample_table on device records of the C3 shape (10 M queries, 2.4 M taxids) with 1 and 100 samples in
   contiguous runs and 100 samples at random, and on the few-species table of scripts/report_bench.py with 100 samples:
   device time by events (best and median of 5) and wall time of the call (host ordering included), beside
   blu_consensus_report on the same records in the same process.
2. The 2 M-query end-to-end use-case (scripts/e2e_bench.py's inputs, query names `S<k>.<q>` in 100 contiguous samples) with
   and without --sample-table, each repetition in a fresh process, the two alternating.
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


def kernel_part(n_q, n_tax):
    import numpy as np
    import torch
    from blutils_amd import engine, report, synth
    tax = synth.make_taxonomy(n_tax, synth.SEEDS["C3"])
    t = engine.Taxonomy(tax.lin_off, tax.lin_node, tax.lin_rank, tax.rank_names, taxon="bacteria", device=0)
    dh = synth.make_hits(tax, n_q, synth.SEEDS["C3"], 4, device="cuda:0")
    rows = t.engine_rows(dh.tax_row).contiguous()
    contiguous = lambda k: (torch.arange(n_q, device="cuda:0", dtype=torch.int64) * k // n_q).to(torch.int32)
    g = torch.Generator(device="cuda:0").manual_seed(7)
    samples = {"1_contiguous": (contiguous(1), 1), "100_contiguous": (contiguous(100), 100),
               "100_random": (torch.randint(0, 100, (n_q,), device="cuda:0", generator=g, dtype=torch.int32), 100)}
    out = {}
    for shape, few, cases in (("c3", 0, ("1_contiguous", "100_contiguous", "100_random")),
                              ("few_species", 10, ("100_contiguous", "100_random"))):
        r = rows
        if few:
            pick = torch.tensor(t.row_map()[0][np.linspace(0, n_tax - 1, few).astype(np.int64)].astype(np.int64), device="cuda:0")
            r = torch.where(rows != -1, pick[dh.bitscore.to(torch.int64) % few].to(torch.int32), rows)
        dh.tax_row = r.contiguous()
        recs = torch.zeros(32 * n_q, dtype=torch.uint8, device="cuda:0")
        engine.run_consensus_device(t, dh.as_dict(), recs, strategy="relaxed")
        torch.cuda.synchronize()
        rdev = []
        for _ in range(5):
            rdev.append(report.consensus_report(t, dh.tax_row, recs, dh.n_hits)["t_device_ms"])
        for case in cases:
            s, ns = samples[case]
            dev, wall, last = [], [], None
            for _ in range(5):
                t0 = time.perf_counter()
                last = report.consensus_sample_table(t, dh.tax_row, recs, dh.n_hits, s, ns)
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(last["t_device_ms"])
            name = f"{shape}_{case}"
            out[name] = {"queries": n_q, "taxa": n_tax, "samples": ns, "paths": int(len(last["paths"])),
                         "cells": int(len(last["cells"])), "table_slots": last["table_slots"], "attempts": last["attempts"],
                         "device_ms_best": round(min(dev), 4), "device_ms_median": round(statistics.median(dev), 4),
                         "device_ms_all": [round(x, 4) for x in dev], "call_ms_best": round(min(wall), 3),
                         "call_ms_median": round(statistics.median(wall), 3),
                         "report_device_ms_best": round(min(rdev), 4), "report_device_ms_median": round(statistics.median(rdev), 4)}
            out[name]["over_report_median"] = round(out[name]["device_ms_median"] / out[name]["report_device_ms_median"], 2)
            print(name, json.dumps(out[name]), flush=True)
        del recs
    return out


def e2e_part(n_q, reps, d):
    os.makedirs(d, exist_ok=True)
    gen = os.path.join(d, "gen_blast")
    subprocess.run(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "scripts", "tools", "gen_blast.c")], check=True)
    tj, cache = os.path.join(d, "tax.blutils.json"), os.path.join(d, "tax.blucache")
    bt = os.path.join(d, f"blast.{n_q}x50.clustered.s100.tsv")
    subprocess.run([gen, "db", tj, "300000"], check=True)
    if not os.path.exists(bt):
        subprocess.run([gen, "table", bt, str(n_q), "50", "300000", "1", "clustered", "100"], check=True)
    from blutils_amd import pipeline
    pipeline.build_db_cache(tj, cache, False)
    outp, tab = os.path.join(d, "consensus.jsonl"), os.path.join(d, "table.tsv")
    call = {False: "pipeline.build_consensus_identities(%r, %r, 'bacteria', 'relaxed', out_format='jsonl', lenient=True, parse=False, out_path=%r)"
                   % (bt, cache, outp),
            True: "pipeline.build_consensus_identities_with_tables(%r, %r, 'bacteria', 'relaxed', out_format='jsonl', lenient=True, parse=False, out_path=%r, sample_table_path=%r)"
                  % (bt, cache, outp, tab)}
    walls = {False: [], True: []}
    for k in range(reps):
        for with_table in (False, True):
            code = ("import sys, json, time; sys.path.insert(0, %r); from blutils_amd import pipeline; t0 = time.perf_counter(); %s; "
                    "print(json.dumps(time.perf_counter() - t0))" % (ROOT, call[with_table]))
            time.sleep(0.5)
            p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-4000:])
                raise SystemExit(1)
            walls[with_table].append(round(json.loads(p.stdout.strip().splitlines()[-1]), 4))
            print("table" if with_table else "plain", walls[with_table][-1], flush=True)
    res = {"queries": n_q, "samples": 100, "wall_s_without": walls[False], "wall_s_with": walls[True],
           "best_without_s": min(walls[False]), "best_with_s": min(walls[True]),
           "median_without_s": statistics.median(walls[False]), "median_with_s": statistics.median(walls[True]),
           "table_bytes": os.path.getsize(tab)}
    res["added_pct_best"] = round(100.0 * (res["best_with_s"] / res["best_without_s"] - 1.0), 2)
    res["added_pct_median"] = round(100.0 * (res["median_with_s"] / res["median_without_s"] - 1.0), 2)
    for f in (outp, tab):
        if os.path.exists(f):
            os.remove(f)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_table_bench.json"))
    ap.add_argument("--queries", type=int, default=10_000_000)
    ap.add_argument("--taxa", type=int, default=2_400_000)
    ap.add_argument("--e2e-queries", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/blu_sample_table_bench")
    ap.add_argument("--skip-e2e", action="store_true")
    args = ap.parse_args()
    res = {"kernel": kernel_part(args.queries, args.taxa)}
    if not args.skip_e2e:
        res["e2e"] = e2e_part(args.e2e_queries, args.reps, args.dir)
    res["targets"] = {"device_over_report": 3.0, "e2e_added_pct": 5.0}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
