#!/usr/bin/env python3
"""Count-table timings -> profiles/count_table_bench.json:

    python scripts/count_table_bench.py [--out profiles/count_table_bench.json] [--rows 200000] [--samples 500]
        [--density 0.05] [--taxa 2400000] [--reps 5]

blu_consensus_sample_table_counts on device records of the C3 shape (one query per row of the table, 2.4 M taxids) with a
synthetic CSR of `rows` x `samples` at `density`: device time by events (best and median of `reps`) and wall time of the call
(host ordering included), beside blu_consensus_sample_table on the same records with one sample per query — the yardstick —
and the traffic floor: the CSR bytes plus one record and one lineage row per query.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(n_q, n_samples, density, n_tax, reps):
    import numpy as np
    import torch
    from blutils_amd import engine, report, synth
    tax = synth.make_taxonomy(n_tax, synth.SEEDS["C3"])
    t = engine.Taxonomy(tax.lin_off, tax.lin_node, tax.lin_rank, tax.rank_names, taxon="bacteria", device=0)
    dh = synth.make_hits(tax, n_q, synth.SEEDS["C3"], 4, device="cuda:0")
    dh.tax_row = t.engine_rows(dh.tax_row).contiguous()
    recs = torch.zeros(32 * n_q, dtype=torch.uint8, device="cuda:0")
    engine.run_consensus_device(t, dh.as_dict(), recs, strategy="relaxed")
    torch.cuda.synchronize()
    # the CSR: a binomial number of distinct samples per row, counts 1 .. 1000
    rng = np.random.default_rng(22)
    lengths = rng.binomial(n_samples, density, n_q)
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    nnz = int(row_ptr[-1])
    sample = np.concatenate([rng.choice(n_samples, int(k), replace=False) for k in lengths]).astype(np.uint32) if nnz else np.zeros(0, np.uint32)
    count = rng.integers(1, 1001, nnz).astype(np.uint32)
    dev = lambda a, dt: torch.from_numpy(a.view(dt)).to("cuda:0")
    d_ptr, d_s, d_c = dev(row_ptr, np.int64), dev(sample, np.int32), dev(count, np.int32)
    one = (torch.arange(n_q, device="cuda:0", dtype=torch.int64) * n_samples // n_q).to(torch.int32)
    out = {}
    for name, call in (("counts", lambda: report.consensus_sample_table_counts(t, dh.tax_row, recs, dh.n_hits, d_ptr, d_s, d_c, n_samples)),
                       ("one_sample_per_query", lambda: report.consensus_sample_table(t, dh.tax_row, recs, dh.n_hits, one, n_samples))):
        devms, wall, last = [], [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            last = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            devms.append(last["t_device_ms"])
        out[name] = {"paths": int(len(last["paths"])), "cells": int(len(last["cells"])), "table_slots": last["table_slots"],
                     "attempts": last["attempts"], "device_ms_best": round(min(devms), 4),
                     "device_ms_median": round(statistics.median(devms), 4), "device_ms_all": [round(x, 4) for x in devms],
                     "call_ms_best": round(min(wall), 3), "call_ms_median": round(statistics.median(wall), 3)}
        print(name, json.dumps(out[name]), flush=True)
    depth = int((tax.lin_off[1:] - tax.lin_off[:-1]).mean())
    floor = 8 * nnz + 8 * (n_q + 1) + 32 * n_q + 4 * (depth + 1) * n_q
    out["shape"] = {"rows": n_q, "samples": n_samples, "density": density, "taxa": n_tax, "non_zeros": nnz, "mean_depth": depth}
    out["traffic_floor_bytes"] = int(floor)
    out["over_one_sample_per_query_median"] = round(out["counts"]["device_ms_median"] / out["one_sample_per_query"]["device_ms_median"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "count_table_bench.json"))
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--samples", type=int, default=500)
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--taxa", type=int, default=2_400_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    res = measure(args.rows, args.samples, args.density, args.taxa, args.reps)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
