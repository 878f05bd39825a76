#!/usr/bin/env python3
"""Rarefaction timings -> profiles/rarefy_bench.json:

    python scripts/rarefy_bench.py [--out profiles/rarefy_bench.json] [--rows 200000] [--samples 500] [--density 0.05]
        [--reads 50000] [--reps 5]

blu_sample_rarefy on the synthetic CSR of scripts/distance_bench.py (`rows` features x `samples` at `density`), its counts
scaled to about `reads` reads a sample, at the depth of the smallest sample (every sample is kept): device time by events
(transpose, radix select, count; best and median of `reps` after one warm-up call), the wall time of the call (validation,
upload, download and the host's assembly included) and the reads walked per second of device time — beside t_device_ms of
blu_sample_distances on the same un-rarefied table, measured in the same run.  Every kept column is checked to sum to the depth.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(n_f, n_samples, density, reads, reps):
    import numpy as np
    from blutils_amd import _native as N
    from blutils_amd import distance
    rng = np.random.default_rng(26)
    lengths = rng.binomial(n_samples, density, n_f)
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    nnz = int(row_ptr[-1])
    sample = np.concatenate([np.sort(rng.choice(n_samples, int(k), replace=False)) for k in lengths]).astype(np.uint32)
    top = max(1, round(2 * reads / (n_f * density)) - 1)            # counts 1 .. top: their mean times the non-zeros of a sample is `reads`
    count = rng.integers(1, top + 1, nnz).astype(np.uint64)
    total = np.zeros(n_samples, np.uint64)
    np.add.at(total, sample, count)
    depth, n_reads = int(total.min()), int(total.sum())
    names = [f"sample-{a}" for a in range(n_samples)]
    out = {"shape": {"rows": n_f, "samples": n_samples, "density": density, "non_zeros": nnz, "reads": n_reads,
                     "reads_per_sample_min_median_max": [int(total.min()), int(np.median(total)), int(total.max())], "depth": depth,
                     "tile": N.RAREFY_TILE, "hash_evaluations_per_read": 9}}
    devms, wall, last = [], [], None
    for _ in range(reps + 1):                       # (the first call loads the code object: not counted)
        t0 = time.perf_counter()
        last = distance.rarefy(row_ptr, sample, count, names, depth, seed=27)
        wall.append((time.perf_counter() - t0) * 1e3)
        devms.append(last["t_device_ms"])
    sums = np.zeros(n_samples, np.uint64)
    np.add.at(sums, last["sample"], last["count"])
    assert len(last["kept_sample"]) == n_samples and (sums == depth).all()
    devms, wall = devms[1:], wall[1:]
    med = statistics.median(devms)
    out["rarefy"] = {"device_ms_best": round(min(devms), 4), "device_ms_median": round(med, 4), "device_ms_all": [round(x, 4) for x in devms],
                     "call_ms_best": round(min(wall), 3), "call_ms_median": round(statistics.median(wall), 3),
                     "reads_per_second_of_device_time": round(n_reads / (med * 1e-3)), "rarefied_non_zeros": int(last["row_ptr"][-1])}
    print("rarefy", json.dumps(out["rarefy"]), flush=True)
    dist = []
    for _ in range(reps + 1):
        dist.append(distance.sample_distances(row_ptr, sample, count, n_samples)["t_device_ms"])
    dist = dist[1:]
    out["distances_unrarefied"] = {"device_ms_best": round(min(dist), 4), "device_ms_median": round(statistics.median(dist), 4),
                                   "device_ms_all": [round(x, 4) for x in dist]}
    print("distances", json.dumps(out["distances_unrarefied"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rarefy_bench.json"))
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--samples", type=int, default=500)
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--reads", type=int, default=50_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    res = measure(args.rows, args.samples, args.density, args.reads, args.reps)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
