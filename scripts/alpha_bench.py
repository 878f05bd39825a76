#!/usr/bin/env python3
"""Alpha-diversity timings -> profiles/alpha_bench.json:

    python scripts/alpha_bench.py [--out profiles/alpha_bench.json] [--rows 200000] [--samples 500] [--density 0.05]
        [--reads 50000] [--reps 5]

blu_sample_alpha on the synthetic CSR of scripts/rarefy_bench.py (`rows` features x `samples` at `density`, about `reads` reads
a sample): raw, and along ladders of 1, 10 and 32 depths up to the smallest sample total (every sample reaches every depth) —
device time by events and the wall time of the call, medians of `reps` after one warm-up call each — beside blu_sample_rarefy
at that depth, measured in the same process.  What is reported is the ladder's device time as a multiple of the single
rarefaction's.  Every present slot is checked to hold its depth (the library checks that itself) and the ladder's last slot is
checked against the rarefied table: the same n, observed, singletons and sum of squares.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(call, reps):
    devms, wall, last = [], [], None
    for _ in range(reps + 1):                       # (the first call loads the code object: not counted)
        t0 = time.perf_counter()
        last = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        devms.append(last["t_device_ms"])
    devms, wall = devms[1:], wall[1:]
    return last, {"device_ms_median": round(statistics.median(devms), 4), "device_ms_all": [round(x, 4) for x in devms],
                  "call_ms_median": round(statistics.median(wall), 3)}


def measure(n_f, n_samples, density, reads, reps):
    import numpy as np
    from blutils_amd import _native as N
    from blutils_amd import distance, diversity
    rng = np.random.default_rng(26)
    lengths = rng.binomial(n_samples, density, n_f)
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    nnz = int(row_ptr[-1])
    sample = np.concatenate([np.sort(rng.choice(n_samples, int(k), replace=False)) for k in lengths]).astype(np.uint32)
    top = max(1, round(2 * reads / (n_f * density)) - 1)
    count = rng.integers(1, top + 1, nnz).astype(np.uint64)
    total = np.zeros(n_samples, np.uint64)
    np.add.at(total, sample, count)
    depth, n_reads = int(total.min()), int(total.sum())
    names = [f"sample-{a}" for a in range(n_samples)]
    out = {"shape": {"rows": n_f, "samples": n_samples, "density": density, "non_zeros": nnz, "reads": n_reads, "depth": depth,
                     "select_tile": N.RAREFY_TILE, "level_tile": N.ALPHA_TILE}}
    rare, out["rarefy"] = timed(lambda: distance.rarefy(row_ptr, sample, count, names, depth, seed=27), reps)
    print("rarefy", json.dumps(out["rarefy"]), flush=True)
    _, out["raw"] = timed(lambda: diversity.alpha(row_ptr, sample, count, names), reps)
    print("raw", json.dumps(out["raw"]), flush=True)
    base = out["rarefy"]["device_ms_median"]
    for k in (1, 10, 32):
        depths = sorted({max(1, j * depth // k) for j in range(1, k + 1)})
        got, res = timed(lambda: diversity.alpha(row_ptr, sample, count, names, depths, seed=27), reps)
        assert got["present"].all() and (got["n"] == np.array(depths, np.uint64)[None, :]).all()
        x = rare["count"]
        for f, w in (("observed", np.ones_like(x)), ("singletons", (x == 1).astype(np.uint64)), ("sum_sq", x * x)):
            sums = np.zeros(n_samples, np.uint64)
            np.add.at(sums, rare["sample"], w)
            assert (sums == got[f][:, -1]).all(), f
        res["depths"] = len(depths)
        res["device_time_as_a_multiple_of_one_rarefaction"] = round(res["device_ms_median"] / base, 3)
        out[f"ladder_{k}"] = res
        print(f"ladder_{k}", json.dumps(res), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alpha_bench.json"))
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
