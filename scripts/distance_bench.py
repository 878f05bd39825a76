#!/usr/bin/env python3
"""Sample-distance timings -> profiles/distance_bench.json:

    python scripts/distance_bench.py [--out profiles/distance_bench.json] [--rows 200000] [--samples 500] [--density 0.05]
        [--reps 5]

blu_sample_distances on a synthetic CSR of `rows` features x `samples` at `density` (the shape of
scripts/count_table_bench.py): device time by events (transpose + pair kernel; best and median of `reps`) and the wall time
of the call (validation, upload and download included), beside the same integers on ONE host thread in the same process
(scripts/probe/distance_host.cpp, a measurement aid): the merge of two sorted lists per pair, which is the device kernel's
order of work, and the row-wise form a sparse table allows.  The host results are compared with the device's.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(n_f, n_samples, density, reps):
    import numpy as np
    from blutils_amd import distance
    rng = np.random.default_rng(26)
    lengths = rng.binomial(n_samples, density, n_f)
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    nnz = int(row_ptr[-1])
    sample = np.concatenate([np.sort(rng.choice(n_samples, int(k), replace=False)) for k in lengths]).astype(np.uint32)
    count = rng.integers(1, 1001, nnz).astype(np.uint64)
    out = {"shape": {"rows": n_f, "samples": n_samples, "density": density, "non_zeros": nnz,
                     "compare_and_adds_by_pair": int(n_samples) * nnz}}
    devms, wall, last = [], [], None
    for _ in range(reps + 1):                       # (the first call loads the code object: not counted)
        t0 = time.perf_counter()
        last = distance.sample_distances(row_ptr, sample, count, n_samples)
        wall.append((time.perf_counter() - t0) * 1e3)
        devms.append(last["t_device_ms"])
    devms, wall = devms[1:], wall[1:]
    out["device"] = {"device_ms_best": round(min(devms), 4), "device_ms_median": round(statistics.median(devms), 4),
                     "device_ms_all": [round(x, 4) for x in devms], "call_ms_best": round(min(wall), 3),
                     "call_ms_median": round(statistics.median(wall), 3)}
    print("device", json.dumps(out["device"]), flush=True)
    probe = C.CDLL(os.path.join(ROOT, "blutils_amd", "lib", "libblu_distance_probe.so"))
    for name in ("distance_host_merge", "distance_host_rows"):
        fn = getattr(probe, name)
        fn.restype = None
        fn.argtypes = [C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        m = np.zeros((n_samples, n_samples), np.uint64)
        s = np.zeros((n_samples, n_samples), np.uint32)
        t0 = time.perf_counter()
        fn(n_f, n_samples, row_ptr.ctypes.data, sample.ctypes.data, count.ctypes.data, m.ctypes.data, s.ctypes.data)
        ms = (time.perf_counter() - t0) * 1e3
        same = bool((m == last["min_sum"]).all() and (s == last["shared"]).all())
        out[name] = {"host_ms_one_thread_one_run": round(ms, 1), "equals_device": same,
                     "over_device_median": round(ms / out["device"]["device_ms_median"], 1)}
        print(name, json.dumps(out[name]), flush=True)
        assert same, name
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_bench.json"))
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--samples", type=int, default=500)
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    res = measure(args.rows, args.samples, args.density, args.reps)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
