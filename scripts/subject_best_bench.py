#!/usr/bin/env python3
"""Best-hit-per-subject timings -> profiles/subject_best_bench.json:

    python scripts/subject_best_bench.py [--out profiles/subject_best_bench.json] [--queries 10000000] [--e2e-queries 2000000]
        [--parent-lib OLD/libblu_consensus.so] [--skip-kernel] [--skip-e2e]

1. blu_hits_subject_keep (the verdicts) and blu_hits_subject_best (verdicts + compaction, device pointers, in place) on device
   tables — the C3 shape (10 M queries x 50 hits) with no duplicate pair (nothing dropped, the compaction skipped), the C3
   shape with every subject written twice (half dropped), and the Zipf table (C5: 1 M queries, 1..5000 hits) of bench.py with
   every subject twice, which exercises the long path — timed by events around the call, median and best of 5 after a
   warm-up, the columns and offsets restored from copies before every call (outside the events).
2. Each timing stands next to its traffic floor at the read-only streaming rate scripts/probe/stream_probe.hip measures on
   the box in the same process.  Verdicts: 8 B read + 4 B written per row.  The compacting call, from the code
   (csrc/subject_kernel.hip: subject_best_device, the device-pointer route), n rows in and k kept: the keep words cleared (4 n
   written) and decided (8 n read, 4 n written), then — only if k < n — their scan (4 n read, 4 n written), the five gathers
   (24 n of columns + 5 x 4 n of keep words read, 24 k written), the copy back to the caller's buffers (24 k read, 24 k
   written) and the offsets; and the unmatched count (4 k read).
3. The 2 M-query end-to-end use-case (scripts/e2e_bench.py's inputs) with and without best_hit_per_subject, each run in a
   fresh process, three alternating pairs, median and best.
4. With --parent-lib the run without the flag also against the parent commit's library (same ABI), whose own run-to-run
   spread, measured in the same session, is the margin the unflagged run has to stay within.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

def stream_rate(torch, gib=4.0):
    """GB/s of the box's read-only streaming probe (None without the probe library)."""
    so = os.path.join(ROOT, "blutils_amd", "lib", "libblu_probe.so")
    if not os.path.exists(so):
        return None
    L = ctypes.CDLL(so)
    L.probe_read.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    nbytes = int(gib * (1 << 30))
    buf = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda").fill_(1)
    sink = torch.zeros(4, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    best = 0.0
    for grid in (2048, 4096, 8192):
        for _ in range(2):
            L.probe_read(buf.data_ptr(), nbytes, sink.data_ptr(), grid, s)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(5):
            L.probe_read(buf.data_ptr(), nbytes, sink.data_ptr(), grid, s)
        b.record()
        torch.cuda.synchronize()
        best = max(best, nbytes * 5 / (a.elapsed_time(b) * 1e-3) / 1e9)
    del buf
    torch.cuda.empty_cache()
    return best


def timed(torch, fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ms), 4), "best_ms": round(min(ms), 4), "all_ms": [round(x, 4) for x in ms]}


TABLES = (dict(name="c3_no_duplicates", config="C3", twice=False),
          dict(name="c3_every_subject_twice", config="C3", twice=True),
          dict(name="zipf_every_subject_twice", config="C5", twice=True))


def floors(n, k):
    """(verdict pass, compacting call) traffic floors in bytes: see the head of this file"""
    keep = 12 * n
    best = 4 * n + keep + 4 * k
    if k < n:
        best += 8 * n + (24 + 20) * n + 24 * k + 48 * k
    return keep, best


def kernel_part(n_q):
    import torch
    from blutils_amd import engine, synth
    rate = stream_rate(torch)
    out = {"stream_gb_s": None if rate is None else round(rate, 1)}
    for w in TABLES:
        cfg = dict(synth.CONFIGS[w["config"]])
        seed = synth.SEEDS[w["config"]]
        tax = synth.make_taxonomy(cfg["n_taxa"], seed, deep=cfg["deep"])
        nq = n_q if w["config"] == "C3" else cfg["n_queries"]
        dh = synth.make_hits(tax, nq, seed, cfg["hits_per_query"], zipf=cfg["zipf"], device="cuda:0", columns="f64")
        n = dh.n_hits
        # the subjects: the row number (no pair twice), or half of it (rows 2 i and 2 i + 1 of the table are one subject; a
        # pair that a segment boundary splits is two pairs)
        row = torch.arange(n, dtype=torch.int64, device="cuda:0")
        dh.acc_rank.copy_(((row // 2 if w["twice"] else row) % (1 << 31)).to(torch.int32))
        del row
        cols = [dh.bitscore, dh.align_len, dh.tax_row, dh.acc_rank, dh.pident]
        orig = [c.clone() for c in cols]
        seg, seg_orig = dh.seg_off, dh.seg_off.clone()
        keep = torch.empty(n, dtype=torch.int32, device="cuda:0")
        counts = {}

        def run(fn, restore):
            ms = []
            for rep in range(6):                     # (the first is the warm-up)
                if restore:
                    for c, o in zip(cols, orig):
                        c.copy_(o)
                    seg.copy_(seg_orig)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()                                 # (synchronises inside: the events bracket the kernels + the count read-backs)
                b.record()
                torch.cuda.synchronize()
                if rep:
                    ms.append(a.elapsed_time(b))
            return {"median_ms": round(statistics.median(ms), 4), "best_ms": round(min(ms), 4), "all_ms": [round(x, 4) for x in ms]}

        t_keep = run(lambda: counts.update(engine.subject_keep_device(seg, cols[0], cols[3], keep)), False)
        t_best = run(lambda: engine.subject_best_device(seg, *cols), True)
        f_keep, f_best = floors(n, counts["n_kept"])
        res = {"queries": nq, "hits": n, "n_kept": counts["n_kept"], "n_thinned": counts["n_thinned"],
               "long_queries": int((seg_orig[1:] - seg_orig[:-1] > 64).sum().item()),
               "keep": t_keep, "keep_floor_bytes": f_keep, "best": t_best, "best_floor_bytes": f_best}
        if rate is not None:
            res["keep_floor_ms_at_stream_rate"] = round(f_keep / rate / 1e6, 4)
            res["best_floor_ms_at_stream_rate"] = round(f_best / rate / 1e6, 4)
            res["keep_over_floor"] = round(t_keep["median_ms"] / res["keep_floor_ms_at_stream_rate"], 3)
            res["best_over_floor"] = round(t_best["median_ms"] / res["best_floor_ms_at_stream_rate"], 3)
        out[w["name"]] = res
        print(w["name"], json.dumps(res), flush=True)
        del dh, cols, orig, seg, seg_orig, keep
        torch.cuda.empty_cache()
    return out


def e2e_part(n_q, reps, d, parent_lib):
    os.makedirs(d, exist_ok=True)
    gen = os.path.join(d, "gen_blast")
    subprocess.run(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "scripts", "tools", "gen_blast.c")], check=True)
    tj, cache = os.path.join(d, "tax.blutils.json"), os.path.join(d, "tax.blucache")
    bt = os.path.join(d, f"blast.{n_q}x50.clustered.tsv")
    subprocess.run([gen, "db", tj, "300000"], check=True)
    if not os.path.exists(bt):
        subprocess.run([gen, "table", bt, str(n_q), "50", "300000", "1", "clustered"], check=True)
    from blutils_amd import pipeline
    pipeline.build_db_cache(tj, cache, False)
    outp = os.path.join(d, "consensus.jsonl")
    plain = ("pipeline.build_consensus_identities(%r, %r, 'bacteria', 'relaxed', out_format='jsonl', lenient=True, parse=False, out_path=%r)"
             % (bt, cache, outp))
    call = {"parent": plain, "without": plain,
            "with": "pipeline.build_consensus_identities(%r, %r, 'bacteria', 'relaxed', out_format='jsonl', lenient=True, "
                    "parse=False, out_path=%r, best_hit_per_subject=True)" % (bt, cache, outp)}
    variants = (["parent"] if parent_lib else []) + ["without", "with"]
    walls = {v: [] for v in variants}
    for _ in range(reps):
        for v in variants:
            code = ("import sys, json, time; sys.path.insert(0, %r); from blutils_amd import pipeline; t0 = time.perf_counter(); %s; "
                    "print(json.dumps(time.perf_counter() - t0))" % (ROOT, call[v]))
            env = dict(os.environ)
            if v == "parent":
                env["BLU_CONSENSUS_LIB"] = parent_lib
            time.sleep(0.5)
            p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-4000:])
                raise SystemExit(1)
            walls[v].append(round(json.loads(p.stdout.strip().splitlines()[-1]), 4))
            print(v, walls[v][-1], flush=True)
    res = {"queries": n_q}
    for v in variants:
        res[v] = {"wall_s": walls[v], "median_s": statistics.median(walls[v]), "best_s": min(walls[v])}
    res["added_pct_median"] = round(100.0 * (res["with"]["median_s"] / res["without"]["median_s"] - 1.0), 2)
    res["added_pct_best"] = round(100.0 * (res["with"]["best_s"] / res["without"]["best_s"] - 1.0), 2)
    if parent_lib:
        spread = max(walls["parent"]) - min(walls["parent"])
        res["parent_spread_s"] = round(spread, 4)
        res["without_minus_parent_median_s"] = round(res["without"]["median_s"] - res["parent"]["median_s"], 4)
        res["unflagged_path_within_parent_spread"] = abs(res["without_minus_parent_median_s"]) <= spread
    if os.path.exists(outp):
        os.remove(outp)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subject_best_bench.json"))
    ap.add_argument("--queries", type=int, default=10_000_000)
    ap.add_argument("--e2e-queries", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/blu_subject_best_bench")
    ap.add_argument("--parent-lib", help="libblu_consensus.so built from the parent commit (same ABI)")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    args = ap.parse_args()
    res = {}
    if not args.skip_kernel:
        res["kernel"] = kernel_part(args.queries)
    if not args.skip_e2e:
        res["e2e"] = e2e_part(args.e2e_queries, args.reps, args.dir, args.parent_lib)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
