#!/usr/bin/env python3
"""Minimum-cover timings -> profiles/min_cover_bench.json:

    python scripts/min_cover_bench.py [--out profiles/min_cover_bench.json] [--queries 10000000] [--e2e-queries 2000000]
        [--parent-lib OLD/libblu_consensus.so] [--skip-kernel] [--skip-e2e] [--min-cover 80]

1. blu_hits_cover_keep (the verdicts) and blu_hits_cover_apply (verdicts + compaction, device pointers, in place) on device
   tables of bench.py's generator — the C3 shape (10 M queries x 50 hits, geometric top groups), the all-tie table (2 M queries
   x 50 hits, the whole segment on the top score) and the Zipf table (C5: 1 M queries, 1..5000 hits), which exercises the long
   path — with engine row ids in the row column (row_map NULL), timed by events around the call, median and best of 5 after a
   warm-up, the columns and offsets restored from copies before every compacting call (outside the events).
2. Each timing stands next to its traffic floor at the read-only streaming rate scripts/probe/stream_probe.hip measures on
   the box in the same process.  Verdicts, from the code (csrc/cover_kernel.hip: cover_keep_device), n rows and q queries: the
   keep words cleared (4 n written), the offsets (8 q), the bit-scores read (4 n), the row ids of the top rows (at most 4 n:
   counted in full) and the keep words written (4 n): 16 n + 8 q; the lcp8 / rmq reads are not counted (they are small tables
   that stay in L2), nor are the long path's further sweeps of its segments.  The compacting call, n rows in and k kept: the
   verdicts, then — only if k < n — the scan of the keep words (4 n read, 4 n written), the five gathers (24 n of columns +
   5 x 4 n of keep words read, 24 k written), the copy back to the caller's buffers (24 k read, 24 k written); and the
   unmatched count (4 k read).
3. The 2 M-query end-to-end use-case (scripts/e2e_bench.py's inputs) with and without min_cover, each run in a fresh process,
   three alternating triples, median and best.
4. With --parent-lib the run without the keyword also against the parent commit's library (same ABI), whose own run-to-run
   spread, measured in the same session, is the margin the run without the keyword has to stay within.  That is the one
   criterion; the kernels' times are reported, not judged.
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


TABLES = (dict(name="c3", config="C3", top_group="geo", queries=None),
          dict(name="all_tie", config="C3", top_group="all", queries=2_000_000),
          dict(name="zipf", config="C5", top_group="geo", queries=None))


def floors(n, q, k):
    """(verdict pass, compacting call) traffic floors in bytes: see the head of this file"""
    keep = 16 * n + 8 * q
    apply = keep + 4 * k
    if k < n:
        apply += 8 * n + (24 + 20) * n + 24 * k + 48 * k
    return keep, apply


def kernel_part(n_q, milli):
    import torch
    from blutils_amd import engine, synth
    rate = stream_rate(torch)
    out = {"stream_gb_s": None if rate is None else round(rate, 1), "min_cover_milli": milli}
    taxa = {}
    for w in TABLES:
        cfg = dict(synth.CONFIGS[w["config"]])
        seed = synth.SEEDS[w["config"]]
        key = (cfg["n_taxa"], cfg["deep"], seed)
        if key not in taxa:
            tax = synth.make_taxonomy(cfg["n_taxa"], seed, deep=cfg["deep"])
            taxa[key] = (tax, engine.Taxonomy(tax.lin_off, tax.lin_node, tax.lin_rank, tax.rank_names, taxon="bacteria", device=0))
        tax, t = taxa[key]
        nq = w["queries"] or (n_q if w["config"] == "C3" else cfg["n_queries"])
        dh = synth.make_hits(tax, nq, seed, cfg["hits_per_query"], zipf=cfg["zipf"], device="cuda:0", columns="f64",
                             top_group=w["top_group"])
        n = dh.n_hits
        for a in range(0, n, 1 << 26):
            b = min(n, a + (1 << 26))
            dh.tax_row[a:b] = t.engine_rows(dh.tax_row[a:b])
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

        t_keep = run(lambda: counts.update(engine.cover_keep_device(t, seg, cols[0], cols[2], milli, keep)), False)
        t_apply = run(lambda: engine.cover_apply_device(t, seg, *cols, milli), True)
        f_keep, f_apply = floors(n, nq, counts["n_kept"])
        res = {"queries": nq, "hits": n, "n_kept": counts["n_kept"], "n_narrowed": counts["n_narrowed"],
               "n_unresolved": counts["n_unresolved"], "long_queries": int((seg_orig[1:] - seg_orig[:-1] > 64).sum().item()),
               "keep": t_keep, "keep_floor_bytes": f_keep, "apply": t_apply, "apply_floor_bytes": f_apply}
        if rate is not None:
            res["keep_floor_ms_at_stream_rate"] = round(f_keep / rate / 1e6, 4)
            res["apply_floor_ms_at_stream_rate"] = round(f_apply / rate / 1e6, 4)
            res["keep_over_floor"] = round(t_keep["median_ms"] / res["keep_floor_ms_at_stream_rate"], 3)
            res["apply_over_floor"] = round(t_apply["median_ms"] / res["apply_floor_ms_at_stream_rate"], 3)
        out[w["name"]] = res
        print(w["name"], json.dumps(res), flush=True)
        del dh, cols, orig, seg, seg_orig, keep
        torch.cuda.empty_cache()
    return out


def e2e_part(n_q, reps, d, parent_lib, cover):
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
                    "parse=False, out_path=%r, min_cover=%r)" % (bt, cache, outp, cover)}
    variants = (["parent"] if parent_lib else []) + ["without", "with"]
    walls, counts = {v: [] for v in variants}, {}
    for _ in range(reps):
        for v in variants:
            code = ("import sys, json, time; sys.path.insert(0, %r); from blutils_amd import pipeline; t0 = time.perf_counter(); r = %s; "
                    "print(json.dumps([time.perf_counter() - t0, r[1].get('min_cover')]))" % (ROOT, call[v]))
            env = dict(os.environ)
            if v == "parent":
                env["BLU_CONSENSUS_LIB"] = parent_lib
            time.sleep(0.5)
            p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-4000:])
                raise SystemExit(1)
            wall, counts[v] = json.loads(p.stdout.strip().splitlines()[-1])
            walls[v].append(round(wall, 4))
            print(v, walls[v][-1], flush=True)
    res = {"queries": n_q, "min_cover": cover, "min_cover_counts": counts.get("with")}
    for v in variants:
        res[v] = {"wall_s": walls[v], "median_s": statistics.median(walls[v]), "best_s": min(walls[v])}
    res["added_pct_median"] = round(100.0 * (res["with"]["median_s"] / res["without"]["median_s"] - 1.0), 2)
    res["added_pct_best"] = round(100.0 * (res["with"]["best_s"] / res["without"]["best_s"] - 1.0), 2)
    if parent_lib:
        spread = max(walls["parent"]) - min(walls["parent"])
        res["parent_spread_s"] = round(spread, 4)
        res["without_minus_parent_median_s"] = round(res["without"]["median_s"] - res["parent"]["median_s"], 4)
        res["run_without_the_keyword_within_parent_spread"] = abs(res["without_minus_parent_median_s"]) <= spread
    if os.path.exists(outp):
        os.remove(outp)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "min_cover_bench.json"))
    ap.add_argument("--queries", type=int, default=10_000_000)
    ap.add_argument("--e2e-queries", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/blu_min_cover_bench")
    ap.add_argument("--parent-lib", help="libblu_consensus.so built from the parent commit (same ABI)")
    ap.add_argument("--min-cover", default="80", help="the percentage both parts run with")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    args = ap.parse_args()
    from blutils_amd import pipeline
    res = {}
    if not args.skip_kernel:
        res["kernel"] = kernel_part(args.queries, pipeline.min_cover_milli(args.min_cover))
    if not args.skip_e2e:
        res["e2e"] = e2e_part(args.e2e_queries, args.reps, args.dir, args.parent_lib, args.min_cover)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
