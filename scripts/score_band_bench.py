#!/usr/bin/env python3
"""Bit-score band timings -> profiles/score_band_bench.json:

    python scripts/score_band_bench.py [--out profiles/score_band_bench.json] [--queries 10000000] [--e2e-queries 2000000]
        [--parent-lib OLD/libblu_consensus.so] [--skip-kernel] [--skip-e2e]

1. blu_hits_score_band in place on device tables — the C3 shape (10 M queries x 50 hits), the all-tie table (2 M queries,
   every hit of a query on the top score) and the Zipf table (C5: 1 M queries, 1..5000 hits) that bench.py uses — for
   --top-percent 0, 1 and 10, timed by events around the call, median and best of 5 after a warm-up, the column restored
   from a copy before every call (outside the events).  Each timing stands next to the traffic floor — 4 B read per hit,
   4 B written per raised hit — at the read-only streaming rate scripts/probe/stream_probe.hip measures on the
   box in the same process.  blu_consensus_run is timed on the column before and after the raise: wider top groups cost the
   engine more, and that cost belongs to the band as much as the pass does.
2. The 2 M-query end-to-end use-case (scripts/e2e_bench.py's inputs) with and without --top-percent 1, each run in a fresh
   process, three alternating pairs, median and best; with --parent-lib the run without the flag also against the parent
   commit's library (same ABI), whose own run-to-run spread is the margin the unflagged run has to stay within.
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

TABLES = (dict(name="c3", config="C3", top_group="geo", queries=None),
          dict(name="all_tie", config="C3", top_group="all", queries=2_000_000),
          dict(name="zipf", config="C5", top_group="geo", queries=None))


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


PERCENTS = ("0", "1", "10")


def kernel_part(n_q):
    import torch
    from blutils_amd import engine, pipeline, synth
    rate = stream_rate(torch)
    out = {"stream_gb_s": None if rate is None else round(rate, 1)}
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
        dh = synth.make_hits(tax, nq, seed, cfg["hits_per_query"], zipf=cfg["zipf"], device="cuda:0", columns="milli",
                             top_group=w["top_group"])
        for a in range(0, dh.n_hits, 1 << 26):
            b = min(dh.n_hits, a + (1 << 26))
            dh.tax_row[a:b] = t.engine_rows(dh.tax_row[a:b])
        hits = dh.as_dict("packed", tax=t)
        col = hits["bitscore"]
        orig = col.clone()
        recs = torch.zeros(32 * nq, dtype=torch.uint8, device="cuda:0")
        res = {"queries": nq, "hits": dh.n_hits,
               "consensus_run_before": timed(torch, lambda: engine.run_consensus_device(t, hits, recs, strategy="relaxed"))}
        for pct in PERCENTS:
            milli = pipeline.top_percent_milli(pct)
            counts = {}

            def band():
                counts.update(engine.score_band_device(hits["seg_off"], col, milli, None))

            ms = []
            for rep in range(6):                     # (the first is the warm-up)
                col.copy_(orig)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                band()                               # (synchronises inside: the events bracket kernel + count read-back)
                b.record()
                torch.cuda.synchronize()
                if rep:
                    ms.append(a.elapsed_time(b))
            floor_bytes = 4 * dh.n_hits + 4 * counts["n_raised"]
            r = {"band": {"median_ms": round(statistics.median(ms), 4), "best_ms": round(min(ms), 4), "all_ms": [round(x, 4) for x in ms]},
                 "n_raised": counts["n_raised"], "n_widened": counts["n_widened"], "floor_bytes": floor_bytes,
                 "floor_ms_at_stream_rate": None if rate is None else round(floor_bytes / rate / 1e6, 4),
                 "consensus_run_after": timed(torch, lambda: engine.run_consensus_device(t, hits, recs, strategy="relaxed"))}
            if rate is not None:
                r["band_over_floor"] = round(r["band"]["median_ms"] / r["floor_ms_at_stream_rate"], 3)
            r["run_after_over_before"] = round(r["consensus_run_after"]["median_ms"] / res["consensus_run_before"]["median_ms"], 3)
            res[f"top_percent_{pct}"] = r
        out[w["name"]] = res
        print(w["name"], json.dumps(res), flush=True)
        del hits, recs, dh, col, orig
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
                    "parse=False, out_path=%r, score_band={'top_percent': '1'})" % (bt, cache, outp)}
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
    res = {"queries": n_q, "top_percent": "1"}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_band_bench.json"))
    ap.add_argument("--queries", type=int, default=10_000_000)
    ap.add_argument("--e2e-queries", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/blu_score_band_bench")
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
