"""`build-db blu` at NCBI scale: fresh-process CLI-equivalent runs of the GPU builder on a synthetic new_taxdump-sized dump
(blutils_amd/synth_taxdump.py) with listings of several sizes.  Reports the stage times from blu_taxdb_stats, input and
output bytes and the wall time of the child process; on the smallest listing it also times the test-only oracle
(oracle/taxdb_oracle.py, the CPU baseline) and checks that both outputs are byte-equal.  Not part of bench.py's line.

    python scripts/db_build_bench.py --nodes 2700000 --accessions 1000000,30000000 --out profiles/db_build_bench.json
"""
import argparse
import json
import os
import shutil
import signal
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHILD = """
import json, sys, time
t0 = time.perf_counter()
from blutils_amd import taxdb
a = json.loads(sys.argv[1])
st = taxdb.build_ref_db_from_ncbi_files("nt", a["dump"], a["out"], accessions_file=a["acc"], replace_rank=[("superkingdom", "d")])
st["child_wall_s"] = time.perf_counter() - t0
print(json.dumps(st))
"""


def run_child(args: dict, timeout: float) -> dict:
    p = subprocess.Popen([sys.executable, "-c", CHILD, json.dumps(args)], cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, start_new_session=True)
    t0 = time.perf_counter()
    try:
        out, err = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)          # the child's whole process group
        p.communicate()
        raise
    wall = time.perf_counter() - t0
    if p.returncode != 0:
        raise RuntimeError(f"child failed ({p.returncode}): {err[-2000:]}")
    st = json.loads(out.strip().splitlines()[-1])
    st["process_wall_s"] = wall
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=2_700_000)
    ap.add_argument("--depth", type=int, default=25)
    ap.add_argument("--accessions", default="1000000,30000000")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--timeout", type=float, default=900)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "db_build_bench.json"))
    a = ap.parse_args()
    from blutils_amd import synth_taxdump
    sizes = [int(x) for x in a.accessions.split(",")]
    tmp = tempfile.mkdtemp(prefix="blu-db-bench-")
    result = {"nodes": a.nodes, "depth": a.depth, "runs": []}
    try:
        t0 = time.perf_counter()
        extra = {f"acc_{n}.txt": n for n in sizes}
        synth_taxdump.make_taxdump(os.path.join(tmp, "dump"), n_nodes=a.nodes, depth=a.depth, n_accessions=1, seed=42,
                                   extra_accessions=extra)
        result["generate_s"] = time.perf_counter() - t0
        print(f"generated in {result['generate_s']:.1f} s", flush=True)
        for n in sizes:
            acc = os.path.join(tmp, "dump", f"acc_{n}.txt")
            out = os.path.join(tmp, f"out_{n}")
            runs = [run_child({"dump": os.path.join(tmp, "dump"), "out": out, "acc": acc}, a.timeout) for _ in range(a.runs)]
            best = min(runs, key=lambda r: r["process_wall_s"])
            rec = {"accession_lines": n, "accession_bytes": os.path.getsize(acc), "best": best,
                   "process_wall_s_all": [r["process_wall_s"] for r in runs]}
            if n == min(sizes) and not a.no_oracle:
                from oracle import taxdb_oracle as orc
                t1 = time.perf_counter()
                doc, tsv, _ = orc.build(os.path.join(tmp, "dump"), acc, replace=[("superkingdom", "d")], source_database="nt")
                rec["oracle_s"] = time.perf_counter() - t1
                j, t = (out + ".blutils.json", out + ".non-mapped.tsv")
                rec["oracle_equal"] = open(j, "rb").read() == doc and open(t, "rb").read() == tsv
            result["runs"].append(rec)
            print(json.dumps(rec), flush=True)
            for f in os.listdir(tmp):
                if f.startswith("out_"):
                    os.remove(os.path.join(tmp, f))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
