"""`build-db lineages` at reference-database scale: fresh-process runs of the GPU builder on seeded lineage tables
(blutils_amd/synth_lineages.py) — a Greengenes2-like one (many lines, few hundred thousand lineages, 7 levels) and a SILVA-like
one (ragged depths).  Reports the stage times of blu_lineage_db_stats (upload, parse, intern, group, render incl. download,
write: the stage table of DESIGN.md §10.2), input and output bytes and the wall time of the child process; on a cut of the
first table it also times the Python restatement (tests/lineage_db_reference.py) and checks that both outputs are byte-equal.
Not part of bench.py's line.

    python scripts/lineage_db_bench.py --out profiles/lineage_db_bench.json
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
from blutils_amd import lineagedb
a = json.loads(sys.argv[1])
st = lineagedb.build_ref_db_from_lineage_table(a["table"], a["out"], a["out"] + ".taxid_map")
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
    ap.add_argument("--gg-lines", type=int, default=20_000_000)
    ap.add_argument("--gg-lineages", type=int, default=300_000)
    ap.add_argument("--silva-lines", type=int, default=2_000_000)
    ap.add_argument("--silva-lineages", type=int, default=150_000)
    ap.add_argument("--restatement-lines", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--timeout", type=float, default=600)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lineage_db_bench.json"))
    a = ap.parse_args()
    from blutils_amd import synth_lineages
    tmp = tempfile.mkdtemp(prefix="blu-lineage-bench-")
    result = {"tables": []}
    try:
        tables = [("greengenes2-like", dict(n_lines=a.gg_lines, n_distinct=a.gg_lineages, depth=7, greengenes=0.3, seed=1)),
                  ("silva-like", dict(n_lines=a.silva_lines, n_distinct=a.silva_lineages, depth=7, ragged=0.5, noise=0.05, header=True, seed=2))]
        for name, kw in tables:
            t0 = time.perf_counter()
            table = synth_lineages.write_table(os.path.join(tmp, name + ".tsv"), **kw)
            rec = {"name": name, "knobs": kw, "generate_s": time.perf_counter() - t0, "table_bytes": os.path.getsize(table)}
            out = os.path.join(tmp, "out_" + name)
            runs = [run_child({"table": table, "out": out}, a.timeout) for _ in range(a.runs)]
            rec["best"] = min(runs, key=lambda r: r["process_wall_s"])
            rec["process_wall_s_all"] = [r["process_wall_s"] for r in runs]
            if name == "greengenes2-like" and a.restatement_lines:
                from tests import lineage_db_reference as R
                with open(table, "rb") as f:
                    data = b"".join(line for _, line in zip(range(a.restatement_lines), f))
                cut = os.path.join(tmp, "cut.tsv")
                with open(cut, "wb") as f:
                    f.write(data)
                got = run_child({"table": cut, "out": os.path.join(tmp, "out_cut")}, a.timeout)
                t1 = time.perf_counter()
                exp = R.build(data, cut, None)
                rec["restatement"] = {"lines": a.restatement_lines, "restatement_s": time.perf_counter() - t1,
                                      "gpu_process_wall_s": got["process_wall_s"],
                                      "equal": all(open(os.path.join(tmp, "out_cut" + ext), "rb").read() == exp[key]
                                                   for ext, key in ((".blutils.json", "doc"), (".non-mapped.tsv", "tsv"), (".taxid_map", "map")))}
            result["tables"].append(rec)
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
