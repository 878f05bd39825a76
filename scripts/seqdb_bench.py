"""Throughput of `build-db kraken2` / the qiime2 sequence export (csrc/seqdb_gpu.hip) on two synthetic listings of several GB:
many short lines (about 1.5 kB) and a few huge ones (100 MB and more).  Records the read, GPU and write stage times, the
end-to-end rate of a fresh `python -m blutils_amd.cli` process, and the restatement's (tests/seqdb_reference.py) rate on a
slice.  Listings and outputs live under a temporary directory (default /tmp) that is removed at the end.

    python scripts/seqdb_bench.py [--gb 3] [--out profiles/seqdb_bench.json]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from blutils_amd import seqdb, synth_seqdb  # noqa: E402
from tests import seqdb_reference as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=3.0, help="size of each listing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqdb_bench.json"))
    ap.add_argument("--tmp", default="/tmp")
    a = ap.parse_args()
    target = int(a.gb * 1e9)
    tmp = tempfile.mkdtemp(prefix="seqdb-bench-", dir=a.tmp)
    res = {"listing_gb": a.gb, "cases": {}}
    try:
        cases = {"short_lines": dict(n_lines=target // 1520, min_len=1000, max_len=2000),
                 "huge_lines": dict(n_lines=1000, long_lines=[int(target / 12)] * 12)}
        for name, kw in cases.items():
            lst = os.path.join(tmp, name + ".txt")
            t0 = time.perf_counter()
            size = synth_seqdb.write_listing(lst, False, seed=7, odd=False, **kw)
            gen_s = time.perf_counter() - t0
            out = os.path.join(tmp, name + "_out")
            os.makedirs(out)
            st = seqdb.export(seqdb.KRAKEN2, os.path.join(out, "library.fna"), os.path.join(out, "prelim_map.txt"),
                              listing_path=lst)
            cmd = [sys.executable, "-m", "blutils_amd.cli", "build-db", "kraken2", "db", "-o", os.path.join(tmp, name + "_cli"),
                   "--listing-file", lst]
            t0 = time.perf_counter()
            subprocess.run(cmd, check=True, cwd=ROOT)
            e2e = time.perf_counter() - t0
            with open(lst, "rb") as f:
                sl = f.read(64 << 20)
            sl = sl[:sl.rfind(b"\n") + 1] if b"\n" in sl else sl
            t0 = time.perf_counter()
            R.kraken2(sl)
            ref_s = time.perf_counter() - t0
            res["cases"][name] = {
                "input_bytes": size, "lines": st["n_lines"], "max_line_bytes": st["max_line_bytes"], "chunks": st["n_chunks"],
                "fna_bytes": st["fna_bytes"], "map_bytes": st["map_bytes"],
                "stage_ms": {"read": st["t_read_ms"], "gpu": st["t_gpu_ms"], "write": st["t_write_ms"], "wall": st["t_wall_ms"]},
                "in_process_gb_per_s": size / st["t_wall_ms"] / 1e6,
                "fresh_process_s": e2e, "fresh_process_gb_per_s": size / e2e / 1e9,
                "reference_slice_bytes": len(sl), "reference_gb_per_s": len(sl) / ref_s / 1e9, "generate_s": gen_s}
            print(name, json.dumps(res["cases"][name]), flush=True)
            for p in (lst, out, os.path.join(tmp, name + "_cli")):
                shutil.rmtree(p, ignore_errors=True) if os.path.isdir(p) else os.remove(p)
        s, h = res["cases"]["short_lines"], res["cases"]["huge_lines"]
        res["gb_per_s_ratio_short_over_huge"] = s["in_process_gb_per_s"] / h["in_process_gb_per_s"]
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps({k: v for k, v in res.items() if k != "cases"}))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
