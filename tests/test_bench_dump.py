"""bench.py --dump-outputs DIR: the records of the last timed step as float64 .npy files (every field exact, level_mask as two
32-bit halves), at most 64 MB, the same seeded sample of queries for the same arguments; --steps sets the timed steps."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from blutils_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = sorted([f for f in engine.RESULT_DTYPE.names if f != "level_mask"] + ["level_mask_lo", "level_mask_hi", "query_index"])


def _bench(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)


def _load(d):
    assert sorted(os.listdir(d)) == [f + ".npy" for f in FIELDS]
    assert sum(os.path.getsize(os.path.join(d, f + ".npy")) for f in FIELDS) <= 64 * 10 ** 6
    arrays = {f: np.load(os.path.join(d, f + ".npy")) for f in FIELDS}
    assert all(a.dtype == np.float64 and a.shape == arrays["query_index"].shape for a in arrays.values())
    return arrays


@pytest.mark.parametrize("n_queries", [1000, 3000000])
def test_dump_is_exact_capped_and_repeatable(tmp_path, monkeypatch, n_queries):
    """Records of random bytes through the dump writer (CPU tensor): every field back bit for bit, a table larger than the cap
    gives the same sorted sample twice."""
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    out = torch.randint(0, 256, (32 * n_queries,), dtype=torch.uint8, generator=torch.Generator().manual_seed(7))
    rec = engine.records_from_tensor(out)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), engine, torch, np, out, n_queries, 0, 0, 1)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    for f in FIELDS:
        assert (a[f].view(np.uint64) == b[f].view(np.uint64)).all(), f
    qi = a["query_index"].astype(np.int64)
    assert len(qi) == min(n_queries, bench.DUMP_QUERIES) and (np.diff(qi) > 0).all() and qi[-1] < n_queries
    r = rec[qi]
    mask = (a["level_mask_hi"].astype(np.uint64) << np.uint64(32)) | a["level_mask_lo"].astype(np.uint64)
    assert (mask == r["level_mask"]).all()
    assert ((a["ident_used"] == r["ident_used"]) | (np.isnan(a["ident_used"]) & np.isnan(r["ident_used"]))).all()
    for f in ("status", "flags", "bean_index", "max_allowed_level", "reached_rank", "max_allowed_rank", "identifier_node", "ref_row"):
        assert (a[f] == r[f]).all(), f


def test_bench_refuses_zero_steps():
    r = _bench(["--gpus", "1", "--steps", "0"])
    assert r.returncode != 0 and "--steps" in r.stderr and r.stdout.strip() == ""


@pytest.mark.gpu
def test_bench_dump_outputs_do_not_depend_on_steps(tmp_path):
    """Two runs of the same workload, 2 and 5 timed steps: both lines say so, both pass the parity gate, and their dumps
    (every query of the table) are identical."""
    import json
    common = ["--gpus", "1", "--warmup", "1", "--queries", "200000", "--taxa", "50000", "--cpu-sample", "20000",
              "--no-cpu-baseline", "--no-secondary"]
    dumps = []
    for steps in (2, 5):
        d = tmp_path / f"steps{steps}"
        r = _bench(common + ["--steps", str(steps), "--dump-outputs", str(d)])
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == steps and "parity gate ok" in r.stderr
        dumps.append(_load(d))
    a, b = dumps
    assert (a["query_index"] == np.arange(200000)).all()
    for f in FIELDS:
        assert (a[f].view(np.uint64) == b[f].view(np.uint64)).all(), f
    assert np.isin(a["status"], [0, 1, 2, 16, 17, 18, 19, 20]).all()
