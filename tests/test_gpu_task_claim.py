"""The stream kernel's task queues at their edges, bit for bit against the columnar oracle.

The waves of a block claim their tasks from a queue (consensus_kernel.hip, the head of the task loop; blu_internal.h:
task_deal / task_of_claim), so which wave — and, at the end of a launch, which block — computes a task depends on timing.
No record may depend on it, no query may be skipped, and the counters must be back where they started after every run.

* Sizes: tables of 10 hits per query with (cus * waves * k + d) * 64 + r queries — k = 0 .. 3 whole rounds of the grid, one
  task less / exactly / one task more, 0, 1 or 63 queries on top — for the builds with 12 (bit-score ring) and 16 (no ring)
  waves per block, and for the f64 layout also by its own builds' 11 and 12.  The empty table is one of them.  Every one is
  a prefix of ONE table whose oracle records are computed once.
* Uneven work: every task of one block's stride has all hits tied (dense steps, list overflow), some tasks hold a 600-row
  query (worklist) — the stride by the milli-percent build's waves per block and by the f64 build's.  That block's queue
  outlasts the others.  One table of 10-hit queries for the ring build, one of
  mixed segment lengths for the build without it.  Each is run twice on the same buffers and three more times from a
  captured graph, the records prefilled with 0xFF before every run: five byte-identical results, equal to the oracle's."""
import numpy as np
import pytest

from blutils_amd import engine, synth
from tests import helpers as H

pytestmark = pytest.mark.gpu

WAVE = 64
HITS = 10
GUARD = 64                      # records behind the table's last one that no run may touch
STRATEGIES = ("relaxed", "cautious")
BUILDS = {12: "ring", 16: "noring"}          # waves per block of the milli-percent builds -> BLU_STREAM_KIND
BLOCKS = {("ring", False): 768, ("ring", True): 704, ("noring", False): 1024, ("noring", True): 768}   # (kind, f64 layout) -> block size


def _cus() -> int:
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def size_of(cus, waves, k, d, r) -> int:
    return (cus * waves * k + d) * WAVE + r


def custom_table(tax, lens: np.ndarray, tied: np.ndarray, seed: int) -> dict:
    """A table with the given segment lengths: side values drawn from a pool of the generator's rows, bit-scores written here —
    query q's top group is its first 1 + Geometric(0.35) rows, or all of them where tied[q]."""
    pool = synth.make_hits(tax, 4096, seed, 50, device="cpu", p_unmatched=0.001).numpy()
    n_pool = len(pool["bitscore"])
    rng = np.random.default_rng(seed)
    n_q = len(lens)
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n_h = int(seg[-1])
    idx = (np.arange(n_h, dtype=np.int64) * 7919 + seed) % n_pool
    qrow = np.repeat(np.arange(n_q), lens)
    j = np.arange(n_h, dtype=np.int64) - seg[:-1][qrow]
    gsz = np.where(tied, lens, np.minimum(lens, rng.geometric(0.35, n_q)))
    top = 200 + rng.integers(0, 1801, n_q)
    h = {"seg_off": seg, "bitscore": np.where(j < gsz[qrow], top[qrow], top[qrow] - 1 - rng.integers(0, 16, n_h)).astype(np.int32)}
    for k in ("tax_row", "pident", "align_len", "acc_rank"):
        h[k] = np.ascontiguousarray(pool[k][idx])
    h["pident_milli"] = np.rint(h["pident"] * 1000.0).astype(np.int64).astype(np.uint32)
    assert np.array_equal(h["pident_milli"].astype(np.float64) / 1000.0, h["pident"])
    return h


def device_buffers(t, h) -> dict:
    """layout -> the device dict engine.run_consensus_device reads, all four built from one upload of the columns."""
    import torch
    base = {"seg_off": torch.from_numpy(h["seg_off"]).cuda(), "bitscore": torch.from_numpy(h["bitscore"]).cuda(),
            "tax_row": torch.from_numpy(t.engine_rows(h["tax_row"]).view(np.int32)).cuda(),
            "align_len": torch.from_numpy(h["align_len"]).cuda(), "acc_rank": torch.from_numpy(h["acc_rank"]).cuda()}
    f64 = dict(base, pident=torch.from_numpy(h["pident"]).cuda())
    milli = dict(base, pident_milli=torch.from_numpy(h["pident_milli"].view(np.int32)).cuda())
    out = {"f64": f64, "milli": milli}
    for layout, cols in (("packed", milli), ("packed64", f64)):
        out[layout] = {"seg_off": base["seg_off"], "bitscore": base["bitscore"], layout: engine.pack_hits_device(t, cols, wide=layout == "packed64")}
    torch.cuda.synchronize()
    return out


ROW_WORDS = {"packed": 4, "packed64": 6}


def prefix(bufs: dict, n_q: int, n_h: int) -> dict:
    """The first n_q queries (n_h rows) of a table on the device: views, nothing is copied."""
    out = {}
    for k, v in bufs.items():
        out[k] = v[: n_q + 1] if k == "seg_off" else v[: n_h * ROW_WORDS.get(k, 1)]
    return out


def first_difference(got: bytes, exp: bytes):
    a = np.frombuffer(got, dtype=np.uint8).reshape(-1, 32)
    b = np.frombuffer(exp, dtype=np.uint8).reshape(-1, 32)
    bad = np.nonzero((a != b).any(axis=1))[0]
    return None if len(bad) == 0 else {"queries": len(bad), "first": int(bad[0]), "first_task": int(bad[0]) // WAVE, "last": int(bad[-1])}


class Table:
    """A table, its oracle records per strategy (computed once), its device buffers and a record buffer with a guard."""

    def __init__(self, tax, h):
        import torch
        self.h, self.n_q = h, len(h["seg_off"]) - 1
        self.t = engine.Taxonomy(tax.lin_off, tax.lin_node, tax.lin_rank, tax.rank_names, taxon="custom", custom=H.CUSTOM_16S, device=0)
        self.exp = {s: H.columnar(tax, h, "custom", s, H.CUSTOM_16S, threads=16).tobytes() for s in STRATEGIES}
        self.bufs = device_buffers(self.t, h)
        self.out = torch.empty(32 * (self.n_q + GUARD), dtype=torch.uint8, device="cuda")

    def run_prefix(self, layout, strategy, n_q, kind):
        """Records of the first n_q queries, the buffer prefilled with 0xFF; checks the launch and the guard."""
        import torch
        n_h = int(self.h["seg_off"][n_q])
        self.out.fill_(0xFF)
        engine.run_consensus_device(self.t, prefix(self.bufs[layout], n_q, n_h), self.out[: 32 * n_q], strategy=strategy)
        torch.cuda.synchronize()
        if n_q:                                       # (an empty table launches nothing)
            name, _, block = engine.last_launch()
            assert "stream" in name and block == BLOCKS[(kind, layout in ("f64", "packed64"))], (name, block, kind, layout)
        got = self.out[: 32 * (n_q + GUARD)].cpu().numpy().tobytes()
        assert got[32 * n_q:] == b"\xff" * (32 * GUARD), ("records written past the table's end", layout, strategy, n_q)
        return got[: 32 * n_q]


@pytest.fixture(scope="module")
def tax():
    return synth.make_taxonomy(3000, 77)


@pytest.fixture(scope="module")
def uniform(tax):
    """The largest size of the sweep; every other size is a prefix of it."""
    n_q = size_of(_cus(), 16, 3, 1, 63)
    assert n_q < 1000000 and n_q * HITS < 10000000
    tb = Table(tax, custom_table(tax, np.full(n_q, HITS, dtype=np.int64), np.zeros(n_q, dtype=bool), 9300))
    yield tb
    tb.t.close()


@pytest.mark.parametrize("k", (0, 1, 2, 3))
@pytest.mark.parametrize("waves", (12, 16))
def test_sizes_around_whole_rounds(uniform, waves, k, monkeypatch):
    kind = BUILDS[waves]
    monkeypatch.setenv("BLU_STREAM_KIND", kind)
    cus = _cus()
    for layout in ("packed", "f64"):
        # the sizes by the waves per block of the milli-percent builds, and by this layout's own (f64: 11 with the ring, 12 without)
        own = BLOCKS[(kind, layout == "f64")] // WAVE
        sizes = {size_of(cus, w, k, d, r) for w in (waves, own) for d in (-1, 0, 1) for r in (0, 1, 63)}
        sizes = sorted(n for n in sizes if n >= 0)            # (k = 0 has nothing below an empty table)
        assert len(sizes) >= (9 if k else 6) and (k != 0 or sizes[0] == 0)
        for n_q in sizes:
            for strategy in STRATEGIES:
                got = uniform.run_prefix(layout, strategy, n_q, kind)
                exp = uniform.exp[strategy][: 32 * n_q]
                assert got == exp, (waves, k, n_q, layout, strategy, first_difference(got, exp))


def uneven_lens_tied(cus: int, waves: int, waves_f64: int, ragged: bool, seed: int):
    """3.5 rounds of the grid and 17 queries: segment lengths, and the queries whose hits all tie — one block's stride of tasks
    by the waves per block of the milli-percent build, and the same block's stride by those of the f64 build of the kind."""
    n_waves = cus * waves
    n_q = (3 * n_waves + n_waves // 2) * WAVE + 17
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 20, n_q) if ragged else np.full(n_q, HITS, dtype=np.int64)
    task = np.arange(n_q) // WAVE
    b = cus // 3
    tied = (task % n_waves >= b * waves) & (task % n_waves < b * waves + waves)
    tied |= (task % (cus * waves_f64) >= b * waves_f64) & (task % (cus * waves_f64) < b * waves_f64 + waves_f64)
    long_q = np.nonzero((task % 97 == 3) & (np.arange(n_q) % WAVE == 5))[0]
    lens[long_q] = 600
    tied[long_q] = False
    assert len(long_q) > 50 and tied.sum() >= 3 * waves * WAVE and n_q < 1000000 and int(lens.sum()) < 10000000
    return lens, tied


@pytest.fixture(scope="module")
def uneven(tax):
    cache = {}

    def get(kind):
        if kind not in cache:
            lens, tied = uneven_lens_tied(_cus(), 12 if kind == "ring" else 16, 11 if kind == "ring" else 12, kind == "noring", 9400 + len(cache))
            cache[kind] = Table(tax, custom_table(tax, lens, tied, 9410 + len(cache)))
        return cache[kind]

    yield get
    for tb in cache.values():
        tb.t.close()


@pytest.mark.parametrize("layout", ("packed", "f64", "milli", "packed64"))
@pytest.mark.parametrize("kind", ("ring", "noring"))
def test_uneven_work_five_runs_identical(uneven, kind, layout, monkeypatch):
    import torch
    monkeypatch.setenv("BLU_STREAM_KIND", kind)
    tb = uneven(kind)
    for strategy in STRATEGIES:
        exp = tb.exp[strategy]
        results = [tb.run_prefix(layout, strategy, tb.n_q, kind) for _ in range(2)]
        # the same launch captured (the workspace exists by now) and replayed: the counters are back where they started
        bufs, out = tb.bufs[layout], tb.out[: 32 * tb.n_q]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            engine.run_consensus_device(tb.t, bufs, out, strategy=strategy)
        for _ in range(3):
            tb.out.fill_(0xFF)
            graph.replay()
            torch.cuda.synchronize()
            got = tb.out.cpu().numpy().tobytes()
            assert got[32 * tb.n_q:] == b"\xff" * (32 * GUARD), ("records written past the table's end", kind, layout, strategy)
            results.append(got[: 32 * tb.n_q])
        del graph
        for i, got in enumerate(results):
            assert got == exp, (kind, layout, strategy, "run %d" % i, first_difference(got, exp))
