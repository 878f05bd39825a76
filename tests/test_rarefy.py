"""`build-distances --rarefy` where no GPU is needed: the stream of a sample against the restatement in
tests/rarefy_reference.py, the refusals of blu_sample_rarefy and blu_distance_matrix_file_with — each before any device is
asked for — the CLI's argument errors, and the restatement itself: its two routes agree and its draw is fair."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from blutils_amd import _native as N
from blutils_amd import cli, distance, pipeline
from tests import rarefy_reference as ref

NO_SUCH_DEVICE = 4095          # a refusal that came before the device was asked for does not say BLU_ERR_NO_DEVICE
HEAD = "#rank\tidentifier\ttaxonomy\ttotal"


def _table(samples, rows):
    """rows: (rank, identifier, taxonomy, cells) -> the sample table's text"""
    out = [HEAD + "".join("\t" + s for s in samples)]
    for rank, ident, tax, cells in rows:
        out.append("\t".join([rank, ident, tax, str(sum(cells))] + [str(c) for c in cells]))
    return "\n".join(out) + "\n"


def test_symbols_struct_sizes_and_constants():
    L = N.lib()
    assert {"blu_rarefy_stream", "blu_sample_rarefy", "blu_rarefied_free"} <= set(N.EXPORTS)
    assert "blu_distance_matrix_file_with" in N.PIPELINE_EXPORTS
    for name in ("blu_rarefy_stream", "blu_sample_rarefy", "blu_rarefied_free", "blu_distance_matrix_file_with"):
        assert hasattr(L, name)
    assert C.sizeof(N.RarefyDesc) == 72 and C.sizeof(N.Rarefied) == 56
    assert C.sizeof(pipeline.DistanceOptions) == 32 and C.sizeof(pipeline.DistanceStats2) == 72
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "blu_consensus.h")).read()
    assert f"#define BLU_RAREFY_TILE {N.RAREFY_TILE}u" in header and "#define BLU_RAREFY_MAX_READS (1ull << 36)" in header
    assert N.RAREFY_MAX_READS == 1 << 36 and f"BLU_ERR_INTERNAL = {N.BLU_ERR_INTERNAL}" in header
    assert L.blu_abi_version() == 5                      # the additions are additive
    # the structs the call before this one had are what they were
    assert C.sizeof(N.DistanceDesc) == 56 and C.sizeof(N.SampleDistance) == 48 and C.sizeof(pipeline.DistanceStats) == 32


def test_mix64_is_the_splitmix64_step():
    # the first outputs of splitmix64 seeded with 0 and with 1234567, as published with the generator
    assert ref.mix64(0) == 0xE220A8397B1DCDAF
    assert ref.mix64(1234567) == 6457827717110365317
    z = np.array([0, 1234567, ref.MASK], dtype=np.uint64)
    assert ref.mix64_np(z).tolist() == [ref.mix64(int(v)) for v in z]


@pytest.mark.parametrize("seed", [0, 1, 2 ** 64 - 1])
@pytest.mark.parametrize("name", [b"", b"S1", b"sample_A.fastq", "prøve-æ".encode(), bytes([0x80, 0xFF, 0x41])])
def test_the_stream_of_a_sample(seed, name):
    got = N.lib().blu_rarefy_stream(seed, name, len(name))
    assert got == ref.stream(seed, name)
    assert ref.fnv1a64(b"") == 0xcbf29ce484222325 and ref.fnv1a64(b"a") == 0xaf63dc4c8601ec8c     # FNV-1a's published vectors
    if isinstance(name, bytes) and name == b"S1":
        assert distance.rarefy_stream(seed, "S1") == got and got != ref.stream(seed, b"S2")


def test_the_two_routes_of_the_restatement_agree():
    rng = np.random.default_rng(5)
    for trial in range(40):
        counts = rng.integers(1, 60, int(rng.integers(1, 30))).tolist()
        n = sum(counts)
        st = ref.stream(trial, f"s{trial}")
        for depth in {1, n // 2 or 1, n - 1 or 1, n}:
            a, b = ref.kept_by_sort(counts, depth, st), ref.kept_by_threshold(counts, depth, st)
            assert a == b and sum(a) == depth and all(0 <= x <= c for x, c in zip(a, counts))
        assert ref.kept_by_sort(counts, n, st) == counts                 # N = D keeps every read
        assert ref.kept_by_sort(counts, n + 1, st) is None and ref.kept_by_threshold(counts, n + 1, st) is None
    csr = ([0, 2, 3, 3, 5], [0, 2, 1, 0, 1], [7, 3, 9, 5, 2])
    assert ref.rarefy(*csr, ["a", "b", "c"], 6, 3, ref.kept_by_sort) == ref.rarefy(*csr, ["a", "b", "c"], 6, 3, ref.kept_by_threshold)


def test_the_restatement_is_a_fair_draw():
    """counts [5000, 3000, 1500, 400, 90, 9, 1] at D = 1000 over seeds 0 .. 399, the sample named S{seed % 7}: every per-feature
    mean within 4 standard errors of the hypergeometric mean D c / N (the bound guards the rule's text, not the kernel)"""
    counts = [5000, 3000, 1500, 400, 90, 9, 1]
    n, depth, seeds = sum(counts), 1000, 400
    draws = np.array([ref.kept_by_threshold(counts, depth, ref.stream(seed, f"S{seed % 7}")) for seed in range(seeds)])
    assert (draws.sum(axis=1) == depth).all()
    worst = 0.0
    for f, c in enumerate(counts):
        p = c / n
        se = math.sqrt(depth * p * (1 - p) * (n - depth) / (n - 1) / seeds)
        worst = max(worst, abs(draws[:, f].mean() - depth * p) / se)
    print(f"largest deviation: {worst:.2f} standard errors")
    assert worst < 4.0


GOOD = dict(row_ptr=[0, 2, 3], sample=[0, 1, 1], count=[5, 6, 7], names=["A", "B"], depth=3)


@pytest.mark.parametrize("what,kwargs,word", [
    ("depth 0", dict(GOOD, depth=0), "depth"),
    ("struct size", dict(GOOD, struct_size=64), "struct_size"),
    ("same name", dict(row_ptr=[0, 3], sample=[0, 1, 2], count=[5, 6, 7], names=["A", "B", "A"], depth=3), "samples 0 and 2"),
    ("2^32 reads", dict(row_ptr=[0, 2], sample=[0, 1], count=[5, 1 << 32], names=["A", "B"], depth=3), "sample 1 has 4294967296"),
    ("2^32 reads over two features", dict(row_ptr=[0, 1, 2], sample=[0, 0], count=[(1 << 32) - 1, 1], names=["A"], depth=3), "sample 0"),
    ("read cap", dict(row_ptr=[0, 17], sample=list(range(17)), count=[(1 << 32) - 1] * 17, names=[f"s{i}" for i in range(17)], depth=1),
     str(N.RAREFY_MAX_READS)),
    ("sample id", dict(row_ptr=[0, 1, 2], sample=[0, 3], count=[1, 1], names=["A", "B", "C"], depth=1), "feature 1"),
    ("unsorted", dict(row_ptr=[0, 1, 3], sample=[0, 2, 1], count=[1, 1, 1], names=["A", "B", "C"], depth=1), "feature 1"),
    ("repeated", dict(row_ptr=[0, 2, 3], sample=[1, 1, 0], count=[1, 1, 1], names=["A", "B", "C"], depth=1), "feature 0"),
    ("zero count", dict(row_ptr=[0, 1, 2, 3], sample=[0, 0, 0], count=[1, 1, 0], names=["A", "B", "C"], depth=1), "feature 2"),
    ("row_ptr", dict(row_ptr=[0, 2, 1, 3], sample=[0, 1, 0], count=[1, 1, 1], names=["A", "B", "C"], depth=1), "feature 1"),
    ("no samples", dict(row_ptr=[0], sample=[], count=[], names=[], depth=1), "n_samples"),
    ("sample cap", dict(row_ptr=[0], sample=[], count=[], names=[f"s{i}" for i in range(N.DISTANCE_MAX_SAMPLES + 1)], depth=1), "n_samples"),
    ("column sum", dict(row_ptr=[0, 1, 2], sample=[1, 1], count=[1 << 62, 1 << 62], names=["A", "B"], depth=1), "2^63"),
])
def test_refusals_come_before_the_device(what, kwargs, word):
    with pytest.raises(N.BluError) as e:
        distance.rarefy(device=NO_SUCH_DEVICE, **kwargs)
    assert e.value.code == N.BLU_ERR_INVALID_ARG, what
    assert "blu_sample_rarefy" in str(e.value) and word in str(e.value), (what, str(e.value))


def test_the_read_cap_counts_only_the_samples_that_reach_the_depth_and_no_kept_sample_needs_no_device():
    # seventeen samples of 2^32 - 1 reads pass the cap together; at a depth none reaches there is nothing to hash: K = 0
    got = distance.rarefy([0, 17], list(range(17)), [(1 << 32) - 1] * 17, [f"s{i}" for i in range(17)], 1 << 32, device=NO_SUCH_DEVICE)
    assert got["kept_sample"].tolist() == [] and got["row_ptr"].tolist() == [0, 0] and got["sample"].size == 0 and got["t_device_ms"] == 0
    got = distance.rarefy([0], [], [], ["A"], 1, device=NO_SUCH_DEVICE)                        # no features at all
    assert got["kept_sample"].tolist() == [] and got["row_ptr"].tolist() == [0]
    # a well-formed call with a sample to rarefy: only now a device is needed
    with pytest.raises(N.BluError) as e:
        distance.rarefy(device=NO_SUCH_DEVICE, **GOOD)
    assert e.value.code == N.BLU_ERR_NO_DEVICE


ROWS = [("-", "unclassified", "", [5, 0, 2]), ("d", "B", "d__B", [40, 31, 9]), ("g", "G", "d__B;g__G", [30, 25, 9])]


def _with(tmp_path, text, **kw):
    p = tmp_path / "table.tsv"
    p.write_text(text)
    return pipeline.distance_matrix_file_with(str(p), str(tmp_path / "m.tsv"), device=NO_SUCH_DEVICE, **kw)


def test_file_level_refusals_come_before_the_device_and_write_nothing(tmp_path):
    good = _table(["S1", "S2", "S3"], ROWS)
    for text, kw, word in (
            (_table(["S1", "S2", "S1"], ROWS), dict(depth=5), "columns 1 and 3 are both named `S1`"),
            (good, dict(depth=46), "the largest, `S1`, has 45 reads"),
            (good, dict(depth=5, struct_size=24), "struct_size"),
            (good, dict(depth=0, rarefied_table=str(tmp_path / "r.tsv")), "needs a depth"),
            (_table(["S1", "S2", "S3"], [("-", "unclassified", "", [1 << 32, 7, 7])]), dict(depth=5), "sample 0 has 4294967296")):
        with pytest.raises(N.BluError) as e:
            _with(tmp_path, text, rarefied_table=kw.pop("rarefied_table", str(tmp_path / "r.tsv")), **kw)
        assert e.value.code == N.BLU_ERR_INVALID_ARG and word in str(e.value), (word, str(e.value))
        assert not (tmp_path / "m.tsv").exists() and not (tmp_path / "r.tsv").exists()
    with pytest.raises(ValueError):
        _with(tmp_path, good, depth=5, metric="euclid")
    with pytest.raises(ValueError, match="need rarefy"):
        distance.build_distances(str(tmp_path / "table.tsv"), str(tmp_path / "m.tsv"), seed=3)


def test_depth_0_is_the_call_it_was_refused_the_same_way_on_a_missing_device(tmp_path):
    p = tmp_path / "table.tsv"
    p.write_text(_table(["S1", "S2", "S3"], ROWS))
    with pytest.raises(N.BluError) as old:
        pipeline.distance_matrix_file(str(p), str(tmp_path / "m.tsv"), device=NO_SUCH_DEVICE)
    with pytest.raises(N.BluError) as new:
        _with(tmp_path, p.read_text(), depth=0)
    assert old.value.code == new.value.code == N.BLU_ERR_NO_DEVICE
    assert str(old.value).split(": ", 1)[1] == str(new.value).split(": ", 1)[1] and "blu_sample_distances" in str(new.value)
    L = pipeline._bind()                                 # NULL options too
    assert L.blu_distance_matrix_file_with(str(p).encode(), None, 0, 0, NO_SUCH_DEVICE, str(tmp_path / "m.tsv").encode(), None, None) == N.BLU_ERR_NO_DEVICE
    assert L.blu_distance_matrix_file_with(str(p).encode(), None, 7, 0, 0, str(tmp_path / "m.tsv").encode(), None, None) == N.BLU_ERR_INVALID_ARG
    assert not (tmp_path / "m.tsv").exists()
    # a well-formed rarefied call: the device is asked for by the rarefaction
    with pytest.raises(N.BluError) as e:
        _with(tmp_path, p.read_text(), depth=5)
    assert e.value.code == N.BLU_ERR_NO_DEVICE and "blu_sample_rarefy" in str(e.value)


def test_cli_argument_errors(capsys):
    bd = ["blastn", "build-distances", "t.tsv", "-o", "m.tsv"]
    bc = ["blastn", "build-consensus", "b.tsv", "-t", "t.json", "--taxon", "bacteria", "--strategy", "relaxed", "--sample-table", "s.tsv"]
    rw = ["blastn", "run-with-consensus", "q.fa", "-d", "db", "-t", "t.json", "--blast-out-file", "b.tsv", "--taxon", "bacteria",
          "--strategy", "relaxed", "--sample-table", "s.tsv"]
    br = ["blastn", "build-report", "doc.json", "--by-sample", "-o", "r.tsv"]
    for argv, word in (
            (bd + ["--seed", "3"], "--rarefy"),
            (bd + ["--rarefied-table", "f.tsv"], "--rarefy"),
            (bd + ["--rarefy", "0"], "--rarefy"),
            (bd + ["--rarefy", "many"], "--rarefy"),
            (bd + ["--rarefy", "5", "--seed", str(2 ** 64)], "--seed"),
            (bc + ["--distance-rarefy", "5"], "--distance-matrix"),
            (bc + ["--distance-matrix", "m.tsv", "--distance-seed", "3"], "--distance-rarefy"),
            (bc + ["--distance-matrix", "m.tsv", "--distance-rarefy", "0"], "--distance-rarefy"),
            (rw + ["--distance-matrix", "m.tsv", "--distance-rarefied-table", "f.tsv"], "--distance-rarefy"),
            (rw + ["--distance-seed", "3"], "--distance-matrix"),
            (br + ["--distance-matrix", "m.tsv", "--distance-seed", "3"], "--distance-rarefy"),
            (br + ["--distance-rarefied-table", "f.tsv"], "--distance-matrix")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv
        assert word in capsys.readouterr().err, argv
    assert not os.path.exists("m.tsv") and not os.path.exists("f.tsv")
