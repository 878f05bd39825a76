"""blu_sample_distances on the GPU against the integers of tests/distance_reference.py, at the seams of the
pair kernel (partners per block, features per chunk), then `build-distances` and `build-consensus --distance-matrix` end to
end: the file byte-equal to the restatement's rendering."""
import gzip
import json
import os
import random

import numpy as np
import pytest

from blutils_amd import _native as N
from blutils_amd import cli, distance
from tests import distance_reference as ref

pytestmark = pytest.mark.gpu

CHUNK, PARTNERS = N.DISTANCE_CHUNK, N.DISTANCE_PARTNERS


def _csr(columns, n_features):
    """per-sample {feature: count} -> CSR over the features"""
    rows = [[] for _ in range(n_features)]
    for s, col in enumerate(columns):
        for f, v in col.items():
            rows[f].append((s, v))
    row_ptr, sample, count = [0], [], []
    for r in rows:
        for s, v in r:                       # (samples ascend: the columns were walked in order)
            sample.append(s)
            count.append(v)
        row_ptr.append(len(sample))
    return row_ptr, sample, count


def _check(columns, n_features):
    S = len(columns)
    row_ptr, sample, count = _csr(columns, n_features)
    got = distance.sample_distances(row_ptr, sample, count, S)
    total, rich, min_sum, shared = ref.integers_dense(columns)
    assert got["total"].tolist() == total and got["richness"].tolist() == rich
    assert got["min_sum"].tolist() == min_sum
    assert got["shared"].tolist() == shared
    # symmetry and the diagonal identities, on what the device wrote
    assert (got["min_sum"] == got["min_sum"].T).all() and (got["shared"] == got["shared"].T).all()
    assert got["min_sum"].diagonal().tolist() == total and got["shared"].diagonal().tolist() == rich
    return got


def _random_columns(S, F, density, seed, top=1000):
    rng = random.Random(seed)
    n = max(1, round(F * density))
    return [{f: rng.randrange(1, top) for f in (range(F) if n >= F else rng.sample(range(F), n))} for _ in range(S)]


def test_the_two_integer_routes_of_the_restatement_agree():
    cols = _random_columns(7, 40, 0.4, 1)
    assert ref.integers(*_csr(cols, 40), 7) == ref.integers_dense(cols)


@pytest.mark.parametrize("S", sorted({1, 2, 64, 65, PARTNERS, PARTNERS + 1, 2 * PARTNERS + 3}))
def test_sample_counts_around_the_partners_of_a_block(S):
    _check(_random_columns(S, 53, 0.3, S), 53)


@pytest.mark.parametrize("F", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK])
def test_non_zeros_only_at_the_ends_of_the_chunks(F):
    ends = sorted({f for f in (0, CHUNK - 1, CHUNK, 2 * CHUNK - 1, F - 1) if f < F})
    cols = [{f: 10 + 3 * k + s for k, f in enumerate(ends)} for s in range(3)]
    cols.append({ends[-1]: 7})                          # only the last feature
    cols.append({ends[0]: 5})                           # only the first
    got = _check(cols, F)
    assert got["shared"][0][1] == len(ends) and got["shared"][3][4] == (1 if len(ends) == 1 else 0)


def test_an_empty_sample_a_feature_in_every_sample_and_counts_of_2_40():
    big = 1 << 40
    cols = _random_columns(5, 100, 0.5, 9)
    cols[2] = {}                                        # no non-zero at all
    for s, c in enumerate(cols):
        if s != 2:
            c[17] = big + s                             # in every other sample
            c[60 + s] = big
    cols.append({17: big, 3: 2 * big})
    got = _check(cols, 100)
    assert got["total"][2] == 0 and got["min_sum"][2].tolist() == [0] * 6 and got["shared"][:, 2].tolist() == [0] * 6
    assert int(got["min_sum"][0][1]) > 1 << 32 and int(got["total"][0]) > 1 << 32
    # every sample has feature 0 .. 4: shared is at least 5 everywhere
    cols = [{f: s + f + 1 for f in range(5)} for s in range(4)]
    assert _check(cols, 5)["shared"].min() == 5


@pytest.mark.parametrize("S,F,density", [(70, 20000, 0.01), (20, 9000, 0.5), (12, CHUNK + 5, 1.0)])
def test_random_csr(S, F, density):
    _check(_random_columns(S, F, density, S + F, top=1 << 20), F)


def test_no_features_at_all():
    got = distance.sample_distances([0], [], [], 3)
    assert got["total"].tolist() == [0, 0, 0] and not got["min_sum"].any() and not got["shared"].any()


NO_SUCH_DEVICE = 4095          # a refusal that came before the device was asked for does not say BLU_ERR_NO_DEVICE


@pytest.mark.parametrize("what,kwargs,word", [
    ("sample id", dict(row_ptr=[0, 1, 2], sample=[0, 3], count=[1, 1], n_samples=3), "feature 1"),
    ("unsorted", dict(row_ptr=[0, 1, 3], sample=[0, 2, 1], count=[1, 1, 1], n_samples=3), "feature 1"),
    ("repeated", dict(row_ptr=[0, 2, 3], sample=[1, 1, 0], count=[1, 1, 1], n_samples=3), "feature 0"),
    ("zero count", dict(row_ptr=[0, 1, 2, 3], sample=[0, 0, 0], count=[1, 1, 0], n_samples=3), "feature 2"),
    ("row_ptr", dict(row_ptr=[0, 2, 1, 3], sample=[0, 1, 0], count=[1, 1, 1], n_samples=3), "feature 1"),
    ("no samples", dict(row_ptr=[0], sample=[], count=[], n_samples=0), "n_samples"),
    ("cap", dict(row_ptr=[0], sample=[], count=[], n_samples=N.DISTANCE_MAX_SAMPLES + 1), "n_samples"),
    ("column sum", dict(row_ptr=[0, 1, 2], sample=[1, 1], count=[1 << 62, 1 << 62], n_samples=2), "2^63"),
    ("struct size", dict(row_ptr=[0], sample=[], count=[], n_samples=1, struct_size=48), "struct_size"),
])
def test_refusals_come_before_the_device(what, kwargs, word):
    with pytest.raises(N.BluError) as e:
        distance.sample_distances(device=NO_SUCH_DEVICE, **kwargs)
    assert e.value.code == N.BLU_ERR_INVALID_ARG, what
    assert word in str(e.value), what


def test_the_cap_itself_is_taken_and_a_missing_device_is_said():
    S = N.DISTANCE_MAX_SAMPLES
    got = distance.sample_distances([0, 2], [0, S - 1], [3, 4], S)
    assert got["min_sum"][0][S - 1] == 3 and got["min_sum"][S - 1][0] == 3 and got["shared"][S - 1][0] == 1 and got["total"][S - 1] == 4
    with pytest.raises(N.BluError) as e:
        distance.sample_distances([0, 1], [0], [1], 1, device=NO_SUCH_DEVICE)
    assert e.value.code == N.BLU_ERR_NO_DEVICE


# ---- end to end ---------------------------------------------------------------------------------------------------------------

def _zymo(golden_dir):
    with gzip.open(os.path.join(golden_dir, "zymo_mock_distilled.json.gz"), "rt") as f:
        cases = json.load(f)["cases"]
    with gzip.open(os.path.join(golden_dir, "zymo_mock_queries.json.gz"), "rt") as f:
        rows = json.load(f)["results"]
    return cases, rows


def test_build_distances_on_the_golden_table(tmp_path, golden_dir, capsys):
    cases, rows = _zymo(golden_dir)
    doc, tab = tmp_path / "doc.json", tmp_path / "table.tsv"
    doc.write_text(json.dumps({"results": [{"query": q, "taxon": None if i is None else cases[i]["taxon"]} for q, i in rows]}))
    bray = tmp_path / "bray.tsv"
    assert cli.main(["blastn", "build-report", str(doc), "--by-sample", "-o", str(tab), "--distance-matrix", str(bray),
                     "--distance-rank", "genus"]) == 0
    text = tab.read_text()
    assert bray.read_text() == ref.matrix_text(text, "g", "bray-curtis")
    names, feats, _ = ref.features(text, "g")
    assert f"distances: {len(feats)} features at genus, 9 samples, {ref.csr(feats)[0][-1]} non-zeros" in capsys.readouterr().err
    for rank in ("g", None):
        for metric in ("bray-curtis", "jaccard"):
            for drop in (False, True):
                out = tmp_path / "m.tsv"
                argv = ["blastn", "build-distances", str(tab), "-o", str(out), "--metric", metric]
                assert cli.main(argv + (["--rank", rank] if rank else []) + (["--drop-unclassified"] if drop else [])) == 0
                assert out.read_text() == ref.matrix_text(text, rank, metric, drop)
    lines = [l.split("\t") for l in out.read_text().splitlines()]
    assert lines[0] == [""] + names and [l[0] for l in lines[1:]] == names
    assert "at no rank" in capsys.readouterr().err
    # a table that does not add up: the message names the line and nothing is written
    bad = tmp_path / "bad.tsv"
    ls = text.splitlines()
    cells = ls[4].split("\t")
    cells[3] = str(int(cells[3]) + 1)
    bad.write_text("\n".join(ls[:4] + ["\t".join(cells)] + ls[5:]) + "\n")
    with pytest.raises(SystemExit, match="line 5:"):
        cli.main(["blastn", "build-distances", str(bad), "-o", str(tmp_path / "no.tsv")])
    assert not (tmp_path / "no.tsv").exists()


def _golden_inputs(tmp_path, taxa, names):
    """the golden's hit table rebuilt: one row per bean occurrence, one query per golden taxon (tests/test_gpu_sample_table.py)"""
    lineages, rows = {}, []
    for name, t in zip(names, taxa):
        for bean in t["consensusBeans"]:
            taxid = lineages.setdefault(bean["taxonomy"], 1000 + len(lineages))
            for k in range(int(bean["occurrences"])):
                a = bean["accessions"][min(k, len(bean["accessions"]) - 1)]
                rows.append(f"{name}\t{a}\t{taxid}\t{t['percIdentity']:.3f}\t{400 + k}\t0\t0\t1\t400\t1\t400\t1e-50\t{int(t['bitScore'])}")
    (tmp_path / "b.tsv").write_text("\n".join(rows) + "\n")
    (tmp_path / "t.json").write_text(json.dumps({"blutilsVersion": "7.1.3", "sourceDatabase": "golden", "taxonomies": [
        {"taxid": v, "rank": "", "numericLineage": k, "textLineage": k, "accessions": []} for k, v in lineages.items()]}))
    return str(tmp_path / "b.tsv"), str(tmp_path / "t.json")


@pytest.mark.parametrize("metric", ["bray-curtis", "jaccard"])
def test_build_consensus_writes_the_matrix_of_its_own_sample_table(tmp_path, golden_dir, metric, capsys):
    cases, rows = _zymo(golden_dir)
    cls = [(q, i) for q, i in rows if i is not None]
    bt, tj = _golden_inputs(tmp_path, [cases[i]["taxon"] for _, i in cls], [q for q, _ in cls])
    doc, tab, out = tmp_path / "doc.json", tmp_path / "table.tsv", tmp_path / "m.tsv"
    assert cli.main(["blastn", "build-consensus", bt, "-t", tj, "--taxon", "bacteria", "--strategy", "relaxed", "--blutils-out-file",
                     str(doc), "--sample-table", str(tab), "--distance-matrix", str(out), "--distance-rank", "g",
                     "--distance-metric", metric]) == 0
    assert out.read_text() == ref.matrix_text(tab.read_text(), "g", metric)
    assert "distances: " in capsys.readouterr().err
    m = [l.split("\t") for l in out.read_text().splitlines()]
    assert len(m) == len(m[0]) and len(m) > 2 and all(m[i][i] == "0.000000" for i in range(1, len(m)))
