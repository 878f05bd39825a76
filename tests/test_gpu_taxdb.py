"""`build-db blu` on the GPU (csrc/taxdb_gpu.hip) against the test-only oracle (oracle/taxdb_oracle.py): every rule case,
the book example, seeded random dumps under every option combination, a large run, and the round trip through
build-consensus and cache-db."""
import json
import os

import numpy as np
import pytest

from blutils_amd import cli, pipeline, synth_taxdump, taxdb
from oracle import taxdb_oracle as orc
from tests import taxdb_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS = os.path.join(ROOT, "tests", "golden", "taxdb_docs_example")


def _cli_build(dump_dir, accessions, out, opts, db="blast/16S"):
    argv = ["build-db", "blu", db, dump_dir, out, "--accessions-file", accessions]
    if opts.get("drop"):
        argv.append("-d")
    for s in opts.get("skip") or []:
        argv += ["-s", str(s)]
    for a, b in opts.get("replace") or []:
        argv += ["-r", f"{a}={b}"]
    assert cli.main(argv) == 0
    j, t = taxdb.output_paths(out)
    return open(j, "rb").read(), open(t, "rb").read()


def _check(dump_dir, accessions, tmp_path, opts, name="out"):
    got_doc, got_tsv = _cli_build(dump_dir, accessions, str(tmp_path / name), opts)
    exp_doc, exp_tsv, st = orc.build(dump_dir, accessions, source_database="blast/16S", **opts)
    assert got_tsv == exp_tsv
    if got_doc != exp_doc:
        k = next(i for i in range(min(len(got_doc), len(exp_doc))) if got_doc[i] != exp_doc[i]) if got_doc[:1] else 0
        raise AssertionError(f"documents differ at byte {k}: got {got_doc[k - 80:k + 80]!r}, expected {exp_doc[k - 80:k + 80]!r}")
    return st


def test_book_example(tmp_path):
    _check(DOCS, os.path.join(DOCS, "accessions.txt"), tmp_path, {})


@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_rule_cases(tmp_path, name):
    kw, opts, _, _ = tc.CASES[name]
    c = tc.write_case(str(tmp_path / "dump"), **kw)
    _check(c["dir"], c["accessions"], tmp_path, opts)


def test_stats_and_errors(tmp_path):
    c = tc.write_case(str(tmp_path / "d"), merged=tc.dmp(99, 50) + tc.dmp(97, 12345), delnodes=tc.dmp(98),
                      accessions="A  99  1\nB  98  2\nC  97  3\nD  -1  4\nE  60  5\nF  50  6\n",
                      lineage="".join(tc.dmp(t, (l + " ") if l else "") for t, l in tc.BASE_LINEAGE.items() if t != 60)
                      + tc.dmp(60, "10 555 70 20 30 40 50 "))
    _, _, exp = orc.build(c["dir"], c["accessions"], drop=True)
    got = taxdb.build_from_files({k: os.path.join(c["dir"], k + ".dmp") for k in taxdb.DUMPS}, c["accessions"],
                                 str(tmp_path / "o"), "db", drop_non_linnaean_taxonomies=True)
    assert {k: got[k] for k in exp} == exp
    bad = tc.write_case(str(tmp_path / "e"), nodes=tc.dmp(1, 1, "no rank") + "2\t|\t1\n", accessions="")
    with pytest.raises(SystemExit, match=r"nodes\.dmp:2: "):
        cli.main(["build-db", "blu", "db", bad["dir"], str(tmp_path / "o2"), "--accessions-file", bad["accessions"]])
    bad = tc.write_case(str(tmp_path / "f"), accessions="A  1  1\nB 2 3\n")
    with pytest.raises(SystemExit, match=r"accessions\.txt:2: "):
        cli.main(["build-db", "blu", "db", bad["dir"], str(tmp_path / "o3"), "--accessions-file", bad["accessions"]])
    bad = tc.write_case(str(tmp_path / "g"), accessions="A  50  1\n",
                        lineage="".join(tc.dmp(t, (l + " ") if l else "") for t, l in tc.BASE_LINEAGE.items() if t != 50)
                        + tc.dmp(50, "10 x7 "))
    with pytest.raises(SystemExit, match=r"taxidlineage\.dmp:\d+: an ancestor that is not a taxid"):
        cli.main(["build-db", "blu", "db", bad["dir"], str(tmp_path / "o4"), "--accessions-file", bad["accessions"]])


OPTION_SETS = [{}, {"drop": True}, {"skip": None}, {"replace": [("superkingdom", "d"), ("clade", "cl"), ("strain", "s")]},
               {"drop": True, "skip": None, "replace": [("superkingdom", "domain"), ("no rank", "k")]}]


@pytest.mark.parametrize("k", range(len(OPTION_SETS)))
def test_seeded_random_dumps(tmp_path, k):
    p = synth_taxdump.make_taxdump(str(tmp_path / "dump"), n_nodes=50_000, depth=14, n_accessions=200_000, seed=100 + k)
    opts = dict(OPTION_SETS[k])
    if "skip" in opts:
        ids = [int(l.split("\t")[0]) for l in open(p["nodes"]).readlines()[:3]]
        opts["skip"] = ids + [2 ** 40]
    st = _check(str(tmp_path / "dump"), p["accessions"], tmp_path, opts)
    assert st["mapped"] > 0 and st["unknown"] > 0 and st["deleted"] > 0 and st["merged_missing"] > 0


def test_large_build_is_exact_and_deterministic(tmp_path):
    """NCBI-shaped scale (BLU_TAXDB_NODES / BLU_TAXDB_ACCESSIONS raise it to the new_taxdump's 2.7 M nodes): the whole
    document and TSV equal the oracle's, the stats equal its counts, two builds are byte-identical."""
    n_nodes = int(os.environ.get("BLU_TAXDB_NODES", "400000"))
    n_acc = int(os.environ.get("BLU_TAXDB_ACCESSIONS", "2000000"))
    p = synth_taxdump.make_taxdump(str(tmp_path / "dump"), n_nodes=n_nodes, depth=25, n_accessions=n_acc, seed=7)
    dumps = {k: p[k] for k in taxdb.DUMPS}
    opts = {"replace": [("superkingdom", "d")]}
    st = taxdb.build_from_files(dumps, p["accessions"], str(tmp_path / "a"), "nt", replace_rank=opts["replace"])
    taxdb.build_from_files(dumps, p["accessions"], str(tmp_path / "b"), "nt", replace_rank=opts["replace"])
    ja, ta = taxdb.output_paths(str(tmp_path / "a"))
    jb, tb = taxdb.output_paths(str(tmp_path / "b"))
    doc, tsv = open(ja, "rb").read(), open(ta, "rb").read()
    assert doc == open(jb, "rb").read() and tsv == open(tb, "rb").read()
    exp_doc, exp_tsv, exp_st = orc.build(str(tmp_path / "dump"), p["accessions"], source_database="nt", **opts)
    assert {k: st[k] for k in exp_st} == exp_st
    assert tsv == exp_tsv
    # a seeded sample of 20 000 taxids entry for entry, then the whole document
    got_e = {e["taxid"]: e for e in json.loads(doc)["taxonomies"]}
    exp_e = {e["taxid"]: e for e in json.loads(exp_doc)["taxonomies"]}
    rng = np.random.default_rng(11)
    sample = rng.choice(sorted(exp_e), size=min(20_000, len(exp_e)), replace=False)
    assert all(got_e[int(t)] == exp_e[int(t)] for t in sample)
    assert doc == exp_doc


@pytest.mark.parametrize("use_taxid", [False, True])
def test_round_trip_through_build_consensus_and_cache(tmp_path, use_taxid):
    """The DB built here is the -t of build-consensus on a BLAST table whose subjects come from it: the loader reads
    lineages this tree produced from NCBI-shaped data.  The result equals the faithful oracle's on the same DB, and the
    binary cache of the built DB gives the same document."""
    from tests.test_gpu_pipeline import _oracle_from_files
    from oracle import oracle as corc
    p = synth_taxdump.make_taxdump(str(tmp_path / "dump"), n_nodes=20_000, depth=12, n_accessions=60_000, seed=5)
    out = str(tmp_path / "db")
    taxdb.build_from_files({k: p[k] for k in taxdb.DUMPS}, p["accessions"], out, "synthetic",
                           replace_rank=[("superkingdom", "d")])
    tj = taxdb.output_paths(out)[0]
    db = json.load(open(tj))
    subj = [(a["accession"], e["taxid"]) for e in db["taxonomies"] for a in e["accessions"]]
    rng = np.random.default_rng(3)
    rows = []
    for q in range(800):
        for j in range(int(rng.integers(1, 8))):
            acc, t = subj[int(rng.integers(0, len(subj)))]
            pid = float(rng.choice([100.0, 99.5, 98.0, 96.0, 91.0, 80.0]))
            bs = int(rng.choice([500, 500, 480, 400]))
            rows.append(f"q{q:06d}\t{acc}\t{t}\t{pid:.3f}\t400\t3\t1\t1\t400\t5\t404\t1e-120\t{bs}")
    bt = tmp_path / "blast.tsv"
    bt.write_text("\n".join(rows) + "\n")
    got, _ = pipeline.build_consensus_identities(str(bt), tj, "bacteria", "relaxed", use_taxid, lenient=True)
    exp = _oracle_from_files(str(bt), tj, use_taxid, "bacteria", "relaxed", None)
    n = 0
    for g in got:
        o = exp[g["query"]]
        if o["status"] != corc.ST_CONSENSUS:
            assert g["taxon"] is None
            continue
        assert g["taxon"] == o["taxon"], g["query"]
        n += 1
    assert n > 200
    cache = str(tmp_path / "db.blucache")
    assert cli.main(["cache-db", tj, cache] + (["-u"] if use_taxid else [])) == 0
    a, _ = pipeline.build_consensus_identities(str(bt), tj, "bacteria", "relaxed", use_taxid, lenient=True, parse=False)
    b, _ = pipeline.build_consensus_identities(str(bt), cache, "bacteria", "relaxed", use_taxid, lenient=True, parse=False)
    ja, jb = json.loads(a), json.loads(b)
    for r in ja["results"] + jb["results"]:
        r["runId"] = None
    assert ja == jb
