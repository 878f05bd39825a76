"""`build-db blu` on the GPU (csrc/taxdb_gpu.hip, csrc/text_dev.h) at the byte-level edges of tests/taxdb_edges.py: every
respelled case, the line counts around the kernels' block sizes and the largest ids around the sort's pass counts give the
oracle's document, TSV and stats byte for byte, twice; every refused case is refused naming file and line and leaves no file
behind."""
import os

import pytest
import torch

from blutils_amd import cli, taxdb
from oracle import taxdb_oracle as orc
from tests import taxdb_edges as te
from tests.test_gpu_taxdb import OPTION_SETS, _cli_build

pytestmark = pytest.mark.gpu
TABLE_BYTES_PER_ID = 27          # taxdb_gpu.hip "tables": four row words, the deleted flag, the rank hash and the rank id


def _diff(what, got, exp):
    if got != exp:
        k = next((i for i in range(min(len(got), len(exp))) if got[i] != exp[i]), min(len(got), len(exp)))
        raise AssertionError(f"{what} differs at byte {k} (lengths {len(got)} / {len(exp)}): got {got[max(k - 80, 0):k + 80]!r}, "
                             f"expected {exp[max(k - 80, 0):k + 80]!r}")


def _check(files, tmp_path, opts=None):
    """The CLI's document and TSV equal the oracle's; a second build through build_from_files writes the same bytes and
    returns the oracle's stats, every key of them."""
    opts = opts or {}
    c = te.write(str(tmp_path / "dump"), files)
    exp_doc, exp_tsv, exp_st = orc.build(c["dir"], c["accessions"], source_database="blast/16S", **opts)
    got_doc, got_tsv = _cli_build(c["dir"], c["accessions"], str(tmp_path / "out"), opts)
    _diff("TSV", got_tsv, exp_tsv)
    _diff("document", got_doc, exp_doc)
    st = taxdb.build_from_files({k: os.path.join(c["dir"], k + ".dmp") for k in taxdb.DUMPS}, c["accessions"], str(tmp_path / "again"),
                                "blast/16S", skip_taxids=opts.get("skip"), replace_rank=opts.get("replace"),
                                drop_non_linnaean_taxonomies=bool(opts.get("drop")))
    assert {k: st[k] for k in exp_st} == exp_st
    j, t = taxdb.output_paths(str(tmp_path / "again"))
    assert open(j, "rb").read() == got_doc and open(t, "rb").read() == got_tsv, "two builds of one input differ"
    return exp_st


def _refused(files, tmp_path, pattern):
    """SystemExit matching pattern; neither output exists afterwards.  (The CLI writes both files only after every check has
    passed, so a refused build leaves nothing; the reference has by then removed and recreated an empty TSV, rs:256-262, and
    never a document.)"""
    c = te.write(str(tmp_path / "dump"), files)
    out = str(tmp_path / "out")
    with pytest.raises(SystemExit, match=pattern):
        cli.main(["build-db", "blu", "db", c["dir"], out, "--accessions-file", c["accessions"]])
    assert [p for p in taxdb.output_paths(out) if os.path.exists(p)] == []


@pytest.mark.parametrize("cls,seed", te.ACCEPTED_IDS, ids=[f"{c}-{s}" for c, s in te.ACCEPTED_IDS])
def test_accepted(tmp_path, cls, seed):
    case = te.accepted(cls, seed)
    st = _check(case["files"], tmp_path)
    for k, v in case["stat"].items():
        assert st[k] == v


@pytest.mark.parametrize("k", range(len(OPTION_SETS)))
@pytest.mark.parametrize("cls,seed", [("lineage_tokens", 0), ("ranks", 0), ("ranks", 1), ("names", 0)])
def test_accepted_under_options(tmp_path, cls, seed, k):
    """-d, -s and -r act on the lineage walk, the ranks and the names: each option set of test_gpu_taxdb on those classes."""
    case = te.accepted(cls, seed)
    opts = dict(OPTION_SETS[k])
    if "skip" in opts:
        lin = te.Doc(case["base"]).d["taxidlineage.dmp"]
        deep = max(lin, key=lambda l: len(l[0][1]))[0][1].split()
        opts["skip"] = [int(deep[0]), int(deep[len(deep) // 2]), int(deep[-1]), 2 ** 40]
    st = _check(case["files"], tmp_path, opts)
    assert st["mapped"] > 0 and (not opts.get("drop") or st["dropped"] > 0)


@pytest.mark.parametrize("name", [n for n, _ in te.COUNTS])
def test_counts(tmp_path, name):
    _check(te.sized_files(**dict(te.COUNTS)[name]), tmp_path)


@pytest.mark.parametrize("name", sorted(te.REFUSED))
def test_refused(tmp_path, name):
    files, bad_file, line = te.REFUSED[name]
    _refused(files, tmp_path, rf"/{bad_file.replace('.', chr(92) + '.')}:{line}: ")


@pytest.mark.parametrize("name", sorted(te.UNREAD_ANCESTORS))
def test_bad_ancestor_of_a_taxid_nobody_names_is_not_read(tmp_path, name):
    _check(te.UNREAD_ANCESTORS[name], tmp_path)


@pytest.mark.parametrize("name", sorted(te.PRECEDENCE))
def test_precedence(tmp_path, name):
    files, bad_file, line = te.PRECEDENCE[name]
    _refused(files, tmp_path, rf"/{bad_file.replace('.', chr(92) + '.')}:{line}: ")


@pytest.mark.parametrize("n,limit", [(2049, 2048), (5000, 4096)])
def test_more_ranks_than_the_table_holds(tmp_path, n, limit):
    """A divergence: the oracle, like the reference, has no rank limit; the builder interns at most 2048 ranks
    in 4096 slots and says so.  The host sees the table's `full` flag before any kernel probes the full table."""
    _refused(te.many_ranks(n), tmp_path, rf"nodes\.dmp has more (?=.*distinct ranks).*\b{limit}\b")


def test_largest_accepted_dump_id(tmp_path):
    """An id of 2^31 - 1 is accepted (2^31 is refused: test_refused[id_2^31-*]); the direct-addressed tables then span
    [0, 2^31).  Runs only where twice their size is free."""
    need = 2 * TABLE_BYTES_PER_ID * (1 << 31)
    free, _ = torch.cuda.mem_get_info()
    print(f"device memory free: {free} bytes, wanted: {need}")
    if free < need:
        pytest.skip(f"{free} bytes of device memory free, {need} wanted (twice the tables over [0, 2^31))")
    top = (1 << 31) - 1
    files = te._dumps()
    files["nodes.dmp"].append(b"%d\t|\t1\t|\tspecies\t|\n" % top)
    files["taxidlineage.dmp"].append(b"%d\t|\t10 %d 40 \t|\n" % (top, top))
    files["names.dmp"].append(b"%d\t|\tTop of the range\t|\t\t|\tscientific name\t|\n" % top)
    files[te.ACC] += [b"E  %d  5\n" % top, b"F  %d  6\n" % (top + 1), b"G  %d  7\n" % (top - 1)]
    files = {n: b"".join(v) for n, v in files.items()}
    c = te.write(str(tmp_path / "dump"), files)
    exp_doc, exp_tsv, exp_st = orc.build(c["dir"], c["accessions"], source_database="blast/16S")
    st = taxdb.build_from_files({k: os.path.join(c["dir"], k + ".dmp") for k in taxdb.DUMPS}, c["accessions"], str(tmp_path / "out"),
                                "blast/16S")
    j, t = taxdb.output_paths(str(tmp_path / "out"))
    _diff("TSV", open(t, "rb").read(), exp_tsv)
    _diff("document", open(j, "rb").read(), exp_doc)
    assert {k: st[k] for k in exp_st} == exp_st and st["mapped"] == 3 and st["mapped_merged"] == 1
