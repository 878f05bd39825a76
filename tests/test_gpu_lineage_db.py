"""`build-db lineages` on the GPU (csrc/lineage_db_gpu.hip) against the plain-Python restatement (tests/lineage_db_reference.py):
the document, the non-mapped TSV, the taxid map and the counts, byte for byte; refusals by table and line; the path dictionary
under narrow hashes and small tables; and the round trip with `build-db blu`, `build-consensus` and `cache-db`."""
import json
import os
import re

import numpy as np
import pytest

from blutils_amd import _native, cli, lineagedb, pipeline, synth_lineages, synth_taxdump, taxdb
from tests import lineage_db_cases as LC
from tests import lineage_db_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "golden", "mock_16S_taxonomies.tsv")
DOCS = os.path.join(ROOT, "tests", "golden", "taxdb_docs_example")
MESSAGE = {"utf8": "the line is not UTF-8", "tab": "no tab between", "id": "an empty ID", "level": "a level without `__`",
           "rank": "a level whose rank is empty", "depth": "more than 64 levels"}
STAT_KEYS = ("data_lines", "taxonomies", "taxa", "empty", "truncated", "max_depth")


def _same(got: bytes, exp: bytes, what: str):
    if got != exp:
        k = next((i for i in range(min(len(got), len(exp))) if got[i] != exp[i]), min(len(got), len(exp)))
        raise AssertionError(f"{what} differs at byte {k} (sizes {len(got)}, {len(exp)}): got {got[max(k - 80, 0):k + 80]!r}, "
                             f"expected {exp[max(k - 80, 0):k + 80]!r}")


def _outputs(tmp_path, name):
    j, t = lineagedb.output_paths(str(tmp_path / name))
    return j, t, str(tmp_path / (name + ".map"))


def _build(tmp_path, data: bytes, replace=None, name="out", **aids):
    """One build through the Python module; returns (doc, tsv, map, stats) after comparing all four with the restatement."""
    table = tmp_path / (name + ".tsv")
    table.write_bytes(data)
    j, t, m = _outputs(tmp_path, name)
    st = lineagedb.build_ref_db_from_lineage_table(str(table), str(tmp_path / name), m, replace, **aids)
    exp = R.build(data, str(table), replace)
    got = tuple(open(p, "rb").read() for p in (j, t, m))
    _same(got[0], exp["doc"], "document")
    _same(got[1], exp["tsv"], "non-mapped TSV")
    _same(got[2], exp["map"], "taxid map")
    assert {k: st[k] for k in STAT_KEYS} == exp["stats"]
    assert st["doc_bytes"] == len(got[0]) and st["tsv_bytes"] == len(got[1]) and st["map_bytes"] == len(got[2])
    assert st["lines"] == len(R.lines_of(data)) and st["input_bytes"] == len(data)
    assert not os.path.exists(m + ".partial")
    return got + (st,)


def _refused(tmp_path, data: bytes, line: int, kind: str, replace=None, name="bad"):
    """The build names the table and the line, as the restatement does, and leaves no file."""
    with pytest.raises(R.LineageError) as e:
        R.build(data, "t", replace)
    assert (e.value.line, e.value.kind) == (line, kind)
    table = tmp_path / (name + ".tsv")
    table.write_bytes(data)
    j, t, m = _outputs(tmp_path, name)
    argv = ["build-db", "lineages", str(table), str(tmp_path / name), "--taxid-map", m]
    for a, b in replace or []:
        argv += ["-r", f"{a}={b}"]
    with pytest.raises(SystemExit, match=re.escape(f"{table}:{line}: {MESSAGE[kind]}")):
        cli.main(argv)
    assert not any(os.path.exists(p) for p in (j, t, m, m + ".partial"))


# ---- rule cases, the mock fixture, the command line -----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_rule_cases(tmp_path, name):
    table, replace, expected = LC.CASES[name]
    if "error" in expected:
        _refused(tmp_path, table, *expected["error"], replace=replace)
        return
    doc, tsv, tmap, _ = _build(tmp_path, table, replace)
    units = [(e["taxid"], e["rank"], e["numericLineage"], e["textLineage"], [(a["accession"], a["oid"]) for a in e["accessions"]])
             for e in json.loads(doc)["taxonomies"]]
    assert units == expected["units"] and tsv == expected["tsv"] and tmap == expected["map"]


def test_mock_fixture_through_the_command_line(tmp_path, capsys):
    out = str(tmp_path / "mock.json")
    m = str(tmp_path / "mock.map")
    assert cli.main(["build-db", "lineages", MOCK, out, "--taxid-map", m]) == 0
    exp = R.build(open(MOCK, "rb").read(), MOCK, None)
    j, t = lineagedb.output_paths(out)
    _same(open(j, "rb").read(), exp["doc"], "document")
    assert open(t, "rb").read() == b"" and open(m, "rb").read() == exp["map"]
    units = json.loads(open(j).read())["taxonomies"]
    assert units[0] == {"taxid": 5, "rank": "f", "numericLineage": "d__1;p__2;c__3;o__4;f__5",
                        "textLineage": "d__2;p__1224;c__1236;o__135622;f__267890",
                        "accessions": [{"accession": "NR025123.135626.Bacb", "oid": "3"}]}
    seven = next(u for u in units if u["taxid"] == 7)
    assert seven["accessions"][:2] == [{"accession": "NR025012.93973.Bac", "oid": "0"}, {"accession": "NR025012.93973.Bac", "oid": "1"}]
    st = exp["stats"]
    assert capsys.readouterr().err.endswith(
        f"lineage table: 53 lines, {st['taxonomies']} taxonomies, {st['taxa']} taxa, 0 without a lineage, 0 truncated, deepest 10 levels\n")


def test_literal_document_and_replace_rank_in_the_head(tmp_path, monkeypatch):
    table = tmp_path / "silva.tsv"
    table.write_bytes(LC.LITERAL_TABLE)
    monkeypatch.chdir(tmp_path)
    assert cli.main(["build-db", "lineages", "silva.tsv", "db", "-r", "SK=d"]) == 0
    assert open("db.blutils.json", "rb").read() == LC.LITERAL_DOC
    assert open("db.non-mapped.tsv", "rb").read() == b"" and not os.path.exists("db.map")
    doc, _, _, _ = _build(tmp_path, LC.LITERAL_TABLE, [("b", "1"), ("a", "2"), ("b", '3"')], name="h")
    assert b'"replaceRank": {\n    "b": "3\\"",\n    "a": "2"\n  },\n' in doc
    doc, _, _, _ = _build(tmp_path, LC.LITERAL_TABLE, [], name="e")
    assert b'"replaceRank": {},\n' in doc


def test_the_tsv_is_recreated_and_the_map_replaced(tmp_path):
    j, t, m = _outputs(tmp_path, "out")
    for p in (t, m):
        open(p, "wb").write(b"stale\n")
    _build(tmp_path, b"a\td__A\n")
    assert open(t, "rb").read() == b"" and open(m, "rb").read() == b"a 1\n"


# ---- seeded random tables -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(4))
def test_seeded_random_tables(tmp_path, k):
    replace = [None, [("d", "sk"), ("clade7", "strain"), ("s", "no rank")], None, [("g", "genus"), ("f", "??x")]][k]
    p = synth_lineages.write_table(str(tmp_path / "in.tsv"), 3000 + 500 * k, [40, 700, 3000, 1500][k], depth=[7, 9, 4, 7][k], seed=20 + k,
                                   ragged=0.2, empty=0.03, greengenes=0.15, noise=0.25, header=k % 2 == 0, confidence=k > 1, crlf=k == 3)
    _, _, _, st = _build(tmp_path, open(p, "rb").read(), replace)
    assert st["empty"] > 0 and st["truncated"] > 0 and st["taxa"] > st["taxonomies"] > 10


# ---- line counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 4095, 4096, 4097])
def test_line_counts(tmp_path, n):
    one = b"".join(b"id%d\td__Bacteria; p__Firmicutes; c__Bacilli\n" % i for i in range(n))
    _, _, _, st = _build(tmp_path, one, name="one")
    assert (st["taxa"], st["taxonomies"]) == ((3, 1) if n else (0, 0))
    own = b"".join(b"id%d\td__Bacteria; p__P%d; c__C%d\n" % (i, i % 7, i) for i in range(n))
    _, _, _, st = _build(tmp_path, own, name="own")
    assert st["taxonomies"] == n and st["taxa"] == (1 + min(n, 7) + n if n else 0)


def test_header_and_comments_only(tmp_path):
    doc, tsv, tmap, st = _build(tmp_path, b"# SILVA 138.1\n\nFeature ID\tTaxon\n# nothing else\n   \n")
    assert doc.endswith(b'"taxonomies": []\n}') and tsv == b"" and tmap == b"" and st["data_lines"] == 0


# ---- depths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 63, 64])
def test_depths(tmp_path, depth):
    _, _, _, st = _build(tmp_path, b"a\td__A\n" + LC.depth_table(depth) + LC.depth_table(depth).replace(b"deep", b"again"))
    assert st["max_depth"] == depth and st["taxa"] == depth + 1


def test_depth_65_is_refused_with_its_line(tmp_path):
    _refused(tmp_path, b"a\td__A\n" + LC.depth_table(64) + LC.depth_table(65), 3, "depth")
    # 65 pieces of which 64 survive are fine: the empty one does not count, the cut one ends the lineage
    _build(tmp_path, b"deep\t;" + LC.depth_table(64)[5:])
    _build(tmp_path, LC.depth_table(64)[:-1] + b";x__;y__z\n", name="cut")


# ---- the path dictionary ----------------------------------------------------------------------------------------------------
def test_same_last_element_under_other_parents_also_when_hashes_collide(tmp_path):
    """Three parents: under a 1-bit hash at least two of the three `g__incertae-sedis` paths share their hash, and every path
    shares it with half the table; they stay three taxa."""
    data = b"".join(b"s%d\tf__Fam%d; g__Incertae_sedis\n" % (i, i % 3) for i in range(9))
    plain = _build(tmp_path, data, name="plain")
    for bits in (1, 2):
        got = _build(tmp_path, data, name="narrow%d" % bits, hash_bits=bits)
        assert got[0].replace(b"narrow%d" % bits, b"plain") == plain[0] and got[1:3] == plain[1:3]
    units = json.loads(plain[0])["taxonomies"]
    assert [u["taxid"] for u in units] == [2, 4, 6] and {u["textLineage"].split(";")[1] for u in units} == {"g__incertae-sedis"}


@pytest.fixture(scope="module")
def taxa_2000(tmp_path_factory):
    """a table of about 2 000 taxa and its 64-bit build"""
    d = tmp_path_factory.mktemp("taxa2000")
    p = synth_lineages.write_table(str(d / "in.tsv"), 2500, 420, depth=7, seed=77, ragged=0.3, greengenes=0.1, noise=0.2)
    data = open(p, "rb").read()
    got = _build(d, data, name="wide")
    assert 1500 < got[3]["taxa"] < 3000
    return data, got


@pytest.mark.parametrize("bits", [1, 4])
def test_narrow_hashes_change_nothing(tmp_path, taxa_2000, bits):
    data, wide = taxa_2000
    got = _build(tmp_path, data, name="wide", hash_bits=bits)
    assert [re.sub(rb'"sourceDatabase": "[^"]*"', b"", x) for x in got[:3]] == [re.sub(rb'"sourceDatabase": "[^"]*"', b"", x) for x in wide[:3]]


@pytest.mark.parametrize("n_taxa, builds", [(7, 1), (8, 1), (9, 2), (1000, 8)])
def test_the_dictionary_grows(tmp_path, n_taxa, builds):
    """16 slots hold 8 paths; the 9th doubles the table once, 1 000 paths double it seven times, to 2 048 slots."""
    data = b"".join(b"s%d\td__Root; p__P%d\n" % (i, i) for i in range(n_taxa - 1)) * 2
    small = _build(tmp_path, data, name="t", initial_slots=16)
    roomy = _build(tmp_path, data, name="t")
    assert small[:3] == roomy[:3] and small[3]["taxa"] == n_taxa
    assert small[3]["n_dictionary_builds"] == builds and roomy[3]["n_dictionary_builds"] == 1


# ---- byte handling ----------------------------------------------------------------------------------------------------------
def test_every_offset_modulo_16(tmp_path):
    """IDs of 1 .. 60 bytes, names of 1 .. 23: line starts, tabs, `;` and line ends fall on every offset modulo 16."""
    lines = [b"i" * a + b"\td__" + b"n" * (1 + a % 23) + b";p__" + b"m" * (1 + (7 * a) % 19) for a in range(1, 61)]
    data = b"\n".join(lines) + b"\n"
    starts = {0} | {i + 1 for i, c in enumerate(data[:-1]) if c == 10}
    assert {s % 16 for s in starts} == set(range(16))
    assert all({i % 16 for i, c in enumerate(data) if c == sep} == set(range(16)) for sep in b"\t;\n")
    _build(tmp_path, data)


def test_line_ends_blanks_and_a_third_column(tmp_path):
    data = (b"Feature ID\tTaxon\tConfidence\r\n"
            b"  a \t d__Bacteria ;\tp__Firmicutes\r\n"               # the second tab ends the lineage
            b"b\tD __ Bacteria;  P__  Firmicutes  ;\t0.9\n"
            b"\r\n"
            b"c\td__Bacteria;p__Firmicutes;c__Bacilli\r\r\n"
            b"\x0bd\x0c\td__Bacteria\x0b;\x0cp__Firmicutes\t\t\t\n"
            b"e\td__Bacteria;p__Firmicutes")                          # no final newline
    doc, _, tmap, st = _build(tmp_path, data)
    assert tmap == b"a 1\nb 2\nc 3\nd 2\ne 2\n" and st["data_lines"] == 5 and st["lines"] == 7


def test_ids_and_names_with_every_kind_of_byte(tmp_path):
    ids = [b'quote"', b"back\\slash", b"ctl\x01\x02\x1f", b"del\x7f", "café".encode(), "\U0001f9a0".encode(), b"b\x08f\x0c",
           b"in ner  blank", b"%d %s"]
    names = [b"Bacillus_A", b"UPPER lower 123", "café".encode(), "éé".encode() + b"x", b"a--b__c", b"(sp.) 7", b"x" * 300]
    data = b"".join(i + b"\td__Bacteria; g__" + names[k % len(names)] + b"\n" for k, i in enumerate(ids))
    doc, _, tmap, _ = _build(tmp_path, data)
    assert [a["accession"].encode() for e in json.loads(doc)["taxonomies"] for a in e["accessions"]].count(b"ctl\x01\x02\x1f") == 1
    assert b'"accession": "ctl\\u0001\\u0002\\u001f"' in doc and b"ctl\x01\x02\x1f 4\n" in tmap


def test_identifiers_and_ids_of_1_to_5000_bytes(tmp_path):
    sizes = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 4095, 4096, 5000]
    data = b"".join(b"I" * n + b"\td__D; g__" + b"aB-" * (n // 3) + b"z" * (n % 3) + b"\n" for n in sizes)
    data += b"".join(b"x\tr" + b"k" * n + b"__v\n" for n in sizes)          # ranks of those sizes too
    _, _, _, st = _build(tmp_path, data)
    assert st["taxonomies"] == 2 * len(sizes)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
BAD = {"utf8": b"x\xe9\td__A", "tab": b"x d__A", "id": b" \td__A", "level": b"x\td__A;Bacteria", "rank": b"x\td__A;__B"}


@pytest.mark.parametrize("kind", sorted(BAD))
@pytest.mark.parametrize("where", ["first", "middle", "last", "last_open"])
def test_one_bad_line(tmp_path, kind, where):
    good = [b"g%d\td__A;p__B%d" % (i, i % 5) for i in range(600)]
    at = {"first": 0, "middle": 300, "last": 600, "last_open": 600}[where]
    lines = good[:at] + [BAD[kind]] + good[at:]
    _refused(tmp_path, b"\n".join(lines) + (b"" if where == "last_open" else b"\n"), at + 1, kind)


def test_two_bad_lines_name_the_lower(tmp_path):
    good = [b"g%d\td__A" % i for i in range(1000)]
    for low, high in (("tab", "utf8"), ("utf8", "tab"), ("level", "id"), ("rank", "level")):
        lines = list(good)
        lines[700], lines[701], lines[999] = BAD[low], BAD[high], BAD[high]
        _refused(tmp_path, b"\n".join(lines) + b"\n", 701, low)
    # a header is not a data line, whatever it holds; a comment is not read at all
    _build(tmp_path, b"# \xff\nFeature ID\tTaxon \xff\na\td__A\n")


def test_refusals_outside_the_table(tmp_path):
    with pytest.raises(SystemExit, match="Invalid lineage table path"):
        cli.main(["build-db", "lineages", str(tmp_path / "none.tsv"), str(tmp_path / "o")])
    (tmp_path / "t.tsv").write_bytes(b"a\td__A\n")
    with pytest.raises(SystemExit, match="cannot create"):
        cli.main(["build-db", "lineages", str(tmp_path / "t.tsv"), str(tmp_path / "no" / "dir" / "o")])


def test_two_builds_are_byte_identical(tmp_path):
    p = synth_lineages.write_table(str(tmp_path / "in.tsv"), 4000, 900, depth=7, seed=5, ragged=0.3, empty=0.02, greengenes=0.1, noise=0.3)
    data = open(p, "rb").read()
    assert _build(tmp_path, data, name="same")[:3] == _build(tmp_path, data, name="same")[:3]


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _qiime_tsv(json_path: str, out: str):
    import ctypes as C
    L = _native.lib()
    L.blu_qiime_taxonomy_tsv.restype = C.c_int
    L.blu_qiime_taxonomy_tsv.argtypes = [C.c_char_p, C.c_int, C.c_char_p]
    assert L.blu_qiime_taxonomy_tsv(json_path.encode(), 0, out.encode()) == 0, _native.last_error()


def _consensus(table: str, tax_file: str, tmp_path, tag: str):
    """document (run ids blanked), report and support table of one build-consensus run"""
    rep, sup = str(tmp_path / (tag + ".report")), str(tmp_path / (tag + ".support"))
    text, _ = pipeline.build_consensus_identities_with_tables(table, tax_file, "bacteria", "relaxed", False, lenient=True, parse=False,
                                                              report_path=rep, support_table_path=sup)
    return re.sub(r'"runId": "[^"]*"', '"runId": ""', text), open(rep, "rb").read(), open(sup, "rb").read()


def _round_trip(tmp_path, dump_dir: str, accessions: str):
    a_out = str(tmp_path / "a.json")
    assert cli.main(["build-db", "blu", "blast/16S", dump_dir, a_out, "--accessions-file", accessions]) == 0
    a_json = taxdb.output_paths(a_out)[0]
    a = json.load(open(a_json))["taxonomies"]
    roots = {str(e["taxid"]) for e in a if e["textLineage"].startswith(";")}
    if roots:
        # `build-db blu` spells a taxon without ancestors `;rank__name`; a lineage table has no empty level, so such a taxon comes
        # back as `rank__name`: its lines are left out of the listing
        kept = [line for line in open(accessions) if line.split("  ")[1] not in roots]
        accessions = str(tmp_path / "accessions_without_roots.txt")
        open(accessions, "w").writelines(kept)
        assert cli.main(["build-db", "blu", "blast/16S", dump_dir, a_out, "--accessions-file", accessions]) == 0
        a = json.load(open(a_json))["taxonomies"]
        assert not any(e["textLineage"].startswith(";") for e in a)
    lineages = [e["textLineage"] for e in a]
    assert len(set(lineages)) == len(lineages) > 1                      # else two old taxids would be one new taxon
    qiime = str(tmp_path / "a_taxonomy.tsv")
    _qiime_tsv(a_json, qiime)
    b_out, b_map = str(tmp_path / "b.json"), str(tmp_path / "b.map")
    assert cli.main(["build-db", "lineages", qiime, b_out, "--taxid-map", b_map]) == 0
    b_json, b_tsv = lineagedb.output_paths(b_out)
    assert open(b_tsv, "rb").read() == b""
    # join on Feature ID: `{taxid}-{oid}-{acc}` carries the old taxid, the map gives the new one
    pairs = set()
    for line in open(b_map, "rb").read().decode().splitlines():
        fid, new = line.rsplit(" ", 1)
        pairs.add((int(fid.split("-", 1)[0]), int(new)))
    old_to_new = dict(pairs)
    assert len(old_to_new) == len(pairs) == len({n for _, n in pairs}) == len(a)         # a bijection, onto the entries of A
    b = {e["taxid"]: e for e in json.load(open(b_json))["taxonomies"]}
    assert all(b[old_to_new[e["taxid"]]]["textLineage"] == e["textLineage"] for e in a)
    # a BLAST table over A's subjects, and the same with column 3 rewritten
    subj = [(acc["accession"], e["taxid"]) for e in a for acc in e["accessions"]]
    rng = np.random.default_rng(3)
    rows = []
    for q in range(300):
        for _ in range(int(rng.integers(1, 8))):
            acc, t = subj[int(rng.integers(0, len(subj)))]
            rows.append([f"q{q:04d}", acc, t, f"{float(rng.choice([100.0, 99.5, 98.0, 96.0, 91.0, 80.0])):.3f}", 400, 3, 1, 1, 400, 5, 404,
                         "1e-120", int(rng.choice([500, 500, 480, 400]))])
    ta, tb = tmp_path / "blast_a.tsv", tmp_path / "blast_b.tsv"
    ta.write_text("".join("\t".join(map(str, r)) + "\n" for r in rows))
    tb.write_text("".join("\t".join(map(str, r[:2] + [old_to_new[r[2]]] + r[3:])) + "\n" for r in rows))
    with_a = _consensus(str(ta), a_json, tmp_path, "a")
    with_b = _consensus(str(tb), b_json, tmp_path, "b")
    assert with_a == with_b and '"taxon"' in with_a[0] and len(with_a[1]) > 100 and len(with_a[2]) > 100
    cache = str(tmp_path / "b.blucache")
    assert cli.main(["cache-db", b_json, cache]) == 0
    assert _consensus(str(tb), cache, tmp_path, "c") == with_b


def test_round_trip_with_build_db_blu_on_the_docs_example(tmp_path):
    _round_trip(tmp_path, DOCS, os.path.join(DOCS, "accessions.txt"))


def test_round_trip_with_build_db_blu_on_a_synthetic_dump(tmp_path):
    p = synth_taxdump.make_taxdump(str(tmp_path / "dump"), n_nodes=3000, depth=10, n_accessions=6000, seed=12, oddities=False)
    _round_trip(tmp_path, str(tmp_path / "dump"), p["accessions"])
