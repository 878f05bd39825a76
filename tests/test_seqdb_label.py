"""`build-db sintax` and `build-db dada2` without a GPU: the label rules of tests/seqdb_label_reference.py
against written-out expectations, the host renderer of the library (`blu_seqdb_render_labels`) against the restatement byte
for byte, through the JSON and through a `cache-db` cache, the command line, and the output's name."""
import json
import os

import pytest

from blutils_amd import _native, cli, pipeline, seqdb
from oracle import taxdb_oracle
from tests import seqdb_label_reference as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS = os.path.join(ROOT, "tests", "golden", "taxdb_docs_example")
FMT = {LR.SINTAX: seqdb.SINTAX, LR.DADA2: seqdb.DADA2}

# (name, lineage, sintax label, dada2 label)
HAND = [
    ("full", "d__bacteria;p__firmicutes;c__bacilli;o__bacillales;f__bacillaceae;g__bacillus;s__bacillus-subtilis",
     "d:bacteria,p:firmicutes,c:bacilli,o:bacillales,f:bacillaceae,g:bacillus,s:bacillus-subtilis",
     "bacteria;firmicutes;bacilli;bacillales;bacillaceae;bacillus;"),
    ("superkingdom_left_out", "no-rank__cellular-organisms;superkingdom__bacteria;p__thermotogota;c__thermotogae",
     "p:thermotogota,c:thermotogae", ""),
    ("superkingdom_after_d", "d__bacteria;superkingdom__eubacteria;clade__x;p__thermotogota",
     "d:bacteria,p:thermotogota", "bacteria;thermotogota;"),
    ("two_g", "d__b;g__first;g__second;s__sp", "d:b,g:first,s:sp", "b;"),
    ("no_separator", "d__b;phylum;c__x", "", ""),
    ("empty_identifier", "d__b;p__;c__x", "", ""),
    ("empty_rank", "d__b;__p;c__x", "", ""),
    ("empty_lineage", "", "", ""),
    ("comma_and_space", "d__b;p__a, b:c\td", "d:b,p:a__b_c_d", "b;a__b_c_d;"),
    ("k_and_no_d", "k__fungi;p__ascomycota;c__x", "k:fungi,p:ascomycota,c:x", "fungi;ascomycota;x;"),
    ("d_and_k", "d__eukaryota;k__fungi;p__ascomycota", "d:eukaryota,k:fungi,p:ascomycota", "eukaryota;ascomycota;"),
    ("missing_o", "d__b;p__p1;c__c1;f__f1;g__g1;s__s1", "d:b,p:p1,c:c1,f:f1,g:g1,s:s1", "b;p1;c1;"),
    ("no_kind", "no-rank__root;clade__x;u__y;undefined__z;strain__w", "", ""),
    ("full_names_and_case", "Domain__B; KINGDOM __K;Phylum__P;class__C;ORDER__O;family__F;Genus__G;species__S",
     "d:B,k:K,p:P,c:C,o:O,f:F,g:G,s:S", "B;P;C;O;F;G;"),
    ("lineage_order_kept", "s__sp;g__ge;d__do", "s:sp,g:ge,d:do", "do;"),
    ("utf8_identifier", "d__b;p__café", "d:b,p:café", "b;café;"),
]


def _document(units):
    return {"blutilsVersion": "8.3.1", "ignoreTaxids": None, "replaceRank": None, "dropNonLinnaeanTaxonomies": False,
            "sourceDatabase": "db", "taxonomies": units}


def _hand_document():
    """One row per hand case: the case's lineage as textLineage, `d__2;g__<taxid>` as numericLineage; taxid 7 twice."""
    units = [{"taxid": 100 + i, "rank": "s", "numericLineage": f"d__2;g__{100 + i}", "textLineage": lin, "accessions": []}
             for i, (_, lin, _, _) in enumerate(HAND)]
    units.append({"taxid": 7, "rank": "s", "numericLineage": "d__2", "textLineage": "d__first", "accessions": []})
    units.append({"taxid": 7, "rank": "s", "numericLineage": "d__3", "textLineage": "d__second", "accessions": []})
    return _document(units)


@pytest.mark.parametrize("name,lineage,sintax,dada2", HAND, ids=[h[0] for h in HAND])
def test_label_rules_by_hand(name, lineage, sintax, dada2):
    assert LR.label(LR.SINTAX, lineage) == sintax
    assert LR.label(LR.DADA2, lineage) == dada2


def test_numeric_lineage_under_use_taxid():
    doc = _document([{"taxid": 1423, "rank": "s", "numericLineage": "no-rank__131567;d__2;p__1239;g__1386;s__1423",
                      "textLineage": "no-rank__cellular-organisms;d__bacteria;p__firmicutes;g__bacillus;s__bacillus-subtilis",
                      "accessions": []}])
    assert LR.render(LR.SINTAX, doc, use_taxid=True) == b"1423\td:2,p:1239,g:1386,s:1423\n"
    assert LR.render(LR.DADA2, doc, use_taxid=True) == b"1423\t2;1239;\n"
    assert LR.render(LR.SINTAX, doc) == b"1423\td:bacteria,p:firmicutes,g:bacillus,s:bacillus-subtilis\n"


def _rendered(tmp_path, fmt, source, use_taxid=False) -> bytes:
    out = tmp_path / f"labels-{len(os.listdir(tmp_path))}.tsv"
    seqdb.render_labels(FMT[fmt], str(source), str(out), use_taxid)
    return out.read_bytes()


@pytest.mark.parametrize("use_taxid", [False, True], ids=["text", "numeric"])
@pytest.mark.parametrize("fmt", [LR.SINTAX, LR.DADA2])
def test_library_renders_the_hand_cases_as_the_restatement(tmp_path, fmt, use_taxid):
    """blu_seqdb_render_labels on the hand cases, from the JSON and from a cache of it: the restatement's bytes, rows with an
    empty label and the repeated taxid included."""
    doc = _hand_document()
    src = tmp_path / "hand.blutils.json"
    src.write_text(json.dumps(doc, ensure_ascii=(fmt == LR.DADA2)))            # (escaped and raw UTF-8 both)
    exp = LR.render(fmt, doc, use_taxid)
    if not use_taxid:
        for i, (_, _, sintax, dada2) in enumerate(HAND):
            assert exp.split(b"\n")[i] == f"{100 + i}\t{sintax if fmt == LR.SINTAX else dada2}".encode()
    assert exp.endswith(b"7\t%s\n7\t%s\n" % ((b"d:2", b"d:3") if use_taxid and fmt == LR.SINTAX else (b"2;", b"3;") if use_taxid else
                                                (b"d:first", b"d:second") if fmt == LR.SINTAX else (b"first;", b"second;")))
    assert _rendered(tmp_path, fmt, src, use_taxid) == exp
    cache = tmp_path / "hand.cache"
    pipeline.build_db_cache(str(src), str(cache), use_taxid=use_taxid)
    assert _rendered(tmp_path, fmt, cache, use_taxid) == exp


@pytest.mark.parametrize("replace", [None, [("superkingdom", "d")]], ids=["as_built", "superkingdom_as_d"])
def test_library_renders_the_docs_example_as_the_restatement(tmp_path, replace):
    """tests/golden/taxdb_docs_example built into a document (the oracle of build-db blu), then both formats, both lineage
    flavours, JSON and cache.  As built its lineages start `no-rank__...;superkingdom__bacteria`: SINTAX labels start at the
    phylum and DADA2 has no first level; with `-r superkingdom=d` both start at the domain."""
    raw, _, _ = taxdb_oracle.build(DOCS, os.path.join(DOCS, "accessions.txt"), replace=replace, source_database="db")
    src = tmp_path / "docs.blutils.json"
    src.write_bytes(raw)
    doc = json.loads(raw)
    sintax = LR.render(LR.SINTAX, doc).split(b"\n")
    if replace is None:
        assert sintax[0] == (b"259354\tp:thermodesulfobacteriota,c:desulfobacteria,o:desulfobacterales,f:desulfatibacillaceae,"
                             b"g:desulfatibacillum,s:desulfatibacillum-alkenivorans")
        assert LR.render(LR.DADA2, doc) == b"259354\t\n1006576\t\n"
    else:
        assert sintax[1].startswith(b"1006576\td:bacteria,p:thermotogota,c:thermotogae,")
        assert LR.render(LR.DADA2, doc).split(b"\n")[1] == b"1006576\tbacteria;thermotogota;thermotogae;petrotogales;petrotogaceae;defluviitoga;"
    for use_taxid in (False, True):
        cache = tmp_path / f"docs-{int(use_taxid)}.cache"
        pipeline.build_db_cache(str(src), str(cache), use_taxid=use_taxid)
        for fmt in (LR.SINTAX, LR.DADA2):
            exp = LR.render(fmt, doc, use_taxid)
            assert _rendered(tmp_path, fmt, src, use_taxid) == exp
            assert _rendered(tmp_path, fmt, cache, use_taxid) == exp


def test_renderer_refusals(tmp_path):
    """A cache of the other lineage flavour, a missing file, a format that has no labels."""
    src = tmp_path / "t.blutils.json"
    src.write_text(json.dumps(_hand_document()))
    cache = tmp_path / "t.cache"
    pipeline.build_db_cache(str(src), str(cache), use_taxid=True)
    with pytest.raises(seqdb.SeqdbError, match="numeric"):
        seqdb.render_labels(seqdb.SINTAX, str(cache), str(tmp_path / "o.tsv"), use_taxid=False)
    with pytest.raises(seqdb.SeqdbError, match="not found"):
        seqdb.render_labels(seqdb.SINTAX, str(tmp_path / "absent.json"), str(tmp_path / "o.tsv"))
    with pytest.raises(seqdb.SeqdbError):
        seqdb.render_labels(seqdb.KRAKEN2, str(src), str(tmp_path / "o.tsv"))
    assert not (tmp_path / "o.tsv").exists()


def test_symbols_and_struct_sizes():
    L = _native.lib()
    assert {"blu_seqdb_export_labelled", "blu_seqdb_render_labels"} <= set(_native.PIPELINE_EXPORTS)
    assert hasattr(L, "blu_seqdb_export_labelled") and hasattr(L, "blu_seqdb_render_labels")
    import ctypes as C
    assert C.sizeof(seqdb.SeqdbLabelDesc) == 48 and C.sizeof(seqdb.SeqdbLabelStats) == 120
    assert C.sizeof(seqdb.SeqdbDesc) == 48 and C.sizeof(seqdb.SeqdbStats) == 88           # the two older structs are as they were


def test_cli_shapes():
    p = cli.build_parser()
    for sub in ("sintax", "dada2"):
        a = p.parse_args(["build-db", sub, "tax.json", "db", "out.fna"])
        assert (a.cmd, a.sub, a.taxonomies_database_path, a.blast_database_path, a.output_sequences_file) == (
            "build-db", sub, "tax.json", "db", "out.fna")
        assert (a.use_taxid, a.listing_file, a.blastdbcmd, a.device) == (False, None, "blastdbcmd", 0)
        a = p.parse_args(["build-db", sub, "tax.cache", "db", "out", "-u", "--listing-file", "l.txt", "--blastdbcmd", "/x/b", "--device", "2"])
        assert (a.use_taxid, a.listing_file, a.blastdbcmd, a.device) == (True, "l.txt", "/x/b", 2)
        with pytest.raises(SystemExit):
            p.parse_args(["build-db", sub, "tax.json", "db"])
        with pytest.raises(SystemExit):
            p.parse_args(["build-db", sub])
    assert "build-db sintax" in cli.__doc__ and "build-db dada2" in cli.__doc__ and "(not in the reference CLI) one FASTA" in cli.__doc__


@pytest.mark.parametrize("build", [seqdb.build_sintax_db_from_blutils_db, seqdb.build_dada2_db_from_blutils_db])
def test_output_name_and_removal_of_an_old_output(tmp_path, monkeypatch, build):
    """The output gets the extension fna (PathBuf::set_extension) and an existing file of that name is removed before the
    library is called; with a listing file neither the database check nor blastdbcmd runs."""
    seen = {}

    def fake(fmt, taxonomies_file, fna_path, use_taxid=False, listing_path=None, input_fd=-1, chunk_bytes=0, device=0):
        seen.update(fmt=fmt, tax=taxonomies_file, fna=fna_path, exists=os.path.lexists(fna_path), u=use_taxid, listing=listing_path)
        return {"n_lines": 0}

    monkeypatch.setattr(seqdb, "export_labelled", fake)
    monkeypatch.setattr(seqdb.taxdb, "validate_blast_database_with_taxdb", lambda p: pytest.fail("database check ran"))
    old = tmp_path / "seqs.fna"
    old.write_text("old")
    build("tax.json", "db", str(tmp_path / "seqs.fasta"), True, listing_file="l.txt")
    assert seen == {"fmt": seqdb.SINTAX if build is seqdb.build_sintax_db_from_blutils_db else seqdb.DADA2, "tax": "tax.json",
                    "fna": str(old), "exists": False, "u": True, "listing": "l.txt"}
    assert not old.exists()
    build("tax.json", "db", str(tmp_path / "plain"), listing_file="l.txt")
    assert seen["fna"] == str(tmp_path / "plain.fna")
    assert seqdb.set_extension("a/b.tar.gz", "fna") == "a/b.tar.fna"
