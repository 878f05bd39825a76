"""Taxon filters on the host parser (device=-1, no GPU): an ingest under a taxon filter gives the columns an
independent reading (tests/ingest_reference.py) gives of the table from which tests/taxon_filter_reference.py deleted the
dropped lines, and the four counts of that restatement."""
import numpy as np
import pytest

from blutils_amd import _native as N
from blutils_amd import cli, pipeline
from tests import hit_filter_reference as hf
from tests import ingest_reference as ref
from tests import taxon_filter_reference as tf


def _table(tmp_path, rows, name="b.tsv", eol="\n", final=True):
    bt = tmp_path / name
    bt.write_bytes((eol.join(rows) + (eol if final else "")).encode())
    return str(bt)


def _check(src, tj, tmp_path, exclude=(), only=(), use_taxid=False, hit=None, device=-1, tax_file=None):
    """ingest of src under the filter == independent reading of filter_text's copy, and the counts; returns (columns, counts)"""
    dst = str(tmp_path / "taxon_copy.tsv")
    keep = (lambda f: hf.keep(f, hit)) if hit else None
    c = tf.filter_text(src, dst, tj, exclude, only, use_taxid, keep)
    got = pipeline.ingest_columns(src, tax_file or tj, use_taxid=use_taxid, device=device, hit_filter=hit,
                                  taxon_filter=pipeline.TaxonFilter(exclude, only))
    hf.assert_columns_equal(got, ref.read_table(dst, tj))
    t = got["taxon_filter"]
    assert (t["n_lines"], t["n_excluded"], t["n_not_only"], t["excluded_by"]) == (c["n_lines"], c["n_excluded"], c["n_not_only"], c["excluded_by"])
    assert (got["n_lines"], got["n_kept"]) == (c["n_lines"], c["n_kept"])
    return got, c


CASES = {
    "exclude": (tf.EXCLUDE, (), False),
    "only": ((), tf.ONLY, False),
    "both": (tf.EXCLUDE, tf.ONLY, False),
    "pattern": (["s__uncultured-b*", "g__Gen1*", "o__*"], (), False),
    "species_spelling": (["species__uncultured-organism", "Species__bac-sp0", " S__arc-sp1"], ["DOMAIN__Bacteria", "domain__Archaea"], False),
    "numeric": (tf.EXCLUDE_NUMERIC, tf.ONLY_NUMERIC, True),
}


@pytest.mark.parametrize("layout", ["grouped", "scrambled"])
@pytest.mark.parametrize("which", list(CASES))
def test_filtered_ingest_is_the_ingest_of_the_filtered_copy(tmp_path, layout, which):
    rng = np.random.default_rng(61)
    rows = tf.make_rows(600, 8, rng)
    if layout == "scrambled":
        rows = hf.scramble(rows, rng)
    src, tj = _table(tmp_path, rows), tf.write_db(tmp_path / "t.json")
    exclude, only, use_taxid = CASES[which]
    got, c = _check(src, tj, tmp_path, exclude, only, use_taxid)
    assert c["n_lines"] == len(rows) and 0 < c["n_kept"] < c["n_lines"]
    assert (c["n_excluded"] > 0) == bool(exclude) and (c["n_not_only"] > 0) == bool(only)
    assert all(n > 0 for n in c["excluded_by"])                            # every element of these lists drops lines
    # unmatched lines pass an exclude list and fail an only list
    assert (int((got["tax_desc_row"] == ref.UNMATCHED).sum()) > 0) == (not only)


@pytest.mark.parametrize("which", ["pid", "aln", "evalue_1e-30", "bits", "all"])
def test_with_thresholds_alongside(tmp_path, which):
    """The taxon counts do not depend on the thresholds; n_kept is what both keep."""
    rng = np.random.default_rng(62)
    src, tj = _table(tmp_path, hf.scramble(tf.make_rows(500, 8, rng), rng)), tf.write_db(tmp_path / "t.json")
    _, alone = _check(src, tj, tmp_path, tf.EXCLUDE, tf.ONLY)
    _, c = _check(src, tj, tmp_path, tf.EXCLUDE, tf.ONLY, hit=hf.FILTERS[which])
    assert 0 < c["n_kept"] < alone["n_kept"]
    assert all(c[k] == alone[k] for k in ("n_lines", "n_excluded", "n_not_only", "excluded_by"))


def test_first_matching_element_in_list_order(tmp_path):
    """taxid 1005 is both `uncultured-*` and under d__Eukaryota (as 1008 is, without the name): the element listed first counts it."""
    tj = tf.write_db(tmp_path / "t.json")
    src = _table(tmp_path, [tf.line("a", 1005), tf.line("a", 1000), tf.line("b", 1008), tf.line("c", 1005)])
    _, c = _check(src, tj, tmp_path, ["d__Eukaryota", "s__uncultured-*"])
    assert c["excluded_by"] == [3, 0]
    _, c2 = _check(src, tj, tmp_path, ["s__uncultured-*", "d__Eukaryota"])
    assert c2["excluded_by"] == [2, 1]
    # the same element twice: the first listing counts
    _, c3 = _check(src, tj, tmp_path, ["d__Eukaryota", "domain__Eukaryota"])
    assert c3["excluded_by"][1] == 0 and c3["excluded_by"][0] == c3["n_excluded"] > 0


def test_lines_without_elements(tmp_path):
    """Unmatched, bad-lineage and empty-lineage lines: kept under exclude, dropped under only."""
    tj = tf.write_db(tmp_path / "t.json")
    rows = [tf.line("u", 1042), tf.line("bad", tf.BAD_TAXID), tf.line("empty", tf.EMPTY_TAXID), tf.line("ok", 1000), tf.line("euk", 1008)]
    src = _table(tmp_path, rows)
    got, c = _check(src, tj, tmp_path, exclude=["d__Eukaryota"])
    assert got["query_names"] == [b"u", b"bad", b"empty", b"ok"] and c["n_excluded"] == 1
    got, c = _check(src, tj, tmp_path, only=["d__Bacteria"])
    assert got["query_names"] == [b"ok"] and c["n_not_only"] == 4
    got, c = _check(src, tj, tmp_path, exclude=["d__Bacteria"], only=["d__Bacteria"])        # exclude wins over only
    assert got["n_kept"] == 0 and (c["n_excluded"], c["n_not_only"]) == (1, 4)
    # nothing left: the result of a zero-byte file
    empty = tmp_path / "empty.tsv"
    empty.write_bytes(b"")
    hf.assert_columns_equal(got, pipeline.ingest_columns(str(empty), tj, device=-1))
    # the bad lineage's first element reached the dictionary but is in no lineage; its other elements are not elements at all
    for el in ("p__only-here", "s__lost"):
        with pytest.raises(N.BluError, match=el):
            pipeline.ingest_columns(src, tj, device=-1, taxon_filter={"exclude": [el]})


def test_a_taxid_listed_twice_takes_its_first_listing(tmp_path):
    dup = (1003, "d__Eukaryota;s__other-listing", "d__2759;s__77")
    tj = tf.write_db(tmp_path / "t.json", duplicate=dup)
    rows = [tf.line("a", 1003), tf.line("a", 1008), tf.line("b", 1003), tf.line("b", 1000)]
    src = _table(tmp_path, rows)
    # the first listing of 1003 is bacterial: the line passes d__Eukaryota although its second listing is there, and both
    # joined rows of the kept line stay
    got, c = _check(src, tj, tmp_path, exclude=["d__Eukaryota"])
    assert c["n_excluded"] == 1 and got["seg_off"].tolist() == [0, 2, 5]
    got, c = _check(src, tj, tmp_path, only=["s__other-listing"])          # names a node, but no line's first listing holds it
    assert c["n_kept"] == 0 and c["n_not_only"] == 4


def test_the_binary_cache(tmp_path):
    rng = np.random.default_rng(63)
    src, tj = _table(tmp_path, hf.scramble(tf.make_rows(300, 8, rng), rng)), tf.write_db(tmp_path / "t.json")
    for use_taxid, exclude, only in ((False, tf.EXCLUDE, tf.ONLY), (True, tf.EXCLUDE_NUMERIC, tf.ONLY_NUMERIC)):
        cache = str(tmp_path / f"t{int(use_taxid)}.cache")
        pipeline.build_db_cache(tj, cache, use_taxid)
        _, c = _check(src, tj, tmp_path, exclude, only, use_taxid, tax_file=cache)
        assert 0 < c["n_kept"] < c["n_lines"]
        for el in ("s__lost", "p__99" if use_taxid else "p__only-here"):       # (in the cache's dictionary, in no lineage)
            with pytest.raises(N.BluError, match=el):
                pipeline.ingest_columns(src, cache, use_taxid=use_taxid, device=-1, taxon_filter={"exclude": [el]})


@pytest.mark.parametrize("eol,final", [("\n", True), ("\r\n", True), ("\n", False), ("\r\n", False)])
def test_line_ends(tmp_path, eol, final):
    rng = np.random.default_rng(64)
    tj = tf.write_db(tmp_path / "t.json")
    _check(_table(tmp_path, tf.make_rows(60, 5, rng), eol=eol, final=final), tj, tmp_path, tf.EXCLUDE, tf.ONLY)


def test_elements_that_are_refused(tmp_path):
    tj = tf.write_db(tmp_path / "t.json")
    src = _table(tmp_path, [tf.line("a", 1000)])
    bad = {"s__no-such-species": "s__no-such-species", "s__nothing-starts-so*": "nothing-starts-so", "k__*": "k__",
           "Bacteria": "Bacteria", "d__": "d__", "__Bacteria": "__Bacteria", "d__Bacteria__x": "d__Bacteria__x", "": "RANK__IDENTIFIER",
           "d__bacteria": "d__bacteria"}                                   # (identifiers are matched as written)
    for el, named in bad.items():
        for key in ("exclude", "only"):
            with pytest.raises(N.BluError, match=named.replace("*", r"\*")) as ei:
                pipeline.ingest_columns(src, tj, device=-1, taxon_filter={key: ["d__Archaea", el]})
            assert ei.value.code == 1, el                                  # BLU_ERR_INVALID_ARG
    # the same elements under the other lineage flavour
    with pytest.raises(N.BluError, match="d__Bacteria"):
        pipeline.ingest_columns(src, tj, use_taxid=True, device=-1, taxon_filter={"exclude": ["d__Bacteria"]})
    # 65 534 exclude elements are taken, 65 535 refused before anything is resolved
    many = ["d__Bacteria"] * 65534
    got = pipeline.ingest_columns(src, tj, device=-1, taxon_filter={"exclude": many})
    assert got["taxon_filter"]["excluded_by"][:2] == [1, 0] and len(got["taxon_filter"]["excluded_by"]) == 65534
    with pytest.raises(N.BluError, match="65535 exclude elements") as ei:
        pipeline.ingest_columns(src, tj, device=-1, taxon_filter={"exclude": many + ["d__Archaea"]})
    assert ei.value.code == 1
    with pytest.raises(ValueError):
        pipeline.ingest_columns(src, tj, device=-1, taxon_filter={"exclude": "d__Bacteria"})
    with pytest.raises(ValueError):
        pipeline.ingest_columns(src, tj, device=-1, taxon_filter={"without": ["d__Bacteria"]})


def test_validation_does_not_depend_on_the_verdict(tmp_path):
    """A malformed line the filter would drop is refused with the message of the call without a filter."""
    tj = tf.write_db(tmp_path / "t.json")
    for bad, what in ((tf.line("x", 1008, aln="4x0"), "numeric"), ("x\tA.1\t1008\t10.0\t400", "columns"), (tf.line("x", 1008, bs="1e12"), "32-bit")):
        src = _table(tmp_path, [tf.line("a", 1000), bad, tf.line("b", 1001)], name="bad.tsv")
        with pytest.raises(N.BluError) as plain:
            pipeline.ingest_columns(src, tj, device=-1)
        with pytest.raises(N.BluError, match=what) as filtered:
            pipeline.ingest_columns(src, tj, device=-1, taxon_filter={"exclude": ["d__Eukaryota"]})
        text = lambda e: str(e.value).split(": ", 1)[1]
        assert text(plain) == text(filtered) and plain.value.code == filtered.value.code
    # column 11 is read only under its own threshold, whatever the taxon verdict
    src = _table(tmp_path, [tf.line("a", 1000), tf.line("e", 1008, ev="n/a")])
    assert pipeline.ingest_columns(src, tj, device=-1, taxon_filter={"exclude": ["d__Eukaryota"]})["n_kept"] == 1
    with pytest.raises(N.BluError, match=r"line 2\b.*numeric"):
        pipeline.ingest_columns(src, tj, device=-1, taxon_filter={"exclude": ["d__Eukaryota"]}, hit_filter={"max_e_value": 1.0})


def test_no_filter_and_an_empty_filter_are_todays_call(tmp_path):
    rng = np.random.default_rng(65)
    src, tj = _table(tmp_path, hf.scramble(tf.make_rows(200, 6, rng), rng)), tf.write_db(tmp_path / "t.json")
    today = pipeline.ingest_columns(src, tj, device=-1)
    assert "n_kept" not in today and "taxon_filter" not in today
    for flt in (None, {}, pipeline.TaxonFilter(), {"exclude": [], "only": None}, {"only": ()}):
        got = pipeline.ingest_columns(src, tj, device=-1, taxon_filter=flt)
        hf.assert_columns_equal(got, today)
        assert "taxon_filter" not in got and "n_kept" not in got
    # the C entry point with two empty lists is the call without it
    import ctypes as C
    L = pipeline._bind()
    c, st = pipeline.IngestColumns(), pipeline.HitSelectionStats()
    empty = pipeline.TaxonFilterC(None, 0, None, 0)
    sel = pipeline.HitSelection(taxon_filter=C.pointer(empty))
    assert L.blu_ingest_columns_selected(src.encode(), tj.encode(), 0, -1, C.byref(sel), C.byref(c), C.byref(st)) == 0
    fst, tst = st.hit_filter, st.taxon_filter
    assert (int(c.n_hits), int(fst.n_lines), int(fst.n_kept)) == (len(today["bitscore"]),) * 3
    assert (int(tst.n_lines), int(tst.n_excluded), int(tst.n_not_only)) == (0, 0, 0)
    L.blu_ingest_columns_free(C.byref(c))


def test_cli_flags(tmp_path):
    ap = cli.build_parser()
    common = ["-t", "t.json", "--taxon", "bacteria", "--strategy", "relaxed"]
    ex_file, on_file = tmp_path / "ex.txt", tmp_path / "on.txt"
    ex_file.write_text("# contaminants\n\n  o__Chloroplast  \ns__uncultured-*\n\n")
    on_file.write_text("d__Bacteria\n#d__Eukaryota\n")
    flags = ["--exclude-taxon", "s__a", "--exclude-taxon", "g__b*", "--only-taxon", "d__Archaea", "--exclude-taxon-file", str(ex_file),
             "--only-taxon-file", str(on_file)]
    for head in (["blastn", "build-consensus", "b.tsv"], ["blastn", "run-with-consensus", "q.fa", "-d", "db", "--blast-out-file", "b.tsv"]):
        a = ap.parse_args(head + common + flags)
        assert cli._taxon_filter(a) == pipeline.TaxonFilter(("s__a", "g__b*", "o__Chloroplast", "s__uncultured-*"), ("d__Archaea", "d__Bacteria"))
        assert cli._taxon_filter(ap.parse_args(head + common)) is None
        assert cli._hit_filter(a) is None
    for sub in ("build-report", "build-tabular"):
        with pytest.raises(SystemExit):
            ap.parse_args(["blastn", sub, "doc.json", "--exclude-taxon", "s__a"])
    with pytest.raises(SystemExit, match="cannot read"):
        cli._taxon_filter(ap.parse_args(["blastn", "build-consensus", "b.tsv"] + common + ["--only-taxon-file", str(tmp_path / "absent")]))
    bc = [a for a in ap._subparsers._group_actions[0].choices["blastn"]._subparsers._group_actions[0].choices["build-consensus"]._actions
          if a.dest in ("exclude_taxon", "only_taxon")]
    assert len(bc) == 2 and all("not in the reference CLI" in a.help for a in bc)


def test_the_lines_on_stderr(capsys):
    stats = {"n_lines": 10, "n_kept": 3, "taxon_filter": {"n_lines": 10, "n_excluded": 5, "n_not_only": 1, "exclude": ["s__a", "g__b*", "o__c"],
                                                           "excluded_by": [4, 0, 1]}}
    cli._say_kept(stats, hit_filter=True)
    assert capsys.readouterr().err == ("taxon filter: excluded 5, not in --only-taxon 1, of 10 lines\n  s__a: 4\n  o__c: 1\n"
                                       "hit filter: kept 3 of 10 lines\n")
    cli._say_kept(stats, hit_filter=False)
    assert "hit filter" not in capsys.readouterr().err
    cli._say_kept({"n_lines": 10, "n_kept": 3})
    assert capsys.readouterr().err == "hit filter: kept 3 of 10 lines\n"
