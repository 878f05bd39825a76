"""One hand-written lineage table per rule of `build-db lineages`, with what the build must give spelled
out by hand: no tests here.  A case is (table, replace, expected); expected is either
  {"units": [(taxid, rank, numericLineage, textLineage, [(accession, oid), ...]), ...], "tsv": bytes, "map": bytes}
or {"error": (1-based line, kind)} with the kinds of tests/lineage_db_reference.py."""

A = ("d__bacteria", "d__bacteria;p__proteobacteria", "d__bacteria;p__proteobacteria;c__gamma")


def ok(units, tsv=b"", tmap=b""):
    return {"units": units, "tsv": tsv, "map": tmap}


def err(line, kind):
    return {"error": (line, kind)}


CASES = {
    # ---- input lines
    "crlf_and_open_last_line": (
        b"a\td__Bacteria\r\nb\td__Bacteria; p__Proteobacteria", None,
        ok([(1, "d", "d__1", A[0], [("a", "0")]), (2, "p", "d__1;p__2", A[1], [("b", "1")])], tmap=b"a 1\nb 2\n")),
    "blank_and_comment_lines_are_skipped": (
        b"\n  \t \r\n# a comment\td__x\n   #another\na\td__Bacteria\n\n", None,
        ok([(1, "d", "d__1", A[0], [("a", "0")])], tmap=b"a 1\n")),
    "header_is_skipped": (
        b"# made by hand\n Feature ID \tTaxon\tConfidence\na\td__Bacteria\n", None,
        ok([(1, "d", "d__1", A[0], [("a", "0")])], tmap=b"a 1\n")),
    "header_only_as_the_first_line": (
        b"a\td__Bacteria\nFeature ID\td__Archaea\n", None,
        ok([(1, "d", "d__1", A[0], [("a", "0")]), (2, "d", "d__2", "d__archaea", [("Feature ID", "1")])],
           tmap=b"a 1\nFeature ID 2\n")),
    "header_must_match_exactly": (
        b"Feature Id\td__Bacteria\n", None, ok([(1, "d", "d__1", A[0], [("Feature Id", "0")])], tmap=b"Feature Id 1\n")),
    "third_column_is_ignored": (
        b"a\td__Bacteria;p__Proteobacteria\t0.99;x__y\tmore\n", None,
        ok([(2, "p", "d__1;p__2", A[1], [("a", "0")])], tmap=b"a 2\n")),
    "id_is_trimmed": (
        b"  a b \t d__Bacteria \n", None, ok([(1, "d", "d__1", A[0], [("a b", "0")])], tmap=b"a b 1\n")),
    "no_tab": (b"a\td__Bacteria\nb d__Bacteria\n", None, err(2, "tab")),
    "empty_id": (b"a\td__Bacteria\n \td__Bacteria\n", None, err(2, "id")),
    "not_utf8": (b"a\td__Bacteria\nb\xff\td__Bacteria\n", None, err(2, "utf8")),
    "not_utf8_in_a_column_nobody_reads": (b"a\td__Bacteria\t\xc3\n", None, err(1, "utf8")),
    "lowest_bad_line_is_named": (b"a\td__Bacteria\nb\tBacteria\nc d\n\xff\tx\n", None, err(2, "level")),
    "oid_counts_data_lines_only": (
        b"Feature ID\tTaxon\n\na\td__Bacteria\n# c\nb\td__\nc\td__Bacteria\n", None,
        ok([(1, "d", "d__1", A[0], [("a", "0"), ("c", "2")])], tsv=b"b\t5\tempty-lineage\n", tmap=b"a 1\nc 1\n")),
    # ---- lineage and levels
    "pieces_are_trimmed_and_empty_ones_skipped": (
        b"a\t ; d__Bacteria ;;  p__Proteobacteria ; \n", None,
        ok([(2, "p", "d__1;p__2", A[1], [("a", "0")])], tmap=b"a 2\n")),
    "blanks_around_the_rank_separator": (
        b"a\td __ Bacteria;P __Proteobacteria\n", None, ok([(2, "p", "d__1;p__2", A[1], [("a", "0")])], tmap=b"a 2\n")),
    "split_at_the_first_double_underscore": (
        b"a\td___Bacteria__x\n", None, ok([(1, "d", "d__1", "d__bacteria-x", [("a", "0")])], tmap=b"a 1\n")),
    "level_without_rank_separator": (b"a\tBacteria;Proteobacteria\n", None, err(1, "level")),
    "single_underscore_is_no_separator": (b"a\td_Bacteria\n", None, err(1, "level")),
    "rank_names_and_letters": (
        b"a\tDomain__A;KINGDOM__B;phylum__C;Class__D;order__E;family__F;genus__G;species__H;undefined__I\n", None,
        ok([(9, "u", "d__1;k__2;p__3;c__4;o__5;f__6;g__7;s__8;u__9", "d__a;k__b;p__c;c__d;o__e;f__f;g__g;s__h;u__i",
             [("a", "0")])], tmap=b"a 9\n")),
    "other_ranks_are_slugs": (
        b"a\td__A;Species Group__B;sub_species__C\n", None,
        ok([(3, "sub-species", "d__1;species-group__2;sub-species__3", "d__a;species-group__b;sub-species__c", [("a", "0")])],
           tmap=b"a 3\n")),
    "empty_rank": (b"a\td__A\nb\td__A;__B\n", None, err(2, "rank")),
    "rank_of_symbols_only": (b"a\t?!__B\n", None, err(1, "rank")),
    "replace_rank_is_exact_on_the_lower_cased_token": (
        b"a\tSK__Bacteria;clade__X;clades__Y\n", [("sk", "Domain"), ("clade", "no rank")],
        ok([(3, "clades", "d__1;no-rank__2;clades__3", "d__bacteria;no-rank__x;clades__y", [("a", "0")])], tmap=b"a 3\n")),
    "replace_rank_last_value_wins": (
        b"a\tx__A\n", [("x", "p"), ("y", "c"), ("x", "f")], ok([(1, "f", "f__1", "f__a", [("a", "0")])], tmap=b"a 1\n")),
    "replace_rank_comes_before_the_letters": (
        b"a\td__A;domain__B\n", [("d", "k")], ok([(2, "d", "k__1;d__2", "k__a;d__b", [("a", "0")])], tmap=b"a 2\n")),
    "replace_rank_to_an_empty_rank": (b"a\td__A\nb\tx__A\n", [("x", "??")], err(2, "rank")),
    "identifier_is_the_slug_of_the_name": (
        b"a\tg__Bacillus_A;s__Bacillus_A sp. 12-X (T)\nb\tg__caf\xc3\xa9 au lait\n", None,
        ok([(2, "s", "g__1;s__2", "g__bacillus-a;s__bacillus-a-sp-12-x-t", [("a", "0")]),
            (3, "g", "g__3", "g__caf-au-lait", [("b", "1")])], tmap=b"a 2\nb 3\n")),
    "greengenes_tail_is_cut": (
        b"a\tk__Bacteria; p__Proteobacteria; c__; o__; f__; g__; s__\n", None,
        ok([(2, "p", "k__1;p__2", "k__bacteria;p__proteobacteria", [("a", "0")])], tmap=b"a 2\n")),
    "levels_behind_an_empty_identifier_are_dropped_unread": (
        b"a\td__Bacteria;p__ ?? ;c__Gamma;no separator here\n", None, ok([(1, "d", "d__1", A[0], [("a", "0")])], tmap=b"a 1\n")),
    "empty_identifier_ends_the_lineage_whatever_its_rank": (
        b"a\td__Bacteria;__;x\n", None, ok([(1, "d", "d__1", A[0], [("a", "0")])], tmap=b"a 1\n")),
    "no_level_survives": (
        b"a\t\nb\td__;p__X\nc\t ; ;\nd\td__Bacteria\n", None,
        ok([(1, "d", "d__1", A[0], [("d", "3")])], tsv=b"a\t1\tempty-lineage\nb\t2\tempty-lineage\nc\t3\tempty-lineage\n",
           tmap=b"d 1\n")),
    # ---- taxa and taxids
    "equal_paths_however_spelled_are_one_taxon": (
        b"a\td__Bacteria;p__Proteobacteria\nb\tD__BACTERIA ; Phylum __ proteobacteria;\nc\tdomain__bacteria!;p__-Proteobacteria-\n", None,
        ok([(2, "p", "d__1;p__2", A[1], [("a", "0"), ("b", "1"), ("c", "2")])], tmap=b"a 2\nb 2\nc 2\n")),
    "same_last_element_under_two_parents": (
        b"a\tf__A;g__Incertae_sedis\nb\tf__B;g__Incertae_sedis\nc\tf__A;g__incertae sedis\n", None,
        ok([(2, "g", "f__1;g__2", "f__a;g__incertae-sedis", [("a", "0"), ("c", "2")]),
            (4, "g", "f__3;g__4", "f__b;g__incertae-sedis", [("b", "1")])], tmap=b"a 2\nb 4\nc 2\n")),
    "same_identifier_at_two_ranks": (
        b"a\tf__X;g__X\nb\tf__X\nc\tg__X\n", None,
        ok([(1, "f", "f__1", "f__x", [("b", "1")]), (2, "g", "f__1;g__2", "f__x;g__x", [("a", "0")]), (3, "g", "g__3", "g__x", [("c", "2")])],
           tmap=b"a 2\nb 1\nc 3\n")),
    "inner_level_first_then_leaf": (
        b"a\td__A;p__B;c__C\nb\td__A;p__B\nc\td__A\n", None,
        ok([(1, "d", "d__1", "d__a", [("c", "2")]), (2, "p", "d__1;p__2", "d__a;p__b", [("b", "1")]),
            (3, "c", "d__1;p__2;c__3", "d__a;p__b;c__c", [("a", "0")])], tmap=b"a 3\nb 2\nc 1\n")),
    "leaf_first_then_inner_level": (
        b"a\td__A\nb\td__A;p__B\nc\td__Z;p__B\nd\td__A;p__B;c__C\n", None,
        ok([(1, "d", "d__1", "d__a", [("a", "0")]), (2, "p", "d__1;p__2", "d__a;p__b", [("b", "1")]),
            (4, "p", "d__3;p__4", "d__z;p__b", [("c", "2")]), (5, "c", "d__1;p__2;c__5", "d__a;p__b;c__c", [("d", "3")])],
           tmap=b"a 1\nb 2\nc 4\nd 5\n")),
    # ---- the document
    "repeated_ids_are_written_twice": (
        b"a\td__A\na\td__A\na\td__B\n", None,
        ok([(1, "d", "d__1", "d__a", [("a", "0"), ("a", "1")]), (2, "d", "d__2", "d__b", [("a", "2")])], tmap=b"a 1\na 1\na 2\n")),
    "ids_are_escaped_in_the_document_only": (
        b'q"\\\x01\x7f\xc3\xa9\td__A\n', None,
        ok([(1, "d", "d__1", "d__a", [('q"\\\x01\x7fé', "0")])], tmap=b'q"\\\x01\x7f\xc3\xa9 1\n')),
    "no_data_lines": (b"# nothing\nFeature ID\tTaxon\n\n", None, ok([])),
    "empty_file": (b"", None, ok([])),
}

# the literal bytes of one small document, head included
LITERAL_TABLE = b"x1\td__Bacteria;p__Firmicutes\nx2\td__Bacteria;p__Firmicutes\n"
LITERAL_DOC = b"""{
  "blutilsVersion": "8.3.1",
  "ignoreTaxids": null,
  "replaceRank": {
    "sk": "d"
  },
  "dropNonLinnaeanTaxonomies": null,
  "sourceDatabase": "silva.tsv",
  "taxonomies": [
    {
      "taxid": 2,
      "rank": "p",
      "numericLineage": "d__1;p__2",
      "textLineage": "d__bacteria;p__firmicutes",
      "accessions": [
        {
          "accession": "x1",
          "oid": "0"
        },
        {
          "accession": "x2",
          "oid": "1"
        }
      ]
    }
  ]
}"""


def depth_table(depth: int) -> bytes:
    """one line of `depth` levels under ranks r0, r1, ..."""
    return b"deep\t" + b";".join(b"r%d__n%d" % (k, k) for k in range(depth)) + b"\n"
