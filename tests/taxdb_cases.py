"""Hand-built taxdumps, one per rule of `build-db blu` (DESIGN.md "Taxonomies database builder"), shared by the oracle
tests (tests/test_taxdb.py) and the GPU tests (tests/test_gpu_taxdb.py).  Each case: the files, the options, and what
the document / TSV must say, written out here."""
from __future__ import annotations

import os

# taxid, rank, scientific name; lineage without the root, as NCBI's taxidlineage.dmp
BASE_NODES = [(1, "no rank", "root"), (10, "superkingdom", "Bacteria"), (70, "clade", "Terrabacteria group"),
              (20, "phylum", "Bacillota"), (30, "class", "Bacilli"), (40, "genus", "Bacillus"),
              (50, "species", "Bacillus subtilis"), (60, "strain", "Bacillus subtilis 168")]
BASE_LINEAGE = {1: "", 10: "", 70: "10", 20: "10 70", 30: "10 70 20", 40: "10 70 20 30", 50: "10 70 20 30 40",
                60: "10 70 20 30 40 50"}
FULL50 = "superkingdom__10;clade__70;p__20;c__30;g__40;s__50"
TEXT50 = "superkingdom__bacteria;clade__terrabacteria-group;p__bacillota;c__bacilli;g__bacillus;s__bacillus-subtilis"


def dmp(*fields) -> str:
    return "\t|\t".join(str(f) for f in fields) + "\t|\n"


def write_case(d: str, nodes=None, names=None, lineage=None, merged="", delnodes="", accessions="", raw_names=None) -> dict:
    """Writes the five dumps and accessions.txt under d; names: extra lines appended after the base names."""
    os.makedirs(d, exist_ok=True)
    nodes = nodes if nodes is not None else "".join(dmp(t, 1, r, "", 0) for t, r, _ in BASE_NODES)
    base_names = "".join(dmp(t, n, "", "scientific name") for t, _, n in BASE_NODES)
    lineage = lineage if lineage is not None else "".join(dmp(t, (l + " ") if l else "") for t, l in BASE_LINEAGE.items())
    raw = lambda x: x if isinstance(x, bytes) else x.encode()          # every file may be given as raw bytes
    files = {"nodes.dmp": raw(nodes), "names.dmp": raw_names if raw_names is not None else (base_names + (names or "")).encode(),
             "taxidlineage.dmp": raw(lineage), "merged.dmp": raw(merged), "delnodes.dmp": raw(delnodes),
             "accessions.txt": raw(accessions)}
    for name, data in files.items():
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    return {"dir": d, "accessions": os.path.join(d, "accessions.txt")}


def _base_names_bytes() -> bytes:
    return "".join(dmp(t, n, "", "scientific name") for t, _, n in BASE_NODES).encode()


# name -> (write_case kwargs, options, {taxid: (numericLineage, textLineage)} expected entries, expected TSV)
CASES = {
    "merged_keeps_old_id": (dict(merged=dmp(99, 50), accessions="A  99  1\n"), {},
                            {99: (FULL50[:-2] + "99", TEXT50)}, ""),
    "deleted_before_merged": (dict(merged=dmp(98, 50), delnodes=dmp(98), accessions="A  98  1\n"), {}, {}, "98\tdeleted\n"),
    "merged_missing": (dict(merged=dmp(97, 12345), accessions="A  97  1\n"), {}, {}, "97\tmerged\n"),
    "unknown": (dict(accessions="A  96  1\nB  0  2\n"), {}, {}, "0\tunknown\n96\tunknown\n"),
    "negative_taxid": (dict(accessions="A  -5  1\n"), {}, {}, "18446744073709551611\tunknown\n"),
    "drop_leaf_vs_ancestor": (dict(accessions="A  60  1\nB  50  2\n"), {"drop": True},
                              {50: ("p__20;c__30;g__40;s__50", "p__bacillota;c__bacilli;g__bacillus;s__bacillus-subtilis")}, ""),
    "replace_ancestors_not_leaf": (dict(accessions="A  60  1\n"), {"replace": [("superkingdom", "d"), ("strain", "s")]},
                                   {60: ("d__10;clade__70;p__20;c__30;g__40;s__50;strain__60",
                                         "d__bacteria;clade__terrabacteria-group;p__bacillota;c__bacilli;g__bacillus;"
                                         "s__bacillus-subtilis;strain__bacillus-subtilis-168")}, ""),
    "skip_ancestors_not_leaf": (dict(accessions="A  50  1\n"), {"skip": [70, 50]},
                                {50: ("superkingdom__10;p__20;c__30;g__40;s__50",
                                      "superkingdom__bacteria;p__bacillota;c__bacilli;g__bacillus;s__bacillus-subtilis")}, ""),
    "missing_or_null_name": (dict(raw_names=_base_names_bytes().replace(b"40\t|\tBacillus\t|\t\t|\tscientific name", b"40\t|\tBacillus\t|\t\t|\tsynonym")
                                  .replace(b"30\t|\tBacilli\t|", b"30\t|\tnull\t|"), accessions="A  50  1\n"), {},
                             {50: (FULL50, TEXT50.replace("c__bacilli;g__bacillus", "c__taxid-30;g__taxid-40"))}, ""),
    "quotes_stripped_before_slug": (dict(names=dmp(50, 'Baci"llus "sub"tilis', "", "scientific name"), accessions="A  50  1\n"), {},
                                    {50: (FULL50, TEXT50.replace("s__bacillus-subtilis", "s__bacillus-subtilis"))}, ""),
    "quote_joins_letters": (dict(names=dmp(40, 'Baci"l"lus', "", "scientific name"), accessions="A  40  1\n"), {},
                            {40: ("superkingdom__10;clade__70;p__20;c__30;g__40",
                                  "superkingdom__bacteria;clade__terrabacteria-group;p__bacillota;c__bacilli;g__bacillus")}, ""),
    "empty_lineage_leading_semicolon": (dict(accessions="A  10  1\n"), {}, {10: (";superkingdom__10", ";superkingdom__bacteria")}, ""),
    "unmapped_ancestor": (dict(lineage="".join(dmp(t, (l + " ") if l else "") for t, l in BASE_LINEAGE.items() if t != 50)
                               + dmp(50, "10 555 70 20 30 40 "), accessions="A  50  1\n"), {}, {50: (FULL50, TEXT50)}, ""),
    "invalid_utf8_line_skipped": (dict(raw_names=_base_names_bytes() + b"20\t|\tBad\xff\xfe\t|\t\t|\tscientific name\t|\n",
                                       accessions="A  30  1\n"), {},
                                  {30: ("superkingdom__10;clade__70;p__20;c__30",
                                        "superkingdom__bacteria;clade__terrabacteria-group;p__bacillota;c__bacilli")}, ""),
    "last_duplicate_wins": (dict(names=dmp(20, "Firmicutes", "", "scientific name"),
                                 nodes="".join(dmp(t, 1, r, "", 0) for t, r, _ in BASE_NODES) + dmp(20, 1, "Class", "", 0),
                                 accessions="A  30  1\n"), {},
                            {30: ("superkingdom__10;clade__70;c__20;c__30",
                                  "superkingdom__bacteria;clade__terrabacteria-group;c__firmicutes;c__bacilli")}, ""),
    "accessions_keep_input_order": (dict(accessions="Z  50  9\nA  40  1\nM  50  3\n"), {},
                                    {50: (FULL50, TEXT50), 40: (FULL50.rsplit(";", 1)[0], TEXT50.rsplit(";", 1)[0])}, ""),
    "escapes_and_extra_pieces": (dict(accessions='A"\\\x01  50  7  extra\nB\t  50 \n'.replace("B\t  50 \n", "B\t  50  \n")), {},
                                 {50: (FULL50, TEXT50)}, ""),
}
