"""Plain-Python restatement of `build-db sintax` and `build-db dada2`: labels from a parsed taxonomies
document, then bytes in and bytes out.  The oracle of tests/test_seqdb_label.py and tests/test_gpu_seqdb_label.py.  Neither
format is in the reference; the line rules are kraken2's and come from tests/seqdb_reference.py."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

from tests import seqdb_reference as R

SINTAX, DADA2 = "sintax", "dada2"
_KINDS = {"d": "d", "domain": "d", "k": "k", "kingdom": "k", "p": "p", "phylum": "p", "c": "c", "class": "c",
          "o": "o", "order": "o", "f": "f", "family": "f", "g": "g", "genus": "g", "s": "s", "species": "s"}
_C_SPACE = " \t\n\v\f\r"
_LOWER = {c: c + 32 for c in range(ord("A"), ord("Z") + 1)}
_UNDERSCORE = {ord(c): "_" for c in ",;:" + _C_SPACE}
_DADA2_LEVELS = "pcofg"


def kind(rank: str) -> Optional[str]:
    """parse_rank (csrc/taxonomy.cpp) as far as the eight kinds go: the rank read as a C string, ASCII letters lowered,
    trimmed of C white space, then a letter or a full name.  `u`, `undefined` and every other word are no kind."""
    return _KINDS.get(rank.split("\0")[0].translate(_LOWER).strip(_C_SPACE))


def label(fmt: str, lineage: str) -> str:
    """The label of one lineage, "" when it has none."""
    first: Dict[str, str] = {}
    order: List[str] = []
    for element in lineage.split(";"):
        parts = element.split("__")
        if len(parts) != 2 or not parts[0] or not parts[1]:      # the taxonomies loader's rule: exactly two parts, here non-empty
            return ""
        k = kind(parts[0])
        if k is not None and k not in first:                     # of two elements of one kind the first counts
            first[k] = parts[1].translate(_UNDERSCORE)
            order.append(k)
    if fmt == SINTAX:
        return ",".join(f"{k}:{first[k]}" for k in order)
    out = []
    for k in ["d" if "d" in first else "k"] + list(_DADA2_LEVELS):
        if k not in first:
            break
        out.append(first[k] + ";")
    return "".join(out)


def _taxid(value) -> int:
    """The loader reads the number as f64 and casts it to i64, saturating."""
    return max(-(1 << 63), min((1 << 63) - 1, int(float(value))))


def rows(fmt: str, document: dict, use_taxid: bool = False) -> List[Tuple[int, bytes]]:
    """(taxid, label) per row of the document's `taxonomies`, in file order"""
    key = "numericLineage" if use_taxid else "textLineage"
    return [(_taxid(u["taxid"]), label(fmt, u[key]).encode("utf-8")) for u in document["taxonomies"]]


def render(fmt: str, document: dict, use_taxid: bool = False) -> bytes:
    """what blu_seqdb_render_labels writes"""
    return b"".join(b"%d\t%s\n" % r for r in rows(fmt, document, use_taxid))


def export(fmt: str, document: dict, listing: bytes, use_taxid: bool = False) -> dict:
    """What one export leaves behind: the dict of seqdb_reference.export ("map" is None and "map_bytes" 0: there is no
    second file; "records" counts the records written and "input_bytes" runs to the first line that was neither written
    nor skipped) plus "n_unknown_taxid" and "n_unlabelled", the lines skipped before that point."""
    table: Dict[int, bytes] = {}
    for taxid, lab in rows(fmt, document, use_taxid):
        table.setdefault(taxid, lab)                               # a taxid listed twice joins its first row
    out, unknown, unlabelled, lines, last = [], 0, 0, 0, 0
    outcome = ("ok",)
    for no, line in R._lines(listing):
        last = no
        try:
            acc, taxid, seq = R._pieces(line, 3, no)
            if not seq.isascii():
                raise R.RefError(no, "nonascii")
            n = R.usize(taxid)
            if n is None:
                raise R.RefError(no, "taxid")
        except R.RefError as e:
            outcome = ("error", no, "pieces" if "Invalid line" in e.why else e.why)
            break
        lines += 1
        lab = table.get(n) if n < 1 << 63 else None                # the join is by value
        if lab is None:
            unknown += 1
        elif not lab:
            unlabelled += 1
        elif fmt == SINTAX:
            out.append(b">" + acc + b";tax=" + lab + b";\n" + seq.upper() + b"\n")
        else:
            out.append(b">" + lab + b"\n" + seq.upper() + b"\n")
    if outcome == ("ok",) and listing and last < R._count_lines(listing):
        outcome = ("stop", last + 1)
    pos = 0
    for _ in range(lines):
        nl = listing.find(b"\n", pos)
        pos = nl + 1 if nl >= 0 else len(listing)
    return {"outcome": outcome, "fna": b"".join(out), "map": None, "records": len(out), "input_bytes": pos, "map_bytes": 0,
            "n_unknown_taxid": unknown, "n_unlabelled": unlabelled}
