"""Byte-level edge inputs of `build-db blu` (DESIGN.md §10.1 "byte handling"): no tests here, only the generator and the case
tables that tests/test_taxdb_edges.py (oracle, no GPU) and tests/test_gpu_taxdb_edges.py (csrc/taxdb_gpu.hip) share.

Accepted inputs are seeded *respellings* of a well-formed `synth_taxdump.make_taxdump` case: every class below is a named
function that rewrites the lines of a `Doc` with spellings the reference reads the same way (a "preserving" case: the
document, the TSV and the stats must equal the base case's) or in a way the oracle follows (the case names what changes).
`FIRED[class]` counts how often a class applied one of its spellings.  Refused inputs are tables of hand-built dumps with one
bad line each (`REFUSED`) or two with a defined winner (`PRECEDENCE`).  The generator writes its own bytes throughout."""
from __future__ import annotations

import collections
import functools
import os
import tempfile
from typing import Callable, Dict, List, Tuple

import numpy as np

from blutils_amd import synth_taxdump
from tests import taxdb_cases as tc

ACC = "accessions.txt"
DUMP_FILES = ("nodes.dmp", "taxidlineage.dmp", "names.dmp", "merged.dmp", "delnodes.dmp")     # the order they are loaded in
FILES = DUMP_FILES + (ACC,)
NCOLS = {"nodes.dmp": 3, "names.dmp": 4, "taxidlineage.dmp": 2, "merged.dmp": 2, "delnodes.dmp": 1}
BLANKS = b" \t\v\f\r"                      # what str::trim removes in the ASCII range (a line holds no \n)
FIRED: collections.Counter = collections.Counter()

# valid text at the edges of the 2/3/4-byte forms, and the ill-formed sequences str::from_utf8 refuses
VALID_UTF8 = [chr(c).encode("utf-8", "surrogatepass") for c in
              (0xE9, 0x7FF, 0x800, 0x4E2D, 0xD7FF, 0xE000, 0xFFFF, 0x10000, 0x1F600, 0x10FFFF)]
INVALID_UTF8 = {"overlong2": b"\xc0\x80", "overlong2_c1": b"\xc1\xbf", "overlong3": b"\xe0\x80\x80", "surrogate": b"\xed\xa0\x80",
                "above_10ffff": b"\xf4\x90\x80\x80", "five_byte_lead": b"\xf8\x88\x80\x80\x80", "lone_continuation": b"\x80",
                "cut_by_ascii": b"\xe2\x82", "lead_ends_line": None, "lead_ends_file": None}


@functools.lru_cache(maxsize=4)
def base_files(seed: int, big: bool = False) -> Dict[str, bytes]:
    """A well-formed dump in exact NCBI syntax with every oddity of make_taxdump: 1000 nodes, depth 14, 1500 accession lines
    (big: 2200 nodes and 3000 lines, for the cases that need 2048 ranks)."""
    with tempfile.TemporaryDirectory() as d:
        synth_taxdump.make_taxdump(d, n_nodes=2200 if big else 1000, depth=14, n_accessions=3000 if big else 1500, seed=901 + seed,
                                   oddities=True)
        return {n: open(os.path.join(d, n), "rb").read() for n in FILES}


class Doc:
    """The six files as editable lines.  A dump line is [fields, separator, tail, end]; a listing line [pieces, separator, end]."""

    def __init__(self, files: Dict[str, bytes]):
        self.d = {n: [[l.split(b"\t|\t"), b"\t|\t", b"\t|", b"\n"] for l in files[n].split(b"\t|\n")[:-1]] for n in DUMP_FILES}
        self.acc = [[l.split(b"  "), b"  ", b"\n"] for l in files[ACC].split(b"\n")[:-1]]
        self.rows = {n: collections.defaultdict(list) for n in DUMP_FILES}           # taxid -> its lines, in file order
        for n in DUMP_FILES:
            for i, l in enumerate(self.d[n]):
                self.rows[n][int(l[0][0])].append(i)
        self.max_id = max([t for n in DUMP_FILES for t in self.rows[n]] + [int(l[0][1]) for l in self.d["merged.dmp"]] + [0])
        named = [int(l[0][1]) for l in self.acc]
        ok = set(self.rows["nodes.dmp"]) & set(self.rows["taxidlineage.dmp"])
        self.emitted = sorted(set(t for t in named if t in ok))                        # taxids with an entry in the document
        self.raw: Dict[str, bytes] = {}                                                   # files replaced wholesale

    def render(self, name: str) -> bytes:
        if name in self.raw:
            return self.raw[name]
        if name == ACC:
            return b"".join(sep.join(p) + end for p, sep, end in self.acc)
        return b"".join(sep.join(f) + tail + end for f, sep, tail, end in self.d[name])

    def files(self) -> Dict[str, bytes]:
        return {n: self.render(n) for n in FILES}

    def sci_name_line(self, t: int):
        """The winning names.dmp line of t (its last scientific name), or None."""
        rows = [i for i in self.rows["names.dmp"].get(t, []) if self.d["names.dmp"][i][0][3] == b"scientific name"]
        return self.d["names.dmp"][rows[-1]] if rows else None

    def plain_named(self, rng, k: int) -> List[int]:
        """k emitted taxids whose winning name is ordinary text (letters and spaces), so that losing or changing it shows."""
        pool = [t for t in self.emitted if (l := self.sci_name_line(t)) is not None and l[0][1].replace(b" ", b"").isalpha()]
        return [pool[int(i)] for i in rng.choice(len(pool), size=k, replace=False)]


def _run(rng, lo=1, hi=4) -> bytes:
    return bytes(BLANKS[int(i)] for i in rng.integers(0, len(BLANKS), int(rng.integers(lo, hi + 1))))


def _run_no_sep(rng) -> bytes:
    """Blanks for a listing piece: a space only between two other blanks, so that no new two-space separator appears."""
    r = bytes(b"\t\v\f\r"[int(i)] for i in rng.integers(0, 4, int(rng.integers(1, 4))))
    return r + (b" " + r[:1] if rng.random() < 0.5 else b"")


def _ascii_gap(rng, f: bytes):
    """A position inside f between two ASCII bytes (None when there is none): a tab put there splits no UTF-8 sequence."""
    pos = [p for p in range(1, len(f)) if f[p - 1] < 0x80 and f[p] < 0x80]
    return pos[int(rng.integers(0, len(pos)))] if pos else None


def _spell_number(rng, v: bytes, tabs: bool) -> bytes:
    """+N, leading zeros up to 30 digits, tabs between digits (dump ids only): the same number to the reference."""
    neg = v.startswith(b"-")
    digits = v.lstrip(b"+-")
    k = int(rng.integers(0, 5))
    if k == 1 or k == 4:
        digits = digits.rjust(int(rng.integers(len(digits), 31)), b"0")
    sign = b"-" if neg else (b"+" if k in (2, 4) else b"")
    out = sign + digits
    if tabs and k in (3, 4) and len(out) > 1:
        p = int(rng.integers(1, len(out)))
        out = out[:p] + b"\t" + out[p:]
    return out


# ---- the classes: fn(doc, rng, variant) -> {"preserving": bool, "changed": [taxids], "stat": {...}} ------------------------

def line_ends(doc, rng, v):
    """0 CRLF, 1 mixed LF / CRLF in one file, 2 mixed and no final newline (all six files), 3 merged and delnodes of 0 bytes,
    4 a listing of 0 bytes."""
    if v >= 3:
        for n in (("merged.dmp", "delnodes.dmp") if v == 3 else (ACC,)):
            doc.raw[n] = b""
            FIRED["line_ends"] += 1
        return {"preserving": False, "changed": "tsv" if v == 3 else "doc"}
    for n in FILES:
        lines = doc.acc if n == ACC else doc.d[n]
        for l in lines:
            l[-1] = b"\r\n" if v == 0 or rng.random() < 0.5 else b"\n"
            FIRED["line_ends"] += 1
        if v == 2 and lines:
            lines[-1][-1] = b""
    return {"preserving": True}


def bars(doc, rng, v):
    """No trailing bar, bars without tabs, exactly ncols pieces, columns and bars beyond the last one read."""
    for n in DUMP_FILES:
        for l in doc.d[n]:
            k = int(rng.integers(0, 6))
            if k == 1:
                l[2] = b""
            elif k == 2:
                l[1], l[2] = b"|", (b"|" if rng.random() < 0.5 else b"")
            elif k == 3:
                l[0], l[2] = l[0][:NCOLS[n]], b""
            elif k == 4:
                l[0] = l[0][:NCOLS[n]] + [b"", b"q|r|", b"|\t||"]
            elif k == 5:
                l[0], l[1], l[2] = l[0][:NCOLS[n]], b"|", b"|||x"
            FIRED["bars"] += k > 0
    return {"preserving": True}


def field_blanks(doc, rng, v):
    """Runs of ' \\t\\v\\f\\r' around every field the loader trims; a tab inside the name, the rank and the name class."""
    for n in DUMP_FILES:
        for l in doc.d[n]:
            f = l[0]
            for k in range(NCOLS[n]):
                if n in ("nodes.dmp", "names.dmp") and k >= 1 and rng.random() < 0.3 and (p := _ascii_gap(rng, f[k])) is not None:
                    f[k] = f[k][:p] + b"\t" + f[k][p:]                      # removed by the loader: Bac\tillus, sci\tentific name
                f[k] = (_run(rng) if rng.random() < 0.6 else b"") + f[k] + (_run(rng) if rng.random() < 0.6 else b"")
                FIRED["field_blanks"] += 1
    for l in doc.acc:
        for k in (0, 2):
            l[0][k] = (_run_no_sep(rng) if rng.random() < 0.5 else b"") + l[0][k] + (_run_no_sep(rng) if rng.random() < 0.5 else b"")
    return {"preserving": True}


def dump_numbers(doc, rng, v):
    """Every dump id as +N, with leading zeros (up to 30 digits) and tabs between digits; merged in both columns.  Variant 2
    adds taxid 0, spelled -0 / 000 / +0, with an accession line that names it."""
    for n in DUMP_FILES:
        for l in doc.d[n]:
            for k in ((0, 1) if n == "merged.dmp" else (0,)):
                l[0][k] = _spell_number(rng, l[0][k], tabs=True)
                FIRED["dump_numbers"] += 1
    if v < 2:
        return {"preserving": True}
    anc = doc.d["taxidlineage.dmp"][doc.rows["taxidlineage.dmp"][doc.emitted[-1]][0]][0][1]
    doc.d["nodes.dmp"].append([[b"-0", b"1", b"species"], b"\t|\t", b"\t|", b"\n"])
    doc.d["taxidlineage.dmp"].append([[b"000", anc], b"\t|\t", b"\t|", b"\n"])
    doc.d["names.dmp"].append([[b"+0", b"Zero taxon", b"", b"scientific name"], b"\t|\t", b"\t|", b"\n"])
    doc.d["merged.dmp"].append([[b"+0\t0", b"0"], b"\t|\t", b"\t|", b"\n"])
    doc.acc.append([[b"ZERO.1", b"0", b"77"], b"  ", b"\n"])
    return {"preserving": False, "changed": [0]}


def acc_taxid_spelling(doc, rng, v):
    """Listing taxids as +N, -0, with leading zeros and blanks of every kind around; no tab inside (that is an error)."""
    for l in doc.acc:
        t = l[0][1]
        t = b"-0" if t == b"0" and rng.random() < 0.5 else _spell_number(rng, t, tabs=False)
        l[0][1] = (_run_no_sep(rng) if rng.random() < 0.5 else b"") + t + (_run_no_sep(rng) if rng.random() < 0.5 else b"")
        FIRED["acc_taxid_spelling"] += 1
    return {"preserving": True}


def acc_taxid_limits(doc, rng, v):
    """Lines whose taxid sits at the i64 limits, around 2^31, and between the largest dump id and 2^31."""
    m = doc.max_id
    vals = [-(1 << 63), (1 << 63) - 1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 1, 1 << 32, m, m + 1, m + 2, -1]
    vals += [int(x) for x in rng.integers(m + 1, 1 << 31, 20)]
    for k, x in enumerate(vals):
        doc.acc.insert(int(rng.integers(0, len(doc.acc) + 1)), [[b"LIM%d.1" % k, b"%d" % x, b"%d" % k], b"  ", b"\n"])
        FIRED["acc_taxid_limits"] += 1
    return {"preserving": False, "changed": "tsv"}


def acc_pieces(doc, rng, v):
    """0: more than three pieces, three spaces in a row (the split is leftmost and non-overlapping).  1: an empty accession,
    an empty oid (three ways), pieces of 1 to 70 000 bytes."""
    if v == 0:
        for l in doc.acc:
            k = int(rng.integers(0, 5))
            if k == 1:
                l[0] = l[0] + [b"extra"]
            elif k == 2:
                l[0] = l[0] + [b"", b"more", b" x "]
            elif k == 3:
                l[0][1] = b" " + l[0][1]            # "A   5": the piece starts with the third space
            elif k == 4:
                l[0][2] = b" " + l[0][2]
            FIRED["acc_pieces"] += k > 0
        return {"preserving": True}
    t = doc.emitted[len(doc.emitted) // 2]
    tb = b"%d" % t
    extra = [[b"", tb, b"7"], [b"A", tb, b""], [b"B", tb, b"", b"9"], [b"C", tb, b" "], [b"", tb, b""], [b"x", tb, b"y"]]
    extra += [[b"L" * n, tb, b"%d" % n] for n in (15, 16, 17, 255, 256, 257, 4096, 70000)]
    extra += [[b"OID", tb, b"7" * 70000, b"z"]]
    for p in extra:
        doc.acc.insert(int(rng.integers(0, len(doc.acc) + 1)), [p, b"  ", b"\n"])
        FIRED["acc_pieces"] += 1
    return {"preserving": False, "changed": [t]}


def escapes(doc, rng, v):
    """Every byte 0x00..0x7f but \\n inside an accession and an oid, singly and in runs of three, and valid 2/3/4-byte text."""
    t = b"%d" % doc.emitted[0]
    for c in range(0x80):
        if c == 0x0A:
            continue
        b1 = bytes([c])
        doc.acc.append([[b"a" + b1 + b"z", t, b"o" + (b1 if c == 0x20 else b1 * 3) + b"z"], b"  ", b"\n"])
        FIRED["escapes"] += 1
    for u in VALID_UTF8:
        doc.acc.append([[u + b"a" + u * 2, t, b"\x1f" + u + b"\x00"], b"  ", b"\n"])
    doc.acc.append([[b"LAST.1", b"%d" % doc.emitted[-1], b"1"], b"  ", b"\n"])      # the last row of the document is plain
    return {"preserving": False, "changed": [doc.emitted[0]]}


def _bad_line(kind: str, body: bytes) -> bytes:
    """The text of a line that is not UTF-8: the sequence inside the body, or a lead byte as its last byte (the caller ends
    the line there, or the file for lead_ends_file)."""
    if INVALID_UTF8[kind] is None:
        return body + (b"\xe2" if kind == "lead_ends_line" else b"\xc3")
    return body[:1] + INVALID_UTF8[kind] + body[1:]


def utf8_dump(doc, rng, v):
    """Valid 2/3/4-byte text in names and ranks (kept); lines that are not UTF-8 vanish: a node, a lineage line, and the
    winning scientific name of a taxid (an earlier duplicate, or taxid-<id>, takes its place)."""
    kinds = list(INVALID_UTF8)
    vict = doc.plain_named(rng, 16)
    for j, t in enumerate(vict[:10]):                                    # valid text: the name, and every other one the rank too
        l = doc.sci_name_line(t)
        l[0][1] = l[0][1][:2] + VALID_UTF8[j] + l[0][1][2:] + VALID_UTF8[(j + v) % 10]
        if j % 2:
            r = doc.d["nodes.dmp"][doc.rows["nodes.dmp"][t][-1]][0]
            r[2] = r[2][:1] + VALID_UTF8[(j + 3) % 10] + r[2][1:]
    todo = []
    for j, t in enumerate(vict[10:16]):                                  # (the lines first: moving one shifts the row numbers)
        n = ("nodes.dmp", "taxidlineage.dmp", "names.dmp")[j % 3]
        todo.append((n, kinds[(6 * v + j) % len(kinds)], doc.sci_name_line(t) if n == "names.dmp" else doc.d[n][doc.rows[n][t][-1]]))
    for n, kind, line in todo:
        if kind == "lead_ends_file":
            doc.d[n] = [l for l in doc.d[n] if l is not line] + [line]
        body = line[1].join(line[0]) + line[2]
        line[0], line[2], line[3] = [_bad_line(kind, body)], b"", (b"" if kind == "lead_ends_file" else line[3])
        FIRED["utf8_dump"] += 1
        FIRED["utf8_dump:" + kind] += 1
    return {"preserving": False, "changed": vict}


def utf8_listing(doc, rng, v):
    """Valid multi-byte accessions are kept; the listing is read up to the first line that is not UTF-8: the valid lines and
    the malformed line after it are never seen."""
    kind = list(INVALID_UTF8)[v % len(INVALID_UTF8)]
    for j, l in enumerate(doc.acc[:40]):
        l[0][0] = VALID_UTF8[j % 10] + l[0][0] + VALID_UTF8[(j + 1) % 10]
        l[0][2] = l[0][2] + VALID_UTF8[(j + 2) % 10] * 2
    k = int(rng.integers(len(doc.acc) // 3, 2 * len(doc.acc) // 3)) if v < len(INVALID_UTF8) else 0     # (the last: nothing is read)
    t = b"%d" % doc.emitted[-1]
    if kind == "lead_ends_file":
        doc.acc[k:] = [[[_bad_line(kind, b"BAD.1  " + t + b"  1")], b"  ", b""]]
    else:
        doc.acc[k:k] = [[[_bad_line(kind, b"BAD.1  " + t + b"  1")], b"  ", b"\n"], [[b"B 2 3"], b"  ", b"\n"],
                        [[b"C", b"1\t2", b"3"], b"  ", b"\n"]]
    FIRED["utf8_listing"] += 1
    FIRED["utf8_listing:" + kind] += 1
    return {"preserving": False, "changed": "doc", "stat": {"accession_lines": k}}


def lineage_tokens(doc, rng, v):
    """Ancestors as +N, zero-padded (30 digits too), wrapped in \\v .. \\f, with quotes and tabs inside; null, "null", nu"ll,
    nu\\tll, empty tokens (runs of spaces) and tokens of quotes only between them: all skipped."""
    fillers = [b"null", b'"null"', b'nu"ll', b"nu\tll", b"", b'""', b"\t", b'"\t"', b'n"u"l"l']
    for l in doc.d["taxidlineage.dmp"]:
        out = []
        for tok in l[0][1].split(b" "):
            if tok:
                k = int(rng.integers(0, 7))
                if k == 1:
                    tok = b"+" + tok
                elif k == 2:
                    tok = tok.rjust(30 if rng.random() < 0.3 else len(tok) + 3, b"0")
                elif k == 3:
                    tok = _run(rng).replace(b" ", b"\v") + b"+" + tok + _run(rng).replace(b" ", b"\f")
                elif k == 4:
                    p = int(rng.integers(0, len(tok) + 1))
                    tok = tok[:p] + (b'"', b"\t", b'"\t"')[int(rng.integers(0, 3))] + tok[p:]
                elif k == 5:
                    tok = b"\r" + tok
                FIRED["lineage_tokens"] += k > 0
            while rng.random() < 0.25:
                out.append(fillers[int(rng.integers(0, len(fillers)))])
            out.append(tok)
        l[0][1] = b" ".join(out)
    return {"preserving": True}


NAME_EDGES = [b"null", b'"null"', b"nu\tll", b'n"ul"l', b"NULL", b"Null", b"nulll", b"nul", b"", b'""', b'"\t"', b"--- ... !!!",
              b"x", b"7", b"Ab c" * 4, b"Ab c" * 4 + b"d", b"abcdefghijklmnop", b"Xy-" * 1666 + b"Zq", b"a\xc2\xa0b", b"x\xe3\x80\x80y z",
              b"A" * 5000, b"!" * 4999 + b"k", b"a\x00b", b"\x00"]


NOT_SCIENTIFIC = [b"Scientific name", b"scientific  name", b'"scientific name"', b"scientific name x", b"scientific nam", b"",
                  b"scientific_name", b"scientific namescientific name", b"cientific name", b"scientific\vname"]


def names(doc, rng, v):
    """The winning name of emitted taxids set to the null spellings, their near misses, empty and symbol-only names (empty
    slug), and names of 1 to 5000 bytes; non-ASCII white space inside a name is kept (it separates slug words); name classes
    that are almost `scientific name`."""
    vict = doc.plain_named(rng, len(NAME_EDGES) + len(NOT_SCIENTIFIC))
    for t, nm in zip(vict, NAME_EDGES):
        doc.sci_name_line(t)[0][1] = nm
        FIRED["names"] += 1
    for t, cls in zip(vict[len(NAME_EDGES):], NOT_SCIENTIFIC):          # the line is no scientific name: the name is lost
        doc.sci_name_line(t)[0][3] = cls
        FIRED["names"] += 1
    return {"preserving": False, "changed": vict}


def ranks(doc, rng, v):
    """0: case, quote and tab variants of each rank (one rank).  1: different ranks with one token.  2-5: 1, 50, 2047 and 2048
    distinct ranks among the nodes that exist (50: one of 0 bytes and one of 300 among them).  6: ranks that are a letter rank
    only once quotes and blanks are gone, and ranks with control bytes (NUL too) and \\v, \\f inside."""
    nodes_l = doc.d["nodes.dmp"]
    if v == 0:
        for l in nodes_l:
            r = bytearray(l[0][2])
            for p in range(len(r)):
                if rng.random() < 0.3:
                    r[p:p + 1] = bytes(r[p:p + 1]).swapcase()
            r = bytes(r)
            for ins in (b'"', b"\t"):
                if rng.random() < 0.4:
                    p = int(rng.integers(0, len(r) + 1))
                    r = r[:p] + ins + r[p:]
            l[0][2] = r
            FIRED["ranks"] += 1
        return {"preserving": True}
    if v == 1:
        same = {b"species group": [b"species  group", b"species-group", b"Species_Group", b"species.group", b"-species group-"],
                b"no rank": [b"no rank"]}
        for l in nodes_l:
            if l[0][2] in same:
                alts = same[l[0][2]]
                l[0][2] = alts[int(rng.integers(0, len(alts)))]
                FIRED["ranks"] += 1
        return {"preserving": True}
    if v == 6:
        odd = [b'" class "', b'"\tSpecies\v"', b"cl\x00ass", b"\x00", b"sub\vclass", b"\x01", b"ord\x7fer", b"a\x1fb", b"genus\x00", b"g\fenus"]
        for k, l in enumerate(nodes_l):
            l[0][2] = odd[k % len(odd)]
            FIRED["ranks"] += 1
        return {"preserving": False, "changed": "doc"}
    n = {2: 1, 3: 50, 4: 2047, 5: 2048}[v]
    exist = set(doc.rows["taxidlineage.dmp"])
    k = 0
    for l in nodes_l:
        t = int(l[0][0])
        j = 0
        if t in exist:
            j, k = k % n, k + 1
        l[0][2] = b"" if (n == 50 and j == 7) else (b"Long rank " + b"w" * 290) if (n == 50 and j == 8) else b'Ra"nk %d' % j if j % 3 else b"rank\t%d" % j
        FIRED["ranks"] += 1
    assert k >= n
    return {"preserving": False, "changed": "doc", "n_ranks": n}


def alignment(doc, rng, v):
    """The first 256 line pairs of nodes, names, taxidlineage and the listing: line k + 1 starts at offset k % 16 modulo 16
    (the line before it is padded with a column nobody reads) and its field read (rank, name, lineage, oid) ends at offset
    k // 16 (blanks before or after the field).  The last line of each file ends the file on the last byte of its field."""
    seen = set()
    for n, col in (("nodes.dmp", 2), ("names.dmp", 1), ("taxidlineage.dmp", 1), (ACC, 2)):
        lines = doc.acc if n == ACC else doc.d[n]
        size = lambda l: len(l[1].join(l[0])) + sum(len(x) for x in l[2:])
        pos = size(lines[0])
        for k in range(min(256, len(lines) - 2)):
            prev, l = lines[k], lines[k + 1]
            want = (k % 16 - pos - 2) % 16
            if n == ACC:
                prev[0] = prev[0] + [b"x" * want]
            else:
                prev[2] = prev[2] + b"\t|" + b"x" * want
            pos += 2 + want
            end = pos + len(l[1].join(l[0][:col + 1]))
            pad = bytes(b"\v\f\r"[i % 3] for i in range((k // 16 - end) % 16))
            l[0][col] = (pad + l[0][col]) if k % 2 else (l[0][col] + pad)
            seen.add((n, pos % 16, (end + len(pad)) % 16))
            pos += size(l)
        last = lines[-1]
        last[0] = last[0][:3 if n == ACC else NCOLS[n]]
        last[-1] = b""
        if n != ACC:
            last[2] = b""
    FIRED["alignment"] += len(seen)
    assert len(seen) == 4 * 256, len(seen)
    return {"preserving": True}


ACCEPTED: Dict[str, Tuple[Callable, int]] = {     # class -> (function, variants / seeds used)
    "line_ends": (line_ends, 5), "bars": (bars, 2), "field_blanks": (field_blanks, 2), "dump_numbers": (dump_numbers, 3),
    "acc_taxid_spelling": (acc_taxid_spelling, 2), "acc_taxid_limits": (acc_taxid_limits, 1), "acc_pieces": (acc_pieces, 2),
    "escapes": (escapes, 1), "utf8_dump": (utf8_dump, 3), "utf8_listing": (utf8_listing, len(INVALID_UTF8) + 1),
    "lineage_tokens": (lineage_tokens, 2), "names": (names, 1), "ranks": (ranks, 7), "alignment": (alignment, 2)}
ACCEPTED_IDS = [(c, s) for c, (_, n) in ACCEPTED.items() for s in range(n)]


@functools.lru_cache(maxsize=None)
def accepted(cls: str, seed: int) -> dict:
    """{"files", "base" (the well-formed files it respells), "big", "preserving", "changed", "stat"} of one respelled case."""
    base = base_files(seed % 2, big=(cls == "ranks" and seed >= 4))
    doc = Doc(base)
    info = ACCEPTED[cls][0](doc, np.random.default_rng([seed, sum(cls.encode())]), seed)
    return {"files": doc.files(), "base": base, "big": cls == "ranks" and seed >= 4, "changed": None, "stat": {}, **info}


# ---- counts: hand-sized dumps around the block sizes of the kernels (256 threads, scan and sort tiles of 4096) ----------------
RANK_CYCLE = [b"no rank", b"superkingdom", b"phylum", b"class", b"order", b"family", b"genus", b"species", b"strain", b"clade"]


def sized_files(n: int, n_acc: int, one_taxid: bool = False, top: int = 0) -> Dict[str, bytes]:
    """n lines in each dump: nodes 1..n (parent k // 2), old ids n+1..2n merged into them, 2n+1..3n deleted; n_acc listing
    lines over all of those and some unknown ids (or all naming one taxid).  top > 3n: one more node with that id, named by
    the listing together with top - 1, top + 1 and ids far beyond."""
    def chain(k):
        out = []
        while k > 1:
            k //= 2
            out.append(k)
        return b"".join(b"%d " % a for a in reversed(out[:-1]))            # the root is not listed
    ids = list(range(1, n + 1))
    f = {"nodes.dmp": b"".join(tc.dmp(k, max(k // 2, 1), RANK_CYCLE[k.bit_length() % 10].decode(), "", 0).encode() for k in ids),
         "taxidlineage.dmp": b"".join(b"%d\t|\t%s\t|\n" % (k, chain(k)) for k in ids),
         "names.dmp": b"".join(b"%d\t|\tTaxon %d\t|\t\t|\tscientific name\t|\n" % (k, k) for k in ids),
         "merged.dmp": b"".join(b"%d\t|\t%d\t|\n" % (n + k, k) for k in ids),
         "delnodes.dmp": b"".join(b"%d\t|\n" % (2 * n + k) for k in ids)}
    span = 3 * n + 5
    tax = [n // 2 + 1] * n_acc if one_taxid else [(k * 7) % span for k in range(n_acc)]
    if top:
        assert top > 3 * n
        f["nodes.dmp"] += tc.dmp(top, 1, "species", "", 0).encode()
        f["taxidlineage.dmp"] += b"%d\t|\t2 4 \t|\n" % top
        f["names.dmp"] += b"%d\t|\tTop taxon\t|\t\t|\tscientific name\t|\n" % top
        tax = [top + 1, top, 1 << 40, top - 1] + tax + [top, top + 1, (1 << 31) + top, -1, top + 2]
    f[ACC] = b"".join(b"ACC%d.1  %d  %d\n" % (k, t, k) for k, t in enumerate(tax))
    return f


SIZES = [0, 1, 255, 256, 257, 4095, 4096, 4097, 8193]
TOPS = [255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24]
COUNTS = ([("lines_%d" % n, dict(n=n, n_acc=n)) for n in SIZES]
          + [("one_taxid_%d" % n, dict(n=max(n // 8, 1), n_acc=n, one_taxid=True)) for n in (1, 257, 4097, 8193)]
          + [("listing_%d_dump_0" % n, dict(n=0, n_acc=n)) for n in (1, 4097)]
          + [("dump_%d_listing_0" % n, dict(n=n, n_acc=0)) for n in (1, 4097)]
          + [("max_id_%d" % t, dict(n=60, n_acc=300, top=t)) for t in TOPS])


# ---- refused inputs -------------------------------------------------------------------------------------------------------
def _dumps() -> Dict[str, List[bytes]]:
    """The well-formed eight-node case of taxdb_cases as lines, plus one merged and one deleted id."""
    return {"nodes.dmp": [tc.dmp(t, 1, r, "", 0).encode() for t, r, _ in tc.BASE_NODES],
            "taxidlineage.dmp": [tc.dmp(t, (l + " ") if l else "").encode() for t, l in tc.BASE_LINEAGE.items()],
            "names.dmp": [tc.dmp(t, n, "", "scientific name").encode() for t, _, n in tc.BASE_NODES],
            "merged.dmp": [tc.dmp(99, 50).encode(), tc.dmp(97, 40).encode()],
            "delnodes.dmp": [tc.dmp(98).encode(), tc.dmp(96).encode()],
            ACC: [b"A  50  1\n", b"B  99  2\n", b"C  98  3\n", b"D  40  4\n"]}


def _with(*edits) -> Dict[str, bytes]:
    """edits: (file, 0-based line, replacement line)."""
    d = _dumps()
    for name, k, line in edits:
        d[name][k] = line
    return {n: b"".join(v) for n, v in d.items()}


BAD_IDS = {"plus": b"+", "minus": b"-", "empty": b"", "two_numbers": b"1 2", "hex": b"0x10", "decimal_point": b"1.0",
           "arabic_indic_digit": "١".encode(), "negative": b"-1", "2^31": b"2147483648", "2^63": b"9223372036854775808",
           "forty_digits": b"1" * 40, "nul_byte_inside": b"1\x002", "vt_inside": b"1\v2"}
REST = {"nodes.dmp": b"\t|\t1\t|\tspecies\t|\n", "taxidlineage.dmp": b"\t|\t10 \t|\n", "names.dmp": b"\t|\tX\t|\t\t|\tscientific name\t|\n",
        "merged.dmp": b"\t|\t50\t|\n", "delnodes.dmp": b"\t|\n"}
BAD_ANCESTORS = {"Null": b"Null", "x7": b"x7", "trailing_minus": b"5-", "plus": b"+", "plus_space": b"+ 5", "2^31": b"2147483648",
                 "2^64": b"18446744073709551616", "25_digits": b"1" * 25, "nul": b"nul", "nulll": b"nulll", "minus_5": b"-5",
                 "vt_inside": b"2\v0", "nul_byte_inside": b"2\x000", "nul_byte": b"\x00"}

# name -> (files, file that is named, 1-based line)
REFUSED: Dict[str, Tuple[Dict[str, bytes], str, int]] = {}
for _n, _few in (("nodes.dmp", b"60\t|\t1\n"), ("names.dmp", b"60\t|\tX\t|\t\n"), ("taxidlineage.dmp", b"60 10 \n"), ("merged.dmp", b"99 50\n")):
    REFUSED["too_few_pieces-" + _n] = (_with((_n, 1, _few)), _n, 2)
for _n in DUMP_FILES:
    REFUSED["empty_line-" + _n] = (_with((_n, 1, b"\n")), _n, 2)
    for _k, _v in BAD_IDS.items():
        REFUSED["id_%s-%s" % (_k, _n)] = (_with((_n, 1, _v + REST[_n])), _n, 2)
for _k, _v in BAD_IDS.items():
    REFUSED["merged_new_id_%s" % _k] = (_with(("merged.dmp", 0, b"99\t|\t" + _v + b"\t|\n")), "merged.dmp", 1)
for _k, _v in {"two_pieces": b"A  50\n", "single_spaces": b"A 50 1\n", "empty_line": b"\n", "taxid_with_tab": b"A  1\t2  3\n",
               "taxid_2^63": b"A  9223372036854775808  3\n", "taxid_two_signs": b"A  --1  3\n", "taxid_empty": b"A    3\n",
               "taxid_blank": b"A  \t  3\n", "taxid_below_i64": b"A  -9223372036854775809  3\n"}.items():
    REFUSED["listing_" + _k] = (_with((ACC, 2, _v)), ACC, 3)
# a bad ancestor in a lineage that is emitted (line 7 is taxid 50, named by the listing, and reached through merged id 99)
for _k, _v in BAD_ANCESTORS.items():
    REFUSED["ancestor_" + _k] = (_with(("taxidlineage.dmp", 6, b"50\t|\t10 " + _v + b" 40 \t|\n")), "taxidlineage.dmp", 7)
# ... and in the lineage of a taxid no accession line names: the reference never parses it, the build succeeds
UNREAD_ANCESTORS = {k: _with(("taxidlineage.dmp", 7, b"60\t|\t10 " + v + b" 50 \t|\n")) for k, v in BAD_ANCESTORS.items()}
ANCESTOR_TAXID = 50           # the oracle's ancestor message names the taxid whose lineage it walks, not the line

# two bad lines: the lower line of one dump, the dump loaded first of two (nodes, taxidlineage, names, merged, delnodes, listing)
PRECEDENCE: Dict[str, Tuple[Dict[str, bytes], str, int]] = {}
for _n in DUMP_FILES:
    _m = len(_dumps()[_n])
    PRECEDENCE["two_lines-" + _n] = (_with((_n, _m - 1, b"\n"), (_n, 0, b"x" + REST[_n])), _n, 1)
PRECEDENCE["two_lines-" + ACC] = (_with((ACC, 3, b"A 5 1\n"), (ACC, 1, b"B  x  2\n")), ACC, 2)
for _a, _b in zip(FILES[:-1], FILES[1:]):
    _second = (_b, 0, b"A 5 1\n" if _b == ACC else b"\n")
    PRECEDENCE["two_files-%s-%s" % (_a, _b)] = (_with(_second, (_a, 1, b"\n")), _a, 2)
PRECEDENCE["listing_before_ancestor"] = (_with(("taxidlineage.dmp", 6, b"50\t|\t10 x7 \t|\n"), (ACC, 3, b"D 40 4\n")), ACC, 4)


def many_ranks(n: int) -> Dict[str, bytes]:
    """n nodes, each with a rank of its own (the oracle has no rank limit; the builder's table holds 2048)."""
    ids = range(1, n + 1)
    return {"nodes.dmp": b"".join(b"%d\t|\t1\t|\tr%d\t|\n" % (k, k) for k in ids),
            "taxidlineage.dmp": b"".join(b"%d\t|\t\t|\n" % k for k in ids),
            "names.dmp": b"".join(b"%d\t|\tT%d\t|\t\t|\tscientific name\t|\n" % (k, k) for k in ids),
            "merged.dmp": b"", "delnodes.dmp": b"", ACC: b"A  1  1\nB  %d  2\n" % n}


def write(d: str, files: Dict[str, bytes]) -> dict:
    """The six files under d through taxdb_cases.write_case; returns its {"dir", "accessions"}."""
    return tc.write_case(d, nodes=files["nodes.dmp"], raw_names=files["names.dmp"], lineage=files["taxidlineage.dmp"],
                         merged=files["merged.dmp"], delnodes=files["delnodes.dmp"], accessions=files[ACC])
