"""Plain-Python restatement of `build-db lineages`, bytes in and bytes out: the document, the non-mapped TSV,
the taxid map and the counts, from dicts and bytes methods alone.  It shares no code with the product; the GPU build
(csrc/lineage_db_gpu.hip) is compared with it byte for byte."""
import re
from typing import Dict, List, Optional, Sequence, Tuple

VERSION = "8.3.1"
MAX_DEPTH = 64
LETTERS = {b"u": b"u", b"undefined": b"u", b"d": b"d", b"domain": b"d", b"k": b"k", b"kingdom": b"k", b"p": b"p",
           b"phylum": b"p", b"c": b"c", b"class": b"c", b"o": b"o", b"order": b"o", b"f": b"f", b"family": b"f",
           b"g": b"g", b"genus": b"g", b"s": b"s", b"species": b"s"}


class LineageError(Exception):
    """A refused table: .line is the 1-based line, .kind one of utf8, tab, id, level, rank, depth."""

    def __init__(self, line: int, kind: str):
        super().__init__(f"line {line}: {kind}")
        self.line, self.kind = line, kind


def slug(b: bytes) -> bytes:
    """slugify_ascii: ASCII lower case, runs of [a-z0-9] joined by '-' (every other byte, those >= 0x80 too, separates)."""
    return b"-".join(re.findall(rb"[a-z0-9]+", b.lower()))


def parse_rank(token: bytes) -> bytes:
    """LinnaeanRank::from_str + Display: lower case and trim, the letter of a Linnaean rank, else the slug."""
    t = token.lower().strip()
    return LETTERS.get(t, slug(t))


def lines_of(data: bytes) -> List[bytes]:
    out = data.split(b"\n")
    if out[-1] == b"":
        out.pop()                      # the text behind the last newline is a line only when there is some
    return out


def jstr(b: bytes) -> bytes:
    """serde_json's escapes; every other byte as it is."""
    esc = {0x22: b'\\"', 0x5C: b"\\\\", 8: b"\\b", 12: b"\\f", 10: b"\\n", 13: b"\\r", 9: b"\\t"}
    return b'"' + b"".join(esc.get(c, b"\\u%04x" % c if c < 0x20 else bytes([c])) for c in b) + b'"'


def build(data: bytes, table_name: str, replace: Optional[Sequence[Tuple[str, str]]] = None) -> Dict[str, object]:
    """-> {"doc", "tsv", "map": bytes, "stats": counts, "taxa": {path: taxid}}; raises LineageError on the lowest bad line.
    replace: the -r pairs as the command line gives them, RANK already lower-cased."""
    rules: Dict[bytes, bytes] = {}
    if replace is not None:
        for a, b in replace:
            rules[a.encode()] = b.encode()              # a repeated key keeps its place and takes the last value
    taxa: Dict[bytes, int] = {}
    units: Dict[int, dict] = {}
    tsv, tmap = [], []
    oid = 0
    header_open = True
    st = {"data_lines": 0, "taxonomies": 0, "taxa": 0, "empty": 0, "truncated": 0, "max_depth": 0}
    for number, line in enumerate(lines_of(data), 1):
        bare = line.strip()
        if bare == b"" or bare.startswith(b"#"):
            continue
        if header_open:
            header_open = False
            if line.split(b"\t")[0].strip() == b"Feature ID":
                continue
        this_oid, oid = oid, oid + 1
        st["data_lines"] += 1
        try:
            line.decode("utf-8")
        except UnicodeDecodeError:
            raise LineageError(number, "utf8") from None
        fields = line.split(b"\t")
        if len(fields) < 2:
            raise LineageError(number, "tab")
        ident = fields[0].strip()
        if ident == b"":
            raise LineageError(number, "id")
        elements: List[bytes] = []
        for piece in fields[1].split(b";"):
            piece = piece.strip()
            if piece == b"":
                continue
            if b"__" not in piece:
                raise LineageError(number, "level")
            token, name = piece.split(b"__", 1)
            if slug(name) == b"":
                st["truncated"] += 1
                break
            if len(elements) == MAX_DEPTH:
                raise LineageError(number, "depth")
            token = token.strip().lower()
            rank = parse_rank(rules.get(token, token))
            if rank == b"":
                raise LineageError(number, "rank")
            elements.append(rank + b"__" + slug(name))
        st["max_depth"] = max(st["max_depth"], len(elements))
        if not elements:
            st["empty"] += 1
            tsv.append(ident + b"\t%d\tempty-lineage\n" % number)
            continue
        ids = []
        for k in range(len(elements)):
            ids.append(taxa.setdefault(b";".join(elements[:k + 1]), len(taxa) + 1))
        unit = units.setdefault(ids[-1], {
            "rank": elements[-1].split(b"__")[0], "text": b";".join(elements),
            "numeric": b";".join(e.split(b"__")[0] + b"__%d" % i for e, i in zip(elements, ids)), "accessions": []})
        unit["accessions"].append((ident, this_oid))
        tmap.append(ident + b" %d\n" % ids[-1])
    st["taxa"], st["taxonomies"] = len(taxa), len(units)

    head = b'{\n  "blutilsVersion": ' + jstr(VERSION.encode()) + b',\n  "ignoreTaxids": null,\n'
    if replace is None:
        head += b'  "replaceRank": null,\n'
    elif not rules:
        head += b'  "replaceRank": {},\n'
    else:
        head += b'  "replaceRank": {\n' + b",\n".join(b"    " + jstr(a) + b": " + jstr(b) for a, b in rules.items()) + b"\n  },\n"
    head += b'  "dropNonLinnaeanTaxonomies": null,\n  "sourceDatabase": ' + jstr(table_name.encode()) + b",\n"
    entries = []
    for taxid in sorted(units):
        u = units[taxid]
        accs = b",\n".join(b'        {\n          "accession": ' + jstr(a) + b',\n          "oid": "%d"\n        }' % o
                           for a, o in u["accessions"])
        entries.append(b'    {\n      "taxid": %d,\n      "rank": "' % taxid + u["rank"] + b'",\n      "numericLineage": "' + u["numeric"]
                       + b'",\n      "textLineage": "' + u["text"] + b'",\n      "accessions": [\n' + accs + b"\n      ]\n    }")
    doc = head + (b'  "taxonomies": [\n' + b",\n".join(entries) + b"\n  ]\n}" if entries else b'  "taxonomies": []\n}')
    return {"doc": doc, "tsv": b"".join(tsv), "map": b"".join(tmap), "stats": st, "taxa": taxa}
