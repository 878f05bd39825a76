"""The column layout of a BLAST table (`--blast-outfmt`) restated in plain Python: the grammar of the format
string, `relayout` (a reference-order table written in another layout) and `to_reference` (its inverse, by the rule the
library is held to).  Test infrastructure: no product code; the expected columns of a laid-out table are
tests/ingest_reference.py's reading of `to_reference(table, spec)`.

The rule: specifiers separated by blanks; an optional leading `6`, any other leading number refused; `std` = BLAST's twelve
standard columns; at most 64 columns after the expansion; none named twice; any other [A-Za-z0-9_]+ token is a column nobody
reads.  Roles by priority, not by position: query = qseqid, qacc, qaccver; subject accession = saccver, sacc, sseqid; taxid =
staxid, staxids; pident, length, bitscore, and (optional) evalue.  A `staxids` field counts up to its first ';'."""
import re

STD = "qseqid sseqid pident length mismatch gapopen qstart qend sstart send evalue bitscore".split()
REFERENCE = "qseqid saccver staxid pident length mismatch gapopen qstart qend sstart send evalue bitscore".split()
REFERENCE_SPEC = "6 " + " ".join(REFERENCE)
MAX_COLUMNS = 64
ROLES = {"query": ("qseqid", "qacc", "qaccver"), "accession": ("saccver", "sacc", "sseqid"), "taxid": ("staxid", "staxids"),
         "perc_identity": ("pident",), "align_length": ("length",), "bit_score": ("bitscore",), "e_value": ("evalue",)}
REFERENCE_COLUMN = {"query": 0, "accession": 1, "taxid": 2, "perc_identity": 3, "align_length": 4, "e_value": 11, "bit_score": 12}


class SpecError(ValueError):
    """A refused format string; `token`: what the message has to name."""

    def __init__(self, token, why):
        super().__init__(f"{why}: {token}")
        self.token = token


def columns_of(spec: str):
    """The column names of a format string, `std` expanded, the leading `6` gone."""
    cols = []
    for k, tok in enumerate(t for t in re.split(r"[ \t]+", spec) if t):
        if not re.fullmatch(r"[A-Za-z0-9_]+", tok):
            raise SpecError(tok, "not a specifier")
        if k == 0 and tok.isdigit():
            if tok != "6":
                raise SpecError(tok, "not format 6")
            continue
        cols += STD if tok == "std" else [tok]
    return cols


def parse_spec(spec: str) -> dict:
    """The layout a format string names: n_columns, one 0-based column per role (e_value: None when absent), taxid_is_list."""
    cols = columns_of(spec)
    if len(cols) > MAX_COLUMNS:
        raise SpecError(cols[MAX_COLUMNS], "more than 64 columns")
    for k, c in enumerate(cols):
        if c in cols[:k]:
            raise SpecError(c, "named twice")
    lay = {"n_columns": len(cols)}
    for role, names in ROLES.items():
        found = [n for n in names if n in cols]
        if not found and role != "e_value":
            raise SpecError(names[0], "missing role")
        lay[role] = cols.index(found[0]) if found else None
    lay["taxid_is_list"] = cols[lay["taxid"]] == "staxids"
    return lay


def is_reference(lay: dict) -> bool:
    return lay == dict(REFERENCE_COLUMN, n_columns=13, taxid_is_list=False)


def _lines(blob: bytes):
    """[(line without its end, end)]: the end is b"\\n", b"\\r\\n", or b"" / b"\\r" on an open last line."""
    out = []
    parts = blob.split(b"\n")
    for k, ln in enumerate(parts):
        last = k == len(parts) - 1
        if last and ln == b"":
            break
        cr = ln.endswith(b"\r")
        out.append((ln[:-1] if cr else ln, (b"\r" if cr else b"") + (b"" if last else b"\n")))
    return out


def relayout(blob13: bytes, spec: str, fillers=None) -> bytes:
    """A table in the reference's thirteen columns written in the layout `spec` names.  Role columns get the role's bytes;
    a column named like one of the reference's other columns (mismatch ... send, or a role's lower-priority name) gets that
    column's bytes; any other column gets fillers[name] — bytes, or a function of the line number — and b"x" without one.
    fillers[";"]: what follows the taxid in a `staxids` role field, the ';' included (default nothing).  Blank lines and line
    ends are kept."""
    fillers = fillers or {}
    cols, lay = columns_of(spec), parse_spec(spec)
    role_at = {lay[r]: r for r in ROLES if lay[r] is not None}
    give = lambda f, i: f(i) if callable(f) else f
    out = []
    for i, (ln, end) in enumerate(_lines(blob13)):
        if not ln:
            out.append(end)
            continue
        src = ln.split(b"\t")
        assert len(src) >= 13, ln
        fields = []
        for k, name in enumerate(cols):
            if k in role_at:
                f = src[REFERENCE_COLUMN[role_at[k]]]
                if role_at[k] == "taxid" and lay["taxid_is_list"]:
                    f += give(fillers.get(";", b""), i)
            elif name in fillers:
                f = give(fillers[name], i)
            elif name in REFERENCE[5:11]:
                f = src[REFERENCE.index(name)]
            else:
                f = b"x"
            fields.append(f)
        out.append(b"\t".join(fields) + end)
    return b"".join(out)


def to_reference(blob: bytes, spec: str) -> bytes:
    """The table rewritten to the reference's thirteen columns: the seven role fields copied as their bytes, `staxids` cut at
    its first ';', everything else b"0" (an absent e-value too).  Blank lines and line ends are kept; a line with fewer fields
    than `spec` names is an AssertionError."""
    lay = parse_spec(spec)
    out = []
    for ln, end in _lines(blob):
        if not ln:
            out.append(end)
            continue
        src = ln.split(b"\t")
        assert len(src) >= lay["n_columns"], ln
        fields = [b"0"] * 13
        for role, at in REFERENCE_COLUMN.items():
            if lay[role] is not None:
                fields[at] = src[lay[role]]
        if lay["taxid_is_list"]:
            fields[2] = fields[2].split(b";", 1)[0]
        out.append(b"\t".join(fields) + end)
    return b"".join(out)


# ---- the layouts the tests run ------------------------------------------------------------------------------------------------
STD_STAXIDS = "6 std staxids"
REVERSED = " ".join(reversed(REFERENCE))
MINIMAL = "qacc sacc staxid pident length evalue bitscore"                                     # seven columns, every one a role
WIDE = ("6 " + " ".join(f"f{k:02d}" for k in range(1, 15))
        + " qseqid f15 saccver f16 staxids f17 pident f18 length f19 evalue f20 bitscore f21 f22 f23")   # 30 columns, roles beyond 13
TAXID_LAST = "qseqid sseqid pident length evalue bitscore qcovs staxids"                      # the taxid is the last field
EMPTY_IN_FRONT = "e1 qseqid e2 saccver e3 staxid e4 pident e5 length e6 evalue e7 bitscore"   # an empty field in front of each role
LAYOUTS = {
    "std_staxids": (STD_STAXIDS, {}),
    "reversed": (REVERSED, {}),
    "minimal": (MINIMAL, {}),
    "wide": (WIDE, {";": lambda i: (b"", b";9606", b";1;2;3")[i % 3]}),
    "taxid_last": (TAXID_LAST, {";": b";b;c"}),
    "empty_in_front": (EMPTY_IN_FRONT, {f"e{k}": b"" for k in range(1, 8)}),
}
