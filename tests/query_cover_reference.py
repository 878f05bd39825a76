"""Query coverage (`--min-query-cover`) restated in plain Python: the resolver of the source from the format
string, the predicate in Python integers, and `drop_lines`, which writes the copy of a table without the lines below the cover.
Test infrastructure: no product code; the expected result of a covered run is the library's own result, through the path
without the flag, on that copy.

The rule: the coverage of a line comes from `qcovhsp` (that column: an integer percent c, kept iff c * 1000 >= P_milli), from
`qstart qend qlen` (kept iff (|qend - qstart| + 1) * 100000 >= P_milli * qlen) or from `qcovs` (as qcovhsp); `auto` takes the
first of the three the format string has.  P has at most three decimals, 0 .. 100: P_milli = 1000 P.  Coverage fields are Int64
fields ([+-]digits) in 0 .. 2^31 - 1, qlen above 0."""
import decimal
import re

from tests import outfmt_reference as R

SOURCES = ("auto", "qcovhsp", "qlen", "qcovs")
NEEDS = {"qcovhsp": ("qcovhsp",), "qlen": ("qstart", "qend", "qlen"), "qcovs": ("qcovs",)}
PRIORITY = ("qcovhsp", "qlen", "qcovs")
INT32_MAX = (1 << 31) - 1


class CoverError(ValueError):
    """A refused source; `missing`: the specifiers the message has to name."""

    def __init__(self, missing):
        super().__init__("missing: " + " ".join(missing))
        self.missing = tuple(missing)


class FieldError(ValueError):
    """A coverage field the parsers refuse; `line`: its 1-based line number."""

    def __init__(self, line, why):
        super().__init__(f"line {line}: {why}")
        self.line = line


def resolve(spec: str, source: str = "auto") -> dict:
    """{source, columns}: the resolved source and the 0-based column of every specifier it reads.  The format string goes
    through the layout's grammar first (R.SpecError); a source whose specifiers it lacks is a CoverError naming them."""
    R.parse_spec(spec)
    cols = R.columns_of(spec)
    assert source in SOURCES
    if source == "auto":
        for s in PRIORITY:
            if all(n in cols for n in NEEDS[s]):
                source = s
                break
        else:
            raise CoverError([n for s in PRIORITY for n in NEEDS[s] if n not in cols])
    missing = [n for n in NEEDS[source] if n not in cols]
    if missing:
        raise CoverError(missing)
    return {"source": source, "columns": {n: cols.index(n) for n in NEEDS[source]}}


def milli(percent) -> int:
    """P_milli, exactly"""
    m = decimal.Decimal(str(percent)) * 1000
    assert m == m.to_integral_value() and 0 <= m <= 100000, percent
    return int(m)


def keeps(source: str, p_milli: int, values) -> bool:
    """values: (c,) for qcovhsp / qcovs, (qstart, qend, qlen) for qlen — Python integers"""
    if source == "qlen":
        qstart, qend, qlen = values
        return (abs(qend - qstart) + 1) * 100000 >= p_milli * qlen
    return values[0] * 1000 >= p_milli


def field_value(field: bytes, line: int, name: str) -> int:
    if not re.fullmatch(rb"[+-]?[0-9]+", field):
        raise FieldError(line, f"{name} does not parse")
    v = int(field)
    if not 0 <= v <= INT32_MAX or (name == "qlen" and v == 0):
        raise FieldError(line, f"{name} outside its range")
    return v


def drop_lines(blob: bytes, spec: str, cover: dict):
    """(the table without the lines below the cover, n_below).  cover: {"percent": P, "source": one of SOURCES}.  Blank lines and
    line ends are kept as they are; every non-empty line's coverage fields are validated (FieldError), kept or not."""
    got = resolve(spec, cover.get("source", "auto"))
    p_milli = milli(cover["percent"])
    at = [(n, got["columns"][n]) for n in NEEDS[got["source"]]]
    out, n_below, line_no = [], 0, 0
    for ln, end in R._lines(blob):
        line_no += 1
        if not ln:
            out.append(end)
            continue
        f = ln.split(b"\t")
        values = [field_value(f[k], line_no, n) for n, k in at]
        if keeps(got["source"], p_milli, values):
            out.append(ln + end)
        else:
            n_below += 1
    return b"".join(out), n_below


# ---- tables with coverage fields ----------------------------------------------------------------------------------------------------
COVER_NAMES = ("qcovhsp", "qstart", "qend", "qlen", "qcovs")


def set_fields(blob: bytes, spec: str, values) -> bytes:
    """The table with the named fields rewritten: values(i) -> {specifier: bytes} for the i-th line (0-based, blank lines
    counted).  If a line carries its padding in a column that is rewritten, the padding moves to the first column that is
    neither a role nor rewritten nor a coverage specifier, whose own byte takes its place: the line keeps its length whenever
    the new fields are as long as the old (one byte in the tables of tests/outfmt_cases.py)."""
    cols, lay = R.columns_of(spec), R.parse_spec(spec)
    roles = {lay[r] for r in R.ROLES if lay[r] is not None}
    out = []
    for i, (ln, end) in enumerate(R._lines(blob)):
        if not ln:
            out.append(end)
            continue
        f = ln.split(b"\t")
        new = values(i)
        free = next(k for k, n in enumerate(cols) if k not in roles and n not in new and n not in COVER_NAMES)
        for name, v in new.items():
            k = cols.index(name)
            if len(f[k]) > 1 and f[k].strip(b"x") in (b"", b"1"):      # (the padded column of outfmt_cases.line)
                f[free], f[k] = f[k], f[free]
            f[k] = v
        out.append(b"\t".join(f) + end)
    return b"".join(out)
