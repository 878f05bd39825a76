"""Tables for the query-cover tests on the GPU (`--min-query-cover`): the byte-level cases of
tests/outfmt_cases.py with one-byte coverage fields written into them (the lines keep their lengths, so the spans hold), and the
threshold-boundary rows.  Test infrastructure: deterministic, no GPU and no product code; expectations come from
tests/query_cover_reference.py (drop_lines), tests/outfmt_reference.py (to_reference) and tests/ingest_reference.py."""
import functools

from tests import ingest_edges as E
from tests import outfmt_cases as K
from tests import query_cover_reference as Q

# per source: the format string with a coverage field first and one with it last, the cover of the byte-level cases, and the
# one-byte fields of line i — about half of the lines lie below the cover, the first line does not
SOURCES = {
    "qcovhsp": {"first": "qcovhsp std staxid", "last": "6 std staxid qcovhsp", "cover": {"percent": "5", "source": "qcovhsp"},
                "fields": lambda i: {"qcovhsp": b"%d" % ((i * 7 + 5) % 10)}},
    "qlen": {"first": "qlen std staxid", "last": "6 std staxid qlen", "cover": {"percent": "50", "source": "qlen"},
             "fields": lambda i: {"qstart": b"%d" % (1 + i % 3), "qend": b"%d" % (1 + (i * 5 + 6) % 7), "qlen": (b"9", b"5", b"3", b"7")[i % 4]}},
    "qcovs": {"first": "qcovs std staxids", "last": "6 std staxids qcovs", "cover": {"percent": "4.5", "source": "auto"},
              "fields": lambda i: {"qcovs": b"%d" % ((i * 3 + 6) % 10)}},
}
ROW_COUNTS = (1, 255, 256, 257, 600)


def _with_fields(source, spec, case) -> E.Case:
    return E.Case(Q.set_fields(case.blob, spec, SOURCES[source]["fields"]), claims=case.claims)


def _registry():
    r = {}
    for source, s in SOURCES.items():
        tail = b";1;2" if source == "qcovs" else b""
        for where in ("first", "last"):
            spec = s[where]
            r[f"{source}/{where}/staged_32768"] = (source, spec, functools.partial(K.stage_case, spec, 32768, 7, tail=tail))
            r[f"{source}/{where}/general_32769"] = (source, spec, functools.partial(K.stage_case, spec, 32769, 3, tail=tail))
            r[f"{source}/{where}/one_line_of_40000_bytes"] = (source, spec, functools.partial(K.long_line_case, spec))
            r[f"{source}/{where}/open_last_line"] = (source, spec, functools.partial(K.stage_case, spec, 32768, 5, open_tail=True, tail=tail))
            r[f"{source}/{where}/crlf"] = (source, spec, functools.partial(K.stage_case, spec, 32768, 9, eol=b"\r\n", tail=tail))
        for n in ROW_COUNTS:
            r[f"{source}/rows_{n}"] = (source, s["last"], functools.partial(K.rows_case, s["last"], n, tail=tail))
    return r


ACCEPTED = _registry()


@functools.lru_cache(maxsize=4)
def accepted_case(name: str) -> E.Case:
    source, spec, build = ACCEPTED[name]
    return _with_fields(source, spec, build())


# ---- threshold boundaries ---------------------------------------------------------------------------------------------------------
LEN_SPEC, HSP_SPEC = "6 std staxid qlen", "6 std staxid qcovhsp"
TOP = (1 << 31) - 1
# (qstart, qend, qlen): the span of 1199 / 1200 / 1201 over 1500 around 80 percent, qstart > qend, one and two of three bases
# around 33.333 / 33.334 / 66.666 / 66.667 percent, a span longer than qlen, and the largest values
LEN_ROWS = [(1, 1199, 1500), (1, 1200, 1500), (1, 1201, 1500), (1200, 1, 1500), (1199, 1, 1500), (1201, 2, 1500), (301, 1500, 1500),
            (2, 2, 3), (1, 2, 3), (3, 1, 3), (7, 7, 1), (1, 400, 300), (0, TOP, TOP), (TOP, 0, TOP), (1, TOP, TOP), (TOP, TOP, TOP), (0, 0, 1),
            (1, 100000, 100000), (1, 99999, 100000), (1, 1, 100000)]
LEN_PERCENTS = ("80", "79.933", "79.934", "80.001", "33.333", "33.334", "66.666", "66.667", "0", "100", "0.001", "99.999")
HSP_VALUES = (0, 1, 79, 80, 81, 99, 100, 101, TOP)
HSP_PERCENTS = ("0", "100", "80", "79.999", "80.001", "0.001", "99.999")


def boundary_table(spec, n=300, top=True) -> bytes:
    """n rows cycling through the boundary values, three rows per query; top=False leaves the largest values out"""
    rows = [K.line(spec, b"q%04d" % (i // 3), b"NR_%06d.1" % (100 + i % 90), tax=100 + i % 90, bs=500 + i % 7) for i in range(n)]
    if "qlen" in spec:
        vals = [v for v in LEN_ROWS if top or max(v) < TOP]
        fields = lambda i: dict(zip(("qstart", "qend", "qlen"), (b"%d" % x for x in vals[i % len(vals)])))
    else:
        vals = [v for v in HSP_VALUES if top or v < TOP]
        fields = lambda i: {"qcovhsp": b"%d" % vals[i % len(vals)]}
    return Q.set_fields(E._table(rows), spec, fields)
