"""Byte-level edge cases for the BLAST table ingest (csrc/ingest_gpu.hip, csrc/pipeline_ingest.cpp): the tables, what each claims
about itself and which parser must end up reading it.  Test infrastructure: deterministic (fixed seeds), no GPU and no product
code; the expected columns come from tests/ingest_reference.py (str.split, float(), int()).

tests/test_ingest_edges.py checks on the bytes that every case lies where it claims and that the CPU parser gives the
expectation; tests/test_gpu_ingest_edges.py holds the GPU parser's three builds to the same expectation and to the path.

A case is a Case: `blob` (the table), `predict` ("gpu": the GPU parser reads it; "cpu": it declines and the CPU parser reads
it; "refused": the CPU parser's error, `message` a fragment of it) and `claims`, what the case says about its own bytes."""
import dataclasses
import functools
import json
import os
import random
import re
import tempfile

from tests import ingest_reference as ref

STAGE_BYTES = 32768
PARSE_BLOCK = 256


# ---- 1. the grammar and range NumState::value takes (csrc/ingest_gpu.hip), restated from its comments ------------------------
_NUM = re.compile(rb"(-?)([0-9]*)(\.?)([0-9]*)(?:[eE]([+-]?)([0-9]{1,3}))?")


def decompose(field: bytes):
    """None when the field is outside the grammar `[-] digits [. digits] [e|E [+|-] 1-3 digits]` with at least one mantissa
    digit; else (negative, mantissa, net exponent = exponent - fraction digits, counted digits, has point, has exponent).
    Counted digits: every digit after the point, and before it every digit from the first nonzero one on."""
    m = _NUM.fullmatch(field)
    if m is None:
        return None
    sign, ip, dot, fp, esign, edigits = m.groups()
    if not ip and not fp:
        return None
    if fp and not dot:
        return None
    counted = len(ip.lstrip(b"0")) + len(fp)
    exp = int(edigits) if edigits else 0
    if esign == b"-":
        exp = -exp
    return sign == b"-", int(ip + fp), exp - len(fp), counted, bool(dot), edigits is not None


def plain_for_gpu(field: bytes) -> bool:
    """NumState::plain: the grammar with at most 15 counted digits, any exponent (the e-value column under its threshold)."""
    d = decompose(field)
    return d is not None and d[3] <= 15


def accepted_by_gpu(field: bytes, integer: bool) -> bool:
    """NumState::value (and, for the Int64 columns, no point and no exponent): what the GPU parser reads itself."""
    d = decompose(field)
    if d is None or d[3] > 15 or not -22 <= d[2] <= 22:
        return False
    return not (integer and (d[4] or d[5]))


def two_roundings(field: bytes) -> float:
    """The mantissa converted to a double first, then one IEEE operation with the exact power of ten: what the one-operation
    fast path would give if it took a mantissa of more than 53 bits."""
    neg, mant, e, _, _, _ = decompose(field)
    assert -22 <= e <= 22
    x = float(mant) * 10.0 ** e if e >= 0 else float(mant) / 10.0 ** -e
    return -x if neg else x


# ---- 2. the form of every parse block, from the bytes alone ---------------------------------------------------------------------
def line_starts(blob: bytes):
    """Start of every line, then the end mark line_start[n]: one past the last newline, or size + 1 for an open last line."""
    starts = [0]
    at = blob.find(b"\n")
    while at >= 0:
        starts.append(at + 1)
        at = blob.find(b"\n", at + 1)
    if starts[-1] == len(blob):           # closed last line: the last entry is the end mark already
        return starts
    return starts + [len(blob) + 1]


def block_forms(blob: bytes):
    """[(span, "staged" | "general")] per run of 256 lines: first line's start rounded down to 16 .. the end mark."""
    ls = line_starts(blob)
    n = len(ls) - 1
    out = []
    for r0 in range(0, n, PARSE_BLOCK):
        span = ls[min(r0 + PARSE_BLOCK, n)] - (ls[r0] & ~15)
        out.append((span, "general" if span > STAGE_BYTES else "staged"))
    return out


# ---- the database ------------------------------------------------------------------------------------------------------------------
UNHIT = ("s__unhit_a", "g__gunhit")                     # taxa of the database that no row of any case hits
TAXID_15 = 123456789012345


def db_json() -> str:
    taxa = [{"taxid": t, "rank": "species", "numericLineage": f"d__2;g__{t // 7};s__{t}",
             "textLineage": f"d__b;g__g{t // 7};s__s{t}", "accessions": []} for t in list(range(100, 200)) + [0, TAXID_15]]
    taxa += [{"taxid": 900001 + k, "rank": "species", "numericLineage": f"d__2;g__900000;s__{900001 + k}",
              "textLineage": f"d__b;g__gunhit;s__unhit_{'ab'[k]}", "accessions": []} for k in range(2)]
    return json.dumps({"blutilsVersion": "x", "sourceDatabase": "y", "taxonomies": taxa})


def write_db(dirname) -> str:
    path = os.path.join(str(dirname), "edges.json")
    with open(path, "w") as f:
        f.write(db_json())
    return path


# ---- 4. the expectation --------------------------------------------------------------------------------------------------------
def expected(blob: bytes, db: str):
    """(columns, checksum) of tests/ingest_reference.py for the table `blob` and the database text `db`."""
    with tempfile.TemporaryDirectory() as d:
        bt, tj = os.path.join(d, "b.tsv"), os.path.join(d, "t.json")
        with open(bt, "wb") as f:
            f.write(blob)
        with open(tj, "w") as f:
            f.write(db)
        t = ref.read_table(bt, tj)
    return t, ref.checksum(t)


# ---- lines -----------------------------------------------------------------------------------------------------------------------
E_VALUE = b"1e-50"


def _b(x) -> bytes:
    return x if isinstance(x, bytes) else str(x).encode()


def line(q, acc, tax=105, pid="99.356", aln=400, bs=845, pad=0, e_value=E_VALUE) -> bytes:
    """One row without its newline; `pad` bytes of filler go into a dead column (never parsed)."""
    return b"\t".join([_b(q), _b(acc), _b(tax), _b(pid), _b(aln), b"1" + b"x" * pad, b"0", b"1", b"400", b"1", b"400",
                       _b(e_value), _b(bs)])


def sized(length: int, q, acc, **kw) -> bytes:
    """A row of exactly `length` bytes (newline not counted)."""
    base = line(q, acc, **kw)
    assert len(base) <= length, (len(base), length)
    out = line(q, acc, pad=length - len(base), **kw)
    assert len(out) == length
    return out


SHORTEST = b"\tA\t1\t1\t1\t\t\t\t\t\t\t\t1"          # the shortest line with 13 columns
SHORTEST_E = b"\tA\t1\t1\t1\t\t\t\t\t\t\t1\t1"       # the same with a plain e-value, for the e-value threshold


@dataclasses.dataclass
class Case:
    blob: bytes
    predict: str = "gpu"
    claims: dict = dataclasses.field(default_factory=dict)
    message: str = None
    builds: bool = True          # accepted cases: also under the drop-nothing hit filter and the taxon filter


def _table(rows, eol=b"\n", open_tail=False) -> bytes:
    return eol.join(rows) + (b"" if open_tail else eol)


# ---- 3a. placement -----------------------------------------------------------------------------------------------------------------
def _offsets_table(last_field=b"845", queries=(b"query_0001",), model_len=69):
    """For k = 0 .. 15 (three rounds): a spacer row sized so that the row after it starts at offset k mod 16, then that row:
    `model_len` bytes with query queries[...] and last field `last_field`.  Every row ends in `last_field`."""
    rows, at = [], 0
    for rnd in range(3):
        for k in range(16):
            want = (k - at - 1) % 16                   # spacer length (without newline) mod 16
            n = 80 + (want - 80) % 16
            rows.append(sized(n, b"spacer%02d" % k, b"NR_%06d.1" % (100 + k), tax=100 + k, bs=last_field))
            at += n + 1
            assert at % 16 == k
            q = queries[(rnd + k) % len(queries)]
            rows.append(sized(model_len, q, b"NR_000105.1", bs=last_field))
            at += model_len + 1
    return rows


def placement_cases():
    c = {}
    rows = _offsets_table()
    c["model_line_offsets"] = Case(_table(rows), claims={"model_len": 70, "starts_mod16": 16, "ends_mod4": 4})
    c["one_byte_last_field"] = Case(_table(_offsets_table(last_field=b"7")), claims={"model_len": 70, "starts_mod16": 16, "last_field_bytes": 1})
    c["empty_and_one_byte_queries"] = Case(_table(_offsets_table(queries=(b"", b"Z"))),
                                           claims={"model_len": 70, "starts_mod16": 16, "model_query_bytes": {0, 1}})
    # (a spacer's end takes every offset mod 4 in front of an empty and of a one-byte query: its newline is the `e` of the mask)
    c["shortest_line"] = Case(_table([SHORTEST] * 600), claims={"line_len": len(SHORTEST) + 1, "rows": 600}, builds=False)
    c["shortest_line_with_e_value"] = Case(_table([SHORTEST_E] * 600), claims={"line_len": len(SHORTEST_E) + 1, "rows": 600})
    c["eol_lf"] = Case(_table(rows))
    c["eol_crlf"] = Case(_table(rows, b"\r\n"), claims={"crlf": True})
    c["eol_open_last_line"] = Case(_table(rows, open_tail=True), claims={"open": True})
    c["eol_open_last_line_ending_in_cr"] = Case(_table(rows, b"\r\n", open_tail=True) + b"\r", claims={"open": True, "last_byte": 13})
    c["a_14th_column"] = Case(_table([r + b"\textra" if i % 3 else r for i, r in enumerate(rows)]), claims={"max_columns": 14})
    c["a_trailing_tab"] = Case(_table([r + b"\t" if i % 2 else r for i, r in enumerate(rows)]), claims={"max_columns": 14})
    for size in (8191, 8192, 8193):
        body = [sized(69, b"query_%04d" % (i // 3), b"NR_%06d.1" % (100 + i % 50), tax=100 + i % 50) for i in range(110)]
        used = sum(len(r) + 1 for r in body)
        body.append(sized(size - used - 1, b"query_last", b"NR_000105.1"))
        c[f"size_{size}"] = Case(_table(body), claims={"size": size})
    body = [sized(69, b"query_%04d" % (i // 3), b"NR_%06d.1" % (100 + i % 50), tax=100 + i % 50) for i in range(110)]
    body.append(sized(8192 - sum(len(r) + 1 for r in body), b"query_last", b"NR_000105.1"))
    c["size_8192_open"] = Case(_table(body, open_tail=True), claims={"size": 8192, "open": True})
    return c


# ---- 3b. the stage bound -----------------------------------------------------------------------------------------------------------
SPANS = (32752, 32767, 32768, 32769, 32784)


def _block(n_lines, n_bytes, tag, start):
    """n_lines rows of n_bytes in all (newlines included), lengths as even as they come; ids from `start`."""
    each, extra = divmod(n_bytes, n_lines)
    return [sized(each - 1 + (1 if i < extra else 0), b"%s_%05d" % (tag, (start + i) // 2), b"NR_%06d.1" % (100 + i % 90), tax=100 + i % 90)
            for i in range(n_lines)]


def stage_case(position: str, span: int, r: int, open_tail=False) -> Case:
    """A table whose block at `position` ("first", "middle", "last", "short_last") has exactly `span` bytes from its first
    line's start rounded down to 16 to the end mark, the line starting r bytes past a multiple of 16; the other blocks take
    the other form."""
    staged = span <= STAGE_BYTES
    other = 256 * (300 if staged else 70)                 # the neighbours: 300-byte lines (general) or 70-byte lines (staged)
    n_before = {"first": 0, "middle": 2, "last": 2, "short_last": 2}[position]
    n_after = {"first": 2, "middle": 2, "last": 0, "short_last": 0}[position]
    n_target = 100 if position == "short_last" else 256
    if position == "first":
        assert r == 0
    rows = []
    for b in range(n_before):
        rows += _block(256, other, b"before%d" % b, 0)
    at = sum(len(x) + 1 for x in rows)
    if n_before:
        fix = (r - at) % 16                                # lengthen the last row before the block so that it starts at r mod 16
        rows[-1] = sized(len(rows[-1]) + fix, b"before_fix", b"NR_000105.1")
        at += fix
        assert at % 16 == r
    rows += _block(n_target, span - r, b"target", 0)      # (an open last line: the end mark is size + 1, as if it were closed)
    for b in range(n_after):
        rows += _block(256, other, b"after%d" % b, 0)
    blob = _table(rows, open_tail=open_tail)
    k = n_before
    return Case(blob, claims={"block": k, "span": span, "form": "staged" if staged else "general", "start_mod16": r,
                              "others": "general" if staged else "staged", "target_lines": n_target, "open": open_tail})


def stage_cases():
    c = {}
    offs = (1, 7, 15, 8, 3)
    for position in ("first", "middle", "last", "short_last"):
        for j, span in enumerate(SPANS):
            r = 0 if position == "first" else offs[j]
            c[f"{position}_{span}_r{r}"] = (position, span, r, False)
    for span in (32768, 32769):
        for r in (0, 15):
            c[f"middle_{span}_r{r}"] = ("middle", span, r, False)
        c[f"last_open_{span}_r5"] = ("last", span, 5, True)
    return c


def long_line_case() -> Case:
    rows = [sized(69, b"query_%04d" % (i // 3), b"NR_%06d.1" % (100 + i % 50), tax=100 + i % 50) for i in range(700)]
    rows[300] = sized(39999, b"query_long", b"NR_000105.1")
    return Case(_table(rows), claims={"longest_line": 40000, "forms": ["staged", "general", "staged"]})


# ---- 3c. row and query counts ------------------------------------------------------------------------------------------------------
ROW_COUNTS = (1, 2, 255, 256, 257, 511, 513, 1023, 1024, 1025, 4095, 4096, 4097)
QUERY_COUNTS = (2, 255, 256, 257, 65536, 65537)


def _row(q: int, i: int) -> bytes:
    return line(b"q%06d" % q, b"NR_%06d.1" % (100 + (i * 7) % 97), tax=100 + (i * 7) % 97, pid="%d.%03d" % (80 + i % 20, i % 1000),
                aln=100 + i % 1900, bs=50 + (i * 13) % 5000)


def rows_case(n: int) -> Case:
    """n rows, three per query, the rows of a query adjacent (a grouped file)."""
    return Case(_table([_row(i // 3, i) for i in range(n)]), claims={"rows": n, "queries": (n + 2) // 3, "grouped": True})


def queries_case(n_q: int) -> Case:
    """Every query once in id order, then a second row for up to 1500 of them in a shuffled order that starts with the highest
    id: rows of a query are not adjacent and the rows of the highest id do not come last."""
    rng = random.Random(n_q)
    again = list(range(n_q - 1)) if n_q <= 1500 else rng.sample(range(n_q - 1), 1499)
    rng.shuffle(again)
    order = list(range(n_q)) + [n_q - 1] + again
    return Case(_table([_row(q, i) for i, q in enumerate(order)]), claims={"rows": len(order), "queries": n_q, "grouped": False,
                                                                          "highest_not_last": True})


def grouping_cases():
    c = {}
    c["one_query_owns_every_row"] = Case(_table([_row(0, i) for i in range(1500)]), claims={"rows": 1500, "queries": 1, "grouped": True})
    c["every_query_one_row"] = Case(_table([_row(i, i) for i in range(1500)]), claims={"rows": 1500, "queries": 1500, "grouped": True})
    c["grouped_except_the_last_row"] = Case(_table([_row(i // 3, i) for i in range(1500)] + [_row(0, 1500)]),
                                            claims={"rows": 1501, "queries": 500, "grouped": False})
    return c


# ---- 3d. numbers: boundary spellings ---------------------------------------------------------------------------------------------
COLUMN = {"subject_taxid": 2, "perc_identity": 3, "align_length": 4, "e_value": 11, "bit_score": 12}
INTEGER = {"subject_taxid": True, "perc_identity": False, "align_length": True, "e_value": False, "bit_score": False}
NUMERIC, RANGE = "numeric column does not parse", "outside the 32-bit range"
Z = "0" * 30
JUNK = ("e", "E+", "1e+", ".", "-", "--1", "1-", "1e5e5", "1..0", "", "1_0", " 1", "1 ", "e5", "1e", "-e1", "1.5.e2", "0x10")

# (spelling, prediction) per column; a refused spelling is (spelling, "refused", message fragment).  The 15 / 16 counted digits
# behind the point are "0." + 14 zeros + "1" and "0." + 15 zeros + "1"; `0.00000000000001` has 14.
BOUNDARY = {
    "perc_identity": (
        [(s, "gpu") for s in ("123456789012345", "0." + "0" * 14 + "1", "0.00000000000001", Z + "123456789012345",
                              Z + ".123456789012345", "1e22", "1e-22", "1.5E+22", "123456789012345e22", "1.23456789012345e-8",
                              "0." + "0" * 14 + "1e37", "1e007", "1e-022", "1E+000", "1.e2", ".5e2", "-.5", "5.", "-0", "-0.0", "0e0", "-1e-22")]
        + [(s, "cpu") for s in ("1234567890123456", "0." + "0" * 15 + "1", "1.000000000000000", "1e23", "1e-23", "1.5e24", "0." + "0" * 14 + "1e38",
                                "1e0007", "1e0000", "+1", "+.5", "nan", "inf", "-inf", "infinity", "NaN")]
        + [(s, "refused", NUMERIC) for s in JUNK]),
    "bit_score": (
        [(s, "gpu") for s in ("123456789.012345", "0." + "0" * 14 + "1", Z + "123456789.012345", "0e22", "1e-22", "0." + "0" * 15 + "e37",
                              "7e002", "1.e2", ".5e2", "-.5", "5.", "-0", "-0.0", "2147483647.999", "-2147483648.999", "2.147483647e9",
                              "2147483647", "-2147483648", "0.2147483647e10", "21474836479e-1")]
        + [(s, "cpu") for s in ("1234567890.123456", "0." + "0" * 15 + "1", "0e23", "1e-23", "0." + "0" * 15 + "e38", "7e0002", "+1")]
        + [(s, "refused", RANGE) for s in ("2147483648", "-2147483649", "2147483648.0", "1e22", "nan", "inf", "-inf")]
        + [(s, "refused", NUMERIC) for s in JUNK]),
    "subject_taxid": (
        [(s, "gpu") for s in (str(TAXID_15), "-5", "-0", "0", Z + "105", "0105", "999999999999999")]
        + [(s, "cpu") for s in ("1234567890123456", "+105", "9223372036854775807", "-9223372036854775808")]
        + [(s, "refused", NUMERIC) for s in ("1.", "1e2", ".", "", "-", "--1", "1-", "9223372036854775808", " 1", "1_0", "nan")]),
    "align_length": (
        [(s, "gpu") for s in ("2147483647", "-2147483648", Z + "400", "-0", "0")]
        + [(s, "cpu") for s in ("+400",)]
        + [(s, "refused", RANGE) for s in ("2147483648", "-2147483649", "123456789012345")]
        + [(s, "refused", NUMERIC) for s in ("400.", "4e2", "", "-", "1-", " 400", "inf")]),
    # column 11 under the e-value threshold: NumState::plain, any exponent
    "e_value": (
        [(s, "gpu") for s in ("123456789012345", "0." + "0" * 14 + "1", Z + "123456789012345", "1e22", "1e23", "1e-23", "1e-180", "1e-999",
                              "1e999", "0." + "0" * 14 + "1e38", "1e007", "1.e2", ".5e2", "5.", "0", "0.0", "-0", "-1", "2e-50")]
        + [(s, "cpu") for s in ("1234567890123456", "0." + "0" * 15 + "1", "1e0007", "+1", "nan", "inf")]
        + [(s, "refused", NUMERIC) for s in JUNK]),
}
MAX_E = 1e10                                           # the threshold that turns column 11 on


def spelling_blob(column: str, spellings) -> bytes:
    """A good row, then one row per spelling with it in `column`."""
    rows = [line(b"q0", b"A.1")]
    for k, s in enumerate(spellings):
        c = line(b"q%d" % (k // 2), b"NR_%06d.1" % (100 + k % 7)).split(b"\t")
        c[COLUMN[column]] = s.encode()
        rows.append(b"\t".join(c))
    return _table(rows)


def accepted_spellings(column):
    return [t[0] for t in BOUNDARY[column] if t[1] == "gpu"]


def other_spellings(column):
    """[(spelling, "cpu" | "refused", message or None)]: one table each, since one of them turns the whole file over."""
    return [(t[0], t[1], t[2] if len(t) > 2 else None) for t in BOUNDARY[column] if t[1] != "gpu"]


# ---- 3e. numbers: two roundings -----------------------------------------------------------------------------------------------------
# 16- and 17-digit mantissas (above 2^53) with a nonzero net exponent: the double of the mantissa times / over the power of ten
# is not float(text).  Found by search against fractions.Fraction; kept as literals.
DOUBLE_ROUNDING = ("36045419051530900e-17", "97760240521923080e-17", "65598406264220498e-3", "43254797720018781e-14",
                   "91618374246574839e-3", "9102273081580125e9", "30769517319522718e-17", "9575043729869395e9",
                   "78056966345783611e-5", "60371092928270316e-3", "34500109046368849e-14", "9886048680452745e-13",
                   "988.6048680452745", "4325.4797720018781e-1")
DOUBLE_ROUNDING_BIT_SCORE = tuple(s for s in DOUBLE_ROUNDING if abs(float(s)) < 2e9)


# ---- 3f. numbers: random spellings of the accepted grammar ------------------------------------------------------------------------
N_RANDOM = 20000


def random_spelling(rng: random.Random, max_decade=None) -> str:
    """A spelling inside the GPU grammar, built (not filtered): nd <= 15 mantissa digits, the point anywhere, zeros after a
    leading point counted, leading zeros before the point free, net exponent in [-22, 22], exponent of one to three digits.
    max_decade: the value stays below 10^max_decade (bit_score: 9)."""
    nd = rng.choice((1, 2, 3, 5, 8, 11, 13, 14, 14, 14, 15, 15, 15, 15))
    pick = rng.random()
    mant = 10 ** 15 - 1 if pick < 0.01 else 5 * 10 ** 14 if pick < 0.02 else rng.randrange(10 ** (nd - 1), 10 ** nd)
    s = str(mant)
    nd = len(s)
    k = rng.randrange(0, nd + 1)                              # digits before the point
    zeros = rng.randrange(0, 16 - nd) if k == 0 and rng.random() < 0.3 else 0
    ip, fp = s[:k], "0" * zeros + s[k:]
    if ip and rng.random() < 0.2:
        ip = "0" * rng.randrange(1, 5) + ip                   # not counted
    if not ip and rng.random() < 0.5:
        ip = "0"
    text = ip + ("." + fp if fp else ("." if ip and rng.random() < 0.1 else ""))
    hi = 22 if max_decade is None else min(22, max_decade - nd)
    near = rng.random()
    net = -22 + rng.randrange(0, 3) if near < 0.3 else hi - rng.randrange(0, 3) if near < 0.6 else rng.randrange(-22, hi + 1)
    exp = net + len(fp)
    if exp != 0 or rng.random() < 0.5:
        digits = "%0*d" % (rng.choice((1, 1, 2, 3)), abs(exp))
        assert len(digits) <= 3
        text += rng.choice("eE") + ("-" if exp < 0 else rng.choice(("", "+"))) + digits
    return ("-" if rng.random() < 0.15 else "") + text


def random_case(column: str, form: str) -> Case:
    rng = random.Random({"perc_identity": 31, "bit_score": 32}[column])
    spellings = [random_spelling(rng, 9 if column == "bit_score" else None) for _ in range(N_RANDOM)]
    rows = []
    for i, s in enumerate(spellings):
        kw = {"pid": s} if column == "perc_identity" else {"bs": s}
        rows.append(line(b"q%05d" % (i // 4), b"NR_%06d.1" % (100 + i % 90), tax=100 + i % 90, pad=200 if form == "general" else 0, **kw))
    return Case(_table(rows), claims={"column": column, "form": form, "spellings": spellings}, builds=False)


# ---- 3g. names ------------------------------------------------------------------------------------------------------------------------
ALPHA = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ"
PREFIX = b"prefixprefixprefix"
FAMILY = ([b"", b"Z"] + [ALPHA[:n - 1] + t for n in (11, 12, 13, 16, 17) for t in (b"x", b"y")]
          + [PREFIX[:n] for n in (11, 12, 13, 15, 16, 17)]
          + [b"\x01", b"\x7f", b"\x80", b"\xff", b"mid\rdle", b" ", b"n" * 300, b"L" * 5000, b"L" * 4999 + b"M"])
SAME8, SAME16, SAME39 = b"SAMEPREF", b"SAME16__SAME16__", b"s" * 39
ACC_FAMILY = FAMILY + [
    SAME8 + b"a", SAME8 + b"b", SAME8 + b"aa",                 # equal in the first 8 bytes, differ at byte 9 (the longer one sorts first)
    SAME16 + b"a", SAME16 + b"b", SAME16 + b"aa",              # equal in the first 16, differ at byte 17
    SAME39 + b"a", SAME39 + b"b", SAME39 + b"aa",              # differ at byte 40
    SAME16, SAME16 + b"\x01",                                   # 16 bytes against 17 with the smallest 17th byte a line can hold
    b"\x80abc", b"\xffabc", b"zabc", b"\x7fabc", b"Aabc",      # high bytes sort above ASCII (unsigned, like String::cmp)
]


def names_case(seed: int = 0, longest: int = 5000) -> Case:
    """Every query family member on rows with several accessions, every accession on rows of several queries, file order
    shuffled.  longest: names beyond it are left out (300: the table fits the parse kernel's stage)."""
    rng = random.Random(100 + seed)
    fam, acc = [x for x in FAMILY if len(x) <= longest], [x for x in ACC_FAMILY if len(x) <= longest]
    pairs = [(fam[i % len(fam)], acc[(i * 5 + i // len(fam)) % len(acc)]) for i in range(9 * len(fam))]
    rng.shuffle(pairs)
    rows = [line(q, a, tax=100 + i % 90, bs=50 + i) for i, (q, a) in enumerate(pairs)]
    return Case(_table(rows), claims={"queries": len(fam), "accessions": len(acc), "form": "staged" if longest <= 300 else "general"})


def nul_name_case() -> Case:
    """A query and an accession holding a NUL byte.  The columns ABI hands the string tables over NUL-separated, so the
    expectation is the checksum, the counts and the tables' byte lengths, not the split lists."""
    rows = [line(q, a, tax=100 + i, bs=50 + i) for i, (q, a) in enumerate(
        [(b"q\0one", b"A\0B"), (b"q", b"A"), (b"q\0one", b"A"), (b"one", b"A\0B"), (b"q\0", b"B"), (b"q", b"A\0")])]
    return Case(_table(rows), claims={"nul": True}, builds=False)


# ---- 3h. declined and refused ----------------------------------------------------------------------------------------------------
def declined_cases():
    rows = [_row(i // 3, i) for i in range(40)]
    c = {}
    c["blank_line_in_the_middle"] = Case(_table(rows[:20] + [b""] + rows[20:]), "cpu")
    c["blank_line_at_the_end"] = Case(_table(rows) + b"\n", "cpu")
    c["crlf_only_line_in_the_middle"] = Case(_table(rows[:20] + [b""] + rows[20:], b"\r\n"), "cpu")
    c["crlf_only_line_at_the_end"] = Case(_table(rows, b"\r\n") + b"\r\n", "cpu")
    c["a_quoted_query"] = Case(_table(rows[:7] + [b'"' + rows[7].replace(b"\t", b'"\t', 1)] + rows[8:]), "cpu")
    c["a_quote_inside_an_accession"] = Case(_table(rows[:7] + [rows[7].replace(b"NR_", b'N"R_', 1)] + rows[8:]), "cpu")
    c["twelve_columns"] = Case(_table(rows[:7] + [b"\t".join(rows[7].split(b"\t")[:12])] + rows[8:]), "refused", message="columns")
    c["twelve_columns_on_the_last_open_line"] = Case(_table(rows + [b"\t".join(rows[7].split(b"\t")[:12])], open_tail=True), "refused",
                                                     message="columns")
    return c


def bs_as_written_case() -> Case:
    """Every bit score is k.5 with k >= 0, `0.5` among them: a min_bit_score of 0.25 is below every score as written and above
    the truncated 0.5, so a filter that compared the truncated column would drop rows."""
    return Case(_table([line(b"q%03d" % (i // 3), b"NR_%06d.1" % (100 + i % 9), bs="%d.5" % (i % 4)) for i in range(300)]),
                claims={"min_bit_score": 0.25})


# ---- the registry: name -> builder of the Case, run on demand ----------------------------------------------------------------------
PLACEMENT = ("model_line_offsets", "one_byte_last_field", "empty_and_one_byte_queries", "shortest_line", "shortest_line_with_e_value",
             "eol_lf", "eol_crlf", "eol_open_last_line", "eol_open_last_line_ending_in_cr", "a_14th_column", "a_trailing_tab",
             "size_8191", "size_8192", "size_8193", "size_8192_open")
GROUPING = ("one_query_owns_every_row", "every_query_one_row", "grouped_except_the_last_row")


def _registry():
    r = {}
    for name in PLACEMENT:
        r[f"placement/{name}"] = functools.partial(lambda n: placement_cases()[n], name)
    for name, args in stage_cases().items():
        r[f"stage/{name}"] = functools.partial(stage_case, *args)
    r["stage/one_line_of_40000_bytes"] = long_line_case
    for n in ROW_COUNTS:
        r[f"rows/{n}"] = functools.partial(rows_case, n)
    for n in QUERY_COUNTS:
        r[f"queries/{n}"] = functools.partial(queries_case, n)
    for name in GROUPING:
        r[f"grouping/{name}"] = functools.partial(lambda n: grouping_cases()[n], name)
    r["names/families"] = names_case
    r["names/families_other_order"] = functools.partial(names_case, 1)
    r["names/families_staged"] = functools.partial(names_case, 2, 300)
    return r


ACCEPTED = _registry()                                  # accepted placement, stage-bound, count and name cases: name -> builder
DECLINED = ("blank_line_in_the_middle", "blank_line_at_the_end", "crlf_only_line_in_the_middle", "crlf_only_line_at_the_end",
            "a_quoted_query", "a_quote_inside_an_accession", "twelve_columns", "twelve_columns_on_the_last_open_line")


@functools.lru_cache(maxsize=4)
def accepted_case(name: str) -> Case:
    return ACCEPTED[name]()


@functools.lru_cache(maxsize=None)
def _db_text():
    return db_json()


@functools.lru_cache(maxsize=4)
def expected_of(name: str):
    """(columns, checksum) of an accepted case, computed once for the tests that share it."""
    return expected(accepted_case(name).blob, _db_text())


# the drop-nothing hit filter (every threshold on) and the taxon filter that names a taxon no row hits
HIT_FILTER_ALL = {"min_perc_identity": -1e300, "min_bit_score": -1e300, "min_align_length": -(1 << 31), "max_e_value": MAX_E}
TAXON_FILTER_UNHIT = {"exclude": [UNHIT[0]]}


def kept_by_e_value(blob: bytes, max_e: float = MAX_E) -> bytes:
    """The table without the rows whose column 11, read by float(), is not <= max_e (a NaN fails, as in IEEE)."""
    return b"".join(ln + b"\n" for ln in blob.split(b"\n") if ln and float(ln.split(b"\t")[11].decode()) <= max_e)
