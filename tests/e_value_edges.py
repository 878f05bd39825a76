"""The e-value threshold decision (csrc/ingest_gpu.hip: e_value_verdict, device_filter, list_undecided, apply_decisions;
DESIGN.md §14.3 "E-values") across thresholds and spellings: the thresholds, the fields and the tables.  Test infrastructure in
the manner of tests/ingest_edges.py: deterministic (fixed seeds), no GPU and no product code.

The expected value of every field is `float(field) <= E` (tests/hit_filter_reference.py), never anything in this file.  `tier`
restates the device's ladder, host constants included, for two purposes only: to classify the cases, so that the tests can assert
what they cover, and to split each threshold's cases into a *decided* table (the restatement decides every field) and an *asked*
table (the restatement leaves every field to the host).  tests/test_e_value_edges.py holds the restatement to float() wherever it
decides and runs the host parser over every table; tests/test_gpu_e_value_edges.py holds the GPU parser to the same tables and to
the trace: a decided table causes no host round trip."""
import collections
import decimal
import functools
import math
import random

from tests import ingest_edges as IE

# ---- the ladder, restated ------------------------------------------------------------------------------------------------------
NEVER, ALWAYS = -(1 << 30), 1 << 30
P10 = [float(10 ** k) for k in range(23)]                 # exact doubles
BAND_LO, BAND_HI = 1e-280, 1e280
BRACKET = 2.0 ** -46
TIERS = ("zero", "negative", "mag_keep", "mag_drop", "one_op", "band_keep", "band_drop", "band_ask", "ask_outside")
UNDECIDED = ("negative", "band_ask", "ask_outside")

Constants = collections.namedtuple("Constants", "k_keep k_drop band e_lo e_hi")


def constants(E: float) -> Constants:
    """device_filter: the two decimal-magnitude bounds, whether the band applies, and the bracket."""
    if not E >= 0.0:                                      # negative or NaN
        return Constants(NEVER, NEVER, False, 0.0, 0.0)
    if E == 0.0:
        return Constants(-325, -322, False, 0.0, 0.0)
    if math.isinf(E):
        return Constants(ALWAYS, ALWAYS, False, 0.0, 0.0)
    t = math.floor(math.log10(E))                         # the library's log10, as the host takes it: trusted to +-1
    return Constants(t - 2, t + 3, BAND_LO <= E <= BAND_HI, E * (1.0 - BRACKET), E * (1.0 + BRACKET))


def tier(mant: int, e: int, neg: bool, E: float):
    """(tier name, decision) for the field mant x 10^e (mant < 10^15) under max_e_value E; decision None: left to the host."""
    assert 0 <= mant < 10 ** 15
    if mant == 0:
        return "zero", E >= 0.0
    if neg:
        return "negative", None
    c = constants(E)
    d = len(str(mant))
    if d + e <= c.k_keep:
        return "mag_keep", True
    if d - 1 + e >= c.k_drop:
        return "mag_drop", False
    m = float(mant)
    if -22 <= e <= 22:
        return "one_op", (m / P10[-e] if e < 0 else m * P10[e]) <= E
    if not c.band:
        return "ask_outside", None
    x = m
    r = e
    while r > 0:
        x *= P10[min(r, 22)]
        r -= 22
    r = -e
    while r > 0:
        x /= P10[min(r, 22)]
        r -= 22
    if x <= c.e_lo:
        return "band_keep", True
    if x >= c.e_hi:
        return "band_drop", False
    return "band_ask", None


# ---- thresholds ----------------------------------------------------------------------------------------------------------------
POWERS = (-280, -279, -100, -45, -44, -30, -23, -22, -5, -1, 0, 1, 5, 22, 23, 44, 100, 279, 280)
INF, NAN = float("inf"), float("nan")


def _families():
    f = {}
    f["powers_of_ten"] = [(f"1e{k}", float(f"1e{k}")) for k in POWERS]
    f["below_powers_of_ten"] = [(f"below_1e{k}", math.nextafter(float(f"1e{k}"), 0.0)) for k in POWERS]
    f["above_powers_of_ten"] = [(f"above_1e{k}", math.nextafter(float(f"1e{k}"), INF)) for k in POWERS]
    f["band_edges"] = [(s, float(s)) for s in ("2.5e-280", "9.9e-281", "4e279", "1.01e280", "3.7e-51", "0.001", "12345.678",
                                               "9.999999999999999e-31")]
    f["outside_band"] = [(s, float(s)) for s in ("5e-324", "1e-320", "2.2250738585072014e-308", "1e-308", "1e-300", "1e300",
                                                 "1.7976931348623157e308")]
    f["special"] = [("0.0", 0.0), ("-0.0", -0.0), ("inf", INF), ("nan", NAN), ("-1.0", -1.0), ("-inf", -INF)]
    return f


FAMILIES = _families()                                    # family -> [(name, E)]
THRESHOLDS = {name: E for fam in FAMILIES.values() for name, E in fam}
FAMILY_OF = {name: fam for fam, members in FAMILIES.items() for name, _ in members}
# the thresholds that also run in the general form and under the taxon-filter build: one per family
ALSO_GENERAL = {"powers_of_ten": "1e-30", "below_powers_of_ten": "below_1e44", "above_powers_of_ten": "above_1e-23",
                "band_edges": "3.7e-51", "outside_band": "1e-300", "special": "0.0"}


def finite_positive(E: float) -> bool:
    return 0.0 < E < INF


def decade(E: float) -> int:
    """floor(log10 E) of E as written: from its shortest spelling that reads back as E (repr), not from a logarithm.  (The
    double 1e-280 lies a little below 10^-280; its decade is -280 all the same.)"""
    return decimal.Decimal(repr(E)).adjusted()


# ---- fields ------------------------------------------------------------------------------------------------------------------------
ZEROS = ("0", "0.0", "-0", "0e-999", "0.000e5", "000")
NEGATIVES = ("-1", "-5", "-0.5", "-1e-50", "-3e-400")
OVER_UNDERFLOW = ("1e999", "9e308", "179769313486231e294", "1e-999", "2e-324", "3e-324", "5e-324", "1e-323", "494065645841246e-338")
COMMON = ZEROS + NEGATIVES + OVER_UNDERFLOW
WIDTHS = (1, 2, 3, 8, 14, 15)
OFFSETS = (0, 1, -1, 2, -2, 10, -10, 14, -14, 15, -15, 20, -20, 100, -100, 1000, -1000)
SPECIAL_DECADES = (-400, -330, -324, -323, -322, -321, -300, -23, -22, 0, 22, 23, 300, 308)

# One case: the field as written, what it decomposes to (ingest_edges.decompose), and the part of the recipe it comes from.
Field = collections.namedtuple("Field", "text neg mant e origin")


def _norm(mant: int, e: int):
    """(mant, e) with mant < 10^15, trailing zeros shed as far as that needs; None when it cannot be had (or mant <= 0)."""
    if mant <= 0:
        return None
    while mant >= 10 ** 15:
        if mant % 10:
            return None
        mant //= 10
        e += 1
    return mant, e


def rounded(E: float, d: int):
    """E as written (repr) rounded to d significant digits, half even: (mantissa of d digits, exponent)."""
    x = decimal.Decimal(repr(E))
    ex = x.adjusted() - (d - 1)
    m = int(x.scaleb(-ex).to_integral_value(rounding=decimal.ROUND_HALF_EVEN))
    return m, ex


def neighbours(E: float):
    """Around E on the d-digit grids: the rounded mantissa plus each offset; at every width from 1 to 15 the rounded mantissa
    itself (the threshold's own spellings); and, where the rounded mantissa is a power of ten, the ten times finer grid just
    below it too, since that is the d-digit grid there."""
    out = []
    for d in range(1, 16):
        m, ex = rounded(E, d)
        for off in (OFFSETS if d in WIDTHS else (0,)):
            out.append(_norm(m + off, ex))
            if d in WIDTHS and off > 0 and m == 10 ** (d - 1):
                out.append(_norm(10 ** d - off, ex - 1))
    return [x for x in out if x is not None]


def magnitude_boundaries(E: float, rng: random.Random):
    """10^(d-1), 10^d - 1 and one random d-digit mantissa with d + e = t - 5 .. t + 6: on, one below and one above both
    magnitude tests (k_keep = t - 2 on d + e, k_drop = t + 3 on d - 1 + e, that is t + 4 on d + e) with the host's t one
    decade to either side of this one as well, which is what "trusted to +-1" allows."""
    t = decade(E)
    out = []
    for d in WIDTHS:
        for mant in (10 ** (d - 1), 10 ** d - 1, rng.randrange(10 ** (d - 1), 10 ** d)):
            for s in range(t - 5, t + 7):
                out.append((mant, s - d))
    return out


def special_fields():
    out = []
    for k in SPECIAL_DECADES:
        out += [(1, k), (10 ** 15 - 1, k - 14)]
    return out


def spell(mant: int, e: int) -> str:
    return str(mant) if e == 0 else f"{mant}e{e}"


def respell(rng: random.Random, mant: int, e: int) -> str:
    """Another spelling of mant x 10^e that decomposes to the same (mant, e): the point moved (zeros behind a leading point
    counted, up to 15 digits in all), leading zeros in front of it free, `E`, `e+`, exponents padded to 2 and 3 digits.  After
    ingest_edges.random_spelling, without its cap on the net exponent."""
    s = str(mant)
    nd = len(s)
    k = rng.randrange(0, nd + 1)                                # digits before the point
    zeros = rng.randrange(0, 16 - nd) if k == 0 and rng.random() < 0.5 else 0
    ip, fp = s[:k], "0" * zeros + s[k:]
    if ip and rng.random() < 0.3:
        ip = "0" * rng.randrange(1, 5) + ip
    if not ip and rng.random() < 0.5:
        ip = "0"
    text = ip + ("." + fp if fp else ("." if rng.random() < 0.2 else ""))
    exp = e + len(fp)
    assert abs(exp) <= 999
    if exp != 0 or rng.random() < 0.5:
        digits = "%0*d" % (rng.choice((1, 2, 2, 3, 3)), abs(exp))
        text += rng.choice("eE") + ("-" if exp < 0 else rng.choice(("", "+"))) + digits
    return text


def _parsed(text: str, origin: str) -> Field:
    neg, mant, e, _, _, _ = IE.decompose(text.encode())
    return Field(text, neg, mant, e, origin)


@functools.lru_cache(maxsize=None)
def fields_for(name: str):
    """Every field of the threshold `name` in a fixed order: the common spellings as written, then each (mant, e) once."""
    E = THRESHOLDS[name]
    rng = random.Random(1000 + list(THRESHOLDS).index(name))
    out, seen = [], set()

    def add(f: Field):
        if (f.neg, f.mant, f.e) not in seen:
            seen.add((f.neg, f.mant, f.e))
            out.append(f)
    for text in COMMON:
        out.append(_parsed(text, "common"))
        seen.add((out[-1].neg, out[-1].mant, out[-1].e))
    if finite_positive(E):
        own = [("neighbour", p) for p in neighbours(E)] + [("magnitude", p) for p in magnitude_boundaries(E, rng)]
        for origin, (mant, e) in own:
            text = respell(rng, mant, e) if rng.random() < 0.1 else spell(mant, e)
            add(Field(text, False, mant, e, origin))
    else:
        for mant, e in special_fields():
            add(Field(spell(mant, e), False, mant, e, "special"))
    return tuple(out)


def expected_keep(text: str, E: float) -> bool:
    """The expected value: float() is correctly rounded, a NaN threshold compares false."""
    return float(text) <= E


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def table(texts, pad=0, eol=b"\n", open_tail=False, pid=None) -> bytes:
    """One line and one query (q%05d) per field; `pid`: per-line perc_identity (default: ingest_edges.line's)."""
    rows = []
    for i, t in enumerate(texts):
        kw = {} if pid is None else {"pid": pid[i]}
        rows.append(IE.line(b"q%05d" % i, b"NR_%06d.1" % (100 + i % 90), tax=100 + i % 90, pad=pad, e_value=t, **kw))
    return eol.join(rows) + (b"" if open_tail else eol)


def general_pad(n_lines: int) -> int:
    """Filler per line that puts a table's first parse block (256 lines, or all of a shorter table) beyond the 32768-byte
    stage: the general form of the parse kernel.  200 bytes when the block is full."""
    return 200 if n_lines >= IE.PARSE_BLOCK else IE.STAGE_BYTES // n_lines + 1


def kept_queries(texts, E: float, passes=None):
    """The queries of the kept lines, in file order: what `query_names` must be."""
    return [b"q%05d" % i for i, t in enumerate(texts) if expected_keep(t, E) and (passes is None or passes[i])]


@functools.lru_cache(maxsize=None)
def split(name: str):
    """(decided fields, asked fields) of a threshold, by the restatement."""
    E = THRESHOLDS[name]
    decided, asked = [], []
    for f in fields_for(name):
        (asked if tier(f.mant, f.e, f.neg, E)[1] is None else decided).append(f)
    return tuple(decided), tuple(asked)


# ---- the undecided list (list_undecided / apply_decisions run on 256-thread grids) -------------------------------------------------
LIST_E = 1e-30
LIST_LINES = 600
ASK_KEPT = ("1e-30", "1.0e-30", "10e-31")                  # inside the bracket; the host keeps them
ASK_DROPPED = "1.00000000000001e-30"                       # inside the bracket; the host drops it
DECIDED_KEPT, DECIDED_DROPPED = "1e-40", "3e-12"           # decided by the magnitude tests


def _list_positions(n: int, where: str):
    if where == "first":
        return [0]
    if where == "last":
        return [LIST_LINES - 1]
    if n == LIST_LINES:
        return list(range(LIST_LINES))
    return sorted(random.Random(n).sample(range(LIST_LINES), n))


# name -> (number of undecided lines, where, which undecided spellings)
LIST_CASES = {
    "one_first": (1, "first", "mixed"), "one_last": (1, "last", "mixed"),
    "n_255": (255, "spread", "mixed"), "n_256": (256, "spread", "mixed"), "n_257": (257, "spread", "mixed"),
    "all_mixed": (LIST_LINES, "all", "mixed"), "all_dropped": (LIST_LINES, "all", "dropped"),
}
LIST_LAYOUTS = {"lf": (b"\n", False), "crlf": (b"\r\n", False), "open_last_line": (b"\n", True)}
LIST_GENERAL = "n_257"                                      # the case that also runs in the general form,
LIST_PAD = 400                                              # with filler enough for its short last block (88 lines) too


def list_case(name: str):
    """The 600 fields of an undecided-list case."""
    n, where, which = LIST_CASES[name]
    at = set(_list_positions(n, where))
    texts, k = [], 0
    for i in range(LIST_LINES):
        if i in at:
            texts.append(ASK_DROPPED if which == "dropped" or k % 4 == 3 else ASK_KEPT[k % 4])
            k += 1
        else:
            texts.append(DECIDED_KEPT if i % 3 else DECIDED_DROPPED)
    return texts


# Lines that fail min_perc_identity and carry an undecidable e-value: never asked about.
PID_MIN = 97.0


def failing_pid_case():
    """(fields, perc_identity per line, passes min_perc_identity per line): every third line fails the identity threshold and
    is spelled like the e-value threshold; the other lines are decided by the magnitude tests."""
    texts, pid, passes = [], [], []
    for i in range(LIST_LINES):
        low = i % 3 == 0
        texts.append((ASK_KEPT + (ASK_DROPPED,))[(i // 3) % 4] if low else (DECIDED_KEPT if i % 2 else DECIDED_DROPPED))
        pid.append("96.999" if low else "99.356")
        passes.append(not low)
    return texts, pid, passes
