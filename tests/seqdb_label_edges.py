"""Byte-level edge inputs of `build-db sintax` and `build-db dada2`: no tests here, only the generator that
tests/test_seqdb_label_edges.py (the restatement alone, no GPU) and tests/test_gpu_seqdb_label_edges.py (seqdb_label_lines,
seqdb_label_ascii and seqdb_write_labelled of csrc/seqdb_gpu.hip) share.

The labelled formats read kraken2's three-piece listing, so a `LabelListing` is a kraken2 `Listing` of tests/seqdb_edges.py
(its pads and its input alignment) that follows the *labelled* output offset of one format instead: a line whose taxid has no
row or whose row has no label has no output bytes.  A case is one taxonomies document (by name, `document(name)`), one listing,
the formats it is meant for (a case placed on output offsets is one format's), its stated outcome and the marks the CPU test
recomputes from the bytes.  Offsets are those of the whole listing, which is one chunk at `chunk_bytes=8192` when it is shorter
than that.

Classes: A the kraken2 cases of tests/seqdb_edges.py against one document that writes, skips for an unknown taxid and skips for
an empty label; B where a byte >= 0x80 lies for seqdb_label_ascii; C lines without bytes for seqdb_write_labelled; D the counts
after a bad line.  The generator writes its own bytes and imports neither the package nor the restatement."""
from __future__ import annotations

import functools
from typing import Dict, List, NamedTuple, Optional, Tuple

from tests import seqdb_edges as E
from tests.seqdb_edges import SLICE, TILE, Case, Listing, seq      # noqa: F401  (Case: what class A is made from)

SINTAX, DADA2 = "sintax", "dada2"
FORMATS = (SINTAX, DADA2)
BOTH = FORMATS
PIECES, NONASCII, TAXID = E.PIECES, E.NONASCII, E.TAXID
PROBE = "é".encode("utf-8")                 # C3 A9
PROBE4 = b"\xf0\x9f\xa6\xa0"
SHORTEST = {SINTAX: 13, DADA2: 5}           # `>A;tax=d:x;\n\n` and `>x;\n\n`

# the edge document: taxid -> bytes of its identifier under `d`; 8 has a row without a label, 9 has no row
IDENT = {1: 1, 2: 13, 3: 14, 4: 15, 5: 16, 6: 17, 7: 300, 10: 5000, 11: 9000}
UNLABELLED, UNKNOWN = 8, 9
WRITTEN, SKIP_U, SKIP_N = "written", "unknown", "unlabelled"
KINDS = (WRITTEN, SKIP_U, SKIP_N)
TAX_OF = {WRITTEN: b"1", SKIP_U: b"%d" % UNKNOWN, SKIP_N: b"%d" % UNLABELLED}
MIX = (WRITTEN, SKIP_U, WRITTEN, SKIP_N, SKIP_N, SKIP_U, WRITTEN, WRITTEN, SKIP_U)


class LabelCase(NamedTuple):
    name: str
    cls: str                             # "A", "B1" ... "D"
    doc: str                             # document(doc)
    fmts: Tuple[str, ...]
    listing: bytes
    outcome: tuple                       # ("ok",), ("stop", line) or ("error", line, reason)
    marks: Dict[str, list]
    min_chunks: Dict[int, int] = {}      # chunk_bytes -> the least number of chunks the reader must make of it
    at_default: bool = False             # position-critical and not one chunk at 8192: the default chunk size too


# ---- the documents -----------------------------------------------------------------------------------------------------
def _document(rows) -> dict:
    """rows: (taxid, textLineage)"""
    return {"blutilsVersion": "8.3.1", "sourceDatabase": "db", "taxonomies": [
        {"taxid": t, "rank": "s", "numericLineage": f"d__{t}", "textLineage": lin, "accessions": []} for t, lin in rows]}


def ident(n: int) -> str:
    return "x" if n == 1 else "L" + "m" * (n - 2) + "R"


NO_LABEL_ROWS = [(t, f"no-rank__cellular-organisms;superkingdom__bacteria;clade__c{t}") for t in range(1, 51)]


@functools.lru_cache(maxsize=None)
def document(name: str) -> dict:
    if name == "corpus":                 # 1 ... 3999: a multiple of 3 has no label, another multiple of 5 no row
        return _document([(t, "clade__x" if t % 3 == 0 else f"d__t{t};p__p{t % 7}") for t in range(1, 4000) if t % 3 == 0 or t % 5])
    if name == "edges":
        return _document(sorted([(t, "d__" + ident(n)) for t, n in IDENT.items()] + [(UNLABELLED, "clade__x")]))
    if name == "no_label":               # what dada2 gets from a database built without `-r superkingdom=d`; no kind for sintax either
        return _document(NO_LABEL_ROWS)
    if name == "no_label_but_the_last":
        return _document(NO_LABEL_ROWS + [(51, "d__last;p__one")])
    raise KeyError(name)


def label_len(fmt: str, taxid: int) -> int:
    """Bytes of the label of a row of the edge document: `d:IDENT` or `IDENT;`; 0 for a line that is skipped."""
    n = IDENT.get(taxid)
    return 0 if n is None else n + (2 if fmt == SINTAX else 1)


def record_len(fmt: str, acc_n: int, taxid: int, seq_n: int) -> int:
    """`>ACC;tax=LABEL;\\nSEQ\\n` or `>LABEL\\nSEQ\\n`"""
    lab = label_len(fmt, taxid)
    return 0 if not lab else (acc_n + 9 if fmt == SINTAX else 3) + lab + seq_n


class LabelListing(Listing):
    """Three-piece lines against the edge document.  out_fmt: the format whose output offset `lout` follows (None: the
    listing is meant for both and nothing is placed on output offsets)."""

    def __init__(self, out_fmt: Optional[str] = None, seed: int = 0):
        super().__init__(E.K, seed)
        self.out_fmt, self.lout = out_fmt, 0

    def rec(self, acc: bytes, tax: bytes, sq: bytes, oid: bytes = b"0", end: bytes = b"\n") -> int:
        start = self.lout
        self.buf += b"  ".join([acc, tax, sq]) + end
        if self.out_fmt:
            self.lout += record_len(self.out_fmt, len(acc), int(tax), len(sq))
        return start

    def raw(self, text: bytes):
        """Whole lines that have no output bytes: skipped, refused, or behind a refused one."""
        self.buf += text

    def good(self, n: int = 1):
        for _ in range(n):
            kind = MIX[self.k % len(MIX)]
            self.rec(self.name(), TAX_OF[kind] if kind != WRITTEN else b"%d" % (1 + self.k % 6), seq(self.k % 23, self.k))

    def lines_before(self) -> int:
        return bytes(self.buf).count(b"\n")

    # ---- output offsets
    def short(self) -> int:
        return self.rec(b"A", b"1", b"")

    def filler(self, n: int) -> int:
        """One record of n output bytes."""
        assert n >= SHORTEST[self.out_fmt], n
        return self.rec(b"F", b"1", seq(n - SHORTEST[self.out_fmt], self.k))

    def out_align(self, off: int, mod: int, r: int):
        """One filler record so that output byte `off` of the next record lies at an output offset that is r modulo mod."""
        gap = (r - self.lout - off) % mod
        while 0 < gap < SHORTEST[self.out_fmt]:
            gap += mod
        if gap:
            self.filler(gap)
        assert (self.lout + off) % mod == r % mod

    def done(self, name: str, cls: str, outcome: tuple = ("ok",), doc: str = "edges", **kw) -> LabelCase:
        return LabelCase(name, cls, doc, (self.out_fmt,) if self.out_fmt else BOTH, bytes(self.buf), outcome, dict(self.marks), **kw)


# ---- A: the §11 corpus ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus() -> List[LabelCase]:
    """Every kraken2 case of tests/seqdb_edges.py, as it is, against the corpus document."""
    cases = [("accepted", E.accepted(c, E.K)) for c, (_, fmts) in E.ACCEPTED.items() if E.K in fmts]
    cases += [("small", c) for c in E.small(E.K)] + [("cuts", c) for c in E.cuts(E.K)]
    cases += [(fn.__name__, c) for fn in (E.stops, E.precedence, E.refused) for c in fn() if c.fmt == E.K]
    return [LabelCase(f"{o}/{c.name}", "A", "corpus", BOTH, c.listing, c.outcome, {**c.marks, "origin": [o]}, c.min_chunks) for o, c in cases]


# ---- B: seqdb_label_ascii ------------------------------------------------------------------------------------------------
PLACES = ("first", "last", "middle")
RESIDUES = list(range(SLICE)) + ["tile"]                 # the probe's first byte at k modulo 16; at 4095 modulo 4096


def _at(L: LabelListing, off: int, k):
    if k == "tile":
        L.before_tile(off, 1)
    else:
        L.align(off, SLICE, k)


def _probe_line(acc: bytes, kind: str, place: str, probe: bytes) -> Tuple[bytes, int]:
    """A line whose sequence holds the probe as its first bytes, its last bytes or in its middle; the probe's offset in it."""
    sq = {"first": probe + b"ACGT", "last": b"ACGT" + probe, "middle": b"AC" + probe + b"GT"}[place]
    head = acc + b"  " + TAX_OF[kind] + b"  "
    return head + sq + b"\n", len(head) + sq.index(probe)


@functools.lru_cache(maxsize=None)
def b1_refused() -> List[LabelCase]:
    out = []
    def one(k, place, kind, probe, tag):
        L = LabelListing()
        L.good(6)
        line, off = _probe_line(L.name(), kind, place, probe)
        _at(L, off, k)
        L.marks["probe"].append((L.pos + off, len(probe), kind, place))
        n = L.lines_before() + 1
        L.raw(line)
        L.good(3)
        out.append(L.done(f"{tag}-{k}-{place}-{kind}", "B1", ("error", n, NONASCII)))
    for i, k in enumerate(RESIDUES):
        for p, place in enumerate(PLACES):
            one(k, place, KINDS[(i + p) % 3], PROBE, "probe")
    for i, k in enumerate((13, 14, 15)):                          # four bytes over two threads
        one(k, "middle", KINDS[i % 3], PROBE4, "probe4")
    for i, d in enumerate((3, 2, 1)):                             # ... and over two blocks: the first byte 3, 2, 1 before 4096 k
        L = LabelListing()
        L.good(6)
        line, off = _probe_line(L.name(), KINDS[i], "middle", PROBE4)
        L.before_tile(off, d)
        L.marks["probe"].append((L.pos + off, 4, KINDS[i], "middle"))
        n = L.lines_before() + 1
        L.raw(line)
        L.good(3)
        out.append(L.done(f"probe4-tile{d}-middle-{KINDS[i]}", "B1", ("error", n, NONASCII)))
    return out


@functools.lru_cache(maxsize=None)
def b2_accepted() -> LabelCase:
    """High bytes outside the sequence piece: the last bytes of the accession, a fourth piece directly behind a third
    separator, and a fourth piece behind a tab that the sequence's trim removes; each at every residue."""
    L = LabelListing()
    L.good(3)
    for i, k in enumerate(RESIDUES):
        for j, where in enumerate(("accession", "fourth", "fourth_after_tab")):
            kind = KINDS[(i + j) % 3]
            acc = L.name()
            if where == "accession":
                line, off = acc + PROBE + b"  " + TAX_OF[kind] + b"  ACGT\n", len(acc)
            elif where == "fourth":
                head = acc + b"  " + TAX_OF[kind] + b"  ACGT  "
                line, off = head + PROBE + b"\n", len(head)
            else:
                head = acc + b"  " + TAX_OF[kind] + b"  ACGT\t  x"
                line, off = head + PROBE + b"y\n", len(head)
            _at(L, off, k)
            L.marks["probe"].append((L.pos + off, 2, kind, where))
            L.raw(line)
    L.good(2)
    return L.done("accepted_high_bytes", "B2", at_default=True)           # three multiples of 4096: 12 KB


# B3: patterns of short lines; `bad` is the index of the one line whose sequence holds the probe
def _b3_patterns():
    acc_ok = lambda t: PROBE + b"  " + t + b"  A\n"               # 9 bytes, the probe in the accession
    plain = lambda t: b"a  " + t + b"  AC\n"                      # 9 bytes
    bad9 = lambda t: b"a  " + t + b"  " + PROBE + b"\n"           # 9 bytes, the probe is the sequence
    bad8 = lambda t: b"  " + t + b"  " + PROBE + b"\n"            # 8 bytes: an empty accession
    empty = lambda t: b"a  " + t + b"  \n"                        # 7 bytes: an empty sequence
    out = {}
    for j in range(16):       # sixteen consecutive 9-byte lines from offset 0 modulo 16: line j starts at 9 j modulo 16
        out[f"later-{j}"] = ([acc_ok] * j + [bad9] + [acc_ok] * (15 - j), j, 0)
        out[f"first_only-{j}"] = ([plain] * j + [bad9] + [plain] * (15 - j), j, 0)
    for ph in range(16):      # shorter spellings at every phase: 8 + 8 bytes; 7 + 8 + 7 bytes (three line starts in a slice)
        out[f"short-{ph}"] = ([lambda t: PROBE + b"  " + t + b"  \n", bad8, plain], 1, ph)
        out[f"three-{ph}"] = ([empty, bad8, empty, plain], 1, ph)
    return out


@functools.lru_cache(maxsize=None)
def b3_several_lines_in_a_slice() -> List[LabelCase]:
    out = []
    for i, (name, (lines, bad, ph)) in enumerate(_b3_patterns().items()):
        L = LabelListing()
        L.good(4)
        L.align(0, SLICE, ph)
        n0 = L.lines_before()
        for j, make in enumerate(lines):
            kind = KINDS[(i + j) % 3]
            text = make(TAX_OF[kind])
            if j == bad:
                L.marks["probe"].append((L.pos + text.index(PROBE), 2, kind, "sequence"))
            L.marks["short_line"].append((L.pos, len(text)))
            L.raw(text)
        L.good(2)
        out.append(L.done(name, "B3", ("error", n0 + bad + 1, NONASCII)))
    return out


EOF_SIZES = [(SLICE, 1), (SLICE, 2), (SLICE, 15), (SLICE, 0), (TILE, 1), (TILE, 0)]


@functools.lru_cache(maxsize=None)
def b4_end_of_file() -> List[LabelCase]:
    """An open last line whose last two bytes are the probe, in its sequence; the same with a final newline."""
    out = []
    for i, (mod, s) in enumerate(EOF_SIZES):
        for end in (b"", b"\n"):
            L = LabelListing()
            L.good(5)
            line = b"Z  " + TAX_OF[KINDS[i % 3]] + b"  AC" + PROBE + end
            L.align(len(line), mod, s)
            L.marks["probe"].append((L.pos + len(line) - len(end) - 2, 2, KINDS[i % 3], "last"))
            n = L.lines_before() + 1
            L.raw(line)
            L.marks["size"].append((mod, s))
            out.append(L.done(f"size_{s}_mod_{mod}-{'newline' if end else 'open'}", "B4", ("error", n, NONASCII)))
    return out


def _body(L: LabelListing, size: int):
    end = L.pos + size
    while L.pos < end:
        L.good(1)


def _bad_line(what: str, kind: str = WRITTEN) -> bytes:
    t = TAX_OF[kind]
    return {NONASCII: b"B  " + t + b"  AC" + PROBE + b"GT\n", PIECES: b"B  " + t + b" ACGT\n", TAXID: b"B  x" + t + b"  ACGT\n",
            "stop": b"B  " + t + b"  AC\xffGT\n"}[what]


@functools.lru_cache(maxsize=None)
def b5_first_of_two() -> List[LabelCase]:
    """Line 3 is bad and so is a line more than 4096 bytes later: another block of one chunk at 8192, another chunk at 4096."""
    out = []
    for first, second in ((NONASCII, NONASCII), (NONASCII, PIECES), (PIECES, NONASCII), (NONASCII, "stop"), ("stop", NONASCII)):
        L = LabelListing()
        L.good(2)
        L.marks["bad"].append(L.pos)
        L.raw(_bad_line(first, SKIP_U))
        _body(L, 4200)
        L.marks["bad"].append(L.pos)
        L.raw(_bad_line(second, SKIP_N))
        L.good(2)
        out.append(L.done(f"{first}_then_{second}", "B5", ("stop", 3) if first == "stop" else ("error", 3, first)))
    return out


@functools.lru_cache(maxsize=None)
def b6_precedence() -> List[LabelCase]:
    out = []
    for name, lines, reason in (("nonascii_then_pieces", [_bad_line(NONASCII), _bad_line(PIECES)], NONASCII),
                                ("pieces_then_nonascii", [_bad_line(PIECES), _bad_line(NONASCII)], PIECES),
                                ("only_the_probe", [PROBE + b"\n"], PIECES)):
        L = LabelListing()
        L.good(1)
        L.raw(b"".join(lines))
        L.good(2)
        out.append(L.done(name, "B6", ("error", 2, reason)))
    return out


# ---- C: seqdb_write_labelled ---------------------------------------------------------------------------------------------
def _skip_line(i: int) -> bytes:
    return b"a  %d  A\n" % (UNKNOWN, UNLABELLED)[i % 2]           # 8 bytes, unknown and unlabelled alternating


def _ordinary(L: LabelListing):
    L.rec(L.name(), b"%d" % (2 + L.k % 5), seq(20 + L.k % 30, L.k))


@functools.lru_cache(maxsize=None)
def c1_tiny_records(fmt: str) -> List[LabelCase]:
    """48 shortest records, the first `>` at output offset 4095 and at 0 modulo 4096."""
    out = []
    for r in (TILE - 1, 0):
        L = LabelListing(fmt)
        _ordinary(L)
        L.out_align(0, TILE, r)
        for _ in range(48):
            L.marks["tiny"].append(L.short())
        _ordinary(L)
        out.append(L.done(f"tiny_from_{r}-{fmt}", "C1"))
    return out


RUNS = (1, 2, 3, 15, 16, 17, 255, 256, 257, 4100)
DS = (-2, -1, 0, 1)


def _skipped_run(L: LabelListing, mod: int, d: int, r: int):
    """A written record that ends d bytes behind a multiple of mod (its last byte at d - 1), r skipped lines, a shortest record,
    an ordinary one."""
    acc, tax, sq = L.name(), b"%d" % (2 + L.k % 5), seq(L.k % 19, L.k)
    L.out_align(record_len(L.out_fmt, len(acc), int(tax), len(sq)), mod, d)
    L.rec(acc, tax, sq)
    L.marks["skipped_run"].append((L.lout, r, mod, L.lines_before()))
    L.raw(b"".join(_skip_line(i) for i in range(r)))
    L.short()
    _ordinary(L)


@functools.lru_cache(maxsize=None)
def c2_skipped_runs(fmt: str) -> List[LabelCase]:
    out = []
    L = LabelListing(fmt)                                         # modulo 16, short runs: one listing
    for r in RUNS[:6]:
        for d in DS:
            _skipped_run(L, SLICE, d, r)
    out.append(L.done(f"runs_to_17_mod_16-{fmt}", "C2"))
    for d in DS:                                                  # 255 ... 257: one listing per d
        L = LabelListing(fmt)
        for r in RUNS[6:9]:
            _skipped_run(L, SLICE, d, r)
        out.append(L.done(f"runs_255_to_257_mod_16_d{d}-{fmt}", "C2"))
    for d in DS:                                                  # 4100 lines: more than 16 blocks of the line kernel
        L = LabelListing(fmt)
        _ordinary(L)
        _skipped_run(L, SLICE, d, 4100)
        out.append(L.done(f"run_4100_mod_16_d{d}-{fmt}", "C2", at_default=True))
    for r in RUNS[:9]:                                            # modulo 4096: one listing each
        for d in DS:
            L = LabelListing(fmt)
            _ordinary(L)
            _skipped_run(L, TILE, d, r)
            out.append(L.done(f"run_{r}_mod_4096_d{d}-{fmt}", "C2"))
    return out


def _line(i: int, kind: str) -> bytes:
    return b"a%03d  %s  %s\n" % (i, TAX_OF[kind] if kind != WRITTEN else b"%d" % (1 + i % 6), seq(3 + i % 5, i))


@functools.lru_cache(maxsize=None)
def c3_ends_of_a_chunk() -> List[LabelCase]:
    out = []
    def case(name, kinds, newline=True):
        L = LabelListing()
        text = b"".join(_line(i, k) for i, k in enumerate(kinds))
        L.raw(text if newline else text[:-1])
        L.marks["kinds"].append(tuple(kinds))
        out.append(L.done(name, "C3"))
    skip = lambda n: [(SKIP_U, SKIP_N)[i % 2] for i in range(n)]
    for n in (1, 256, 257):
        case(f"first_{n}_skipped", skip(n) + [WRITTEN] * 20)
        case(f"last_{n}_skipped", [WRITTEN] * 20 + skip(n))
        case(f"last_{n}_skipped_open", [WRITTEN] * 20 + skip(n), newline=False)
    case("only_the_first_written", [WRITTEN] + skip(299))
    case("only_the_last_written", skip(299) + [WRITTEN])
    case("only_the_last_written_open", skip(299) + [WRITTEN], newline=False)
    case("only_line_257_written", skip(256) + [WRITTEN] + skip(143))
    return out


TOTALS = (5, 13, 15, 16, 17, 4095, 4096, 4097, 8192, 8193)


@functools.lru_cache(maxsize=None)
def c4_totals(fmt: str) -> List[LabelCase]:
    """Outputs of exactly that many bytes: pad records (one, or one and a shortest), then skipped lines up to the end."""
    out = []
    for total in TOTALS:
        if total < SHORTEST[fmt]:
            continue
        L = LabelListing(fmt)
        L.raw(_skip_line(0))
        if total >= 2 * SHORTEST[fmt]:
            L.filler(total - SHORTEST[fmt])
            L.raw(_skip_line(1))
            L.short()
        else:
            L.filler(total)
        L.raw(b"".join(_skip_line(i) for i in range(3)))
        L.marks["total"].append(total)
        out.append(L.done(f"output_of_{total}_bytes-{fmt}", "C4", at_default=L.pos >= 8192))
    return out


LONG_AT = tuple(range(4090, 4098))


@functools.lru_cache(maxsize=None)
def c5_long_pieces(fmt: str) -> List[LabelCase]:
    """A label of 5000 and of 9000 bytes (sintax: an accession of 5000 bytes too) whose first byte lies at output offset
    4090 ... 4097 modulo 4096, followed directly by a shortest record."""
    out = []
    for what in ("label_5000", "label_9000") + (("accession_5000",) if fmt == SINTAX else ()):
        for at in LONG_AT:
            L = LabelListing(fmt)
            _ordinary(L)
            acc = b"Q" * 5000 if what == "accession_5000" else L.name()
            tax = {"label_5000": b"10", "label_9000": b"11", "accession_5000": b"3"}[what]
            off = 1 if fmt == DADA2 or what == "accession_5000" else 1 + len(acc) + 5
            L.out_align(off, TILE, at)
            L.marks["long"].append((L.lout + off, 5000 if what != "label_9000" else 9000, what))
            L.rec(acc, tax, seq(7, at))
            L.marks["tiny"].append(L.short())
            _ordinary(L)
            out.append(L.done(f"{what}_at_{at}-{fmt}", "C5", at_default=L.pos >= 8192))
    return out


@functools.lru_cache(maxsize=None)
def c6_no_label() -> List[LabelCase]:
    """400 lines over taxids 1 ... 60 against 50 rows none of which has a label, and against the same rows and one labelled
    row behind them (taxid 51)."""
    listing = b"".join(b"n%d  %d  %s\n" % (i, 1 + (i * 7) % 60, seq(10 + i % 13, i)) for i in range(400))
    marks = {"taxids": [1 + (i * 7) % 60 for i in range(400)]}
    return [LabelCase("no_row_has_a_label", "C6", "no_label", BOTH, listing, ("ok",), marks),
            LabelCase("only_the_last_row_has_a_label", "C6", "no_label_but_the_last", BOTH, listing, ("ok",), marks)]


# ---- D: counts stop at the bad line --------------------------------------------------------------------------------------
D_REASONS = (PIECES, NONASCII, TAXID, "stop")
D_PLACES = ("line_1", "line_257", "last_of_a_chunk", "first_of_the_next_chunk")


def _mixed(n: int, total: Optional[int] = None, salt: int = 0) -> bytes:
    """n lines of all three kinds; of total bytes in all when that is given (the sequences make the length)."""
    fixed = [len(b"h%d  %s  \n" % (i, TAX_OF[MIX[(i + salt) % 9]])) for i in range(n)]
    extra = [3 + i % 4 for i in range(n)]
    if total is not None:
        rest = total - sum(fixed)
        assert rest >= n
        extra = [rest // n + (1 if i < rest % n else 0) for i in range(n)]
    return b"".join(b"h%d  %s  %s\n" % (i, TAX_OF[MIX[(i + salt) % 9]], seq(extra[i], i)) for i in range(n))


@functools.lru_cache(maxsize=None)
def d_counts() -> List[LabelCase]:
    """A head of mixed lines, one bad line, a tail of 300 mixed lines that share the bad line's chunk.  The counts are the head's."""
    out = []
    for what in D_REASONS:
        for place in D_PLACES:
            bad = _bad_line(what, SKIP_U)
            head = {"line_1": b"", "line_257": _mixed(256), "last_of_a_chunk": _mixed(300, TILE - len(bad)),
                    "first_of_the_next_chunk": _mixed(300, TILE)}[place]
            L = LabelListing()
            L.raw(head)
            n_head = L.lines_before()
            L.marks["bad"].append((L.pos, len(bad)))
            L.marks["head"].append(tuple(sum(MIX[i % 9] == k for i in range(n_head)) for k in KINDS))
            L.raw(bad + _mixed(300, salt=4))
            out.append(L.done(f"{what}-{place}", "D", ("stop", n_head + 1) if what == "stop" else ("error", n_head + 1, what)))
    return out


@functools.lru_cache(maxsize=None)
def edge_cases() -> List[LabelCase]:
    """Classes B, C and D."""
    out = b1_refused() + [b2_accepted()] + b3_several_lines_in_a_slice() + b4_end_of_file() + b5_first_of_two() + b6_precedence()
    for fmt in FORMATS:
        out += c1_tiny_records(fmt) + c2_skipped_runs(fmt)
    out += c3_ends_of_a_chunk()
    for fmt in FORMATS:
        out += c4_totals(fmt) + c5_long_pieces(fmt)
    return out + c6_no_label() + d_counts()
