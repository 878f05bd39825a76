"""Byte-level edge inputs of `build-db kraken2` and `build-db qiime2`: no tests here, only the generator
that tests/test_seqdb_edges.py (the restatement alone, no GPU) and tests/test_gpu_seqdb_edges.py (csrc/seqdb_gpu.hip) share.

A `Listing` writes whole lines and knows its file offset, so that a case can be put where the kernels' geometry lies: a run
of spaces starting at a given offset modulo 16 (one thread's bytes) or a few bytes before a multiple of 4096 (one block's
tile), a character split across such a boundary, a record boundary at a given *output* offset.  The gap before a case is
filled with pad lines, well-formed records of their own whose accession is `P`, `Px`, `Pxx`, ...  Every case leaves a mark
(its kind and its offsets) that the CPU test checks on the bytes and on the restatement's output.  Offsets are those of the
whole listing, which is one chunk with `chunk_bytes=0`.

Accepted cases of one class share one listing (`accepted(cls, fmt, seed, lead)`); small listings whose property is their
size or their end (`small(fmt)`), the chunk-cut listings (`cuts(fmt)`) and the refused or stopped ones (`stops()`,
`refused()`, `precedence()`) are lists of `Case`.  A refused case states its outcome, ("stop", line) or ("error", line,
reason); the CPU test holds the restatement to it.  The generator writes its own bytes throughout and imports neither the
package nor the restatement."""
from __future__ import annotations

import collections
import functools
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

K, Q = "kraken2", "qiime2"
FORMATS = (K, Q)
SLICE, TILE = 16, 4096                  # bytes per thread and per block of the byte kernels and of the .fna writer
MINPAD = 12                             # the shortest pad line both formats can spell, and a little more
MINOUT = 20                             # ... and the shortest pad record
PIECES, NONASCII, TAXID = "pieces", "nonascii", "taxid"     # the reasons of an error, in the order a line is checked
CHUNKS = (4096, 8192, 0)

VALID = [chr(c).encode("utf-8") for c in (0x80, 0x7FF, 0x800, 0xD7FF, 0xE000, 0xFFFF, 0x10000, 0x10FFFF)]
INVALID = {"lone_80": b"\x80", "lone_bf": b"\xbf", "c0": b"\xc0\x80", "c1": b"\xc1\xbf", "e0_80": b"\xe0\x80\x80", "e0_9f": b"\xe0\x9f\xbf",
           "f0_80": b"\xf0\x80\x80\x80", "f0_8f": b"\xf0\x8f\xbf\xbf", "ed_a0": b"\xed\xa0\x80", "ed_bf": b"\xed\xbf\xbf",
           "f4_90": b"\xf4\x90\x80\x80", "f4_bf": b"\xf4\xbf\xbf\xbf", "f5": b"\xf5\x80\x80\x80", "f8": b"\xf8\x88\x80\x80\x80", "fe": b"\xfe",
           "ff": b"\xff", "fourth_continuation": b"\xf0\x9f\xa6\xa0\x80",
           # a lead byte whose continuation bytes are cut short by whatever follows: a letter, the newline or the end of the file
           "cut2": b"\xc2", "cut3": b"\xe2\x82", "cut3_1": b"\xe2", "cut4": b"\xf0\x9f\xa6", "cut4_2": b"\xf0\x9f", "cut4_1": b"\xf0"}


class Case(NamedTuple):
    name: str
    fmt: str
    listing: bytes
    outcome: tuple                       # ("ok",), ("stop", line) or ("error", line, reason)
    marks: Dict[str, list]
    min_chunks: Dict[int, int] = {}      # chunk_bytes -> the least number of chunks the reader must make of it


def seq(n: int, k: int = 0) -> bytes:
    return (b"acgtRYKMswbdhvNn" * (n // 16 + 2))[k % 16:k % 16 + n]


def n_pieces(fmt: str) -> int:
    return 3 if fmt == K else 4


class Listing:
    def __init__(self, fmt: str, seed: int = 0, lead: int = 0):
        self.fmt, self.seed = fmt, seed
        self.buf = bytearray()
        self.out: Optional[int] = 0      # the output offset, while only rec() has written (None afterwards)
        self.marks: Dict[str, list] = collections.defaultdict(list)
        self.k = 0
        if lead:
            self.pad(lead)

    @property
    def pos(self) -> int:
        return len(self.buf)

    def name(self) -> bytes:
        self.k += 1
        return b"A%d.%d" % (self.k, self.seed)

    def raw(self, text: bytes):
        """Whole lines as they are; the output offset is not followed past them."""
        self.buf += text
        self.out = None

    def rec(self, acc: bytes, tax: bytes, sq: bytes, oid: bytes = b"0", end: bytes = b"\n") -> int:
        """A plainly spelled line (pieces without blanks around them); returns the output offset of its record."""
        start = self.out
        self.buf += b"  ".join([acc, tax, sq] if self.fmt == K else [acc, tax, oid, sq]) + end
        if self.out is not None:
            self.out += self.header(acc, tax, oid) + len(sq) + ((len(sq) - 1) // 80 if sq and self.fmt == K else 0) + 1
        return start

    def header(self, acc: bytes, tax: bytes, oid: bytes = b"0") -> int:
        """Bytes of `>kraken:taxid|TAX|ACC\\n` or `>TAX-OID-ACC\\n`."""
        return 14 + len(tax) + 1 + len(acc) + 1 if self.fmt == K else 1 + len(tax) + 1 + len(oid) + 1 + len(acc) + 1

    def good(self, n: int = 1):
        for _ in range(n):
            self.rec(self.name(), b"%d" % (self.k + 1), seq(20 + self.k % 50, self.k + self.seed))

    # ---- input offsets
    def pad(self, n: int):
        """Pad lines of n bytes in all (n >= MINPAD), none longer than 300."""
        assert n >= MINPAD, n
        fixed = 7 if self.fmt == K else 10                               # "  1  a\n", "  1  0  a\n"
        while n:
            m = n if n < 300 else 150
            self.rec(b"P" + b"x" * (m - fixed - 1), b"1", b"a")
            n -= m

    def align(self, off: int, mod: int, r: int):
        """Pads so that the byte `off` bytes into the next line lies at an offset that is r modulo mod."""
        gap = (r - self.pos - off) % mod
        while 0 < gap < MINPAD:
            gap += mod
        if gap:
            self.pad(gap)
        assert (self.pos + off) % mod == r % mod

    def to(self, offset: int):
        """Pads up to that offset."""
        if offset != self.pos:
            self.pad(offset - self.pos)

    def before_tile(self, off: int, d: int):
        """... d bytes before a multiple of 4096 (at it, for d = 0; after it, for d < 0)."""
        self.align(off, TILE, -d)

    # ---- output offsets
    def out_pad(self, n: int):
        """Pad records of n output bytes in all (n >= MINOUT): empty sequences, the accession makes the length."""
        assert n >= MINOUT, n
        fixed = self.header(b"", b"1") + 1
        while n:
            m = n if n < 300 else 150
            self.rec(b"P" + b"x" * (m - fixed - 1), b"1", b"")
            n -= m

    def out_align(self, off: int, mod: int, r: int):
        """Pads so that output byte `off` of the next record lies at an output offset that is r modulo mod."""
        gap = (r - self.out - off) % mod
        while 0 < gap < MINOUT:
            gap += mod
        if gap:
            self.out_pad(gap)
        assert (self.out + off) % mod == r % mod

    def case(self, name: str, outcome: tuple = ("ok",), **kw) -> Case:
        return Case(name, self.fmt, bytes(self.buf), outcome, dict(self.marks), **kw)


# ---- class 1: separator parity ---------------------------------------------------------------------------------------------
SHORT_RUNS = list(range(1, 41))
LONG_RUNS = list(range(4094, 4101)) + list(range(8190, 8195))         # at most three tiles: spaces_before is linear per thread
WHERE = ("acc_taxid", "before_seq", "after_seq")
PLACES = ("front", "after_seq")             # front: between accession and taxid, or before the sequence where kraken2 needs a number


def run_line(fmt: str, where: str, n: int, name: bytes) -> Optional[Tuple[bytes, bytes]]:
    """(the text before a run of n spaces, the text after it) of a line both formats accept, or None where they do not.
    Between accession and taxid the parity of n decides which piece is which: qiime2 copies whatever results (`A` and four
    spaces: an empty taxid, the rest moves up); kraken2 needs a number there, which holds for n <= 3."""
    if where == "acc_taxid":
        if fmt == Q:
            return name, b"T7  O8  Sacgt  Xtra  Y  Z\n"
        return (name, b"7  8  acgt  9  c\n") if n <= 3 else None
    if where == "before_seq":                                    # n = 1: "7 acgt" (kraken2: no number), "0 acgt" (an oid as good as any)
        if fmt == Q:
            return name + b"  7  0", b"acgt  c  d\n"
        return (name + b"  7", b"acgt  c\n") if n >= 2 else None
    mid = b"  7  acgt" if fmt == K else b"  7  0  acgt"         # one space stays inside the sequence, two or more end it
    return name + mid, b"tail  x\n"


def _put_run(L: Listing, where: str, n: int, place) -> bool:
    parts = run_line(L.fmt, where, n, L.name())
    if parts is None:
        return False
    place(len(parts[0]))
    L.marks["run"].append((L.pos + len(parts[0]), n, where))
    L.raw(parts[0] + b" " * n + parts[1])
    return True


def parity_short(L: Listing):
    """Runs of 1..40 spaces at the three places, each starting at every offset modulo 16; blanks of every kind around the
    pieces, and pieces that are blanks only."""
    for n in SHORT_RUNS:
        for r in range(SLICE):
            for where in WHERE:
                _put_run(L, where, n, lambda off: L.align(off, SLICE, r))
    k, q = L.fmt == K, L.fmt == Q
    L.marks["blanks"].append(L.pos)
    L.raw(b"\tB1\x0b  \x0c7\r  " + (b"" if k else b"\x0b0\t  ") + b"\tac gt\x0b \r\n")
    L.raw(b" \x0b \x0c  7  " + (b"" if k else b"\t \x0b  ") + b"acgt\n")            # the accession (and the oid) blanks only
    L.raw(b"B3  \r7\t  " + (b"" if k else b"9  ") + b"\t \x0b \x0c\r\n")              # the sequence blanks only: empty
    L.raw(b" B4 \t  7  " + (b"" if k else b"9  ") + b"\x0cac\tgt  \x0b  \x0b\n")     # blanks inside the sequence stay
    L.good(2)


def _put_at(L: Listing, place: str, n: int, put):
    """The run at that place; `front` is between accession and taxid, and before the sequence where that is refused
    (kraken2 and n > 3: the taxid would be empty).  One space before a kraken2 sequence is refused too: n = 1 has no front
    place but the first."""
    for where in (("acc_taxid", "before_seq") if place == "front" else (place,)):
        if _put_run(L, where, n, put):
            return
    raise AssertionError((L.fmt, place, n))


def parity_tile(L: Listing, place: str, lengths):
    """Each of those short runs beginning 0, 1, 2 and 3 bytes before a multiple of 4096, at one place."""
    for n in lengths:
        for d in range(4):
            _put_at(L, place, n, lambda off: L.before_tile(off, d))
    L.good(2)


def parity_long(L: Listing, n: int):
    """A run of about one or two tiles at both places: starting at every offset modulo 16, and beginning 0..3 bytes before
    a multiple of 4096.  The walk back through the run crosses thread slices and tiles."""
    for place in PLACES:
        for r in range(SLICE):
            _put_at(L, place, n, lambda off: L.align(off, SLICE, r))
        for d in range(4):
            _put_at(L, place, n, lambda off: L.before_tile(off, d))
    L.good(2)


# ---- class 2: UTF-8 --------------------------------------------------------------------------------------------------------
def _with_text(L: Listing, piece: int, text: bytes) -> Tuple[bytes, int]:
    """A line whose piece holds x + text + y; returns it and the offset of text in it."""
    p = [L.name(), b"7", b"acgt"] if L.fmt == K else [L.name(), b"7", b"0", b"acgt"]
    off = sum(len(x) + 2 for x in p[:piece]) + 1
    p[piece] = b"x" + text + b"y"
    return b"  ".join(p) + b"\n", off


def utf8_ok(L: Listing):
    """Each valid character at the ends of the 2-, 3- and 4-byte forms, split after each of its bytes by a 16-byte boundary
    and by a multiple of 4096, in every piece that may hold it (kraken2: the accession, copied into both files)."""
    pieces = (0,) if L.fmt == K else (0, 1, 2, 3)
    i = 0
    for ch in VALID:
        for s in range(1, len(ch)):
            for piece in pieces:
                line, off = _with_text(L, piece, ch + b"-" + ch)
                L.align(off + s, SLICE, 0)
                L.marks["char"].append((L.pos + off, len(ch), piece))
                L.raw(line)
            line, off = _with_text(L, pieces[i % len(pieces)], ch)
            L.before_tile(off + s, 0)
            L.marks["char"].append((L.pos + off, len(ch), pieces[i % len(pieces)]))
            L.raw(line)
            i += 1
    L.good(2)


def _stop_case(name: str, fmt: str, piece: int, form: bytes, place: str, s: int = 0) -> Case:
    L = Listing(fmt)
    if place == "first":
        L.marks["bad"].append((0, len(form)))
        L.raw(form + b"A  7  " + (b"" if fmt == K else b"0  ") + b"acgt\n")
        L.good(2)
        return L.case(name, ("stop", 1))
    L.good(5)
    if place in ("eof", "eol"):                                  # the last bytes of the line: of the file too, for eof
        head = b"Z  7  ac" if fmt == K else b"Z  7  0  ac"
        if place == "eof":
            L.align(len(head) + len(form), SLICE, s)         # the zero pad is read from the same or from the next slice
        L.marks["bad"].append((L.pos + len(head), len(form)))
        L.raw(head + form + (b"" if place == "eof" else b"\nC  3  gg\nbroken\n"))
    else:
        line, off = _with_text(L, piece, form)
        if place == "tile":
            L.before_tile(off + s, 0)
        else:
            L.align(off + s, SLICE, 0)
        L.marks["bad"].append((L.pos + off, len(form)))
        L.raw(line + b"C  3  0  gg\nbroken\n")
    n = bytes(L.buf).count(b"\n", 0, L.marks["bad"][0][0]) + 1
    return L.case(name, ("stop", n))


@functools.lru_cache(maxsize=None)
def stops() -> List[Case]:
    """Every ill-formed sequence ends the listing quietly at its line, in whichever piece it stands: split at each of its
    bytes by a 16-byte boundary, split by a multiple of 4096, as the first bytes of the listing, before a newline, and as
    the last bytes of a listing without a final newline (the check then reads the zero pad)."""
    out, i = [], 0
    for name, form in INVALID.items():
        for s in (range(1, len(form)) if len(form) > 1 else (0, 1)):      # one byte: the last of a slice, the first of the next
            fmt = FORMATS[i % 2]
            out.append(_stop_case(f"{name}-slice{s}", fmt, i % n_pieces(fmt), form, "slice", s))
            i += 1
        fmt = FORMATS[i % 2]
        s = 1 + i % (len(form) - 1) if len(form) > 1 else i % 2          # one byte: the first of a tile, the last of one
        out.append(_stop_case(f"{name}-tile", fmt, i % n_pieces(fmt), form, "tile", s))
        i += 1
    for name in INVALID:
        out.append(_stop_case(f"{name}-first", FORMATS[i % 2], 0, INVALID[name], "first"))
        i += 1
    for name in ("cut2", "cut3", "cut3_1", "cut4", "cut4_2", "cut4_1"):
        out.append(_stop_case(f"{name}-eol", FORMATS[i % 2], 0, INVALID[name], "eol"))
        i += 1
    for name in INVALID:
        for s in ((0, 1) if name.startswith("cut") else (i % 2,)):        # the file ends with a slice, or one byte into the next
            out.append(_stop_case(f"{name}-eof{s}", FORMATS[i % 2], 0, INVALID[name], "eof", s))
            i += 1
    # two ill-formed bytes in one chunk: the first line wins
    for fmt in FORMATS:
        L = Listing(fmt)
        L.good(3)
        L.raw(b"B\xff  7  " + (b"" if fmt == K else b"0  ") + b"ac\n")
        L.good(2)
        L.raw(b"C  7  " + (b"" if fmt == K else b"0  ") + b"a\x80c\n")
        out.append(L.case(f"two_bad_bytes-{fmt}", ("stop", 4)))
    return out


# ---- class 3: output alignment ---------------------------------------------------------------------------------------------
WRAP_LENGTHS = [0, 1, 79, 80, 81, 159, 160, 161, 162]
LONG_LENGTHS = [4080, 4095, 4096, 4097]


def out_small(L: Listing):
    """qiime2 records of 5, 6, 7, ... output bytes (five: `>--\\n\\n`, from a line of six spaces), so that one writer thread
    covers three or four of them, at every output offset modulo 16 and at the tile edge."""
    assert L.fmt == Q
    def tiny(n):                                                 # a record of n >= 5 output bytes
        extra = n - 5
        if extra == 0:
            start = L.out
            L.buf += b"      \n"
            L.out += 5
        else:
            start = L.rec(b"c" * (extra // 4), b"7" * (extra // 4), b"g" * (extra - 3 * (extra // 4)), oid=b"o" * (extra // 4))
        L.marks["record"].append((start, n))
    for r in range(SLICE):                                       # four five-byte records from output offset r modulo 16
        L.out_align(0, SLICE, r)
        for _ in range(4):
            tiny(5)
    for n in range(5, 41):
        tiny(n)
        tiny(5)
        tiny(6)
    for d, n in ((0, 5), (0, 9), (5, 5), (3, 9), (4, 5), (16, 16), (1, 17), (15, 5)):     # starts at, ends at and straddles 4096 k
        L.out_align(0, TILE, -d)
        L.marks["tile_record"].append((L.out, n))
        tiny(n)
        tiny(5)
    L.good(2)


def out_wrap(L: Listing):
    """kraken2 sequences around the 80-column wrap: every length at every output offset modulo 16; the inserted newline at
    output offsets 15 and 0 modulo 16 and on both sides of a tile edge."""
    assert L.fmt == K
    def put(n, align):
        acc, tax = L.name(), b"%d" % n
        align(L.header(acc, tax))
        start = L.rec(acc, tax, seq(n, L.k))
        L.marks["wrap"].append((start, L.header(acc, tax), n))
    for n in WRAP_LENGTHS:
        for r in range(SLICE):
            put(n, lambda h: L.out_align(0, SLICE, r))
    for n in (81, 161, 162) + tuple(LONG_LENGTHS):
        for r in (15, 0):
            put(n, lambda h: L.out_align(h + 80, SLICE, r))      # body byte 80 is the first inserted newline
        for r in (TILE - 1, 0):
            put(n, lambda h: L.out_align(h + 80, TILE, r))
    L.good(2)


# ---- class 4: lines and taxids ---------------------------------------------------------------------------------------------
TAXIDS_OK = ([b"18446744073709551615", b"+18446744073709551615", b"+0", b"0", b"0" * 100, b"+" + b"0" * 99 + b"7"]
             + [b"%d" % 10 ** e for e in range(20)] + [b"%d" % (10 ** e - 1) for e in range(20)])
TAXIDS_BAD = {"2^64": b"18446744073709551616", "plus": b"+", "empty": b"", "two_numbers": b"1 2"}


def taxids(L: Listing):
    """Accepted kraken2 taxids: the largest usize, +0, a hundred zeros, every power of ten and each one less (the digit
    counts of prelim_map.txt)."""
    assert L.fmt == K
    for t in TAXIDS_OK:
        L.marks["taxid"].append((L.k, t))
        L.rec(L.name(), t, seq(5 + L.k % 7))


ACCEPTED = {"parity_short": (parity_short, FORMATS), "utf8_ok": (utf8_ok, FORMATS), "out_small": (out_small, (Q,)),
            "out_wrap": (out_wrap, (K,)), "taxids": (taxids, (K,))}
# class 1 against the tile edge is several listings, to keep each at a few hundred KB: the short runs by place and by half of
# the lengths, the long runs one length each
TILE_PARTS = {f"parity_tile-{p}-{lo}": (p, list(range(lo, lo + 20))) for p in PLACES for lo in (1, 21)}
for _name, (_p, _ns) in TILE_PARTS.items():
    ACCEPTED[_name] = (functools.partial(parity_tile, place=_p, lengths=_ns), FORMATS)
for _n in LONG_RUNS:
    ACCEPTED[f"parity_long-{_n}"] = (functools.partial(parity_long, n=_n), FORMATS)
ACCEPTED_IDS = [(c, f) for c, (_, fmts) in ACCEPTED.items() for f in fmts]


@functools.lru_cache(maxsize=None)
def accepted(cls: str, fmt: str, seed: int = 0, lead: int = 0) -> Case:
    """The listing of one class.  seed: other names and sequence letters; lead: so many bytes of pad lines first, which moves
    every case and lets the pads before each put it back in its place."""
    L = Listing(fmt, seed, lead)
    ACCEPTED[cls][0](L)
    return L.case(f"{cls}-{fmt}")


@functools.lru_cache(maxsize=None)
def small(fmt: str) -> List[Case]:
    """Accepted listings whose property is their size or their end."""
    out = []
    for n in (1, 2, 3, 4, 15, 16, 17, 33, 4096):                  # a run of spaces ends a listing without a final newline
        for s in ((0, 1, 15) if n < 100 else (0,)):
            L = Listing(fmt)
            L.good(3)
            head = L.name() + (b"  7  acgt" if fmt == K else b"  7  0  acgt")
            L.align(len(head) + n, SLICE, s)                      # the listing ends s bytes into a slice
            L.marks["run"].append((L.pos + len(head), n, "end"))
            L.raw(head + b" " * n)
            out.append(L.case(f"run_{n}_ends_the_listing-{s}"))
    for ch in VALID:                                              # a character as the first bytes; as the last, without a newline
        L = Listing(fmt)
        L.marks["char"].append((0, len(ch), 0))
        L.raw(ch + b"A  7  " + (b"" if fmt == K else b"0  ") + b"acgt\n")
        L.good(1)
        out.append(L.case(f"first_bytes_{ch.hex()}"))
        L = Listing(fmt)
        L.good(2)
        # qiime2 copies a sequence that ends with it; a kraken2 sequence is ASCII: pieces "", "7", "" and then text nobody reads
        head = b"  7    Z" if fmt == K else b"Z" + ch + b"  7  0  ac"
        L.marks["char"].append((L.pos + len(head), len(ch), -1))
        L.raw(head + ch)
        out.append(L.case(f"last_bytes_{ch.hex()}"))
    for n in (1, 255, 256, 257):                                  # line counts around a block of line threads
        L = Listing(fmt)
        L.good(n)
        out.append(L.case(f"lines_{n}"))
    L = Listing(fmt)                                              # CRLF throughout, the last line without either
    for i in range(257):
        L.rec(L.name(), b"%d" % i, seq(i % 90), end=b"\r\n" if i < 256 else b"")
    out.append(L.case("crlf"))
    if fmt == Q:                                                  # a line that is exactly its separators
        L = Listing(fmt)
        L.raw(b"      \n      \r\n      ")
        out.append(L.case("only_separators"))
    for total in (3 * SLICE - 1, 3 * SLICE, 3 * SLICE + 1, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1):     # output sizes
        L = Listing(fmt)
        L.out_pad(total)
        L.marks["total"].append(total)
        out.append(L.case(f"output_of_{total}_bytes"))
    return out


# ---- class 5: chunk cuts ---------------------------------------------------------------------------------------------------
def _body(L: Listing, size: int):
    """Lines of mixed lengths, about size bytes."""
    rng = np.random.default_rng([L.seed, 77])
    end = L.pos + size
    while L.pos < end:
        n = int(rng.integers(0, 200)) if rng.random() < 0.9 else int(rng.integers(200, 1500))
        L.rec(L.name(), b"%d" % int(rng.integers(0, 10 ** int(rng.integers(1, 12)))), seq(n, L.k))


def _line_of(L: Listing, n: int, end: bytes = b"\n"):
    """A line of exactly n bytes with its ending."""
    fixed = len(b"  ".join([b"L", b"7"] + ([] if L.fmt == K else [b"0"]) + [b""])) + len(end)
    L.rec(b"L", b"7", seq(n - fixed, L.k), end=end)


def least_chunks(listing: bytes, chunk: int) -> int:
    """A bound from the reader's rules.  A slot holds chunk bytes, or the carried rest of a line and half a chunk more, and
    doubles while it holds no newline.  With no line longer than half a chunk the carry is shorter than that, the bytes read
    behind it end its line, and the slot never grows: every chunk is chunk bytes at most.  Otherwise a slot stops doubling
    once the longest line fits, below 2 (longest + chunk) bytes."""
    longest = max(len(x) + 1 for x in listing.split(b"\n"))
    cap = chunk if longest <= chunk // 2 else 2 * (longest + chunk)
    return -(-len(listing) // cap)


@functools.lru_cache(maxsize=None)
def cuts(fmt: str) -> List[Case]:
    """Listings for chunk_bytes 4096 and 8192 (the reader cuts a chunk at its last newline and carries the rest): a leading
    pad of 0 or 12..75 bytes moves the same lines through every position of the cut modulo 64; then lines and bytes put
    against byte 4096 and 8192.  min_chunks: what the reader must at least make of it."""
    out = []
    def done(L, name):
        out.append(L.case(name, min_chunks={c: least_chunks(bytes(L.buf), c) for c in (4096, 8192)}))
    for p in [0] + list(range(MINPAD, MINPAD + 64)):
        L = Listing(fmt, lead=p)
        _body(L, 13000)
        done(L, f"lead_{p}")
    for at in (4095, 4096, 8191, 8192):                           # a newline at that byte
        L = Listing(fmt)
        L.good(3)
        L.to(at + 1 - 40)
        _line_of(L, 40)
        assert L.buf[at] == 10
        L.marks["newline_at"].append(at)
        _body(L, 6000)
        done(L, f"newline_at_{at}")
    for n in (4096, 4097, 8192):                                  # a line of exactly that size, first and after a short line
        for first in (True, False):
            L = Listing(fmt)
            if not first:
                L.good(1)
            L.marks["line"].append((L.pos, n))
            _line_of(L, n)
            _body(L, 3000)
            done(L, f"line_of_{n}-{'first' if first else 'second'}")
    L = Listing(fmt)                                              # \r at 4095, \n at 4096
    L.good(3)
    L.to(4097 - 40)
    _line_of(L, 40, b"\r\n")
    assert L.buf[4095:4097] == b"\r\n"
    L.marks["newline_at"].append(4096)
    _body(L, 3000)
    done(L, "crlf_across_4096")
    for ch in VALID[1:]:                                          # a character across 4096 (in the accession)
        L = Listing(fmt)
        L.good(3)
        L.before_tile(1 + len(ch) // 2, 0)
        L.marks["char"].append((L.pos + 1, len(ch), 0))
        L.rec(b"x" + ch + b"y", b"7", b"acgt")
        _body(L, 3000)
        done(L, f"char_{ch.hex()}_across_4096")
    for newline in (True, False):                                 # a file of exactly 4096 bytes
        L = Listing(fmt)
        _body(L, 3900)
        _line_of(L, 4096 - L.pos, b"\n" if newline else b"")
        assert L.pos == 4096
        out.append(L.case(f"file_of_4096-{'newline' if newline else 'no_newline'}", min_chunks={4096: 1 if newline else 2, 8192: 1}))
    for c in (4096, 8192):                                        # a line of three chunks, then short lines: the slot has grown
        L = Listing(fmt)
        L.good(2)
        _line_of(L, 3 * c)
        _body(L, 20000)
        out.append(L.case(f"line_of_three_chunks_of_{c}", min_chunks={c: 2}))
    return out


# ---- class 7 and the refused cases of the other classes --------------------------------------------------------------------
def _bad(fmt: str, what: str) -> bytes:
    """One line with that problem (or those, joined by +)."""
    k = fmt == K
    return {"stop": b"B\xff  7  " + (b"" if k else b"0  ") + b"ac\n",
            PIECES: b"B  7" + (b"" if k else b"  0") + b"\n",
            NONASCII: "B  7  acé\n".encode(), TAXID: b"B  x7  ac\n",
            "stop+" + PIECES: b"B\xff  7\n", "stop+" + NONASCII: b"B  7  \xc3\xa9\xff\n",
            "stop+" + TAXID: b"B  x\xff  ac\n", PIECES + "+" + TAXID: b"B  x7\n", PIECES + "+" + NONASCII: "B  é\n".encode(),
            NONASCII + "+" + TAXID: "B  x7  acé\n".encode()}[what]


def _winner(what: str) -> str:
    """the stop, then the pieces, then a non-ASCII sequence, then the taxid."""
    return what.split("+")[0]


@functools.lru_cache(maxsize=None)
def precedence() -> List[Case]:
    out = []
    def case(fmt, name, first, second, far):
        L = Listing(fmt)
        L.good(5)
        L.raw(_bad(fmt, first))
        if second:
            if far:
                _body(L, 9000)                                    # more than a chunk of 8192 later
            else:
                L.good(1)
            L.raw(_bad(fmt, second))
        L.good(2)
        w = _winner(first)
        out.append(L.case(f"{name}-{fmt}", ("stop", 6) if w == "stop" else ("error", 6, w)))
    for far in (False, True):
        d = "two_chunks" if far else "one_chunk"
        case(K, f"error_before_stop-{d}", TAXID, "stop", far)
        case(Q, f"error_before_stop-{d}", PIECES, "stop", far)
        case(K, f"stop_before_error-{d}", "stop", PIECES, far)
        case(Q, f"stop_before_error-{d}", "stop", PIECES, far)
    case(K, "two_errors-taxid_pieces", TAXID, PIECES, False)
    case(K, "two_errors-pieces_taxid", PIECES, TAXID, False)
    case(K, "two_errors-nonascii_pieces", NONASCII, PIECES, False)
    case(Q, "two_errors-pieces_pieces", PIECES, PIECES, False)
    for both in ("stop+" + PIECES, "stop+" + NONASCII, "stop+" + TAXID, PIECES + "+" + TAXID, PIECES + "+" + NONASCII, NONASCII + "+" + TAXID):
        case(K, "one_line-" + both, both, None, False)
    case(Q, "one_line-stop+" + PIECES, "stop+" + PIECES, None, False)
    for fmt, what in ((K, TAXID), (K, NONASCII), (K, PIECES), (Q, PIECES)):     # an error three chunks of 8192 in
        L = Listing(fmt)
        _body(L, 20000)
        n = bytes(L.buf).count(b"\n") + 1
        L.raw(_bad(fmt, what))
        L.good(2)
        out.append(L.case(f"error_chunks_in-{what}-{fmt}", ("error", n, what)))
    return out


@functools.lru_cache(maxsize=None)
def refused() -> List[Case]:
    """The refused spellings of classes 1 to 4, one line each, after five good lines."""
    out = []
    def one(fmt, name, line, reason, before=5):
        L = Listing(fmt)
        L.good(before)
        L.raw(line)
        L.good(1)
        out.append(L.case(f"{name}-{fmt}", ("error", before + 1, reason)))
    for n in (4, 5, 16, 17, 4096):                                # class 1: the run makes the kraken2 taxid empty
        one(K, f"run_{n}_empties_the_taxid", b"A" + b" " * n + b"7  8  acgt\n", TAXID)
    one(K, "run_1_joins_taxid_and_sequence", b"A  7 acgt  c\n", TAXID)
    one(K, "run_3_is_one_separator", b"A   7 acgt\n", PIECES)
    one(Q, "run_5_is_two_separators", b"A     7 acgt\n", PIECES)
    for i, ch in enumerate(VALID):                                # class 2: valid text where kraken2 wants ASCII or a number
        one(K, f"sequence_{ch.hex()}", b"A  7  ac" + ch + b"gt\n", NONASCII)
        one(K, f"taxid_{ch.hex()}", b"A  7" + ch + b"  acgt\n", TAXID)
    L = Listing(K)                                                # ... and as the last bytes of a listing without a newline
    L.good(5)
    L.raw(b"A  7  acg" + VALID[2])
    out.append(L.case("sequence_ends_the_listing-kraken2", ("error", 6, NONASCII)))
    # class 3: a non-ASCII byte ends one sequence and another starts the next one.  (The two cannot share one writer thread's
    # 16 bytes: the newline and a kraken2 header of 16 bytes or more, `>kraken:taxid||` and a newline with both pieces empty,
    # lie between them.  The thread holds the last sequence byte of the first record and the start of the second.)  The
    # first line is named.
    for r in (0, 9, 15):
        L = Listing(K)
        L.good(3)
        acc = L.name()
        L.out_align(L.header(acc, b"7") + 4, SLICE, r)            # the last sequence byte at output offset r modulo 16
        n = bytes(L.buf).count(b"\n") + 1
        L.marks["nonascii_at"].append(L.out + L.header(acc, b"7") + 4)
        L.raw(acc + b"  7  acg" + VALID[0] + b"\n" + b"  7  " + VALID[0] + b"acg\n")
        L.good(1)
        out.append(L.case(f"nonascii_ends_one_and_starts_the_next-{r}", ("error", n, NONASCII)))
    for name, t in TAXIDS_BAD.items():                            # class 4
        one(K, "taxid_" + name, b"A  " + t + b"  acgt\n", TAXID)
    one(K, "line_of_cr", b"\r\n", PIECES)
    one(Q, "line_of_cr", b"\r\n", PIECES)
    one(K, "line_of_its_separators", b"    \n", TAXID)            # pieces "", "", "": the taxid is empty
    one(K, "empty_line", b"\n", PIECES)
    one(K, "first_line", b"A  7\n", PIECES, before=0)
    return out
