"""Case families for the minimum cover's kernels (csrc/cover_kernel.hip) at the sorted positions a real
taxonomy has: up to 2^20 + 39, where the long kernel's radix selection leaves digit 0 of its first two passes and the range
minimum reads the sparse table up to level 16.  No product code is here and none is imported: a group is a list of
(row reference, score), the expected value is tests/min_cover_reference.keep on the lineage tuples of the rows it names.

The large table (`LARGE_ROWS` rows): the row at sorted position p has as its lineage the seven base-8 digits of p, most
significant first, level l using the node ids 100 l + digit.  Then, from the positions alone,

    share(a, b) = the leading base-8 digits a and b have in common (7 when a == b)
    lcp8[i]     = share(i, i + 1) = 6 - (trailing octal 7s of i)
    d*          = the deepest level at which one digit prefix holds `need` of the group

which `closed_form` states once more next to the dict reference.  The rows are given to the library in a seeded permutation
(`large_matrix`), so the row map is not the identity.  Row references: a sorted position on the large table, a row index on
the small tree (`small_tree`: the four-level tree of tests/test_gpu_min_cover_edges.py), -1 an unmatched row.

`median`, `selection_trace` and `range_parts` say where a group lies for the coverage claims of tests/test_min_cover_edges.py
and for failure messages: the sorted median, its digit in each of the four selection passes (7 + 6 + 6 + 6 bits) with the
count still to skip on entry and on exit, and the 16-entry blocks a range [lo, hi) of lcp8 decomposes into.

Two things this table cannot do, both argued in `range_family`: a range that holds whole blocks never has its unique minimum
among its right edge entries, and from level 14 on no range has a unique minimum outside the overlap of its two entries.  The
stepped table (`stepped_lineage_of`: the same rows under three heads, so that lcp8 has one entry of 1 near its start and one
of 0 near its end) puts a unique minimum into each of the five places at every level (`stepped_range_family`)."""
import functools

import numpy as np

from tests import min_cover_reference as ref

TOP, UNDER = 1000, 995
UNMATCHED_ROW = -1
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
LARGE_ROWS = (1 << 20) + 40
LEVELS = 7                                           # base-8 digits of a position below 8^7 = 2^21
PAD = 70                                             # lower-scored rows that make a segment a long one (> 64 rows)
SEL_SHIFT, SEL_BITS = (18, 12, 6, 0), (7, 6, 6, 6)   # the selection's digits over the 25 position bits
SPREAD_N = (9, 10, 65, 66, 257, 1000)
QUERY_COUNTS = (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 1040)
RANGE_PLACES = ("left edge", "first entry", "second entry", "overlap")


# ---- the large table ------------------------------------------------------------------------------------------------------------

def lineage_of(p):
    return tuple(100 * l + ((p >> (3 * (LEVELS - 1 - l))) & 7) for l in range(LEVELS))


@functools.lru_cache(None)
def large_matrix():
    """(lineage matrix [LARGE_ROWS, 7] int32 in row order, position of every row): row r is the row at sorted position perm[r]"""
    perm = np.random.default_rng(5).permutation(LARGE_ROWS)
    shifts = 3 * (LEVELS - 1 - np.arange(LEVELS))
    m = (100 * np.arange(LEVELS)[None, :] + ((perm[:, None] >> shifts[None, :]) & 7)).astype(np.int32)
    return m, perm


def share(a, b):
    x = a ^ b
    return LEVELS if x == 0 else LEVELS - (x.bit_length() + 2) // 3


@functools.lru_cache(None)
def lcp8():
    """lcp8[i] = share(i, i + 1) for i < LARGE_ROWS - 1, from the trailing octal 7s of i"""
    i1 = np.arange(1, LARGE_ROWS, dtype=np.int64)
    low = i1 & -i1                                                       # 2^(trailing zero bits of i + 1)
    tz = np.round(np.log2(low)).astype(np.int64)
    return (LEVELS - 1 - tz // 3).astype(np.int64)


def closed_form(positions, milli):
    """(d*, verdicts) of a top group of large-table positions, from digit prefixes"""
    need = ref.need_rows(len(positions), milli)
    for d in range(LEVELS, -1, -1):
        pre = [p >> (3 * (LEVELS - d)) for p in positions]
        best = max(set(pre), key=pre.count)
        if pre.count(best) >= need:
            return d, [int(x == best) for x in pre]
    raise AssertionError("level 0 holds every row")


# ---- the stepped table ---------------------------------------------------------------------------------------------------------

STEP_1, STEP_2 = 10, (1 << 20) + 30


def stepped_lineage_of(p):
    """LARGE_ROWS rows again: [1, 1] + the digits of p below STEP_1, [1, 2] + digits below STEP_2, [2] + digits from there on — the
    sorted position is still p, every digit carry now lies two (one) levels deeper, and lcp8 has one entry of 1 (STEP_1 - 1, in
    block 0) and one of 0 (STEP_2 - 1, the fourteenth entry of the last block but one): a unique minimum for ranges of any length"""
    head = (1, 1) if p < STEP_1 else (1, 2) if p < STEP_2 else (2,)
    return head + lineage_of(p)


def stepped_share(a, b):
    part = lambda p: 0 if p < STEP_1 else 1 if p < STEP_2 else 2
    if part(a) != part(b):
        return 1 if max(part(a), part(b)) == 1 else 0
    return (1 if part(a) == 2 else 2) + share(a, b)


@functools.lru_cache(None)
def stepped_matrix():
    """as large_matrix: ([LARGE_ROWS, 9] int32 padded with -1, position of every row)"""
    perm = np.random.default_rng(6).permutation(LARGE_ROWS)
    shifts = 3 * (LEVELS - 1 - np.arange(LEVELS))
    dig = (100 * np.arange(LEVELS)[None, :] + ((perm[:, None] >> shifts[None, :]) & 7)).astype(np.int32)
    m = np.full((LARGE_ROWS, LEVELS + 2), -1, np.int32)
    m[:, 0] = np.where(perm < STEP_2, 1, 2)
    m[:, 1] = np.where(perm < STEP_1, 1, 2)
    m[:, 2:] = dig
    last = perm >= STEP_2
    m[last, 1:LEVELS + 1] = dig[last]
    m[last, LEVELS + 1] = -1
    return m, perm


@functools.lru_cache(None)
def stepped_lcp8():
    out = lcp8() + 2
    out[STEP_2:] -= 1
    out[STEP_1 - 1], out[STEP_2 - 1] = 1, 0
    return out


# ---- the small tree -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def small_tree():
    """120 rows: three phyla x three families x three genera x three species, the phyla and the families as rows of their own,
    in an order that is not the sorted one"""
    lins = [[p, 10 + f, 20 + g, 30 + s] for p in range(3) for f in range(3) for g in range(3) for s in range(3)]
    lins += [[p] for p in range(3)] + [[p, 10 + f] for p in range(3) for f in range(3)]
    perm = np.random.default_rng(3).permutation(len(lins))
    return [lins[i] for i in perm]


def small_row(lineage):
    return small_tree().index(list(lineage))


def small_group(rng, n, outliers, genus=(1, 11, 21)):
    """n rows: species of one genus, the rows at the indices `outliers` replaced by rows of another phylum"""
    rows = [small_row(list(genus) + [30 + int(rng.integers(0, 3))]) for _ in range(n)]
    for at in outliers:
        rows[at] = small_row([2, 10 + int(rng.integers(0, 3)), 20, 30])
    return rows


# ---- a group --------------------------------------------------------------------------------------------------------------------

class Group:
    """One query: family, name, tree ("large", "stepped": references are sorted positions; "small": row indices), rows [(ref, score)]"""

    def __init__(self, family, name, rows, tree="large", **claims):
        self.family, self.name, self.tree, self.rows, self.claims = family, name, tree, [(int(r), int(s)) for r, s in rows], claims

    def top(self):
        """the references of the top group, in row order"""
        if not self.rows:
            return []
        t = max(s for _, s in self.rows)
        return [r for r, s in self.rows if s == t]

    def lineages(self):
        """one per row, as min_cover_reference.keep takes them"""
        if self.tree == "large":
            return [None if r < 0 else lineage_of(r) for r, _ in self.rows]
        if self.tree == "stepped":
            return [stepped_lineage_of(r) for r, _ in self.rows]
        return [None if r < 0 else tuple(small_tree()[r]) for r, _ in self.rows]

    def where(self):
        """for a failure message: family, group, the sorted median position and its four digits"""
        text = f"family {self.family} group {self.name}"
        top = self.top()
        if self.tree in ("large", "stepped") and len(top) > 1 and min(top) >= 0:
            m = median(top)
            text += f": median at sorted position {m}, digits {digits(m)}"
        return text


def reference(groups, milli):
    """min_cover_reference.keep on the groups as the queries of one table: (seg_off, verdicts, depths, counts)"""
    seg, bs, lin = [0], [], []
    for g in groups:
        bs += [s for _, s in g.rows]
        lin += g.lineages()
        seg.append(len(bs))
    return (seg,) + ref.keep(seg, bs, lin, milli)


def median(top):
    return sorted(top)[len(top) // 2]


def digits(pos):
    return tuple((pos >> s) & ((1 << b) - 1) for s, b in zip(SEL_SHIFT, SEL_BITS))


def selection_trace(top):
    """Per pass: (the median's digit, rows still to skip on entry, on exit, rows in the median's bin, rows in the bins before
    it) among the rows that share the median's higher digits — from the sorted list, no histogram is walked."""
    s = sorted(top)
    at, m = len(s) // 2, s[len(s) // 2]
    out = []
    for shift, bits in zip(SEL_SHIFT, SEL_BITS):
        bucket_first = sum(1 for p in s if (p >> (shift + bits)) < (m >> (shift + bits)))
        in_bucket = [p for p in s if (p >> (shift + bits)) == (m >> (shift + bits))]
        before = sum(1 for p in in_bucket if (p >> shift) < (m >> shift))
        in_bin = sum(1 for p in in_bucket if (p >> shift) == (m >> shift))
        left_in = at - bucket_first
        out.append(((m >> shift) & ((1 << bits) - 1), left_in, left_in - before, in_bin, before))
    return out


def _pad(key):
    """PAD rows under the top group, anywhere in the large table"""
    return [((key * 7919 + j * 104729 + 11) % LARGE_ROWS, UNDER - j % 3) for j in range(PAD)]


# ---- family: spread -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def spread_family():
    """For n in SPREAD_N and a clade level 1 .. 6, four groups: exactly `need` rows (at 50.001 %) inside one clade of that level,
    the other n - need anywhere, shuffled — the majority is as tight as it can be, so a median taken one index off may leave
    the clade.  Each as a long segment, and as the whole of a short one where n <= 64."""
    rng = np.random.default_rng(21)
    out = []
    for n in SPREAD_N:
        need = ref.need_rows(n, 50001)
        for level in range(1, LEVELS):
            size = 8 ** (LEVELS - level)
            for g in range(4):
                clade = int(rng.integers(0, LARGE_ROWS // size))                # (the clades that lie in the table whole)
                rows = np.concatenate([clade * size + rng.integers(0, size, need), rng.integers(0, LARGE_ROWS, n - need)])
                rows = rows[rng.permutation(n)]
                for form in (("short", "long") if n <= 64 else ("long",)):
                    out.append(Group("spread", f"n {n} level {level} group {g} {form}",
                                     [(p, TOP) for p in rows] + (_pad(len(out)) if form == "long" else []),
                                     n=n, level=level, form=form, need=need))
    return out


# ---- family: digit --------------------------------------------------------------------------------------------------------------

def _block_of_eight(base):
    b = base & ~7
    return [b, b + 1, b + 3, b + 4, b + 7]


@functools.lru_cache(None)
def digit_family():
    """Nine rows, need 5: five majority rows in one block of eight and four outliers exactly 2^s from them, s a digit boundary of
    the selection — all below (the median is the first majority row), all above (the last) or two on each side — with the
    majority first or last in row order.  The majority sits in each top digit 0 .. 4 with its lower 6-bit digits 0, 63 and
    mid-range (in top digit 4, which holds 40 rows, the last digit 0, 16 and 32).  Every arrangement that lies inside the table
    is there.  Second form: the outliers in the neighbouring top digit with a smaller next digit than the majority's, which a
    selection that does not filter by the chosen prefix counts into its later passes.  All long segments."""
    out = []

    def add(name, major, outliers, **claims):
        if min(outliers) < 0 or max(outliers) >= LARGE_ROWS:
            return
        for order in ("majority first", "majority last"):
            top = major + outliers if order == "majority first" else outliers + major
            out.append(Group("digit", f"{name}, {order}", [(p, TOP) for p in top] + _pad(len(out)), **claims))

    for s in (18, 12, 6):
        for t in range(5):
            for low in ((0, 63, 29) if t < 4 else (0, 32, 16)):
                base = (t << 18) | ((low << 12) | (low << 6) | low if t < 4 else low)
                major = _block_of_eight(base)
                for side, signs in (("below", (-1, -1, -1, -1)), ("above", (1, 1, 1, 1)), ("split", (-1, -1, 1, 1))):
                    add(f"s {s} top digit {t} low digits {low} outliers {side}", major,
                        [p + sg * (1 << s) for p, sg in zip(major, signs)], s=s, t=t, low=low, side=side, form=1)
    for t in range(4):
        major = _block_of_eight((t << 18) | (40 << 12) | (21 << 6) | 8)
        for side, t2 in (("below", t - 1), ("above", t + 1)):
            if t2 < 0:
                continue
            outliers = [(t2 << 18) + ((5 << 12) | (33 << 6) if t2 < 4 else 0) + i for i in range(4)]
            add(f"second form top digit {t} outliers in top digit {t2}", major, outliers, s=None, t=t, low=None, side=side, form=2)
    return out


# ---- family: bin edge -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def bin_edge_family():
    """Nine rows, need 5, for each selection pass: the median as the first row of its bin with the four outliers in the two
    bins in front of it under the same higher digits (the count to skip equals the rows in front: `left == s_hist[dgt]` on the
    way), and as the last row of its bin with the outliers in the two bins behind.  The majority is five rows of one block of
    eight, or one row five times (in the last pass only that puts five rows into one bin).  All long segments."""
    out = []
    for p, shift in enumerate(SEL_SHIFT):
        for edge in ("first", "last"):
            tops = ((2, 3) if edge == "first" else (0, 1)) if p == 0 else (0, 3)
            for t in tops:
                base = (t << 18) | (33 << 12) | (20 << 6) | 40
                for style, major in (("block", _block_of_eight(base)), ("equal", [base] * 5)):
                    end = min(major) if edge == "first" else max(major)
                    sg = -1 if edge == "first" else 1
                    outliers = [end + sg * k * (1 << shift) for k in (1, 1, 2, 2)]
                    assert 0 <= min(outliers) and max(outliers) < LARGE_ROWS
                    top = (outliers[:2] + major + outliers[2:])
                    out.append(Group("bin edge", f"pass {p} median {edge} of its bin, top digit {t}, {style} majority",
                                     [(x, TOP) for x in top] + _pad(len(out)), p=p, edge=edge))
    return out


# ---- family: range --------------------------------------------------------------------------------------------------------------

def range_parts(lo, hi):
    """[lo, hi) of lcp8, lo < hi, as the whole 16-entry blocks b0 .. b1 - 1 and the entries at either edge: (b0, b1, k) with
    2^k <= b1 - b0 < 2^(k + 1), k None without a whole block"""
    b0, b1 = (lo + 15) >> 4, hi >> 4
    return b0, b1, ((b1 - b0).bit_length() - 1 if b0 < b1 else None)


def range_place(lo, hi, z):
    """where entry z of [lo, hi) lies: an edge, the first or the second sparse-table entry alone, or both"""
    b0, b1, k = range_parts(lo, hi)
    if k is None:
        return "one block" if b0 > b1 else ("left edge" if z < (b0 << 4) else "right edge")
    zb = z >> 4
    if zb < b0:
        return "left edge"
    if zb >= b1:
        return "right edge"
    first, second = zb < b0 + (1 << k), zb >= b1 - (1 << k)
    return "overlap" if first and second else "first entry" if first else "second entry"


def _range_group(name, lo, hi, form, **claims):
    """lo, hi, hi and a row of another top digit at 75 %: need 3 of 4, the median by position is hi, d* = share(lo, hi) = min
    lcp8[lo .. hi), and the far row goes unless lo and hi share nothing themselves"""
    far = next(f for f in (hi ^ (1 << 19), hi ^ (1 << 18), hi ^ (1 << 20)) if f < LARGE_ROWS)
    rows = [(far, TOP), (hi, TOP), (lo, TOP), (hi, TOP)] + (_pad(lo + hi) if form == "long" else [])
    return Group("range", f"{name} lo {lo} hi {hi} {form}", rows, lo=lo, hi=hi, form=form, **claims)


@functools.lru_cache(None)
def range_family():
    """Pairs (lo, hi) around z = X - 1, X an odd multiple of 8^j (j = 2 .. 6): lcp8[z] = 6 - j is the range's unique minimum as
    long as the range stays inside (X - 8^j, X + 8^j).  For every k = 0 .. 13 that such a range can have (16 (2^k + 2) + 31 entries
    below 8^j), z is put among the left edge entries, into the first sparse-table entry alone, the second alone and their
    overlap, at either end of each, with lo and hi on and off a block edge; then lo = 0, hi = LARGE_ROWS - 1 and the ranges
    of k = 14, 15 and 16.  Each pair once short and once long.

    What no table of digit lineages gives: (1) the deepest carry of a range that holds a whole block is at an index = 63 mod
    64, the last entry of a 16-block, and the right edge [16 b1, hi) never holds a block's last entry — the right edge has the
    unique minimum of no such range (the binary table of test_gpu_min_cover_edges.py, whose lcp8 dips in front of and behind
    every block edge, is what holds the edges to account); (2) a range of 2^14 + 1 blocks or more spans 2^18 positions and a
    second entry as deep as the deepest, so for k = 14 the unique minimum exists only in the overlap and for k = 15, 16 (more
    than 2^19 positions: two or more zeros of lcp8, 2^18 apart) the minimum 0 is never unique.  stepped_range_family fills
    both in on a table of its own.  `claims["unique"]` says which
    groups have a unique minimum; tests/test_min_cover_edges.py counts the places from the positions."""
    out = []

    def add(name, lo, hi, **claims):
        if not (0 <= lo < hi < LARGE_ROWS):
            return
        if claims["unique"]:                                             # (kept only where z is the one minimum: see above)
            part = lcp8()[lo:hi]
            if int((part == part.min()).sum()) != 1 or lo + int(part.argmin()) != claims["z"]:
                return
        for form in ("short", "long"):
            out.append(_range_group(name, lo, hi, form, **claims))

    for j in range(2, LEVELS):
        step = 8 ** j
        x = step * (((1 << 19) // step) | 1)
        z, zb = x - 1, (x - 1) >> 4
        for k in range(0, 14):
            d = 1 if k == 0 else 3 if k == 1 else (1 << k) + 2
            if 16 * d >= 2 * step:
                continue
            ends = []                                                    # (b0, b1) with z where it is wanted
            ends += [("left edge", zb + 1, zb + 1 + d), ("left edge", zb + 1, zb + 1 + (1 << k))]
            if k >= 1:
                ends += [("first entry", zb, zb + d), ("second entry", zb + 1 - d, zb + 1)]
            if k >= 2:
                ends += [("first entry", zb - 1, zb - 1 + d), ("second entry", zb + 2 - d, zb + 2)]
                ends += [("overlap", zb - 2, zb - 2 + d), ("overlap", zb + 1 - (1 << k), zb + 1 - (1 << k) + d)]
            ends += [("overlap", zb, zb + (1 << k))]
            for n_e, (place, b0, b1) in enumerate(ends):
                for lo, hi in ((16 * b0, 16 * b1), (16 * b0 - 3, 16 * b1 + 5)):
                    if place == "left edge":                             # z = 16 b0 - 1: the first entry of the range, or its fourth
                        lo = z if hi == 16 * b1 else z - 3
                    add(f"j {j} k {k} minimum in the {place} ({n_e})", lo, hi, j=j, k=k, place=place, z=z, unique=True)
    # level 14: only the overlap can hold the one zero of a range between two others
    z = 3 * (1 << 18) - 1
    zb = z >> 4
    for b0, b1 in ((zb - 3, zb - 3 + (1 << 14) + 2), (zb - (1 << 14) + 2, zb + 2), (zb - 100, zb - 100 + (1 << 14))):
        for lo, hi in ((16 * b0, 16 * b1), (16 * b0 - 3, 16 * b1 + 5)):
            add("j 6 k 14 minimum in the overlap", lo, hi, j=6, k=14, place="overlap", z=z, unique=True)
    # levels 15 and 16, the table's two ends: share(lo, hi) = 0 with several zeros in the range
    n = LARGE_ROWS
    for lo, hi in ((0, (1 << 19) + 100), ((1 << 19) - 37, n - 1), (5, (1 << 19) + (1 << 18)), (0, (1 << 20) - 1),
                   (0, n - 1), (5, n - 1), (15, n - 1), (0, (1 << 20) + 16), (15, (1 << 20) + 16), (16, n - 1), (17, (1 << 20) + 31)):
        add("table ends", lo, hi, j=6, k=range_parts(lo, hi)[2], place=None, z=None, unique=False)
    for lo, hi in ((0, 1), (0, 64), (n - 2, n - 1), (n - 41, n - 1), ((1 << 20) - 1, 1 << 20), ((1 << 20) - 17, n - 1)):
        add("table ends", lo, hi, j=None, k=range_parts(lo, hi)[2], place=None, z=None, unique=False)
    return out


@functools.lru_cache(None)
def stepped_range_family():
    """What range_family cannot reach, on the stepped table: the unique minimum at STEP_1 - 1 (entry 9 of block 0: the left edge,
    the first entry alone, the overlap) or at STEP_2 - 1 (entry 13 of block 65537: the right edge, the second entry alone, the
    overlap), for every level k = 0 .. 16.  lo, hi, hi and a far row at 75 % as in range_family: d* = 1 (the far row, beyond
    STEP_2, goes) or 0."""
    out = []
    zb2 = (STEP_2 - 1) >> 4
    for k in range(17):
        d = 1 if k == 0 else 3 if k == 1 else (1 << k) + 1 if k == 16 else (1 << k) + 2
        pairs = [("left edge", lo, 16 * (1 + (1 << k)) + r) for lo, r in ((STEP_1 - 1, 0), (3, 7))]
        pairs += [("overlap", lo, 16 * (1 << k) + r) for lo, r in ((0, 0), (0, 9))]
        pairs += [("right edge", 16 * (zb2 - x) - e, STEP_2 + r) for x, e, r in ((1 << k, 0, 0), (d, 3, 1))]
        pairs += [("overlap", 16 * (zb2 + 1 - (1 << k)) - e, 16 * (zb2 + 1) + r) for e, r in ((0, 0), (5, 7))]
        if k >= 1:
            pairs += [("first entry", lo, 16 * d + r) for lo, r in ((0, 0), (0, 11))]
            pairs += [("second entry", 16 * (zb2 + 1 - d) - e, 16 * (zb2 + 1) + r) for e, r in ((0, 0), (3, 7))]
        for place, lo, hi in pairs:
            z = STEP_1 - 1 if lo < STEP_1 else STEP_2 - 1
            if not (0 <= lo <= z < hi < LARGE_ROWS) or (z == STEP_1 - 1 and hi >= STEP_2):
                continue
            far = LARGE_ROWS - 1 - k % 5 if z == STEP_1 - 1 else k % STEP_1
            for form in ("short", "long"):
                rows = [(far, TOP), (hi, TOP), (lo, TOP), (hi, TOP)] + (_pad(lo + hi) if form == "long" else [])
                out.append(Group("range", f"stepped table k {k} minimum in the {place} lo {lo} hi {hi} {form}", rows, tree="stepped",
                                 lo=lo, hi=hi, form=form, k=k, place=place, z=z, unique=True))
    # hi on a step: lcp8[hi], the first entry a range does not hold, is the table's deepest
    for lo, hi in [(0, STEP_1 - 1), (3, STEP_1 - 1)] + [(STEP_2 - 4 - 16 * (1 << k), STEP_2 - 1) for k in (0, 5, 10, 16)]:
        for form in ("short", "long"):
            rows = [(LARGE_ROWS - 1, TOP), (hi, TOP), (lo, TOP), (hi, TOP)] + (_pad(lo + hi) if form == "long" else [])
            out.append(Group("range", f"stepped table hi on a step lo {lo} hi {hi} {form}", rows, tree="stepped",
                             lo=lo, hi=hi, form=form, k=range_parts(lo, hi)[2], place=None, z=None, unique=False))
    return out


# ---- family: queries ------------------------------------------------------------------------------------------------------------

def _query_kinds(rng, q, is_long, name):
    """one query on the small tree: narrowed, unresolved, empty, one row, kept whole — by q — or a long one (narrowed)"""
    under = lambda k: [(int(rng.integers(0, len(small_tree()))), UNDER - int(rng.integers(0, 40))) for _ in range(k)]
    if is_long:
        rows = [(r, TOP) for r in small_group(rng, 10, [int(rng.integers(0, 10))])]
        return Group("queries", f"{name} query {q} long", rows[:5] + under(PAD) + rows[5:], tree="small")
    kind = q % 5
    if kind == 0:
        rows = [(r, TOP) for r in small_group(rng, 5 + q % 6, [q % 5])] + under(q % 4)
    elif kind == 1:
        rows = [(r, TOP) for r in small_group(rng, 6, [])] + [(UNMATCHED_ROW, TOP)] + under(q % 3)
    elif kind == 2:
        rows = []
    elif kind == 3:
        rows = [(int(rng.integers(0, len(small_tree()))), TOP)] + under(1) * (q % 2)
    else:
        rows = [(r, TOP) for r in small_group(rng, 7, [])] + under(q % 5)
    return Group("queries", f"{name} query {q} kind {kind}", rows, tree="small")


@functools.lru_cache(None)
def queries_family():
    """{query count: groups}: narrowed, unresolved, empty, single-row and kept queries in turn, long queries first, last and every
    41st in between (from 5 queries on) — counts either side of a wave's four queries, a block's sixteen, the 64 counter
    words' 1024 queries and the scan's block"""
    out = {}
    for count in QUERY_COUNTS:
        rng = np.random.default_rng(100 + count)
        longs = {0, count - 1} | set(range(20, count, 41)) if count >= 5 else ({1} if count == 3 else set())
        out[count] = [_query_kinds(rng, q, q in longs, f"count {count}") for q in range(count)]
    return out


REPEAT_BLOCK, REPEAT_TIMES = 42, 7000                # 294 000 queries, every seventh long


@functools.lru_cache(None)
def repeated_block():
    """42 queries to be repeated REPEAT_TIMES times: every seventh long (65 .. 75 rows), the others of 0 .. 5 rows"""
    rng = np.random.default_rng(77)
    out = []
    for q in range(REPEAT_BLOCK):
        if q % 7 == 3:
            rows = [(r, TOP) for r in small_group(rng, 9 + q % 2, [q % 9])]
            under = [(int(rng.integers(0, len(small_tree()))), UNDER) for _ in range(56 + q % 11)]
            out.append(Group("queries", f"block query {q} long", rows[:4] + under + rows[4:], tree="small"))
        else:
            kind = q % 6
            rows = {0: [], 1: [(5, TOP)], 2: [(r, TOP) for r in small_group(rng, 5, [q % 5])],
                    3: [(r, TOP) for r in small_group(rng, 3, [])] + [(UNMATCHED_ROW, TOP)],
                    4: [(r, TOP) for r in small_group(rng, 2, [])] + [(7, UNDER)], 5: [(9, TOP), (8, UNDER)]}[kind]
            out.append(Group("queries", f"block query {q} kind {kind}", rows, tree="small"))
    return out


# ---- family: scores -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def scores_family():
    """INT32_MAX on top; every row INT32_MIN (the segment is the top group); both in one segment; a negative top; the only top
    rows in the last partial 256-row sweep of segments of 257, 300 and 513 rows; top groups of 256 and 257 rows"""
    rng = np.random.default_rng(31)
    n_small = len(small_tree())
    any_rows = lambda k: [int(rng.integers(0, n_small)) for _ in range(k)]
    out = []

    def add(name, rows):
        out.append(Group("scores", name, rows, tree="small"))

    for form, pad in (("short", 0), ("long", PAD)):
        g = small_group(rng, 10, [3])
        add(f"INT32_MAX on top, {form}", [(r, INT32_MAX) for r in g] + [(r, INT32_MAX - 1 - k % 2) for k, r in enumerate(any_rows(pad + 3))])
        add(f"every row INT32_MIN, {form}", [(r, INT32_MIN) for r in small_group(rng, 10 + pad, [0, 5 + pad])])
        g = small_group(rng, 10, [9])
        add(f"INT32_MAX over INT32_MIN, {form}", [(r, INT32_MIN) for r in any_rows(3 + pad // 2)] + [(r, INT32_MAX) for r in g]
            + [(r, INT32_MIN) for r in any_rows(pad // 2)])
        g = small_group(rng, 10, [0])
        add(f"a negative top, {form}", [(r, -5) for r in g] + [(r, -6 - k % 7) for k, r in enumerate(any_rows(pad + 2))])
        add(f"INT32_MIN + 1 over INT32_MIN, {form}", [(r, INT32_MIN + 1) for r in g] + [(r, INT32_MIN) for r in any_rows(pad + 2)])
    for length in (257, 300, 513):
        n_top = length - (length - 1) // 256 * 256
        g = small_group(rng, n_top, [n_top // 2] if n_top >= 5 else [])
        add(f"the top rows in the last sweep of {length} rows", [(r, TOP - 1 - k % 50) for k, r in enumerate(any_rows(length - n_top))] + [(r, TOP) for r in g])
    for n_top in (256, 257):
        g = small_group(rng, n_top, [0, 100, n_top - 1])
        add(f"a top group of {n_top} rows", [(r, TOP) for r in g] + [(r, UNDER) for r in any_rows(20)])
        add(f"a top group of {n_top} rows behind lower rows", [(r, UNDER) for r in any_rows(20)] + [(r, TOP) for r in g])
    return out


FAMILIES = ("spread", "digit", "bin edge", "range", "queries", "scores")
# the percentages each family is checked at; at the last of each some group has need * 100000 == n * milli exactly
MILLIS = {"spread": (50001, 80000), "digit": (50001, 100000), "bin edge": (50001, 100000), "range": (75000,),
          "queries": (50001, 80000), "scores": (50001, 100000, 80000)}
