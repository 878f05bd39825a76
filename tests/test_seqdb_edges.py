"""The byte-level edge cases of `build-db kraken2` and `build-db qiime2` (tests/seqdb_edges.py) against the restatement alone,
without a GPU: the generator is deterministic, every class puts its cases where it says (checked on the listing's bytes and
on the restatement's output), every accepted case is accepted and every refused one is refused at its line for its reason
with the records before it, and moving the cases by pad bytes changes nothing but the pads."""
import re

import pytest

from tests import seqdb_edges as E
from tests import seqdb_reference as R

SLICE, TILE = E.SLICE, E.TILE
PAD_RECORD = {E.K: re.compile(rb">kraken:taxid\|1\|Px*\nA?\n"), E.Q: re.compile(rb">1-0-Px*\na?\n")}


def _ref(case):
    return R.export(case.fmt == E.Q, case.listing)


def _runs(case):
    """The marked runs, each checked to be exactly n spaces between two other bytes."""
    b = case.listing
    for start, n, where in case.marks["run"]:
        assert b[start:start + n] == b" " * n and b[start - 1:start] != b" " and b[start + n:start + n + 1] != b" "
        assert (start + n == len(b)) == (where == "end")
    return case.marks["run"]


def _record_of_line(case, start):
    """The restatement's record of the one line that holds offset start."""
    b = case.listing
    ls = b.rfind(b"\n", 0, start) + 1
    le = b.find(b"\n", start)
    return R.export(case.fmt == E.Q, b[ls:le + 1])["fna"]


def test_generator_is_deterministic_per_seed():
    for cls, fmt in E.ACCEPTED_IDS:
        a = E.accepted(cls, fmt, 3).listing
        E.accepted.cache_clear()
        assert E.accepted(cls, fmt, 3).listing == a
        assert E.accepted(cls, fmt, 4).listing != a
    for fn in (E.stops, E.refused, E.precedence):
        a = [c.listing for c in fn()]
        fn.cache_clear()
        assert [c.listing for c in fn()] == a
    for fmt in E.FORMATS:
        a = [c.listing for c in E.cuts(fmt) + E.small(fmt)]
        E.cuts.cache_clear()
        E.small.cache_clear()
        assert [c.listing for c in E.cuts(fmt) + E.small(fmt)] == a


@pytest.mark.parametrize("cls,fmt", E.ACCEPTED_IDS, ids=[f"{c}-{f}" for c, f in E.ACCEPTED_IDS])
def test_accepted_listings_are_accepted_and_of_moderate_size(cls, fmt):
    case = E.accepted(cls, fmt)
    r = _ref(case)
    assert r["outcome"] == ("ok",) and r["records"] == case.listing.count(b"\n") and r["input_bytes"] == len(case.listing)
    assert len(case.listing) < 500_000


@pytest.mark.parametrize("fmt", E.FORMATS)
def test_parity_short_fires(fmt):
    case = E.accepted("parity_short", fmt)
    runs = _runs(case)
    for where in E.WHERE:
        ns = [n for n in E.SHORT_RUNS if E.run_line(fmt, where, n, b"A") is not None]
        assert {(n, s % SLICE) for s, n, w in runs if w == where} == {(n, r) for n in ns for r in range(SLICE)}
        assert ns == E.SHORT_RUNS or (fmt == E.K and where != "after_seq")
    assert any(s // SLICE != (s + n - 1) // SLICE for s, n, _ in runs) and any(s // TILE != (s + n - 1) // TILE for s, n, _ in runs)
    # which piece is which, stated by hand: a run of n spaces is n // 2 separators and, for odd n, a blank that is trimmed
    for start, n, where in runs:
        rec = _record_of_line(case, start)
        if where == "after_seq":
            assert rec.endswith(b"\n" + (b"acgt tail" if n == 1 else b"acgt").upper() + b"\n" if fmt == E.K else
                                b"\n" + (b"acgt tail" if n == 1 else b"acgt") + b"\n")
        elif where == "before_seq":
            body = b"" if n >= 4 else b"acgt" if n >= 2 else b"c"
            assert rec.endswith(b"\n" + (body.upper() if fmt == E.K else body) + b"\n")
        elif fmt == E.Q:
            pieces = ([b"T7", b"O8", b"Sacgt"] if n in (2, 3) else [b"O8", b"Sacgt", b"Xtra"] if n == 1 else
                      [b"", b"T7", b"O8"] if n in (4, 5) else [b"", b"", b"T7"] if n in (6, 7) else [b"", b"", b""])
            acc = rec[rec.index(b"-", rec.index(b"-") + 1) + 1:rec.index(b"\n")]
            assert rec == b">" + pieces[0] + b"-" + pieces[1] + b"-" + acc + b"\n" + pieces[2] + b"\n"
            assert (b" T7" in acc) == (n == 1)
        else:
            acc = case.listing[case.listing.rfind(b"\n", 0, start) + 1:start]
            assert rec == (b">kraken:taxid|8|" + acc + b" 7\nACGT\n" if n == 1 else b">kraken:taxid|7|" + acc + b"\n8\n")
    # blanks of every kind around the pieces, pieces of blanks only
    at = case.marks["blanks"][0]
    got = R.export(fmt == E.Q, case.listing[at:])["fna"]
    if fmt == E.K:
        assert got.startswith(b">kraken:taxid|7|B1\nAC GT\n>kraken:taxid|7|\nACGT\n>kraken:taxid|7|B3\n\n>kraken:taxid|7|B4\nAC\tGT\n")
    else:
        assert got.startswith(b">7-0-B1\nac gt\n>7--\nacgt\n>7-9-B3\n\n>7-9-B4\nac\tgt\n")


def _front(fmt, n):
    """Where a run at the `front` place stands: after the accession, unless kraken2 would find its taxid empty."""
    return "acc_taxid" if fmt == E.Q or n <= 3 else "before_seq"


def _check_records(case, runs):
    for start, n, where in runs:
        rec = _record_of_line(case, start)
        if where == "after_seq":
            assert rec.lower().endswith(b"\nacgt tail\n" if n == 1 else b"\nacgt\n")
        elif n >= 8:
            assert rec.endswith(b"\n\n")                         # every piece after the first is empty


@pytest.mark.parametrize("fmt", E.FORMATS)
def test_parity_at_the_tile_edge_fires(fmt):
    """Every run of 1..40 spaces begins 0, 1, 2 and 3 bytes before a multiple of 4096, at both places."""
    seen = set()
    for name, (place, lengths) in E.TILE_PARTS.items():
        case = E.accepted(name, fmt)
        runs = _runs(case)
        assert {(n, -s % TILE, w) for s, n, w in runs} == {(n, d, _front(fmt, n) if place == "front" else place) for n in lengths for d in range(4)}
        assert all((s + n - 1) // TILE > (s - 1) // TILE for s, n, _ in runs if n > 4)      # the run crosses a multiple of 4096
        _check_records(case, runs)
        seen |= {(n, -s % TILE, place) for s, n, _ in runs}
    assert seen == {(n, d, p) for n in E.SHORT_RUNS for d in range(4) for p in E.PLACES}


@pytest.mark.parametrize("n", E.LONG_RUNS)
@pytest.mark.parametrize("fmt", E.FORMATS)
def test_parity_long_fires(fmt, n):
    """A run of 4094..4100 and 8190..8194 spaces starts at every offset modulo 16 and 0..3 bytes before a multiple of 4096, at
    both places, and spans one or two tile edges."""
    case = E.accepted(f"parity_long-{n}", fmt)
    runs = _runs(case)
    assert {m for _, m, _ in runs} == {n} and n <= 3 * TILE
    for where in (_front(fmt, n), "after_seq"):
        starts = [s for s, _, w in runs if w == where]
        assert {s % SLICE for s in starts} == set(range(SLICE)) and {-s % TILE for s in starts} >= {0, 1, 2, 3}
    edges = [(s + n - 1) // TILE - s // TILE for s, _, _ in runs]          # multiples of 4096 inside the run
    assert min(edges) >= (n - 1) // TILE and max(edges) == (n - 2) // TILE + 1 >= 1
    _check_records(case, runs)


@pytest.mark.parametrize("fmt", E.FORMATS)
def test_utf8_ok_fires(fmt):
    case = E.accepted("utf8_ok", fmt)
    b = case.listing
    r = _ref(case)
    seen = set()
    for start, n, piece in case.marks["char"]:
        ch = b[start:start + n]
        assert ch in E.VALID and len(ch.decode("utf-8")) == 1
        for s in range(1, n):
            if (start + s) % SLICE == 0:
                seen.add((ch, s, piece, "slice"))
            if (start + s) % TILE == 0:
                seen.add((ch, s, "tile"))
    pieces = (0,) if fmt == E.K else (0, 1, 2, 3)
    assert {x for x in seen if x[-1] == "slice"} == {(ch, s, p, "slice") for ch in E.VALID for s in range(1, len(ch)) for p in pieces}
    assert {x for x in seen if x[-1] == "tile"} == {(ch, s, "tile") for ch in E.VALID for s in range(1, len(ch))}
    for ch in E.VALID:                                            # copied: kraken2 into both files
        assert r["fna"].count(ch) == b.count(ch) > 0
        assert fmt == E.Q or r["map"].count(ch) == b.count(ch)


def test_out_small_fires():
    case = E.accepted("out_small", E.Q)
    fna = _ref(case)["fna"]
    starts = [m.start() for m in re.finditer(rb">", fna)]
    for start, n in case.marks["record"]:
        assert start in starts and fna[start + n - 1:start + n + 1] == b"\n>" and fna[start:start + n].count(b">") == 1
    assert b">--\n\n" in fna and {n for _, n in case.marks["record"]} >= set(range(5, 41))
    assert {s % SLICE for s, n in case.marks["record"] if n == 5} == set(range(SLICE))
    assert {(s + n) % SLICE for s, n in case.marks["record"]} == set(range(SLICE))
    per_slice = {}
    for s in starts:
        per_slice[s // SLICE] = per_slice.get(s // SLICE, 0) + 1
    assert max(per_slice.values()) == 4                           # one writer thread, four records
    edge = [(s % TILE, (s + n) % TILE, s // TILE != (s + n - 1) // TILE) for s, n in case.marks["tile_record"]]
    assert any(a == 0 for a, _, _ in edge) and any(e == 0 for _, e, _ in edge) and any(x and e for _, e, x in edge)
    assert len(fna) > 2 * TILE


def test_out_wrap_fires():
    case = E.accepted("out_wrap", E.K)
    fna = _ref(case)["fna"]
    newline = set()
    for start, h, n in case.marks["wrap"]:
        assert fna[start:start + 14] == b">kraken:taxid|" and fna[start + h - 1] == 10
        body = fna[start + h:fna.find(b">", start + 1) if b">" in fna[start + 1:start + h + n + n // 80 + 3] else len(fna)]
        assert body.endswith(b"\n") and len(body.replace(b"\n", b"")) == n and all(len(x) <= 80 for x in body.split(b"\n"))
        assert body.count(b"\n") == 1 + (n - 1) // 80 if n else body == b"\n"
        if n > 80:
            assert fna[start + h + 80] == 10
            newline.add((n, (start + h + 80) % SLICE))
            newline.add((n, "tile", (start + h + 80) % TILE))
    assert {(n, s % SLICE) for s, _, n in case.marks["wrap"]} >= {(n, r) for n in E.WRAP_LENGTHS for r in range(SLICE)}
    assert {n for _, _, n in case.marks["wrap"]} == set(E.WRAP_LENGTHS + E.LONG_LENGTHS)
    for n in (81, 161, 162, 4080, 4095, 4096, 4097):
        assert {(n, 15), (n, 0), (n, "tile", TILE - 1), (n, "tile", 0)} <= newline


def test_taxids_fire():
    case = E.accepted("taxids", E.K)
    r = _ref(case)
    lines = r["map"].split(b"\n")
    texts = [t for _, t in case.marks["taxid"]]
    assert [b"18446744073709551615", b"+0", b"0" * 100] == [t for t in texts if t in (b"18446744073709551615", b"+0", b"0" * 100)]
    assert {len(b"%d" % int(t)) for t in texts} == set(range(1, 21))
    for (k, t), line in zip(case.marks["taxid"], lines):
        assert line.split(b"\t")[2] == b"%d" % int(t) and line.split(b"|")[1] == b"%d" % int(t)
        assert b">kraken:taxid|" + t + b"|" in r["fna"]          # the header keeps the spelling
    for e in range(20):
        assert b"%d" % 10 ** e in texts and b"%d" % (10 ** e - 1) in texts


@pytest.mark.parametrize("fmt", E.FORMATS)
def test_small_listings_fire(fmt):
    names = set()
    for case in E.small(fmt):
        r = _ref(case)
        b = case.listing
        assert r["outcome"] == ("ok",) and r["input_bytes"] == len(b), case.name
        names.add(case.name)
        for total in case.marks.get("total", []):
            assert len(r["fna"]) == total
        for start, n, where in (_runs(case) if "run" in case.marks else []):
            assert where == "end" and not b.endswith(b"\n") and len(b) % SLICE == int(case.name.rsplit("-", 1)[1])
            assert r["fna"].lower().endswith(b"\nacgt\n")         # the trailing run is trimmed or ends the sequence
        for start, n, piece in case.marks.get("char", []):
            assert b[start:start + n] in E.VALID and (start == 0 or start + n == len(b))
        if case.name.startswith("lines_"):
            assert r["records"] == int(case.name[6:]) == b.count(b"\n")
    crlf, = [c for c in E.small(fmt) if c.name == "crlf"]
    assert crlf.listing.count(b"\r\n") == crlf.listing.count(b"\n") == 256
    assert b"\r" not in _ref(crlf)["fna"]
    assert {f"output_of_{t}_bytes" for t in (47, 48, 49, 4095, 4096, 4097)} <= names and {"lines_1", "lines_255", "lines_256", "lines_257"} <= names
    if fmt == E.Q:
        assert R.qiime2_sequences(b"      \n      \r\n      ")[0] == b">--\n\n" * 3


@pytest.mark.parametrize("fmt", E.FORMATS)
def test_cuts_fire(fmt):
    cases = {c.name: c for c in E.cuts(fmt)}
    firsts = set()
    for name, case in cases.items():
        b = case.listing
        r = _ref(case)
        assert r["outcome"] == ("ok",) and r["input_bytes"] == len(b), name
        assert set(case.min_chunks) <= {4096, 8192} and all(v >= 1 for v in case.min_chunks.values())
        if name.startswith("lead_"):
            firsts.add((b.find(b"\n") + 1) % 64 if int(name[5:]) else 0)
            assert len(b) > 3 * 4096 and case.min_chunks[4096] >= 4
        for at in case.marks.get("newline_at", []):
            assert b[at] == 10
        for pos, n in case.marks.get("line", []):
            assert b[pos + n - 1] == 10 and b.count(b"\n", pos, pos + n) == 1 and n in (4096, 4097, 8192)
        for start, n, _ in case.marks.get("char", []):
            assert start < TILE < start + n and b[start:start + n] in E.VALID
    assert firsts == set(range(64))                               # the lines after the pad pass every position modulo 64
    assert cases["crlf_across_4096"].listing[4095:4097] == b"\r\n"
    for name in ("file_of_4096-newline", "file_of_4096-no_newline"):
        assert len(cases[name].listing) == 4096 and cases[name].listing.endswith(b"\n") == (name.endswith("-newline"))
    for c in (4096, 8192):
        b = cases[f"line_of_three_chunks_of_{c}"].listing
        assert max(len(x) for x in b.split(b"\n")) == 3 * c - 1 and b.count(b"\n") > 50
    assert {f"newline_at_{a}" for a in (4095, 4096, 8191, 8192)} <= set(cases)
    assert {f"line_of_{n}-{w}" for n in (4096, 4097, 8192) for w in ("first", "second")} <= set(cases)


def test_stops_fire():
    """Every ill-formed form, at every split, stops the restatement at the stated line with the records before it."""
    per_form = {}
    for case in E.stops():
        b = case.listing
        r = _ref(case)
        assert r["outcome"] == case.outcome and case.outcome[0] == "stop", case.name
        assert r["records"] == case.outcome[1] - 1 and r["fna"].count(b">") == r["records"]
        assert r["input_bytes"] == len(b"".join(x + b"\n" for x in b.split(b"\n")[:r["records"]]))
        if case.name.startswith("two_bad_bytes"):
            assert b.count(b"\xff") == 1 and b.count(b"\x80") == 1 and b.index(b"\xff") < b.index(b"\x80")
            continue
        form, place = case.name.rsplit("-", 1)
        (start, n), = case.marks["bad"]
        assert b[start:start + n] == E.INVALID[form]
        assert b.count(b"\n", 0, start) + 1 == case.outcome[1]
        with pytest.raises(UnicodeDecodeError):
            b[b.rfind(b"\n", 0, start) + 1:(b.find(b"\n", start) + 1) or len(b)].decode("utf-8")
        if place.startswith("slice"):
            s = int(place[5:])
            assert (start + s) % SLICE == 0 if n > 1 else start % SLICE == (0, 15)[s]
        elif place == "tile":
            assert start // TILE != (start + n - 1) // TILE if n > 1 else start % TILE in (0, TILE - 1)
        elif place == "first":
            assert start == 0
        elif place == "eol":
            assert b[start + n] == 10
        else:
            assert start + n == len(b) and len(b) % SLICE == int(place[3:])
        per_form.setdefault(form, set()).add(place)
    for form, text in E.INVALID.items():
        want = {f"slice{s}" for s in (range(1, len(text)) if len(text) > 1 else (0, 1))} | {"tile", "first"}
        assert want <= per_form[form] and per_form[form] & {"eof0", "eof1"}, form
        assert not form.startswith("cut") or {"eol", "eof0", "eof1"} <= per_form[form]
    # the forms the issue lists, each by its first bytes
    heads = {E.INVALID[f][:2] for f in E.INVALID}
    assert {b"\xc0\x80", b"\xc1\xbf", b"\xe0\x80", b"\xe0\x9f", b"\xf0\x80", b"\xf0\x8f", b"\xed\xa0", b"\xed\xbf", b"\xf4\x90", b"\xf5\x80",
            b"\xff", b"\x80"} <= heads


@pytest.mark.parametrize("fn", [E.refused, E.precedence], ids=["refused", "precedence"])
def test_refused_cases_are_refused_at_their_line_for_their_reason(fn):
    kinds = set()
    for case in fn():
        b = case.listing
        r = _ref(case)
        assert r["outcome"] == case.outcome, case.name
        line = case.outcome[1]
        before = b"".join(b.split(b"\n")[k] + b"\n" for k in range(line - 1))
        good = R.export(case.fmt == E.Q, before)
        assert good["outcome"] == ("ok",) and good["fna"] == r["fna"] and good["records"] == r["records"] == line - 1
        assert r["input_bytes"] == len(before) and (r["map"] is None) == (case.fmt == E.Q or case.outcome[0] == "error")
        assert r["map_bytes"] == len(good["map"] or b"")
        kinds.add(case.outcome[0] if case.outcome[0] == "stop" else case.outcome[2])
        for at in case.marks.get("nonascii_at", []):              # the last sequence byte of the first bad record, were it written
            acc = b.split(b"\n")[line - 1].split(b"  ")[0]
            assert at == len(good["fna"]) + len(b">kraken:taxid|7|" + acc + b"\nacg" + E.VALID[0]) - 1
            assert at % SLICE == int(case.name.rsplit("-", 1)[1]) and b.split(b"\n")[line].startswith(b"  7  " + E.VALID[0])
    assert kinds >= {E.PIECES, E.TAXID, E.NONASCII}
    if fn is E.precedence:
        assert "stop" in kinds
        far = [c for c in fn() if "two_chunks" in c.name]
        assert len(far) == 4 and all(c.listing.rfind(b"\xff") - c.listing.find(b"B") > 8192 or c.listing.find(b"\xff") < c.listing.rfind(b"B  7") - 8192
                                     for c in far)


@pytest.mark.parametrize("cls,fmt", E.ACCEPTED_IDS, ids=[f"{c}-{f}" for c, f in E.ACCEPTED_IDS])
def test_moving_the_cases_by_pad_bytes_changes_only_the_pads(cls, fmt):
    """A lead of 37 bytes moves every case; the pads before each put it back.  Without the pad records the output is the same."""
    a, b = E.accepted(cls, fmt), E.accepted(cls, fmt, 0, 37)
    assert a.listing != b.listing and (cls == "taxids" or not b.listing.endswith(a.listing))      # (taxids: nothing is aligned)
    ra, rb = _ref(a), _ref(b)
    assert rb["outcome"] == ("ok",)
    strip = lambda fna: PAD_RECORD[fmt].sub(b"", fna)
    assert strip(ra["fna"]) == strip(rb["fna"]) and len(strip(ra["fna"])) > 0
    if cls != "taxids":
        assert ra["fna"] != rb["fna"]
    assert {k: len(v) for k, v in a.marks.items()} == {k: len(v) for k, v in b.marks.items()}
