"""`build-db kraken2` and `build-db qiime2` on the GPU (csrc/seqdb_gpu.hip) at the byte-level edges of tests/seqdb_edges.py.
One rule throughout: for one listing, the files an export leaves, its outcome (ok, a quiet invalid-UTF-8 stop at line L, or an
error naming line L with its reason) and the counts in its stats equal the restatement's (tests/seqdb_reference.py), whatever
`chunk_bytes` is (4096, the floor; 8192; 0, the default, where the whole listing is one chunk and the generator's offsets are
the kernels') and whether the listing comes from a file or through a pipe fed in irregular pieces.  After an error the .fna
holds the records before the bad line and neither prelim_map.txt nor its .partial file exists."""
import os
import re
import threading

import numpy as np
import pytest

from blutils_amd import seqdb
from tests import seqdb_edges as E
from tests import seqdb_reference as R

pytestmark = pytest.mark.gpu
REASONS = (("Invalid line detected", E.PIECES), ("0x80", E.NONASCII), ("taxid is not", E.TAXID))


def _same(what, got: bytes, exp: bytes):
    if got != exp:
        k = next((i for i in range(min(len(got), len(exp))) if got[i] != exp[i]), min(len(got), len(exp)))
        raise AssertionError(f"{what}: {len(got)} vs {len(exp)} bytes, first difference at {k}: got {got[max(0, k - 60):k + 60]!r}, "
                             f"expected {exp[max(0, k - 60):k + 60]!r}")


def _feed(fd: int, data: bytes, seed: int):
    """Writes data in pieces of 1..7000 bytes and closes fd; a reader that has gone away ends it."""
    rng = np.random.default_rng(seed)
    try:
        pos = 0
        while pos < len(data):
            n = int(rng.integers(1, 7001))
            pos += os.write(fd, data[pos:pos + n])
    except BrokenPipeError:
        pass
    finally:
        os.close(fd)


def _export(d, fmt: str, listing: bytes, chunk: int, pipe: bool) -> dict:
    """One export into the new directory d: {"outcome", "fna", "map" (None: no such file), "partial", "stats"}."""
    d.mkdir()
    fna, prelim = d / ("library.fna" if fmt == E.K else "seqs.fna"), d / "prelim_map.txt"
    args = (seqdb.KRAKEN2, str(fna), str(prelim)) if fmt == E.K else (seqdb.QIIME2, str(fna), None)
    feeder, rd = None, -1
    if pipe:
        rd, wr = os.pipe()
        feeder = threading.Thread(target=_feed, args=(wr, listing, len(listing) + chunk))
        feeder.start()
        kw = dict(listing_path="the pipe", input_fd=rd)
    else:
        (d / "listing.txt").write_bytes(listing)
        kw = dict(listing_path=str(d / "listing.txt"))
    try:
        st = seqdb.export(*args, chunk_bytes=chunk, **kw)
        outcome = ("stop", st["invalid_utf8_line"]) if st["invalid_utf8_line"] else ("ok",)
    except seqdb.SeqdbError as e:
        m = re.search(r": line (\d+): (.*)$", str(e))
        assert m, str(e)
        outcome = ("error", int(m.group(1)), next((r for text, r in REASONS if text in m.group(2)), m.group(2)))
        st = e.stats
    finally:
        if pipe:
            os.close(rd)                                         # (a feeder still writing gets EPIPE)
            feeder.join()
    return {"outcome": outcome, "fna": fna.read_bytes(), "map": prelim.read_bytes() if prelim.exists() else None,
            "partial": os.path.exists(str(prelim) + ".partial"), "stats": st}


def _check(tmp_path, case, runs) -> dict:
    """The case under every (chunk_bytes, pipe) of runs against the restatement; returns {(chunk, pipe): n_chunks}."""
    exp = R.export(case.fmt == E.Q, case.listing)
    assert exp["outcome"] == case.outcome, case.name
    n_chunks = {}
    for chunk, pipe in runs:
        what = f"{case.name} chunk_bytes={chunk} {'pipe' if pipe else 'file'}"
        got = _export(tmp_path / f"{len(os.listdir(tmp_path))}", case.fmt, case.listing, chunk, pipe)
        assert got["outcome"] == exp["outcome"], what
        _same(what + " .fna", got["fna"], exp["fna"])
        assert not got["partial"], what
        st = got["stats"]
        if exp["map"] is None:
            assert got["map"] is None, what + ": prelim_map.txt exists"
        else:
            _same(what + " prelim_map.txt", got["map"], exp["map"])
        if exp["outcome"][0] != "error":
            assert st["invalid_utf8_line"] == (exp["outcome"][1] if exp["outcome"][0] == "stop" else 0), what
        assert (st["n_lines"], st["input_bytes"], st["fna_bytes"], st["map_bytes"]) == (
            exp["records"], exp["input_bytes"], len(exp["fna"]), exp["map_bytes"]), what     # (map_bytes after an error: of the records kept)
        if chunk in case.min_chunks:
            assert st["n_chunks"] >= case.min_chunks[chunk], what
        n_chunks[(chunk, pipe)] = st["n_chunks"]
    for chunk in {c for c, _ in runs}:                            # the reader fills a chunk before it cuts: pieces do not matter
        assert len({n for (c, _), n in n_chunks.items() if c == chunk}) == 1, (case.name, n_chunks)
    return n_chunks


ALL_RUNS = [(c, p) for c in E.CHUNKS for p in (False, True)]
CUT_RUNS = [(4096, False), (4096, True), (8192, False), (8192, True)]
DEFAULT_TOO = CUT_RUNS + [(0, False)]


def _part(cases, k, n):
    return cases[k::n]


def _sampled(cases, at_default):
    """(case, runs) for the many stop cases and small listings.  A call at the default chunk size pins 1 GiB and takes a
    third of a second.  A listing of less than 8192 bytes is one chunk of the same bytes at 8192 and at the default size, so
    such cases run at 4096 and 8192, from the file and the pipe, and those that at_default(index, case) picks at the
    default size too; a larger listing always does."""
    return [(c, DEFAULT_TOO if len(c.listing) >= 8192 or at_default(i, c) else CUT_RUNS) for i, c in enumerate(cases)]


@pytest.mark.parametrize("cls,fmt", E.ACCEPTED_IDS, ids=[f"{c}-{f}" for c, f in E.ACCEPTED_IDS])
def test_accepted(tmp_path, cls, fmt):
    """Classes 1 to 4 and 6: all accepted cases of a class in one listing; a wrong byte shows with its offset.  (The many
    listings of class 1 against the tile edge go through the pipe at 4096 only.)"""
    case = E.accepted(cls, fmt)
    n = _check(tmp_path, case, [(4096, False), (4096, True), (8192, False), (0, False)] if "-" in cls else ALL_RUNS)
    assert n[(0, False)] == 1
    if len(case.listing) > 20000:
        assert n[(4096, False)] >= n[(8192, False)] > 1


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("fmt", E.FORMATS)
def test_small_listings(tmp_path, fmt, k):
    """Listings that end in a run of spaces or in a character without a newline (the zero pad is read), that start with one,
    of 1, 255, 256 and 257 lines, with CRLF, and whose output is 47..49, 4095..4097 and 8192, 8193 bytes."""
    every_third = lambda i, case: i % 3 == 0                  # (which ones is decided by their position, nothing else)
    for case, runs in _part(_sampled(E.small(fmt), every_third), k, 4):
        _check(tmp_path, case, runs)


@pytest.mark.parametrize("k", range(8))
def test_invalid_utf8_stops(tmp_path, k):
    """Class 2: every ill-formed sequence at every split stops the export at its line, in kraken2 and in qiime2.  Each form
    runs at the default chunk size as the first bytes of a listing, the cut-short ones as the last bytes of one too."""
    picked = lambda i, c: c.name.endswith("-first") or c.name.startswith("two_bad") or (c.name.startswith("cut") and "-eof" in c.name)
    for case, runs in _part(_sampled(E.stops(), picked), k, 8):
        _check(tmp_path, case, runs)


@pytest.mark.parametrize("k", range(6))
def test_refused(tmp_path, k):
    """The refused spellings of classes 1 to 4: the line, the reason, the records before it, no prelim_map.txt."""
    for case in _part(E.refused(), k, 6):
        _check(tmp_path, case, DEFAULT_TOO)


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("fmt", E.FORMATS)
def test_chunk_cuts(tmp_path, fmt, k):
    """Class 5: lines against the reader's cuts at 4096 and 8192 bytes, from the file and through the pipe."""
    for case in _part(E.cuts(fmt), k, 4):
        n = _check(tmp_path, case, CUT_RUNS + ([(0, False)] if case.name.startswith(("file_of", "line_of_three")) else []))
        if case.name.startswith("file_of_4096"):                  # exactly one chunk's worth: one chunk with the newline, two without
            assert n[(4096, False)] == case.min_chunks[4096] and n[(8192, False)] == 1
        if case.name.startswith("line_of_three_chunks"):
            c = int(case.name.rsplit("_", 1)[1])
            assert n[(c, False)] < -(-len(case.listing) // c)     # the slot has grown: later chunks hold more than chunk_bytes


@pytest.mark.parametrize("k", range(6))
def test_precedence(tmp_path, k):
    """Class 7: an error before a stop and a stop before an error, in one chunk and in two; two errors; two problems on one
    line; an error several chunks in.  The .fna holds the records before the bad line at every chunk size."""
    for case in _part(E.precedence(), k, 6):
        _check(tmp_path, case, ALL_RUNS if "two_chunks" in case.name or "chunks_in" in case.name else DEFAULT_TOO)
