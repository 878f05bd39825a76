"""`build-db sintax` and `build-db dada2` on the GPU (csrc/seqdb_gpu.hip: seqdb_label_lines, seqdb_label_ascii,
seqdb_write_labelled) at the byte-level edges of tests/seqdb_label_edges.py.  One rule throughout, that of
tests/test_gpu_seqdb_label.py: for one taxonomies document and one listing the .fna an export leaves, its outcome (ok, a quiet
invalid-UTF-8 stop at line L, or an error naming line L with its reason) and `n_unknown_taxid`, `n_unlabelled`, `n_lines` less
the skipped lines, `input_bytes`, `fna_bytes`, `n_rows` and `label_bytes` equal the restatement's
(tests/seqdb_label_reference.py), in both formats.

Every case runs at `chunk_bytes` 4096 and 8192; a listing shorter than 8192 bytes is then one chunk and the generator's offsets
are the kernels'.  A call at the default chunk size pins 1 GiB and takes a third of a second, so it is made for the cases that
ask for it (position-critical and longer than 8192 bytes), for every other listing of 8192 bytes or more but the leading-pad
sweep of the chunk cuts (whose property is the reader's cut, which the default size does not make), and for every seventh of
the rest, by position in the list.  The first case of every class also goes through a pipe fed in irregular pieces."""
import functools
import json
import os
import re
import threading

import numpy as np
import pytest

from blutils_amd import seqdb
from tests import seqdb_label_edges as G
from tests import seqdb_label_reference as LR

pytestmark = pytest.mark.gpu
FMT = {G.SINTAX: seqdb.SINTAX, G.DADA2: seqdb.DADA2}
REASONS = (("Invalid line detected", G.PIECES), ("0x80", G.NONASCII), ("taxid is not", G.TAXID))
DOCS = ("corpus", "edges", "no_label", "no_label_but_the_last")


@pytest.fixture(scope="module")
def tax(tmp_path_factory):
    """{document name: the path of its taxonomies file}, written once"""
    d = tmp_path_factory.mktemp("label_edges_tax")
    out = {}
    for name in DOCS:
        out[name] = str(d / f"{name}.blutils.json")
        with open(out[name], "w") as f:
            json.dump(G.document(name), f)
    return out


@functools.lru_cache(maxsize=None)
def _expected(cls: str, name: str, fmt: str) -> dict:
    """The restatement's export of one case, computed once and left unchanged."""
    case = next(c for c in (G.corpus() if cls == "A" else G.edge_cases()) if c.cls == cls and c.name == name)
    return LR.export(fmt, G.document(case.doc), case.listing)


@functools.lru_cache(maxsize=None)
def _label_bytes(doc: str, fmt: str) -> int:
    return sum(len(lab) for _, lab in LR.rows(fmt, G.document(doc)))


def _same(what, got: bytes, exp: bytes):
    if got != exp:
        k = next((i for i in range(min(len(got), len(exp))) if got[i] != exp[i]), min(len(got), len(exp)))
        raise AssertionError(f"{what}: {len(got)} vs {len(exp)} bytes, first difference at {k}: got {got[max(0, k - 60):k + 60]!r}, "
                             f"expected {exp[max(0, k - 60):k + 60]!r}")


def _feed(fd: int, data: bytes, seed: int):
    rng = np.random.default_rng(seed)
    try:
        pos = 0
        while pos < len(data):
            pos += os.write(fd, data[pos:pos + int(rng.integers(1, 7001))])
    except BrokenPipeError:
        pass
    finally:
        os.close(fd)


def _export(d, fmt: str, tax_path: str, listing: bytes, chunk: int, pipe: bool) -> dict:
    d.mkdir()
    fna = d / "seqs.fna"
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
        st = seqdb.export_labelled(FMT[fmt], tax_path, str(fna), chunk_bytes=chunk, **kw)
        outcome = ("stop", st["invalid_utf8_line"]) if st["invalid_utf8_line"] else ("ok",)
    except seqdb.SeqdbError as e:
        m = re.search(r": line (\d+): (.*)$", str(e))
        assert m, str(e)
        outcome = ("error", int(m.group(1)), next((r for text, r in REASONS if text in m.group(2)), m.group(2)))
        st = e.stats
    finally:
        if pipe:
            os.close(rd)
            feeder.join()
    return {"outcome": outcome, "fna": fna.read_bytes(), "stats": st}


def _check(tmp_path, tax, case, runs):
    """One case in each of its formats under every (chunk_bytes, pipe) of runs, whole, against the restatement."""
    for fmt in case.fmts:
        exp = _expected(case.cls, case.name, fmt)
        assert exp["outcome"] == case.outcome, (case.name, fmt)
        for chunk, pipe in runs:
            what = f"{case.cls} {case.name} {fmt} chunk_bytes={chunk} {'pipe' if pipe else 'file'}"
            got = _export(tmp_path / f"run-{len(os.listdir(tmp_path))}", fmt, tax[case.doc], case.listing, chunk, pipe)
            st = got["stats"]
            assert got["outcome"] == exp["outcome"], what
            _same(what + " .fna", got["fna"], exp["fna"])
            if exp["outcome"][0] != "error":
                assert st["invalid_utf8_line"] == (exp["outcome"][1] if exp["outcome"][0] == "stop" else 0), what
            assert (st["n_unknown_taxid"], st["n_unlabelled"]) == (exp["n_unknown_taxid"], exp["n_unlabelled"]), what
            assert st["n_lines"] - st["n_unknown_taxid"] - st["n_unlabelled"] == exp["records"], what
            assert (st["input_bytes"], st["fna_bytes"]) == (exp["input_bytes"], len(exp["fna"])), what
            assert st["n_rows"] == len(G.document(case.doc)["taxonomies"]), what
            assert st["label_bytes"] == _label_bytes(case.doc, fmt), what
            if chunk == 0:
                assert st["n_chunks"] == (1 if case.listing else 0), what
            if chunk in case.min_chunks:
                assert st["n_chunks"] >= case.min_chunks[chunk], what


def _runs(i: int, case, pipe: bool):
    runs = [(4096, False), (8192, False)]
    if case.at_default or (len(case.listing) >= 8192 and not case.name.startswith("cuts/lead_")) or i % 7 == 3:      # (7: coprime with every number of parts below)
        runs.append((0, False))
    return runs + ([(4096, True)] if pipe else [])


def _go(tmp_path, tax, cases, k=0, n=1):
    """Part k of n of the cases; the first case of the list through the pipe too."""
    for i, case in list(enumerate(cases))[k::n]:
        _check(tmp_path, tax, case, _runs(i, case, pipe=i == 0))


# ---- A -------------------------------------------------------------------------------------------------------------------
A_ORIGINS = {"accepted": 10, "small": 8, "cuts": 8, "stops": 8, "precedence": 4, "refused": 6}      # parts: a few seconds each


@pytest.mark.parametrize("origin,k", [(o, k) for o, n in A_ORIGINS.items() for k in range(n)])
def test_corpus(tmp_path, tax, origin, k):
    """Class A: every kraken2 case of tests/seqdb_edges.py (separator parity across slices and tiles, UTF-8 stops, chunk cuts
    with their `min_chunks`, precedence, refusals) through seqdb_label_lines, against a document that writes some lines and
    skips others for each of the two reasons."""
    cases = [c for c in G.corpus() if c.marks["origin"][0] == origin]
    assert cases
    _go(tmp_path, tax, cases, k, A_ORIGINS[origin])


# ---- B -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(6))
def test_b1_nonascii_at_every_slice_position(tmp_path, tax, k):
    """A sequence byte >= 0x80 at every offset modulo 16 and at 4095 modulo 4096 (a character split across two threads and
    across two blocks), first, last and inside the sequence, in lines that would be written, that have no row and whose row
    has no label: the error names the line, the records and the counts are those before it."""
    _go(tmp_path, tax, G.b1_refused(), k, 6)


def test_b2_high_bytes_outside_the_sequence(tmp_path, tax):
    """The same bytes at the same positions as the last bytes of an accession and in a fourth piece: accepted."""
    _go(tmp_path, tax, [G.b2_accepted()])


@pytest.mark.parametrize("k", range(6))
def test_b3_several_lines_in_one_slice(tmp_path, tax, k):
    """Lines of 7 to 9 bytes: the thread steps from the line of its first byte to the line of the bad byte, past accepted
    bytes >= 0x80 in earlier lines of the same 16 bytes."""
    _go(tmp_path, tax, G.b3_several_lines_in_a_slice(), k, 6)


def test_b4_b5_b6_end_of_file_first_of_two_and_precedence(tmp_path, tax):
    """The bad bytes as the last of the file at sizes 1, 2, 15, 0 modulo 16 and 1, 0 modulo 4096, with an open last line and
    with a newline; two bad lines in two blocks (at 4096: in two chunks), the first is named; pieces before nonascii."""
    _go(tmp_path, tax, G.b4_end_of_file())
    _go(tmp_path, tax, G.b5_first_of_two())
    _go(tmp_path, tax, G.b6_precedence())


# ---- C -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", G.FORMATS)
def test_c1_tiny_records(tmp_path, tax, fmt):
    """48 shortest records (5 bytes in dada2, 13 in sintax): several record starts in every 16 output bytes, from output offsets
    4095 and 0 modulo 4096."""
    _go(tmp_path, tax, G.c1_tiny_records(fmt))


@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("fmt", G.FORMATS)
def test_c2_skipped_runs_at_every_boundary(tmp_path, tax, fmt, k):
    """Runs of 1 ... 4100 skipped lines behind a record that ends 2 and 1 bytes before, at and 1 byte behind a multiple of 16
    and of 4096; a shortest record follows.  The 4100-line runs at the default chunk size too."""
    _go(tmp_path, tax, G.c2_skipped_runs(fmt), k, 3)


def test_c3_skipped_lines_at_the_ends_of_a_chunk(tmp_path, tax):
    """The first and the last 1, 256 and 257 lines skipped, with and without a final newline; one written line: the first,
    the last, line 257."""
    _go(tmp_path, tax, G.c3_ends_of_a_chunk())


@pytest.mark.parametrize("fmt", G.FORMATS)
def test_c4_output_totals(tmp_path, tax, fmt):
    """Outputs of 5 (dada2), 13, 15, 16, 17, 4095, 4096, 4097, 8192 and 8193 bytes, skipped lines behind the last record."""
    _go(tmp_path, tax, G.c4_totals(fmt))


@pytest.mark.parametrize("k", range(2))
@pytest.mark.parametrize("fmt", G.FORMATS)
def test_c5_long_pieces(tmp_path, tax, fmt, k):
    """A label of 5000 and of 9000 bytes and (sintax) an accession of 5000 bytes, first byte at output offset 4090 ... 4097
    modulo 4096: whole slices and a whole tile inside one piece; a shortest record directly behind."""
    _go(tmp_path, tax, G.c5_long_pieces(fmt), k, 2)


def test_c6_no_row_has_a_label(tmp_path, tax):
    """50 rows without a label (what dada2 makes of a database built without `-r superkingdom=d`): the label blob is empty, the
    .fna too, every joined line is counted; with a labelled row behind them the blob starts at that row."""
    none, one = G.c6_no_label()
    for fmt in G.FORMATS:
        exp = _expected(none.cls, none.name, fmt)
        assert _label_bytes(none.doc, fmt) == 0 and exp["fna"] == b"" and exp["n_unlabelled"] == sum(t <= 50 for t in none.marks["taxids"])
        assert _label_bytes(one.doc, fmt) > 0 and _expected(one.cls, one.name, fmt)["records"] > 0
    _check(tmp_path, tax, none, [(4096, False), (8192, False), (0, False), (4096, True)])
    _check(tmp_path, tax, one, [(4096, False), (8192, False), (0, False)])


# ---- D -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(4))
def test_d_counts_stop_at_the_bad_line(tmp_path, tax, k):
    """A refused line of each reason and an invalid-UTF-8 stop at line 1, at line 257, as the last line of a 4096-byte chunk
    and as the first of the next, with 300 lines of all three kinds behind it in its chunk: `n_unknown_taxid` and `n_unlabelled`
    count the lines before it only."""
    _go(tmp_path, tax, G.d_counts(), k, 4)
