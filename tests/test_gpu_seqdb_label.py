"""`build-db sintax` and `build-db dada2` on the GPU (csrc/seqdb_gpu.hip: seqdb_label_lines, seqdb_label_ascii,
seqdb_write_labelled).  One rule throughout: for one taxonomies document and one listing, the .fna an export
leaves, its outcome (ok, a quiet invalid-UTF-8 stop at line L, or an error naming line L with its reason) and the counts in
its stats equal the restatement's (tests/seqdb_label_reference.py) at `chunk_bytes` 4096 (the floor), 8192 and 0 (the
default: the whole listing is one chunk), from a file and, in one case, through a pipe fed in irregular pieces.

A label of one byte cannot exist (the shortest are `d:x` and `x;`), so the boundary cases use identifiers of 1, 13 to 17 and
300 bytes: labels of 3, 15 to 19 and 302 bytes in sintax, of 2, 14 to 18 and 301 bytes in dada2."""
import json
import os
import re
import threading

import numpy as np
import pytest

from blutils_amd import seqdb
from tests import seqdb_label_reference as LR

pytestmark = pytest.mark.gpu
FMT = {LR.SINTAX: seqdb.SINTAX, LR.DADA2: seqdb.DADA2}
FORMATS = [LR.SINTAX, LR.DADA2]
CHUNKS = [4096, 8192, 0]
REASONS = (("Invalid line detected", "pieces"), ("0x80", "nonascii"), ("taxid is not", "taxid"))
ALPHABET = b"acgtnACGTNryswkmbdhvRYSWKMBDHV-*"
IDENT_LENGTHS = [1, 13, 14, 15, 16, 17, 300]


def _seq(n: int, salt: int = 0) -> bytes:
    return bytes(ALPHABET[(i * 7 + salt) % len(ALPHABET)] for i in range(n))


def _document(rows):
    """rows: (taxid, textLineage)"""
    return {"blutilsVersion": "8.3.1", "sourceDatabase": "db", "taxonomies": [
        {"taxid": t, "rank": "s", "numericLineage": f"d__{t}", "textLineage": lin, "accessions": []} for t, lin in rows]}


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


def _export(d, fmt: str, tax: str, listing: bytes, chunk: int, pipe: bool) -> dict:
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
        st = seqdb.export_labelled(FMT[fmt], tax, str(fna), chunk_bytes=chunk, **kw)
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


def _check(tmp_path, fmt, doc, listing: bytes, runs=None, name="") -> dict:
    """The export under every (chunk_bytes, pipe) of runs against the restatement, whole; returns the restatement's dict."""
    tax = tmp_path / f"tax-{len(os.listdir(tmp_path))}.blutils.json"
    tax.write_text(json.dumps(doc))
    exp = LR.export(fmt, doc, listing)
    for chunk, pipe in runs or [(c, False) for c in CHUNKS]:
        what = f"{name} {fmt} chunk_bytes={chunk} {'pipe' if pipe else 'file'}"
        got = _export(tmp_path / f"run-{len(os.listdir(tmp_path))}", fmt, str(tax), listing, chunk, pipe)
        st = got["stats"]
        print(what, got["outcome"], {k: v for k, v in st.items() if not k.startswith("t_")})
        assert got["outcome"] == exp["outcome"], what
        _same(what + " .fna", got["fna"], exp["fna"])
        if exp["outcome"][0] != "error":
            assert st["invalid_utf8_line"] == (exp["outcome"][1] if exp["outcome"][0] == "stop" else 0), what
        assert (st["n_unknown_taxid"], st["n_unlabelled"]) == (exp["n_unknown_taxid"], exp["n_unlabelled"]), what
        assert st["n_lines"] - st["n_unknown_taxid"] - st["n_unlabelled"] == exp["records"], what
        assert (st["input_bytes"], st["fna_bytes"]) == (exp["input_bytes"], len(exp["fna"])), what
        assert st["n_rows"] == len(doc["taxonomies"]), what
        assert st["label_bytes"] == sum(len(lab) for _, lab in LR.rows(fmt, doc)), what
        if chunk == 0:
            assert st["n_chunks"] == (1 if listing else 0), what
        elif len(listing) > 3 * chunk and exp["outcome"] == ("ok",):
            assert st["n_chunks"] > 2, what
    return exp


# ---- output boundaries -------------------------------------------------------------------------------------------------
def _boundary_doc():
    """taxid 1 + k: an identifier of IDENT_LENGTHS[k] bytes under `d`"""
    return _document([(1 + k, "d__" + ("x" if n == 1 else "L" + "m" * (n - 2) + "R")) for k, n in enumerate(IDENT_LENGTHS)])


def _markers(fmt, acc_n, lab_n, seq_n):
    """offsets in one record of the bytes whose place matters, by name"""
    if fmt == LR.SINTAX:
        return {">": 0, ";tax=": 1 + acc_n, "tax=_end": 5 + acc_n, "label_first": 6 + acc_n, "label_last": 5 + acc_n + lab_n,
                ";": 6 + acc_n + lab_n, "header_nl": 7 + acc_n + lab_n, "final_nl": 8 + acc_n + lab_n + seq_n}
    return {">": 0, "label_first": 1, "label_last": lab_n, "header_nl": 1 + lab_n, "final_nl": 2 + lab_n + seq_n}


def _record_len(fmt, acc_n, lab_n, seq_n):
    return _markers(fmt, acc_n, lab_n, seq_n)["final_nl"] + 1


def _boundary_listing(fmt):
    """Pairs of a filler record and a probe record.  The filler's sequence is sized so that one named byte of the probe lands
    at a chosen output offset: every residue modulo 16 for every name (short fillers), and the last byte of a 4096-byte output
    tile and the first byte of the next for every name (fillers that run up to the tile's end).  Returns the listing and
    {name: set of absolute output offsets}."""
    lab_of = {1 + k: len(LR.label(fmt, "d__" + "x" * n)) for k, n in enumerate(IDENT_LENGTHS)}
    lines, at, where = [], 0, {}
    idx = 0

    def put(acc_n, taxid, seq_n):
        nonlocal at
        lines.append(b"%s  %d  %s\n" % (b"A" * acc_n, taxid, _seq(seq_n, len(lines))))
        for name, off in _markers(fmt, acc_n, lab_of[taxid], seq_n).items():
            where.setdefault(name, set()).add(at + off)
        at += _record_len(fmt, acc_n, lab_of[taxid], seq_n)

    names = list(_markers(fmt, 1, 1, 1))
    targets = [(name, r, False) for name in names for r in range(16)] + [(name, r, True) for name in names for r in (4095, 0)]
    for name, r, tile in targets:
        acc_n, taxid, seq_n = 1 + idx % 20, 1 + idx % len(IDENT_LENGTHS), idx % 41
        idx += 1
        off = _markers(fmt, acc_n, lab_of[taxid], seq_n)[name]
        base = _record_len(fmt, 1, lab_of[1], 0)                   # the shortest filler
        mod = 4096 if tile else 16
        fill = (r - (at + base + off)) % mod                      # sequence bytes the filler needs
        put(1, 1, fill)
        assert (at + off) % mod == r
        put(acc_n, taxid, seq_n)
    return b"".join(lines), where


@pytest.mark.parametrize("fmt", FORMATS)
def test_output_boundaries(tmp_path, fmt):
    """`>`, `;tax=`, the label's first and last byte, `;` + newline and the record's final newline on every output offset modulo
    16 and on both sides of a 4096-byte output boundary; accessions of 1 to 20 bytes, sequences of 0 to 40, every label length.
    The placement is checked on the generator's own offsets, which the expected bytes confirm.  Once through a pipe."""
    listing, where = _boundary_listing(fmt)
    assert len(listing) < 400_000
    for name, offsets in where.items():
        assert {o % 16 for o in offsets} == set(range(16)), name
        assert {4095, 0} <= {o % 4096 for o in offsets}, name
    exp = _check(tmp_path, fmt, _boundary_doc(), listing, [(c, False) for c in CHUNKS] + [(4096, True)], "boundaries")
    assert exp["outcome"] == ("ok",) and exp["records"] == listing.count(b"\n")
    for o in where[">"]:
        assert exp["fna"][o:o + 1] == b">"
    for o in where["final_nl"]:
        assert exp["fna"][o:o + 1] == b"\n"
    for o in where["label_first"]:
        assert exp["fna"][o:o + 1] in (b"d", b"x", b"L")


@pytest.mark.parametrize("fmt", FORMATS)
def test_length_sweep_upper_case_and_no_wrap(tmp_path, fmt):
    """Accessions of 1 to 20 bytes against sequences of 0 to 40, then sequences of 4080 to 4097 bytes: lower-case and IUPAC
    letters come out upper-cased, on one line however long."""
    lines = [b"%s  %d  %s\n" % (b"NR_%d" % 10 ** (a - 4) if a > 3 else b"Q" * a, 1 + (a + s) % len(IDENT_LENGTHS), _seq(s, a))
             for s in range(41) for a in (1 + s % 20, 1 + (s * 7 + 3) % 20)]
    lines += [b"long%d  %d  %s\n" % (n, 1 + n % len(IDENT_LENGTHS), _seq(n, n)) for n in range(4080, 4098)]
    assert {len(l.split(b"  ")[0]) for l in lines[:82]} == set(range(1, 21))
    exp = _check(tmp_path, fmt, _boundary_doc(), b"".join(lines), name="sweep")
    assert exp["records"] == len(lines)
    body = exp["fna"].split(b"\n")[1::2]
    assert len(body) == len(lines)                                    # header, sequence, header, sequence, ...: no wrap
    assert [len(b) for b in body[82:]] == list(range(4080, 4098))
    assert all(b == b.upper() for b in body) and set(body[-1]) == set(ALPHABET.upper())


# ---- the join ----------------------------------------------------------------------------------------------------------
def _mix(k: int) -> int:
    """TaxidMap::mixk (csrc/ingest.h)"""
    x = (k * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
    return x ^ (x >> 32)


def _displacements(taxids, cap):
    """Linear probing as TaxidMap does it: how far from its home slot each key ends up."""
    used, out = set(), []
    for t in taxids:
        home = i = _mix(t) & (cap - 1)
        while i in used:
            i = (i + 1) & (cap - 1)
        used.add(i)
        out.append((i - home) & (cap - 1))
    return out


@pytest.mark.parametrize("fmt", FORMATS)
def test_join_by_value(tmp_path, fmt):
    """Present and absent taxids; `+5`, `007` and a hundred leading zeros join rows 5 and 7; 2^64 - 1 and 2^63 are usize values
    no row has, 2^63 - 1 is the largest a row can have; 2^64 is not a usize: an error at its line, with the records before it kept."""
    doc = _document([(5, "d__five;p__v"), (7, "d__seven;p__vii"), (9223372036854775807, "d__max"), (0, "d__zero")])
    taxids = [b"5", b"6", b"+5", b"007", b"0" * 100 + b"7", b"18446744073709551615", b"9223372036854775808", b"7", b"+0", b"000",
              b"50", b"57", b"75", b"4", b"9223372036854775807"]
    listing = b"".join(b"acc%d  %s  %s\n" % (i, t, _seq(30 + i, i)) for i, t in enumerate(taxids))
    exp = _check(tmp_path, fmt, doc, listing * 40, name="join")
    assert (exp["records"], exp["n_unknown_taxid"], exp["n_unlabelled"]) == (8 * 40, 7 * 40, 0)
    assert exp["fna"].count(b"seven") == 3 * 40 and exp["fna"].count(b"five") == 2 * 40 and exp["fna"].count(b"zero") == 2 * 40
    bad = listing * 40 + b"accX  18446744073709551616  ACGT\n" + listing
    exp = _check(tmp_path, fmt, doc, bad, name="join-2^64")
    assert exp["outcome"] == ("error", 15 * 40 + 1, "taxid") and exp["records"] == 8 * 40


@pytest.mark.parametrize("fmt", FORMATS)
def test_join_through_probe_chains(tmp_path, fmt):
    """2000 rows whose taxids are consecutive multiples of the table's capacity (4096 for 2000 keys) plus a constant, and 2000
    whose home slots (by the table's own hash, restated here) all lie in eight adjacent slots, so that probes run through
    chains of hundreds of entries.  Every row is looked up, and so are absent taxids with the same home slots."""
    cap = 4096
    multiples = [3 + cap * k for k in range(1, 2001)]
    k = np.arange(1, 1_500_000, dtype=np.uint64)
    x = k * np.uint64(0x9E3779B97F4A7C15)
    near = [int(v) for v in k[((x ^ (x >> np.uint64(32))) & np.uint64(cap - 1)) < 8]]
    assert len(near) >= 2200 and all(_mix(v) & (cap - 1) < 8 for v in near[:50])
    crowded, absent = near[:2000], near[2000:2200]
    assert max(_displacements(crowded, cap)) > 1000
    for name, taxids in (("multiples", multiples), ("crowded", crowded)):
        doc = _document([(t, f"d__t{t}" if i % 50 else "clade__none") for i, t in enumerate(taxids)])
        ask = taxids[::-1] + [t + 1 for t in multiples[:200]] + absent
        listing = b"".join(b"a%d  %d  %s\n" % (i, t, _seq(i % 23, i)) for i, t in enumerate(ask))
        exp = _check(tmp_path, fmt, doc, listing, name=name)
        present, bare = set(taxids), set(taxids[::50])
        assert exp["n_unknown_taxid"] == sum(t not in present for t in ask) >= 200
        assert exp["n_unlabelled"] == sum(t in bare for t in ask) >= 40
        assert exp["records"] == sum(t in present and t not in bare for t in ask) >= 1960


# ---- skipped lines -----------------------------------------------------------------------------------------------------
SKIP_DOC = _document([(1, "d__bacteria;p__firmicutes;g__bacillus"), (2, "clade__unranked"), (4, "d__b;g__")])


def _skip_line(i: int, taxid: int) -> bytes:
    return b"acc%04d  %d  %s\n" % (i, taxid, _seq(20 + i % 9, i))


@pytest.mark.parametrize("fmt", FORMATS)
def test_skipped_lines(tmp_path, fmt):
    """The first line, the last line, every other line and every line of more than one 4096-byte chunk skipped; unknown taxids
    (3) and rows without a label (2: no kind; 4: an empty identifier) mixed, both counted."""
    n = 600                                                            # ~ 24 kB: six chunks at 4096
    cases = {
        "first": [3] + [1] * (n - 1),
        "last_without_newline": [1] * (n - 1) + [2],
        "written_last_without_newline": [3] + [1] * (n - 1),
        "every_other": [1, 3] * (n // 2),
        "a_chunk_and_more": [1] * 150 + [3, 2, 4] * 100 + [1] * 150,   # 300 lines of ~ 40 bytes: 12 kB without a record
        "mixed": [(1, 3, 1, 2, 2, 4, 1, 1, 3)[i % 9] for i in range(n)],
    }
    for name, taxids in cases.items():
        listing = b"".join(_skip_line(i, t) for i, t in enumerate(taxids))
        if "without_newline" in name:
            listing = listing[:-1]
        exp = _check(tmp_path, fmt, SKIP_DOC, listing, name=name)
        assert exp["outcome"] == ("ok",)
        assert exp["records"] == taxids.count(1) and exp["n_unknown_taxid"] == taxids.count(3)
        assert exp["n_unlabelled"] == taxids.count(2) + taxids.count(4)


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_line_skipped_and_empty_inputs(tmp_path, fmt):
    """Every line of the listing skipped: an empty .fna and outcome ok, at every chunk size; so for an empty listing, and for a
    taxonomies file without rows."""
    listing = b"".join(_skip_line(i, (3, 2)[i % 2]) for i in range(400))
    exp = _check(tmp_path, fmt, SKIP_DOC, listing, name="all_skipped")
    assert exp == {**exp, "outcome": ("ok",), "fna": b"", "records": 0, "n_unknown_taxid": 200, "n_unlabelled": 200}
    assert _check(tmp_path, fmt, SKIP_DOC, b"", name="empty_listing")["fna"] == b""
    exp = _check(tmp_path, fmt, _document([]), b"".join(_skip_line(i, 1) for i in range(50)), name="no_rows")
    assert exp["fna"] == b"" and exp["n_unknown_taxid"] == 50


# ---- refusals and the stop ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(3))
@pytest.mark.parametrize("fmt", FORMATS)
def test_refusals_and_the_quiet_stop(tmp_path, fmt, part):
    """Too few pieces, a sequence byte >= 0x80 (in a line that would be written and in one that would be skipped: the refusals
    are decided before the join) and a taxid that is not a usize, each several chunks into the listing: the error names the
    line and the .fna holds the records before it.  A line that is not UTF-8 stops the export quietly.  Two problems on one line
    and on two lines keep kraken2's precedence."""
    head = [_skip_line(i, (1, 1, 3, 1, 2)[i % 5]) for i in range(500)]         # ~ 20 kB
    tail = [_skip_line(i, 1) for i in range(500, 520)]
    bad = {
        "pieces": (b"acc  1 ACGT\n", ("error", 501, "pieces")),
        "one_piece": (b"\n", ("error", 501, "pieces")),
        "nonascii_written": (b"acc  1  AC\xc3\xa9GT\n", ("error", 501, "nonascii")),
        "nonascii_skipped": (b"acc  3  AC\xc3\xa9GT\n", ("error", 501, "nonascii")),
        "nonascii_unlabelled": (b"acc  2  \xc3\xa9\n", ("error", 501, "nonascii")),
        "nonascii_accession_is_fine": (b"acc\xc3\xa9  1  ACGT\n", ("ok",)),
        "taxid_word": (b"acc  x1  ACGT\n", ("error", 501, "taxid")),
        "taxid_minus": (b"acc  -1  ACGT\n", ("error", 501, "taxid")),
        "taxid_empty": (b"acc    ACGT  ACGT\n", ("error", 501, "taxid")),
        "nonascii_and_taxid": (b"acc  x1  AC\xc3\xa9GT\n", ("error", 501, "nonascii")),
        "taxid_then_pieces": (b"acc  x1  ACGT\nacc  1 ACGT\n", ("error", 501, "taxid")),
        "invalid_utf8": (b"acc  1  AC\xffGT\n", ("stop", 501)),
        "invalid_utf8_in_a_skipped_line": (b"a\xc3  3  ACGT\n", ("stop", 501)),
        "invalid_utf8_then_error": (b"acc  1  AC\xffGT\nacc  1 ACGT\n", ("stop", 501)),
        "error_then_invalid_utf8": (b"acc  1 ACGT\nacc  1  AC\xffGT\n", ("error", 501, "pieces")),
    }
    for name, (line, outcome) in list(bad.items())[part::3]:
        exp = _check(tmp_path, fmt, SKIP_DOC, b"".join(head) + line + b"".join(tail), name=name)
        assert exp["outcome"] == outcome, name
        if outcome != ("ok",):
            assert exp["records"] == 300 and exp["n_unknown_taxid"] == 100 and exp["n_unlabelled"] == 100, name
            assert exp["input_bytes"] == len(b"".join(head)), name
