"""`build-db kraken2` and `build-db qiime2` on the GPU (csrc/seqdb_gpu.hip) against the plain-Python restatement
(tests/seqdb_reference.py): the hand cases, seeded random listings at several chunk sizes, errors several chunks in, the
pipe from a stand-in blastdbcmd, the round trip from `build-db blu`, and a run of about 1 GB."""
import hashlib
import os
import sys

import pytest

from blutils_amd import cli, seqdb, synth_seqdb
from tests import seqdb_reference as R
from tests import taxdb_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS = os.path.join(ROOT, "tests", "golden", "taxdb_docs_example")
CHUNKS = [4096, 65536, 0]


def _kraken(tmp_path, listing: bytes, chunk=0, name="k"):
    src = tmp_path / (name + ".txt")
    src.write_bytes(listing)
    out = tmp_path / name
    out.mkdir(exist_ok=True)
    st = seqdb.export(seqdb.KRAKEN2, str(out / "library.fna"), str(out / "prelim_map.txt"), listing_path=str(src),
                      chunk_bytes=chunk)
    return (out / "library.fna").read_bytes(), (out / "prelim_map.txt").read_bytes(), st


def _qiime(tmp_path, listing: bytes, chunk=0, name="q"):
    src = tmp_path / (name + ".txt")
    src.write_bytes(listing)
    fna = tmp_path / (name + ".fna")
    st = seqdb.export(seqdb.QIIME2, str(fna), None, listing_path=str(src), chunk_bytes=chunk)
    return fna.read_bytes(), st


def _same(got: bytes, exp: bytes):
    if got != exp:
        k = next((i for i in range(min(len(got), len(exp))) if got[i] != exp[i]), min(len(got), len(exp)))
        raise AssertionError(f"{len(got)} vs {len(exp)} bytes, first difference at {k}: got {got[max(0, k - 60):k + 60]!r}, "
                             f"expected {exp[max(0, k - 60):k + 60]!r}")


def _seq(n):
    return (b"acgtRYKMswbdhvNn" * (n // 16 + 1))[:n]


HAND_K = (b"X1  007  acgtn\nX2  +5  RyKmSwBdHvN\r\nX3  12  gg  extra  more\n X4   3   tt \n"
          + b"".join(b"L%d  %d  %s\n" % (n, n + 1, _seq(n)) for n in (0, 1, 79, 80, 81, 160, 161))
          + b"A   1  g\nlast  9  acg")
HAND_Q = (b"A1  7  0  acGT\nA2  +5  1  \r\nA3  007  2  nn  x\n A4  \t8\t  3   ry\nA    1  g  c\n"
          + b"".join(b"L%d  %d  %d  %s\n" % (n, n, n, _seq(n)) for n in (0, 1, 79, 80, 81, 160, 161)) + b"E  1  2  tail")


@pytest.mark.parametrize("chunk", CHUNKS)
def test_hand_cases(tmp_path, chunk):
    fna, prelim, st = _kraken(tmp_path, HAND_K, chunk)
    efna, eprelim, stop = R.kraken2(HAND_K)
    _same(fna, efna)
    _same(prelim, eprelim)
    assert st["invalid_utf8_line"] == 0 and st["n_lines"] == HAND_K.count(b"\n") + 1
    got, st = _qiime(tmp_path, HAND_Q, chunk)
    _same(got, R.qiime2_sequences(HAND_Q)[0])


@pytest.mark.parametrize("chunk", CHUNKS)
def test_invalid_utf8_stop(tmp_path, chunk):
    pre = b"".join(b"A%d  %d  %s\n" % (i, i, _seq(i % 200)) for i in range(300))
    pre_q = b"".join(b"A%d  %d  0  %s\n" % (i, i, _seq(i % 200)) for i in range(300))
    for bad in (b"\xff", b"\xc3(", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xe2\x82"):
        listing = pre + b"B  2  c" + bad + b"c\n" + b"C  3  gg\nbroken\n"
        fna, prelim, st = _kraken(tmp_path, listing, chunk)
        efna, eprelim, stop = R.kraken2(listing)
        assert stop == 301 and st["invalid_utf8_line"] == 301
        _same(fna, efna)
        _same(prelim, eprelim)
        ql = pre_q + b"B  2  0  c" + bad + b"\n"
        got, st = _qiime(tmp_path, ql, chunk)
        _same(got, R.qiime2_sequences(ql)[0])
        assert st["invalid_utf8_line"] == 301
    ok = "A  1  0  café \U0001f9a0\n".encode()          # valid UTF-8 is copied by qiime2
    got, st = _qiime(tmp_path, ok, chunk)
    assert got == R.qiime2_sequences(ok)[0] and st["invalid_utf8_line"] == 0


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("chunk", CHUNKS)
def test_random_listings(tmp_path, seed, chunk):
    for qiime in (False, True):
        path = tmp_path / "l.txt"
        synth_seqdb.write_listing(str(path), qiime, 3000, seed, max_len=700, long_lines=[10_000, 150_000])
        listing = path.read_bytes()
        if qiime:
            got, st = _qiime(tmp_path, listing, chunk)
            _same(got, R.qiime2_sequences(listing)[0])
        else:
            fna, prelim, st = _kraken(tmp_path, listing, chunk)
            efna, eprelim, _ = R.kraken2(listing)
            _same(fna, efna)
            _same(prelim, eprelim)
        assert st["max_line_bytes"] >= 150_000
        if chunk == 4096:
            assert st["n_chunks"] > 10


def _error_case(tmp_path, listing, line, chunk, qiime=False):
    with pytest.raises(R.RefError) as e:
        (R.qiime2_sequences if qiime else R.kraken2)(listing)
    assert e.value.line == line
    with pytest.raises(seqdb.SeqdbError, match=f"line {line}:"):
        (_qiime if qiime else _kraken)(tmp_path, listing, chunk)


@pytest.mark.parametrize("chunk", [4096, 65536])
def test_errors_several_chunks_in(tmp_path, chunk):
    pre = b"".join(b"A%d  %d  %s\n" % (i, i, _seq(500)) for i in range(1000))   # about 520 kB: many chunks
    _error_case(tmp_path, pre + b"B  2\n" + b"C  1  a\n", 1001, chunk)
    _error_case(tmp_path, pre + b"B  -2  aa\n", 1001, chunk)
    _error_case(tmp_path, pre + "B  2  acé\n".encode(), 1001, chunk)
    _error_case(tmp_path, pre + b"\n", 1001, chunk)
    q = b"".join(b"A%d  %d  7  %s\n" % (i, i, _seq(500)) for i in range(1000))
    _error_case(tmp_path, q + b"B  2  seq\n", 1001, chunk, qiime=True)


def test_kraken2_taxid_error_leaves_no_prelim_map(tmp_path):
    listing = b"A  1  aa\n" * 5000 + b"B  x1  cc\n" + b"C  3  gg\n"
    out = tmp_path / "out"
    with pytest.raises(SystemExit, match="line 5001"):
        cli.main(["build-db", "kraken2", "db", "-o", str(out), "--listing-file", str(_write(tmp_path, listing))])
    assert not (out / "prelim_map.txt").exists()
    assert sorted(os.listdir(out)) == ["library.fna"]
    with pytest.raises(SystemExit, match="0x80"):
        cli.main(["build-db", "kraken2", "db", "-o", str(out), "--listing-file",
                  str(_write(tmp_path, "A  1  aç\n".encode()))])
    assert not (out / "prelim_map.txt").exists()


def _write(tmp_path, data: bytes, name="listing.txt"):
    p = tmp_path / name
    p.write_bytes(data)
    return p


def test_line_longer_than_the_chunk(tmp_path):
    listing = b"A  1  acg\nB  2  " + _seq(300_000) + b"\nC  3  t\n"
    fna, prelim, st = _kraken(tmp_path, listing, 4096)
    efna, eprelim, _ = R.kraken2(listing)
    _same(fna, efna)
    _same(prelim, eprelim)
    assert st["max_line_bytes"] == 300_006


STANDIN = """#!{py}
import sys, shutil
with open({listing!r}, "rb") as f:
    shutil.copyfileobj(f, sys.stdout.buffer, 1 << 16)
"""


def _db(tmp_path):
    d = tmp_path / "db"
    d.mkdir(exist_ok=True)
    (d / "nt.00.nsq").write_bytes(b"")
    (d / "taxdb.btd").write_bytes(b"")
    return str(d / "nt")


def test_pipe_from_blastdbcmd(tmp_path):
    lk, lq = tmp_path / "k.txt", tmp_path / "q.txt"
    synth_seqdb.write_listing(str(lk), False, 4000, 11, max_len=2000, long_lines=[200_000])
    synth_seqdb.write_listing(str(lq), True, 4000, 12, max_len=2000)
    for lst in (lk, lq):
        exe = tmp_path / ("blastdbcmd_" + lst.stem)
        exe.write_text(STANDIN.format(py=sys.executable, listing=str(lst)))
        exe.chmod(0o755)
    out = tmp_path / "kout"
    assert cli.main(["build-db", "kraken2", _db(tmp_path), "-o", str(out), "--blastdbcmd", str(tmp_path / "blastdbcmd_k")]) == 0
    efna, eprelim, _ = R.kraken2(lk.read_bytes())
    _same((out / "library.fna").read_bytes(), efna)
    _same((out / "prelim_map.txt").read_bytes(), eprelim)
    doc = tmp_path / "t.blutils.json"
    doc.write_bytes(b'{"blutilsVersion":"v","sourceDatabase":"d","taxonomies":[]}')
    assert cli.main(["build-db", "qiime2", str(doc), str(tmp_path / "tax"), _db(tmp_path), str(tmp_path / "seqs"),
                     "--blastdbcmd", str(tmp_path / "blastdbcmd_q")]) == 0
    _same((tmp_path / "seqs.fna").read_bytes(), R.qiime2_sequences(lq.read_bytes())[0])
    # an invalid-UTF-8 stop ends the run early: the child is killed and the command succeeds
    lst = _write(tmp_path, lq.read_bytes()[:50_000].rsplit(b"\n", 1)[0] + b"\n\xff\n" + lq.read_bytes(), "bad.txt")
    (tmp_path / "blastdbcmd_bad").write_text(STANDIN.format(py=sys.executable, listing=str(lst)))
    (tmp_path / "blastdbcmd_bad").chmod(0o755)
    st = seqdb.export_from_blastdbcmd(seqdb.QIIME2, "db", str(tmp_path / "b.fna"), None, str(tmp_path / "blastdbcmd_bad"))
    assert st["invalid_utf8_line"] > 0
    _same((tmp_path / "b.fna").read_bytes(), R.qiime2_sequences(lst.read_bytes())[0])


def _three_piece_case():
    for name in sorted(tc.CASES):
        kw = tc.CASES[name][0]
        acc = kw.get("accessions", "")
        lines = [l for l in acc.split("\n") if l]
        if len(lines) >= 2 and all(len(l.split("  ")) >= 3 for l in lines):
            return name
    raise AssertionError("no rule case with a three-piece accession listing")


@pytest.mark.parametrize("use_taxid", [False, True])
def test_round_trip_from_build_db_blu(tmp_path, use_taxid):
    name = _three_piece_case()
    kw, opts, _, _ = tc.CASES[name]
    c = tc.write_case(str(tmp_path / "dump"), **kw)
    assert cli.main(["build-db", "blu", "blast/16S", c["dir"], str(tmp_path / "ref"), "--accessions-file", c["accessions"]]) == 0
    doc = tmp_path / "ref.blutils.json"
    acc_lines = open(c["accessions"], "rb").read().splitlines()
    listing = b"".join(l.rstrip(b"\r\n") + b"  " + _seq(50 + 37 * i) + b"\n" for i, l in enumerate(acc_lines))
    lst = _write(tmp_path, listing, "seqs.txt")
    argv = ["build-db", "qiime2", str(doc), str(tmp_path / "tax"), "blast/16S", str(tmp_path / "seqs"), "--listing-file", str(lst)]
    assert cli.main(argv + (["-u"] if use_taxid else [])) == 0
    tsv = (tmp_path / "tax.tsv").read_bytes()
    _same(tsv, R.qiime2_taxonomies(doc.read_bytes(), use_taxid))
    assert tsv.count(b"\n") > 1
    _same((tmp_path / "seqs.fna").read_bytes(), R.qiime2_sequences(listing)[0])


def _digest(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def test_large_listing(tmp_path):
    """About 1 GB: three sequences of 100 MB and more among 400 k short lines; exact against the restatement, and repeated
    runs byte-identical."""
    lst = tmp_path / "big.txt"
    synth_seqdb.write_listing(str(lst), False, 400_000, 99, max_len=3000, long_lines=[100_000_000, 130_000_000, 110_000_000])
    listing = lst.read_bytes()
    assert len(listing) > 900_000_000
    out = tmp_path / "o1"
    out.mkdir()
    st = seqdb.export(seqdb.KRAKEN2, str(out / "library.fna"), str(out / "prelim_map.txt"), listing_path=str(lst),
                      chunk_bytes=256 << 20)
    efna, eprelim, _ = R.kraken2(listing)
    del listing
    _same((out / "prelim_map.txt").read_bytes(), eprelim)
    got = (out / "library.fna").read_bytes()
    assert got == efna, "library.fna differs from the restatement"
    del got, efna
    assert st["max_line_bytes"] >= 130_000_000 and st["n_chunks"] >= 4
    d1 = _digest(out / "library.fna")
    out2 = tmp_path / "o2"
    out2.mkdir()
    seqdb.export(seqdb.KRAKEN2, str(out2 / "library.fna"), str(out2 / "prelim_map.txt"), listing_path=str(lst))
    assert _digest(out2 / "library.fna") == d1
    assert _digest(out2 / "prelim_map.txt") == _digest(out / "prelim_map.txt")
