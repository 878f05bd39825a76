"""`build-db kraken2` and `build-db qiime2` without a GPU: the restatement against hand-written bytes, the command line,
the output names, the database checks, the blastdbcmd call, the host TSV writer's JSON rules, and the gfx950 build of
csrc/seqdb_gpu.hip."""
import json
import os
import re
import subprocess
import sys

import pytest

from tests import seqdb_reference as R
from blutils_amd import _native, cli, seqdb, taxdb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wrap(s: bytes) -> bytes:
    return b"\n".join(s[i:i + 80] for i in range(0, len(s), 80))


@pytest.mark.parametrize("n", [0, 1, 79, 80, 81, 160, 161])
def test_kraken2_wraps_at_80(n):
    seq = (b"acgtRYKM" * 30)[:n]
    fna, prelim, stop = R.kraken2(b"AB1.1  9606  " + seq + b"\n")
    up = seq.upper()
    body = b"\n".join(up[i:i + 80] for i in range(0, n, 80))
    assert fna == b">kraken:taxid|9606|AB1.1\n" + body + b"\n"
    assert prelim == b"TAXID\tkraken:taxid|9606|AB1.1\t9606\n"
    assert stop is None
    assert fna.count(b"\n") == 2 + max(0, (n - 1) // 80)


def test_kraken2_hand_cases():
    listing = (b"X1  007  acgtn\n"                   # leading zeros: the header keeps the text, prelim_map the number
               b"X2  +5  RyKmSwBdHvN\r\n"           # CRLF; a leading '+'; IUPAC letters upper-cased
               b"X3  12  gg  extra  more\n"         # later pieces are ignored: a separator ends the sequence
               b" X4   3   tt ")                   # pieces trimmed; the last line has no newline
    fna, prelim, stop = R.kraken2(listing)
    assert fna == (b">kraken:taxid|007|X1\nACGTN\n>kraken:taxid|+5|X2\nRYKMSWBDHVN\n>kraken:taxid|12|X3\nGG\n"
                   b">kraken:taxid|3|X4\nTT\n")
    assert prelim == (b"TAXID\tkraken:taxid|7|X1\t7\nTAXID\tkraken:taxid|5|X2\t5\nTAXID\tkraken:taxid|12|X3\t12\n"
                      b"TAXID\tkraken:taxid|3|X4\t3\n")
    assert stop is None


def test_qiime2_hand_cases():
    listing = b"A1  7  0  acGT\nA2  +5  1  \r\nA3  007  2  nn  x\n A4  \t8\t  3   ry"
    fna, stop = R.qiime2_sequences(listing)
    assert fna == b">7-0-A1\nacGT\n>+5-1-A2\n\n>007-2-A3\nnn\n>8-3-A4\nry\n"
    assert stop is None


def test_three_spaces_and_four_spaces_split_greedily():
    # "a   b": pieces "a", " b"; "a    b": "a", "", "b"
    fna, prelim, _ = R.kraken2(b"A   1  g\n")
    assert fna == b">kraken:taxid|1|A\nG\n"
    with pytest.raises(R.RefError) as e:
        R.kraken2(b"A    1  g\n")                  # the taxid piece is empty
    assert e.value.line == 1
    fna, _ = R.qiime2_sequences(b"A    1  g\n")
    assert fna == b">-1-A\ng\n"


def test_invalid_utf8_stops_quietly():
    listing = b"A  1  aa\nB  2  c\xffc\nC  3  gg\n"
    fna, prelim, stop = R.kraken2(listing)
    assert fna == b">kraken:taxid|1|A\nAA\n" and prelim == b"TAXID\tkraken:taxid|1|A\t1\n" and stop == 2
    fna, stop = R.qiime2_sequences(b"A  1  0  aa\n\xc3(  2  1  c\nC  3  2  gg\n")
    assert fna == b">1-0-A\naa\n" and stop == 2
    # a line after the stop is never read: its error does not count
    assert R.kraken2(b"A  1  aa\n\xed\xa0\x80  2  c\nbad\n")[2] == 2


@pytest.mark.parametrize("listing,line", [(b"A  1  aa\nB  2\n", 2), (b"A  1  aa\n\n", 2), (b"A\n", 1),
                                          (b"A  1  a\nB  2  b\nC  3", 3)])
def test_too_few_pieces_is_an_error(listing, line):
    with pytest.raises(R.RefError) as e:
        R.kraken2(listing)
    assert e.value.line == line


def test_qiime2_needs_four_pieces():
    with pytest.raises(R.RefError) as e:
        R.qiime2_sequences(b"A  1  0  aa\nB  2  cc\n")
    assert e.value.line == 2


@pytest.mark.parametrize("taxid", [b"-5", b"", b"+", b"1.0", b"18446744073709551616", b"0x10", b"1 2"])
def test_kraken2_taxid_that_is_not_usize(taxid):
    with pytest.raises(R.RefError) as e:
        R.kraken2(b"A  1  aa\nB  " + taxid + b"  cc\n")
    assert e.value.line == 2
    assert R.usize(b"18446744073709551615") == (1 << 64) - 1


def test_kraken2_non_ascii_sequence_is_an_error():
    with pytest.raises(R.RefError) as e:
        R.kraken2("A  1  aa\nB  2  acé\n".encode())
    assert e.value.line == 2
    fna, _ = R.qiime2_sequences("B  2  0  acé\n".encode())   # qiime2 copies it
    assert fna == ">2-0-B\nacé\n".encode()


# ---- command line and names

def test_cli_shapes():
    ap = cli.build_parser()
    with pytest.raises(SystemExit):
        ap.parse_args(["build-db", "kraken2", "db"])              # -o is required
    a = ap.parse_args(["build-db", "kraken2", "db", "-o", "out"])
    assert (a.blast_database_path, a.output_directory, a.listing_file, a.blastdbcmd, a.device) == ("db", "out", None, "blastdbcmd", 0)
    a = ap.parse_args(["build-db", "qiime2", "t.blutils.json", "tax", "db", "seqs", "-u"])
    assert (a.taxonomies_database_path, a.output_taxonomies_file, a.blast_database_path, a.output_sequences_file,
            a.use_taxid) == ("t.blutils.json", "tax", "db", "seqs", True)
    assert ap.parse_args(["build-db", "qiime2", "t", "o", "d", "s"]).use_taxid is False
    with pytest.raises(SystemExit):
        ap.parse_args(["build-db", "qiime2", "t", "o", "d"])
    for sub in ("kraken2", "qiime2"):
        h = [a for a in ap._subparsers._group_actions[0].choices["build-db"]._subparsers._group_actions[0].choices[sub]._actions]
        helps = {x.dest: x.help or "" for x in h}
        for k in ("listing_file", "blastdbcmd", "device"):
            assert "not in the reference CLI" in helps[k]


@pytest.mark.parametrize("given,tsv,fna", [("out", "out.tsv", "out.fna"), ("out.txt", "out.tsv", "out.fna"),
                                           ("d/x.y.z", "d/x.y.tsv", "d/x.y.fna"), (".hidden", ".hidden.tsv", ".hidden.fna")])
def test_set_extension(given, tsv, fna):
    assert seqdb.set_extension(given, "tsv") == tsv
    assert seqdb.set_extension(given, "fna") == fna


def _db(tmp_path, with_taxdb=True):
    d = tmp_path / "db"
    d.mkdir()
    (d / "nt.00.nsq").write_bytes(b"")
    if with_taxdb:
        (d / "taxdb.btd").write_bytes(b"")
    return str(d / "nt")


def test_database_checks(tmp_path):
    with pytest.raises(Exception):
        taxdb.validate_blast_database_with_taxdb(str(tmp_path / "missing" / "nt"))
    with pytest.raises(taxdb.TaxdbError):
        taxdb.validate_blast_database_with_taxdb(_db(tmp_path, with_taxdb=False))


def test_kraken2_resets_the_output_directory_before_the_check(tmp_path):
    out = tmp_path / "out"
    out.mkdir()
    (out / "old.txt").write_text("x")
    with pytest.raises(SystemExit):
        cli.main(["build-db", "kraken2", str(tmp_path / "nodb" / "nt"), "-o", str(out)])
    assert out.is_dir() and os.listdir(out) == []
    out.rmdir()
    out.write_text("a file")                                       # a file is removed too
    with pytest.raises(SystemExit):
        cli.main(["build-db", "kraken2", str(tmp_path / "nodb" / "nt"), "-o", str(out)])
    assert out.is_dir() and os.listdir(out) == []


def _doc(units, **top):
    d = {"blutilsVersion": "8.3.1", "ignoreTaxids": None, "replaceRank": None, "dropNonLinnaeanTaxonomies": False,
         "sourceDatabase": "db", "taxonomies": units}
    d.update(top)
    return json.dumps(d, indent=2).encode()


UNITS = [{"taxid": 9606, "rank": "s", "numericLineage": "d__2759;s__9606", "textLineage": "d__eukaryota;s__homo-sapiens",
          "accessions": [{"accession": "NM_1.1", "oid": "0"}, {"accession": "NM_2.1", "oid": "5"}]},
         {"taxid": 7, "rank": "g", "numericLineage": "g__7", "textLineage": "g__café \"q\"",
          "accessions": []},
         {"taxid": 10, "rank": "s", "numericLineage": "s__10", "textLineage": "s__x\ty",
          "accessions": [{"accession": "ABé", "oid": "9"}]}]


def _tsv(tmp_path, doc: bytes, use_taxid=False):
    src = tmp_path / "t.blutils.json"
    src.write_bytes(doc)
    out = tmp_path / "t.tsv"
    L = _native.lib()
    L.blu_qiime_taxonomy_tsv.restype = C_INT
    rc = L.blu_qiime_taxonomy_tsv(str(src).encode(), 1 if use_taxid else 0, str(out).encode())
    return rc, (out.read_bytes() if out.exists() else None)


import ctypes
C_INT = ctypes.c_int


@pytest.mark.parametrize("use_taxid", [False, True])
def test_tsv_writer_matches_the_restatement(tmp_path, use_taxid):
    doc = _doc(UNITS)
    rc, got = _tsv(tmp_path, doc, use_taxid)
    assert rc == 0, _native.last_error()
    exp = R.qiime2_taxonomies(doc, use_taxid)
    assert got == exp
    if use_taxid:
        assert exp == b"Feature ID\tTaxon\n9606-0-NM_1.1\td__2759;s__9606\n9606-5-NM_2.1\td__2759;s__9606\n10-9-AB\xc3\xa9\ts__10\n"
    else:
        assert b"10-9-AB\xc3\xa9\ts__x\ty\n" in exp


def test_tsv_writer_accepts_what_serde_accepts(tmp_path):
    extra = dict(UNITS[0], unknown={"a": [1, 2.5e3, None, True]})
    doc = _doc([extra], ignoreTaxids=[1, 2], replaceRank={"a": "b", "a": "c"}, somethingElse=[[]])
    doc = doc.replace(b'"d__2759;s__9606"', b'"d__2759;\\ud83e\\udda0s__9606\\/"')
    rc, got = _tsv(tmp_path, doc, True)
    assert rc == 0, _native.last_error()
    assert got == R.qiime2_taxonomies(doc, True)
    assert "\U0001f9a0".encode() in got
    minimal = b'{"blutilsVersion":"v","sourceDatabase":"d","taxonomies":[]}  \n'
    assert _tsv(tmp_path, minimal)[1] == b"Feature ID\tTaxon\n" == R.qiime2_taxonomies(minimal, False)


BAD = {
    "missing_top": b'{"blutilsVersion":"v","taxonomies":[]}',
    "missing_unit": b'{"blutilsVersion":"v","sourceDatabase":"d","taxonomies":[{"taxid":1,"rank":"s","numericLineage":"",'
                    b'"textLineage":""}]}',
    "missing_accession_oid": b'{"blutilsVersion":"v","sourceDatabase":"d","taxonomies":[{"taxid":1,"rank":"s",'
                             b'"numericLineage":"","textLineage":"","accessions":[{"accession":"a"}]}]}',
    "duplicate_top": b'{"blutilsVersion":"v","blutilsVersion":"v","sourceDatabase":"d","taxonomies":[]}',
    "duplicate_taxid": b'{"blutilsVersion":"v","sourceDatabase":"d","taxonomies":[{"taxid":1,"taxid":2,"rank":"s",'
                       b'"numericLineage":"","textLineage":"","accessions":[]}]}',
    "duplicate_optional": b'{"blutilsVersion":"v","ignoreTaxids":null,"ignoreTaxids":null,"sourceDatabase":"d","taxonomies":[]}',
    "taxid_negative": None, "taxid_float": None, "taxid_exp": None, "taxid_string": None, "taxid_minus_zero": None,
    "taxid_overflow": None, "taxid_leading_zero": None,
    "optional_wrong_type": b'{"blutilsVersion":"v","dropNonLinnaeanTaxonomies":"yes","sourceDatabase":"d","taxonomies":[]}',
    "ignore_wrong_type": b'{"blutilsVersion":"v","ignoreTaxids":[-1],"sourceDatabase":"d","taxonomies":[]}',
    "bad_escape": b'{"blutilsVersion":"\\x","sourceDatabase":"d","taxonomies":[]}',
    "lone_surrogate": b'{"blutilsVersion":"\\ud800","sourceDatabase":"d","taxonomies":[]}',
    "lone_trailing_surrogate": b'{"blutilsVersion":"\\udc00x","sourceDatabase":"d","taxonomies":[]}',
    "raw_control": b'{"blutilsVersion":"a\tb","sourceDatabase":"d","taxonomies":[]}',
    "trailing": b'{"blutilsVersion":"v","sourceDatabase":"d","taxonomies":[]} x',
    "invalid_utf8": b'{"blutilsVersion":"\xff","sourceDatabase":"d","taxonomies":[]}',
    "not_an_object": b'[]',
    "empty": b'',
}
for _k, _v in (("taxid_negative", b"-1"), ("taxid_float", b"1.0"), ("taxid_exp", b"1e3"), ("taxid_string", b'"1"'),
               ("taxid_minus_zero", b"-0"), ("taxid_overflow", b"18446744073709551616"), ("taxid_leading_zero", b"01")):
    BAD[_k] = (b'{"blutilsVersion":"v","sourceDatabase":"d","taxonomies":[{"taxid":' + _v +
               b',"rank":"s","numericLineage":"","textLineage":"","accessions":[]}]}')


@pytest.mark.parametrize("name", sorted(BAD))
def test_tsv_writer_rejects_what_serde_rejects(tmp_path, name):
    doc = BAD[name]
    with pytest.raises((ValueError, UnicodeDecodeError, UnicodeEncodeError)):
        R.qiime2_taxonomies(doc, False)
    rc, got = _tsv(tmp_path, doc)
    assert rc == _native.BLU_OK + 8 or rc != 0
    assert got is None                                           # no TSV is left behind
    assert not (tmp_path / "t.tsv.partial").exists()


def test_tsv_writer_refuses_a_binary_cache(tmp_path):
    src = tmp_path / "c.bin"
    src.write_bytes(b"BLUDBC01" + b"\0" * 100)
    rc = _native.lib().blu_qiime_taxonomy_tsv(str(src).encode(), 0, str(tmp_path / "t.tsv").encode())
    assert rc != 0
    assert "cache-db" in _native.last_error()


def test_qiime2_writes_the_tsv_before_the_failing_database_check(tmp_path):
    src = tmp_path / "t.blutils.json"
    src.write_bytes(_doc(UNITS))
    with pytest.raises(SystemExit):
        cli.main(["build-db", "qiime2", str(src), str(tmp_path / "tax.txt"), str(tmp_path / "nodb" / "nt"),
                  str(tmp_path / "seqs")])
    assert (tmp_path / "tax.tsv").read_bytes() == R.qiime2_taxonomies(_doc(UNITS), False)
    assert not (tmp_path / "seqs.fna").exists()


STANDIN = """#!{py}
import sys
open({rec!r}, "w").write("\\n".join(sys.argv[1:]))
sys.stdout.buffer.write(open({listing!r}, "rb").read())
sys.exit({rc})
"""


def _standin(tmp_path, listing: bytes, rc=0):
    rec = str(tmp_path / "argv.txt")
    lst = tmp_path / "listing.txt"
    lst.write_bytes(listing)
    exe = tmp_path / "blastdbcmd"
    exe.write_text(STANDIN.format(py=sys.executable, rec=rec, listing=str(lst), rc=rc))
    exe.chmod(0o755)
    return str(exe), rec


@pytest.mark.parametrize("fmt,outfmt", [(seqdb.KRAKEN2, "%a  %T  %s"), (seqdb.QIIME2, "%a  %T  %o  %s")])
def test_blastdbcmd_call(tmp_path, monkeypatch, fmt, outfmt):
    """The exact argv, and the child's stdout handed to the library as a descriptor (the library is stubbed here: it reads
    the pipe to its end, as blu_seqdb_export does)."""
    listing = b"A  1  0  acgt\n" * 1000
    exe, rec = _standin(tmp_path, listing)
    seen = {}

    def fake_export(f, fna, map_path=None, listing_path=None, input_fd=-1, chunk_bytes=0, device=0):
        data = b""
        while True:
            b = os.read(input_fd, 1 << 16)
            if not b:
                break
            data += b
        seen["data"] = data
        return {"invalid_utf8_line": 0}

    monkeypatch.setattr(seqdb, "export", fake_export)
    seqdb.export_from_blastdbcmd(fmt, "/some/db", str(tmp_path / "o.fna"), None, executable=exe)
    assert open(rec).read().split("\n") == ["-entry", "all", "-db", "/some/db", "-outfmt", outfmt]
    assert seen["data"] == listing
    exe, rec = _standin(tmp_path, b"", rc=3)
    with pytest.raises(seqdb.SeqdbError, match="blastdbcmd failed"):
        seqdb.export_from_blastdbcmd(fmt, "/some/db", str(tmp_path / "o.fna"), None, executable=exe)


def test_seqdb_kernels_build_for_gfx950():
    """csrc/seqdb_gpu.hip compiles for gfx950; every seqdb_* kernel runs at 4 waves per SIMD or more, without scratch."""
    csrc = os.path.join(ROOT, "blutils_amd", "csrc")
    p = subprocess.run(["make", "-s", "-C", csrc, "resource-usage-of", "SRC=seqdb_gpu.hip"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: \S*?(seqdb_[a-z0-9_]+?)E", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split()[0]] = int(m.group(2))
    assert {"seqdb_scan_bytes", "seqdb_sep_write", "seqdb_lines", "seqdb_write_fna", "seqdb_write_map"} <= set(usage)
    for k, u in usage.items():
        assert u["Occupancy"] >= 4 and u["ScratchSize"] == 0, (k, u)
