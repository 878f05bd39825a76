"""Plain-Python restatement of `blu build-db kraken2` and `blu build-db qiime2`, bytes in and bytes out: the oracle of
tests/test_seqdb.py and tests/test_gpu_seqdb.py.  Every rule cites its line in the reference
(K = core/src/use_cases/build_kraken_db_from_ncbi_files/, Q = core/src/use_cases/build_qiime_db_from_blutils_db/mod.rs)."""
from __future__ import annotations

import json
import re
from typing import List, Optional, Tuple

_USIZE = re.compile(rb"\+?[0-9]+")


class RefError(Exception):
    """The reference panics (or, for the divergences DESIGN.md lists, this engine refuses) at 1-based `line`.  `fna` is the
    output written before that line (what the .fna holds after an error), `records` their number and `prelim`
    the prelim_map.txt lines of those records (kraken2; the file itself is not left behind)."""

    def __init__(self, line: int, why: str, fna: bytes = b"", records: int = 0, prelim: bytes = b""):
        self.line, self.why, self.fna, self.records, self.prelim = line, why, fna, records, prelim
        super().__init__(f"line {line}: {why}")


class Result(tuple):
    """What a restated function returns: the tuple its docstring names, and `records`, the number of records written."""
    records = 0

    def __new__(cls, items, records: int):
        self = super().__new__(cls, items)
        self.records = records
        return self


def _lines(listing: bytes):
    """BufRead::read_line (K generate_fasta_file.rs:64, Q:122): each line with its newline; an Err (not UTF-8) ends the loop."""
    pos, no = 0, 0
    while pos < len(listing):
        nl = listing.find(b"\n", pos)
        end = len(listing) if nl < 0 else nl + 1
        line = listing[pos:end]
        no += 1
        try:
            line.decode("utf-8")
        except UnicodeDecodeError:
            return
        yield no, line
        pos = end


def _pieces(line: bytes, k: int, no: int) -> List[bytes]:
    """buf_line.split("  ") and k times .next().expect(er_msg).trim() (K rs:69-75, Q:127-134); str::trim on ASCII white space"""
    parts = line.split(b"  ")
    if len(parts) < k:
        raise RefError(no, "Invalid line detected on blastdbcmd response")
    return [p.strip() for p in parts[:k]]


def usize(text: bytes) -> Optional[int]:
    """<usize as FromStr>: one optional leading '+', decimal digits, below 2^64"""
    if not _USIZE.fullmatch(text):
        return None
    v = int(text)
    return v if v < 1 << 64 else None


def kraken2(listing: bytes) -> Tuple[bytes, bytes, Optional[int]]:
    """(library.fna, prelim_map.txt, the line of an invalid-UTF-8 stop or None), with .records"""
    fna, heads, stop = [], [], None
    last = 0
    for no, line in _lines(listing):
        last = no
        try:
            acc, taxid, seq = _pieces(line, 3, no)
            if not seq.isascii():               # divergence: to_uppercase/chunks(80) work on chars
                raise RefError(no, "the sequence holds a byte >= 0x80")
            up = seq.upper()                              # K rs:80-89: to_uppercase, chunks(80), join("\n")
            body = b"\n".join(up[i:i + 80] for i in range(0, len(up), 80))
            n = usize(taxid)                              # K rs:98: taxid.parse().unwrap()
            if n is None:                                 # (the reference has written this line's record by then; here the
                raise RefError(no, "the taxid is not an unsigned integer")    # .fna holds the records before the bad line)
        except RefError as e:
            raise RefError(e.line, e.why, b"".join(fna), len(fna), _prelim(heads)) from None
        fna.append(b">kraken:taxid|" + taxid + b"|" + acc + b"\n" + body + b"\n")   # K rs:78-79
        heads.append((acc, n))
    if listing and last < _count_lines(listing):
        stop = last + 1
    return Result((b"".join(fna), _prelim(heads), stop), len(fna))


def _prelim(heads) -> bytes:
    return b"".join(b"TAXID\tkraken:taxid|%d|%s\t%d\n" % (n, acc, n) for acc, n in heads)   # generate_taxonomies_file.rs:28-36


def qiime2_sequences(listing: bytes) -> Tuple[bytes, Optional[int]]:
    """(the .fna, the line of an invalid-UTF-8 stop or None), with .records; Q:127-145"""
    out, last = [], 0
    for no, line in _lines(listing):
        last = no
        try:
            acc, taxid, oid, seq = _pieces(line, 4, no)
        except RefError as e:
            raise RefError(e.line, e.why, b"".join(out), len(out)) from None
        out.append(b">" + taxid + b"-" + oid + b"-" + acc + b"\n" + seq + b"\n")
    stop = last + 1 if listing and last < _count_lines(listing) else None
    return Result((b"".join(out), stop), len(out))


def export(qiime: bool, listing: bytes) -> dict:
    """What one export of the listing leaves behind, for a test to compare whole: "outcome" is ("ok",), ("stop", line) or
    ("error", line, reason) with reason "pieces", "nonascii" or "taxid"; "fna" the .fna (after an error: the records before
    the bad line); "map" prelim_map.txt (None for qiime2 and after an error: the file does not exist); "records" their
    number, "input_bytes" the offset of the first line that gave none and "map_bytes" the prelim_map.txt bytes of those
    records (after an error too, when no file is left)."""
    try:
        r = qiime2_sequences(listing) if qiime else kraken2(listing)
        fna, prelim, stop, records = r[0], (None if qiime else r[1]), r[-1], r.records
        map_bytes = len(prelim or b"")
        outcome = ("ok",) if stop is None else ("stop", stop)
    except RefError as e:
        reason = "pieces" if "Invalid line" in e.why else "nonascii" if "0x80" in e.why else "taxid"
        fna, prelim, records, outcome, map_bytes = e.fna, None, e.records, ("error", e.line, reason), len(e.prelim)
    pos = 0
    for _ in range(records):
        nl = listing.find(b"\n", pos)
        pos = nl + 1 if nl >= 0 else len(listing)
    return {"outcome": outcome, "fna": fna, "map": prelim, "records": records, "input_bytes": pos, "map_bytes": map_bytes}


def _count_lines(listing: bytes) -> int:
    return listing.count(b"\n") + (0 if listing.endswith(b"\n") else 1)


class _Int:
    def __init__(self, text: str):
        self.text = text


def _no_dups(pairs):
    keys = [k for k, _ in pairs]
    return {"__pairs__": pairs, "__keys__": keys}


def _u64(v) -> bool:
    return isinstance(v, _Int) and not v.text.startswith("-") and int(v.text) < 1 << 64


def _struct(obj, known, required, what):
    """serde's derived Deserialize for a struct: unknown fields skipped, a known field twice is an error, required fields"""
    if not isinstance(obj, dict) or "__pairs__" not in obj:
        raise ValueError(f"invalid type: expected {what}")
    seen = {}
    for k, v in obj["__pairs__"]:
        if k in known:
            if k in seen:
                raise ValueError(f"duplicate field `{k}`")
            seen[k] = v
    for k in required:
        if k not in seen:
            raise ValueError(f"missing field `{k}`")
    return seen


def _string(v, what):
    if not isinstance(v, str):
        raise ValueError(f"invalid type for {what}")
    v.encode("utf-8")                                     # a lone surrogate from \\uD800 cannot be a Rust String
    return v


def qiime2_taxonomies(document: bytes, use_taxid: bool) -> bytes:
    """serde_json::from_str::<TaxonomiesMap> (Q:30-44, taxonomies_map.rs) then the TSV of Q:46-84.  ValueError: serde rejects it."""
    text = document.decode("utf-8")                       # read_to_string
    def bad_constant(c):
        raise ValueError(f"invalid number {c}")
    doc = json.loads(text, object_pairs_hook=_no_dups, parse_int=_Int, parse_constant=bad_constant)
    top = _struct(doc, {"blutilsVersion", "ignoreTaxids", "replaceRank", "dropNonLinnaeanTaxonomies", "sourceDatabase",
                        "taxonomies"}, ("blutilsVersion", "sourceDatabase", "taxonomies"), "struct TaxonomiesMap")
    _string(top["blutilsVersion"], "blutilsVersion")
    _string(top["sourceDatabase"], "sourceDatabase")
    ign = top.get("ignoreTaxids")
    if ign is not None and not (isinstance(ign, list) and all(_u64(x) for x in ign)):
        raise ValueError("invalid type for ignoreTaxids")
    rep = top.get("replaceRank")
    if rep is not None:
        if not (isinstance(rep, dict) and "__pairs__" in rep):
            raise ValueError("invalid type for replaceRank")
        for _, v in rep["__pairs__"]:
            _string(v, "replaceRank")
    drop = top.get("dropNonLinnaeanTaxonomies")
    if drop is not None and not isinstance(drop, bool):
        raise ValueError("invalid type for dropNonLinnaeanTaxonomies")
    if not isinstance(top["taxonomies"], list):
        raise ValueError("invalid type for taxonomies")
    out = [b"Feature ID\tTaxon\n"]                        # Q:49-54
    for unit in top["taxonomies"]:
        u = _struct(unit, {"taxid", "rank", "numericLineage", "textLineage", "accessions"},
                    ("taxid", "rank", "numericLineage", "textLineage", "accessions"), "struct TaxonomyMapUnit")
        if not _u64(u["taxid"]):
            raise ValueError("invalid type for taxid")
        for k in ("rank", "numericLineage", "textLineage"):
            _string(u[k], k)
        if not isinstance(u["accessions"], list):
            raise ValueError("invalid type for accessions")
        lineage = u["numericLineage"] if use_taxid else u["textLineage"]       # Q:69-73
        for a in u["accessions"]:
            a = _struct(a, {"accession", "oid"}, ("accession", "oid"), "struct Accession")
            line = f"{int(u['taxid'].text)}-{_string(a['oid'], 'oid')}-{_string(a['accession'], 'accession')}\t{lineage}\n"
            out.append(line.encode("utf-8"))              # Q:64-75
    return b"".join(out)
