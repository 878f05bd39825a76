"""Plain-Python restatement of `blu build-db kraken2` and `blu build-db qiime2`, bytes in and bytes out: the oracle of
tests/test_seqdb.py and tests/test_gpu_seqdb.py.  Every rule cites its line in the reference
(K = core/src/use_cases/build_kraken_db_from_ncbi_files/, Q = core/src/use_cases/build_qiime_db_from_blutils_db/mod.rs)."""
from __future__ import annotations

import json
import re
from typing import List, Optional, Tuple

_USIZE = re.compile(rb"\+?[0-9]+")


class RefError(Exception):
    """The reference panics (or, for the divergences DESIGN.md lists, this engine refuses) at 1-based `line`."""

    def __init__(self, line: int, why: str):
        self.line = line
        super().__init__(f"line {line}: {why}")


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
    """(library.fna, prelim_map.txt, the line of an invalid-UTF-8 stop or None)"""
    fna, heads, stop = [], [], None
    last = 0
    for no, line in _lines(listing):
        last = no
        acc, taxid, seq = _pieces(line, 3, no)
        if not seq.isascii():                   # divergence: to_uppercase/chunks(80) work on chars
            raise RefError(no, "the sequence holds a byte >= 0x80")
        up = seq.upper()                                  # K rs:80-89: to_uppercase, chunks(80), join("\n")
        body = b"\n".join(up[i:i + 80] for i in range(0, len(up), 80))
        fna.append(b">kraken:taxid|" + taxid + b"|" + acc + b"\n" + body + b"\n")   # K rs:78-79
        n = usize(taxid)                                  # K rs:98: taxid.parse().unwrap()
        if n is None:
            raise RefError(no, "the taxid is not an unsigned integer")
        heads.append((acc, n))
    if listing and last < _count_lines(listing):
        stop = last + 1
    prelim = b"".join(b"TAXID\tkraken:taxid|%d|%s\t%d\n" % (n, acc, n) for acc, n in heads)   # generate_taxonomies_file.rs:28-36
    return b"".join(fna), prelim, stop


def qiime2_sequences(listing: bytes) -> Tuple[bytes, Optional[int]]:
    """(the .fna, the line of an invalid-UTF-8 stop or None); Q:127-145"""
    out, last = [], 0
    for no, line in _lines(listing):
        last = no
        acc, taxid, oid, seq = _pieces(line, 4, no)
        out.append(b">" + taxid + b"-" + oid + b"-" + acc + b"\n" + seq + b"\n")
    stop = last + 1 if listing and last < _count_lines(listing) else None
    return b"".join(out), stop


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
