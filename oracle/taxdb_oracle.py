"""TEST-ONLY oracle of `blu build-db blu`: a string-faithful Python restatement of the reference's
core/src/use_cases/build_blutils_db_from_ncbi_files/ (build_taxonomy_database.rs, load_dump_file.rs,
build_accessions_map.rs) with the order the reference leaves to HashMap iteration pinned down (ascending taxid).

Nothing under blutils_amd/ imports this module; the product path is csrc/taxdb_gpu.hip.  DESIGN.md "Taxonomies
database builder" lists every rule below with the test that covers it.
"""
from __future__ import annotations

import json
import os
import re
from typing import Dict, List, Optional, Sequence, Tuple

_WS = b" \t\n\x0b\x0c\r"                 # str::trim on the ASCII range (non-ASCII white space: parity unpinned)
_INT = re.compile(rb"[+-]?[0-9]+\Z")
ID_LIMIT = 1 << 31                        # every id of the dump files must lie in [0, 2^31) (rs:193-197 parse::<i32>)
LETTERS = {"u": "u", "undefined": "u", "d": "d", "domain": "d", "k": "k", "kingdom": "k", "p": "p", "phylum": "p",
           "c": "c", "class": "c", "o": "o", "order": "o", "f": "f", "family": "f", "g": "g", "genus": "g",
           "s": "s", "species": "s"}        # linnaean_ranks.rs:59-69 and Display :75-90


class TaxdbError(Exception):
    pass


def slugify(b: bytes) -> bytes:
    """taxonomy.cpp slugify_ascii: [a-z0-9] runs joined by '-'; every other byte (>= 0x80 too) separates."""
    out = bytearray()
    pending = False
    for c in b:
        if 65 <= c <= 90:
            c += 32
        if 97 <= c <= 122 or 48 <= c <= 57:
            if pending and out:
                out.append(45)
            pending = False
            out.append(c)
        else:
            pending = True
    return bytes(out)


def rank_token(rank: bytes) -> Tuple[bytes, bool]:
    """LinnaeanRank::from_str (linnaean_ranks.rs:55-71) then Display; (token, is_other)."""
    low = rank.lower().strip(_WS)
    s = low.decode("utf-8", "replace")
    if s in LETTERS:
        return LETTERS[s].encode(), False
    return slugify(low), True           # Other(slugify!(x)), printed through slugify!(.., separator = "-") (rs:394,432)


def _lines(data: bytes) -> List[bytes]:
    """BufRead::lines: split on '\\n', the last piece only when not empty."""
    parts = data.split(b"\n")
    if parts and parts[-1] == b"":
        parts.pop()
    return parts


def _valid_utf8(b: bytes) -> bool:
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def _dump_id(v: bytes, path: str, lineno: int) -> int:
    if not _INT.match(v):
        raise TaxdbError(f"{path}:{lineno}: non-numeric id {v!r}")
    x = int(v)
    if not 0 <= x < ID_LIMIT:
        raise TaxdbError(f"{path}:{lineno}: id {x} outside 0..2147483647")
    return x


def read_dump(path: str, ncols: int):
    """load_dump_file.rs:37-57: invalid UTF-8 lines skipped, fields split on '|', trimmed, tabs removed; a missing
    field is an error.  Yields (1-based line, [field 0 .. ncols-1])."""
    with open(path, "rb") as f:
        data = f.read()
    for i, line in enumerate(_lines(data)):
        if not _valid_utf8(line):
            continue
        fields = line.split(b"|")
        if len(fields) < ncols:
            raise TaxdbError(f"{path}:{i + 1}: {len(fields)} fields, {ncols} needed")
        yield i + 1, [fields[k].strip(_WS).replace(b"\t", b"") for k in range(ncols)]


def read_accessions(path: str):
    """build_accessions_map.rs:39-74: read_line until the first line that is not UTF-8 (the loop ends there), pieces on
    two spaces, trimmed; taxid as i64 cast to u64.  Yields (1-based line, taxid u64, accession, oid)."""
    with open(path, "rb") as f:
        data = f.read()
    for i, line in enumerate(_lines(data)):
        if not _valid_utf8(line):
            return
        pieces = line.split(b"  ")
        if len(pieces) < 3:
            raise TaxdbError(f"{path}:{i + 1}: {len(pieces)} fields separated by two spaces, 3 needed")
        acc, tax, oid = (p.strip(_WS) for p in pieces[:3])
        if not _INT.match(tax) or not -(1 << 63) <= int(tax) < (1 << 63):
            raise TaxdbError(f"{path}:{i + 1}: invalid taxid {tax!r}")
        yield i + 1, int(tax) & ((1 << 64) - 1), acc, oid


def _jstr(b: bytes) -> str:
    return json.dumps(b.decode("utf-8"), ensure_ascii=False)      # serde_json's escapes (\u00xx lower-case hex)


def build(taxdump_dir: str, accessions_path: str, skip: Optional[Sequence[int]] = None,
          replace: Optional[Sequence[Tuple[str, str]]] = None, drop: bool = False, source_database: str = "",
          version: str = "8.3.1", dumps: Optional[Dict[str, str]] = None):
    """Returns (document bytes, TSV bytes, stats dict).  `replace` = the -r pairs in command-line order."""
    p = dumps or {k: os.path.join(taxdump_dir, k + ".dmp") for k in ("nodes", "names", "taxidlineage", "merged", "delnodes")}
    st = dict(nodes=0, names=0, lineage_tokens=0, accession_lines=0, distinct_taxids=0, mapped=0, mapped_merged=0,
              deleted=0, merged_missing=0, unknown=0, dropped=0, unmapped_ancestors=0, nonascii_names=0)
    nodes: Dict[int, bytes] = {}
    for ln, (t, _, rank) in ((ln, f) for ln, f in read_dump(p["nodes"], 3)):
        nodes[_dump_id(t, p["nodes"], ln)] = rank.replace(b'"', b"").lower()      # rs:199-206 (last line wins)
        st["nodes"] += 1
    lineage: Dict[int, bytes] = {}
    for ln, (t, lin) in read_dump(p["taxidlineage"], 2):
        lin = lin.replace(b'"', b"")                                            # rs:216-223
        lineage[_dump_id(t, p["taxidlineage"], ln)] = lin
        st["lineage_tokens"] += sum(1 for tok in lin.split(b" ") if tok and tok != b"null")
    names: Dict[int, bytes] = {}
    for ln, (t, name, _, cls) in read_dump(p["names"], 4):
        tid = _dump_id(t, p["names"], ln)
        if cls == b"scientific name":                                            # load_names_dataframe.rs:20-32
            names[tid] = name
            st["names"] += 1
            st["nonascii_names"] += any(c >= 0x80 for c in name)
    merged: Dict[int, int] = {}
    for ln, (a, b) in read_dump(p["merged"], 2):
        merged[_dump_id(a, p["merged"], ln)] = _dump_id(b, p["merged"], ln)
    deleted = set(_dump_id(t, p["delnodes"], ln) for ln, (t,) in read_dump(p["delnodes"], 1))

    # nodes ⋈ lineage (inner), then names (left): rs:120-160; a taxid without a lineage line does not exist
    def node(tid):
        if tid not in nodes or tid not in lineage:
            return None
        name = names.get(tid, b"null").replace(b'"', b"")                       # a left-join miss prints as null
        if name == b"" or name == b"null":
            name = b"taxid-%d" % tid                                              # rs:226-231
        return nodes[tid], name, lineage[tid]

    acc: Dict[int, List[Tuple[bytes, bytes]]] = {}
    for _, tid, a, o in read_accessions(accessions_path):
        acc.setdefault(tid, []).append((a, o))
        st["accession_lines"] += 1
    st["distinct_taxids"] = len(acc)
    rep = dict(replace or [])                                                    # HashMap: a repeated key keeps its last value
    rep_b = {k.encode(): v.encode() for k, v in rep.items()}
    skip_set = set(skip or [])

    entries, tsv = [], []
    for tid in sorted(acc):
        rec = node(tid)                                                          # rs:283-343
        via_merged = False
        if rec is None:
            if tid in deleted:
                tsv.append(b"%d\tdeleted\n" % tid); st["deleted"] += 1; continue
            if tid in merged:
                rec = node(merged[tid])
                if rec is None:
                    tsv.append(b"%d\tmerged\n" % tid); st["merged_missing"] += 1; continue
                via_merged = True
            else:
                tsv.append(b"%d\tunknown\n" % tid); st["unknown"] += 1; continue
        rank, name, lin = rec
        levels = []
        for tok in lin.split(b" "):                                              # rs:345-424
            if tok == b"" or tok == b"null":
                continue
            tok = tok.strip(_WS)
            if not re.match(rb"\+?[0-9]+\Z", tok):
                raise TaxdbError(f"{p['taxidlineage']}: non-numeric ancestor {tok!r} in the lineage of {tid}")
            a = int(tok)
            if a >= ID_LIMIT:
                raise TaxdbError(f"{p['taxidlineage']}: ancestor {a} outside 0..2147483647 in the lineage of {tid}")
            if a in skip_set:
                continue
            arec = node(a)
            if arec is None:
                st["unmapped_ancestors"] += 1
                continue
            token, other = rank_token(rep_b.get(arec[0], arec[0]))                # rs:377-398: replaced, then parsed
            if other and drop:
                continue
            levels.append((b"%s__%d" % (token, a), token + b"__" + slugify(arec[1])))
        leaf, other = rank_token(rank)                                           # rs:426-438: not replaced
        if other and drop:
            st["dropped"] += 1
            continue
        st["mapped_merged" if via_merged else "mapped"] += 1
        num = b";".join(x for x, _ in levels) + b";" + leaf + b"__%d" % tid   # rs:443-466
        txt = b";".join(y for _, y in levels) + b";" + leaf + b"__" + slugify(name)
        entries.append((tid, leaf, num, txt, acc[tid]))

    out = ["{\n", f'  "blutilsVersion": {json.dumps(version)},\n']
    if skip is None:
        out.append('  "ignoreTaxids": null,\n')
    else:
        out.append('  "ignoreTaxids": [' + ",".join(f"\n    {int(s)}" for s in skip) + ("\n  ],\n" if skip else "],\n"))
    if replace is None:
        out.append('  "replaceRank": null,\n')
    else:
        order = list(dict.fromkeys(k for k, _ in replace))
        out.append('  "replaceRank": {' + ",".join(f"\n    {json.dumps(k, ensure_ascii=False)}: "
                                                    f"{json.dumps(rep[k], ensure_ascii=False)}" for k in order)
                   + ("\n  },\n" if order else "},\n"))
    out.append(f'  "dropNonLinnaeanTaxonomies": {"true" if drop else "false"},\n')
    out.append(f'  "sourceDatabase": {json.dumps(source_database, ensure_ascii=False)},\n')
    if not entries:
        out.append('  "taxonomies": []\n}')
        return "".join(out).encode(), b"".join(tsv), st
    out.append('  "taxonomies": [\n')
    head = "".join(out).encode()
    body = []
    for k, (tid, leaf, num, txt, accs) in enumerate(entries):
        e = [b"    {\n", b'      "taxid": %d,\n' % tid, b'      "rank": "' + leaf + b'",\n',
             b'      "numericLineage": "' + num + b'",\n', b'      "textLineage": "' + txt + b'",\n',
             b'      "accessions": [\n']
        for j, (a, o) in enumerate(accs):
            e.append(b'        {\n          "accession": ' + _jstr(a).encode() + b',\n          "oid": '
                     + _jstr(o).encode() + b"\n        }" + (b",\n" if j + 1 < len(accs) else b"\n"))
        e.append(b"      ]\n    }" + (b",\n" if k + 1 < len(entries) else b"\n"))
        body.append(b"".join(e))
    return head + b"".join(body) + b"  ]\n}", b"".join(tsv), st


def output_paths(path: str) -> Tuple[str, str]:
    """rs:240-270: set_extension("json") first, then <parent>/<stem>.blutils.json and <parent>/<stem>.non-mapped.tsv."""
    parent, name = os.path.split(path)
    stem = name.rsplit(".", 1)[0] if ("." in name.lstrip(".")) else name
    return os.path.join(parent, stem + ".blutils.json"), os.path.join(parent, stem + ".non-mapped.tsv")
