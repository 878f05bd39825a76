"""Tables for the column-layout tests (`--blast-outfmt`): the golden table the equivalence tests relay, and the
byte-level cases of tests/ingest_edges.py built directly in a layout, their spans recomputed for the relaid bytes.  Test
infrastructure: deterministic, no GPU and no product code; expectations come from tests/outfmt_reference.py (to_reference) and
tests/ingest_reference.py (read_table)."""
import functools
import gzip
import json
import os

from tests import ingest_edges as E
from tests import outfmt_reference as R

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the golden table: tests/golden/zymo_mock_distilled.json.gz as one row per bean occurrence, one query per case, the numbers
# varied so that every filter, the best hit per subject, the band and the cover have something to cut
@functools.lru_cache(maxsize=None)
def golden_table():
    """(table in the reference's columns, taxonomies JSON text)"""
    with gzip.open(os.path.join(GOLDEN_DIR, "zymo_mock_distilled.json.gz"), "rt") as f:
        cases = json.load(f)["cases"]
    lineages, rows = {}, []
    for i, c in enumerate(cases):
        t, k = c["taxon"], 0
        for bean in t["consensusBeans"]:
            taxid = lineages.setdefault(bean["taxonomy"], 1000 + len(lineages))
            for j in range(int(bean["occurrences"])):
                acc = bean["accessions"][min(j, len(bean["accessions"]) - 1)]
                pid = "%.3f" % (t["percIdentity"] - 1.5 * (k % 5))
                rows.append("\t".join([f"smp{i % 3}.{i}", acc, str(taxid if (i + k) % 41 else 77), pid, str(400 + k if k % 7 else 150),
                                       "0", "0", "1", "400", "1", "400", ("1e-50", "1e-5", "0.002", "1e-4")[k % 4],
                                       str(int(t["bitScore"]) - 7 * (k % 3))]))
                k += 1
    db = {"blutilsVersion": "7.1.3", "sourceDatabase": "golden", "taxonomies": [
        {"taxid": v, "rank": "", "numericLineage": k, "textLineage": k, "accessions": []} for k, v in lineages.items()]}
    return ("\n".join(rows) + "\n").encode(), json.dumps(db)


# every selection at once: the four hit filters, a taxon filter, the best hit per subject, the band, the cover
SELECT_ALL = {"hit_filter": {"min_perc_identity": 90.0, "min_align_length": 200, "max_e_value": 1e-4, "min_bit_score": 100.0},
              "taxon_filter": {"exclude": ["f__listeriaceae"]}, "best_hit_per_subject": True, "score_band": {"top_percent": "2"},
              "min_cover": "80"}
# what of it the ingest-columns call takes without a device
SELECT_HOST = {k: SELECT_ALL[k] for k in ("hit_filter", "taxon_filter")}


# ---- lines built in a layout -------------------------------------------------------------------------------------------------------
def pad_column(spec: str) -> int:
    """the first column of the layout nobody reads: where a line's filler bytes go"""
    lay = R.parse_spec(spec)
    roles = {lay[r] for r in R.ROLES if lay[r] is not None}
    return next(k for k in range(lay["n_columns"]) if k not in roles)


def line(spec, q, acc, tax=105, pid="99.356", aln=400, bs=845, pad=0, e_value=E.E_VALUE, tail=b"") -> bytes:
    """One row in the layout, without its newline: the roles' bytes, `1` in every other column, `pad` more bytes in the first
    column nobody reads; tail: what follows the taxid in a `staxids` field."""
    lay = R.parse_spec(spec)
    f = [b"1"] * lay["n_columns"]
    for role, v in (("query", q), ("accession", acc), ("taxid", E._b(tax) + tail), ("perc_identity", pid), ("align_length", aln),
                    ("bit_score", bs), ("e_value", e_value)):
        if lay[role] is not None:
            f[lay[role]] = E._b(v)
    if pad:
        f[pad_column(spec)] += b"x" * pad
    return b"\t".join(f)


def sized(spec, length, q, acc, **kw) -> bytes:
    base = line(spec, q, acc, **kw)
    assert len(base) <= length, (len(base), length)
    out = line(spec, q, acc, pad=length - len(base), **kw)
    assert len(out) == length
    return out


def _block(spec, n_lines, n_bytes, tag, tail=b""):
    """n_lines rows of n_bytes in all (newlines included), lengths as even as they come"""
    each, extra = divmod(n_bytes, n_lines)
    return [sized(spec, each - 1 + (1 if i < extra else 0), b"%s_%05d" % (tag, i // 2), b"NR_%06d.1" % (100 + i % 90), tax=100 + i % 90,
                  tail=tail if i % 2 else b"") for i in range(n_lines)]


def stage_case(spec, span, r, open_tail=False, eol=b"\n", tail=b"") -> E.Case:
    """tests/ingest_edges.py's stage_case at "middle" (or "last" when the last line is open), in the layout: block 2 has exactly
    `span` bytes from its first line's start rounded down to 16 to the end mark and starts r bytes past a multiple of 16; the
    other blocks take the other form."""
    assert eol == b"\n" or not open_tail
    staged = span <= E.STAGE_BYTES
    other = 256 * (420 if staged else 120)                # the neighbours: 420-byte lines (general) or 120-byte lines (staged)
    rows = []
    for b in range(2):
        rows += _block(spec, 256, other, b"before%d" % b)
    at = sum(len(x) + len(eol) for x in rows)
    fix = (r - at) % 16
    rows[-1] = sized(spec, len(rows[-1]) + fix, b"before_fix", b"NR_000105.1")
    assert (at + fix) % 16 == r
    # (with CR LF every line carries one byte more: the block's rows are built one byte shorter)
    rows += _block(spec, 256, span - r - (256 if eol != b"\n" else 0), b"target", tail=tail)
    if not open_tail:
        for b in range(2):
            rows += _block(spec, 256, other, b"after%d" % b)
    blob = eol.join(rows) + (b"" if open_tail else eol)
    return E.Case(blob, claims={"block": 2, "span": span, "form": "staged" if staged else "general", "start_mod16": r,
                                "others": "general" if staged else "staged"})


def long_line_case(spec) -> E.Case:
    rows = [sized(spec, 110, b"query_%04d" % (i // 3), b"NR_%06d.1" % (100 + i % 50), tax=100 + i % 50) for i in range(700)]
    rows[300] = sized(spec, 39999, b"query_long", b"NR_000105.1")
    return E.Case(E._table(rows), claims={"forms": ["staged", "general", "staged"]})


def rows_case(spec, n, tail=b"") -> E.Case:
    """n rows, three per query"""
    rows = [line(spec, b"q%06d" % (i // 3), b"NR_%06d.1" % (100 + (i * 7) % 97), tax=100 + (i * 7) % 97, pid="%d.%03d" % (80 + i % 20, i % 1000),
                 aln=100 + i % 1900, bs=50 + (i * 13) % 5000, tail=tail if i % 2 else b"") for i in range(n)]
    return E.Case(E._table(rows), claims={"rows": n})


SHORTEST_MINIMAL = b"\tA\t1\t1\t1\t1\t1"               # the shortest line of the seven-column layout with a plain e-value


def plain_form(blob: bytes, spec: str) -> bool:
    """The host-side reading alone: no blank line, no quote in the two names, every numeric role inside the GPU parser's grammar
    (tests/ingest_edges.py: accepted_by_gpu, plain_for_gpu), as many fields as the layout names — the GPU parser has no reason
    to hand the file to the host parser."""
    lay = R.parse_spec(spec)
    for ln, _ in R._lines(blob):
        if not ln:
            return False
        f = ln.split(b"\t")
        if len(f) < lay["n_columns"] or b'"' in f[lay["query"]] or b'"' in f[lay["accession"]]:
            return False
        tax = f[lay["taxid"]].split(b";", 1)[0] if lay["taxid_is_list"] else f[lay["taxid"]]
        if not (E.accepted_by_gpu(tax, True) and E.accepted_by_gpu(f[lay["perc_identity"]], False)
                and E.accepted_by_gpu(f[lay["align_length"]], True) and E.accepted_by_gpu(f[lay["bit_score"]], False)):
            return False
        if lay["e_value"] is not None and not E.plain_for_gpu(f[lay["e_value"]]):
            return False
    return True


# ---- the registry of the accepted byte-level cases: name -> (format string, builder of the Case) -----------------------------------
def _registry():
    r = {}
    for name in ("reversed", "wide"):
        spec, tail = R.LAYOUTS[name][0], (b";1;2" if name == "wide" else b"")
        for span, off in zip(E.SPANS, (1, 7, 15, 8, 3)):
            r[f"{name}/span_{span}_r{off}"] = (spec, functools.partial(stage_case, spec, span, off, tail=tail))
        r[f"{name}/open_last_line_32768_r5"] = (spec, functools.partial(stage_case, spec, 32768, 5, open_tail=True, tail=tail))
        for span in (32768, 32769):
            r[f"{name}/crlf_{span}_r9"] = (spec, functools.partial(stage_case, spec, span, 9, eol=b"\r\n", tail=tail))
        r[f"{name}/one_line_of_40000_bytes"] = (spec, functools.partial(long_line_case, spec))
        for n in (1, 255, 256, 257, 513):
            r[f"{name}/rows_{n}"] = (spec, functools.partial(rows_case, spec, n, tail=tail))
    # the taxid as a `;` list at the end of the line (the middle: `wide`, above), at the stage bound and in the general form
    for span in (32768, 32769):
        r[f"taxid_last/span_{span}_r11"] = (R.TAXID_LAST, functools.partial(stage_case, R.TAXID_LAST, span, 11, tail=b";b;c"))
        r[f"taxid_last/crlf_{span}_r2"] = (R.TAXID_LAST, functools.partial(stage_case, R.TAXID_LAST, span, 2, eol=b"\r\n", tail=b";b;c"))
    r["minimal/shortest_line"] = (R.MINIMAL, lambda: E.Case(E._table([SHORTEST_MINIMAL] * 600), claims={"rows": 600, "line_len": len(SHORTEST_MINIMAL) + 1}))
    return r


ACCEPTED = _registry()


@functools.lru_cache(maxsize=4)
def accepted_case(name: str) -> E.Case:
    return ACCEPTED[name][1]()


@functools.lru_cache(maxsize=4)
def expected_of(name: str):
    """(columns, checksum): tests/ingest_reference.py on the case rewritten to the reference's columns, computed once"""
    return E.expected(R.to_reference(accepted_case(name).blob, ACCEPTED[name][0]), E._db_text())


# ---- the three parse modes: a table with both forms, e-values spelled like the threshold, taxa on and off the lists -----------------
MODE_MAX_E = 1e-30
MODES = {"plain": {}, "hit_filter": {"hit_filter": {"max_e_value": MODE_MAX_E, "min_perc_identity": 85.0}},
         "taxon_filter": {"taxon_filter": {"exclude": ["s__s105", "g__g15"], "only": ["d__b"]}},
         "taxon_and_hit_filter": {"taxon_filter": {"exclude": ["g__g16"]}, "hit_filter": {"max_e_value": MODE_MAX_E, "min_bit_score": 60.0}}}


def modes_table(spec, tail=b"") -> bytes:
    """600 rows: the first 300 short (a staged block), the others 300 bytes longer (general blocks); every fifth e-value is the
    threshold's own spelling, which the device leaves to the host, every seventh lies above it; a few taxids the database lacks."""
    rows = []
    for i in range(600):
        ev = b"1e-30" if i % 5 == 0 else b"1.0e-30" if i % 11 == 0 else b"3e-12" if i % 7 == 0 else b"1e-50"
        rows.append(line(spec, b"q%05d" % (i // 4), b"NR_%06d.1" % (100 + (i * 7) % 97), tax=100 + (i * 7) % 97 if i % 29 else 5555,
                         pid="%d.%03d" % (80 + i % 20, i % 1000), aln=100 + i % 1900, bs=50 + (i * 13) % 5000, e_value=ev,
                         pad=300 if i >= 300 else 0, tail=tail if i % 2 else b""))
    return E._table(rows)
