"""Independent statement of the hit filters (include/blu_pipeline.h: blu_hit_filter), written with nothing
but Python's `bytes.split`, `float()` and `int()` — both correctly rounded, so `float(field) <= E` IS the strtod decision
the parsers are held to.  Test infrastructure in the manner of tests/ingest_reference.py: shares no code with either
product parser.

The rule under test: a filtered run gives what the unfiltered run gives on `filter_text`'s copy of the table.
"""
import json

KEYS = ("min_perc_identity", "min_align_length", "max_e_value", "min_bit_score")


def keep(fields, flt) -> bool:
    """fields: the tab-separated fields of one line (bytes or str); flt: dict with some of KEYS (None / absent = not given)."""
    f = [x.decode() if isinstance(x, bytes) else x for x in fields]
    if flt.get("min_perc_identity") is not None and not float(f[3]) >= flt["min_perc_identity"]:
        return False
    if flt.get("min_align_length") is not None and not int(f[4]) >= flt["min_align_length"]:
        return False
    if flt.get("max_e_value") is not None and not float(f[11]) <= flt["max_e_value"]:
        return False
    if flt.get("min_bit_score") is not None and not float(f[12]) >= flt["min_bit_score"]:     # as written: no truncation
        return False
    return True


def filter_text(src, dst, flt):
    """Copies the kept lines of `src` to `dst` verbatim (line ends included); returns (lines, kept) over non-empty lines."""
    data = open(src, "rb").read()
    out, n_lines, n_kept = [], 0, 0
    pos = 0
    while pos < len(data):
        nl = data.find(b"\n", pos)
        end = len(data) if nl < 0 else nl + 1
        raw = data[pos:end]
        pos = end
        body = raw[:-1] if raw.endswith(b"\n") else raw
        if body.endswith(b"\r"):
            body = body[:-1]
        if not body:
            out.append(raw)
            continue
        n_lines += 1
        if keep(body.split(b"\t"), flt):
            n_kept += 1
            out.append(raw)
    open(dst, "wb").write(b"".join(out))
    return n_lines, n_kept


# ---- tables in which every threshold cuts ----------------------------------------------------------------------------------
E_FORMS = ["0.0", "1e-05", "1E-5", "0.00001", "9.99e-06", "1.01e-05", "3e-180", "5e-324", "1e-400", "2.5e-31", "1e-30", "7e-51",
           "1e-50", "4.2e-49", "0.001", "1e-100"]


def write_db(path, n=3000, duplicate=None):
    """taxids 100 .. 100 + n - 1; duplicate: a taxid listed a second time at the end (the left join doubles its hits)."""
    entry = lambda t: {"taxid": 100 + t, "rank": "species", "numericLineage": f"d__2;g__{t // 7};s__{100 + t}",
                       "textLineage": f"d__b;g__g{t // 7};s__s{t}", "accessions": []}
    tx = [entry(t) for t in range(n)]
    if duplicate is not None:
        tx.append(entry(duplicate - 100))
    open(path, "w").write(json.dumps({"blutilsVersion": "x", "sourceDatabase": "y", "taxonomies": tx}))
    return str(path)


def make_rows(n_q, hits, rng, long_names=False, sample_names=False):
    """BLAST-shaped lines whose columns 3, 4, 11 and 12 vary widely: perc_identity 80 .. 100, align_length 100 .. 1999,
    e-values from E_FORMS and 1e-3 .. 1e-179, bit-scores 50 .. 199999 as integers, x.5 and 1.148e+05."""
    rows = []
    for q in range(n_q):
        if long_names:      # lines of 128 bytes and more: the parse kernel's general form
            name = f"query_with_a_very_long_identifier_for_the_general_form_of_the_parse_kernel_{q:07d}/1_" + "x" * 60
        elif sample_names:
            name = f"s{q % 3}.{q}"
        else:
            name = f"q{q:06d}"
        for j in range(int(rng.integers(1, hits + 1))):
            t = int(rng.integers(0, 3100))                       # some taxids are not in the DB
            bs = int(rng.integers(50, 200000))
            bs_txt = f"{bs / 1000:.3f}e+03" if bs >= 99999 else (f"{bs}.5" if j % 5 == 0 else str(bs))
            acc = f"NR_{t:06d}.1" if t % 3 else f"a_much_longer_accession_string_{t:08d}.12"
            k = int(rng.integers(0, 3 * len(E_FORMS)))
            ev = E_FORMS[k] if k < len(E_FORMS) else f"{10.0 ** -int(rng.integers(3, 180)):.2e}"
            rows.append(f"{name}\t{acc}\t{100 + t}\t{80 + int(rng.integers(0, 20001)) / 1000:.3f}\t{int(rng.integers(100, 2000))}"
                        f"\t1\t0\t1\t400\t1\t400\t{ev}\t{bs_txt}")
    return rows


def scramble(rows, rng, ways=4):
    """rows of one query no longer contiguous; their relative (file) order survives"""
    order = sorted(range(len(rows)), key=lambda i: (int(rng.integers(0, ways)), i))
    return [rows[i] for i in order]


FILTERS = {
    "pid": {"min_perc_identity": 90.0},
    "aln": {"min_align_length": 1000},
    "evalue": {"max_e_value": 1e-50},
    "evalue_1e-5": {"max_e_value": 1e-5},
    "evalue_1e-30": {"max_e_value": 1e-30},
    "bits": {"min_bit_score": 60000.0},
    "all": {"min_perc_identity": 85.0, "min_align_length": 500, "max_e_value": 1e-30, "min_bit_score": 20000.25},
}


def assert_columns_equal(got, exp):
    import numpy as np
    for k in ("seg_off", "bitscore", "align_len", "tax_desc_row", "acc_rank"):
        assert np.array_equal(got[k], exp[k]), k
    assert np.array_equal(got["pident"].view(np.uint64), exp["pident"].view(np.uint64))      # bit for bit
    assert got["query_names"] == exp["query_names"] and got["accessions"] == exp["accessions"]
