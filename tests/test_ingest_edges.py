"""The byte-level edge cases of the BLAST table ingest (tests/ingest_edges.py) without a GPU: every case lies where it claims
(recomputed from its bytes), every spelling has the grammar verdict its prediction needs, and the CPU parser (device=-1) gives
the independent reading (tests/ingest_reference.py) or the stated error on every one of them.  tests/test_gpu_ingest_edges.py
runs the same cases through the GPU parser."""
import numpy as np
import pytest

from blutils_amd import _native as N
from blutils_amd import pipeline
from tests import ingest_edges as E
from tests import ingest_reference as ref


# ---- shared with the GPU module -------------------------------------------------------------------------------------------------
def assert_columns_equal(got, exp):
    for k in ("seg_off", "bitscore", "align_len", "tax_desc_row", "acc_rank"):
        assert np.array_equal(got[k], exp[k]), k
    assert np.array_equal(got["pident"].view(np.uint64), exp["pident"].view(np.uint64)), "pident"      # bit for bit
    assert got["query_names"] == exp["query_names"], "query_names"
    assert got["accessions"] == exp["accessions"], "accessions"


def write(tmp_path, blob):
    bt = tmp_path / "edges.tsv"
    bt.write_bytes(blob)
    return str(bt), E.write_db(tmp_path)


def check_table(bt, tj, exp, ck, device, path, builds=True, names=True):
    """One table through ingest_columns and ingest_only on `device`, then (builds) under the drop-nothing hit filter and the
    taxon filter that names an unhit taxon: the unfiltered columns every time, on the parser `path`."""
    got = pipeline.ingest_columns(bt, tj, device=device)
    assert pipeline.last_ingest_path() == path
    if names:
        assert_columns_equal(got, exp)
    st, got_ck = pipeline.ingest_only(bt, tj, False, device=device)
    assert pipeline.last_ingest_path() == path
    assert got_ck == ck
    assert st["n_hits"] == len(exp["bitscore"]) and st["n_queries"] == len(exp["query_names"])
    assert st["n_unmatched_rows"] == int((exp["tax_desc_row"] == ref.UNMATCHED).sum())
    if not builds:
        return
    for kw in ({"hit_filter": E.HIT_FILTER_ALL}, {"taxon_filter": E.TAXON_FILTER_UNHIT}):
        got = pipeline.ingest_columns(bt, tj, device=device, **kw)
        assert pipeline.last_ingest_path() == path, kw
        assert got["n_kept"] == got["n_lines"] == len(exp["bitscore"]), kw
        assert_columns_equal(got, exp)
        if "taxon_filter" in kw:
            assert got["taxon_filter"]["n_excluded"] == 0 and got["taxon_filter"]["excluded_by"] == [0]


def check_case(tmp_path, case, device, exp=None):
    """A Case on `device` (-1: the CPU parser, whatever the prediction; 0: the path the case predicts)."""
    bt, tj = write(tmp_path, case.blob)
    if case.predict == "refused":
        with pytest.raises(N.BluError, match=case.message) as e:
            pipeline.ingest_columns(bt, tj, device=device)
        return e.value.code
    t, ck = exp if exp is not None else E.expected(case.blob, E.db_json())
    check_table(bt, tj, t, ck, device, "cpu" if device < 0 else case.predict, builds=case.builds and case.predict == "gpu")
    return None


# ---- the generator: every case lies where it claims -----------------------------------------------------------------------------
def _lines(blob):
    ls = E.line_starts(blob)
    out = []
    for a, b in zip(ls, ls[1:]):
        ln = blob[a:b - 1]
        out.append((a, ln[:-1] if ln.endswith(b"\r") else ln))
    return out


@pytest.mark.parametrize("name", sorted(E.ACCEPTED))
def test_case_lies_where_it_claims(name):
    case = E.accepted_case(name)
    c, blob = case.claims, case.blob
    lines = _lines(blob)
    forms = E.block_forms(blob)
    assert case.predict == "gpu" and all(len(ln.split(b"\t")) >= 13 for _, ln in lines)
    # every dead column 11 is a plain e-value when the case runs under the e-value threshold
    if case.builds:
        assert all(E.plain_for_gpu(ln.split(b"\t")[11]) and float(ln.split(b"\t")[11]) <= E.MAX_E for _, ln in lines)
    if "model_len" in c:
        ls = E.line_starts(blob)
        model = [(a, blob[a:b]) for a, b in zip(ls, ls[1:]) if b - a == c["model_len"]]
        assert {a % 16 for a, _ in model} == set(range(16)) and len({a % 4 for a, _ in model}) == 4
        assert {(a + len(ln) - 1) % 4 for a, ln in model} == set(range(4))                    # the newline: every offset mod 4
        if "last_field_bytes" in c:
            assert all(len(ln.split(b"\t")[-1]) == 1 for _, ln in lines)
            assert {a % 4 for a, _ in lines} == set(range(4))        # (a start 3 bytes into a word behind `\t7\n` among them)
        if "model_query_bytes" in c:
            # in front of an empty and of a one-byte query, the previous line's newline at every offset mod 4
            for n in (0, 1):
                assert {(a - 1) % 4 for a, ln in model if len(ln.split(b"\t")[0]) == n} == set(range(4)), n
    if "line_len" in c:
        assert len(lines) == c["rows"] and len(blob) == c["rows"] * c["line_len"] and c["line_len"] >= 4
    if c.get("crlf"):
        assert blob.count(b"\r\n") == blob.count(b"\n") == len(lines)
    if c.get("open"):
        assert not blob.endswith(b"\n")
    if "last_byte" in c:
        assert blob[-1] == c["last_byte"]
    if "max_columns" in c:
        assert {len(ln.split(b"\t")) for _, ln in lines} == {13, c["max_columns"]}
    if "size" in c:
        assert len(blob) == c["size"]
    if "span" in c:
        k = c["block"]
        assert forms[k] == (c["span"], c["form"]) and c["form"] == ("general" if c["span"] > 32768 else "staged")
        assert all(f == c["others"] for j, (_, f) in enumerate(forms) if j != k) and len(forms) >= 3
        assert E.line_starts(blob)[k * 256] % 16 == c["start_mod16"]
        assert len(lines) - k * 256 == c["target_lines"] or (len(forms) > k + 1 and c["target_lines"] == 256)
    if "forms" in c:
        assert [f for _, f in forms] == c["forms"] and max(len(ln) + 1 for _, ln in lines) == c["longest_line"]
    if "rows" in c:
        assert len(lines) == c["rows"]
    if "form" in c and "span" not in c:
        assert {f for _, f in forms} == {c["form"]}
    if "queries" in c:
        qs = [ln.split(b"\t")[0] for _, ln in lines]
        assert len(set(qs)) == c["queries"]
        ids = {}
        seq = [ids.setdefault(q, len(ids)) for q in qs]
        if "grouped" in c:
            assert (seq == sorted(seq)) == c["grouped"]
        if c.get("highest_not_last"):
            assert seq[-1] != max(seq) and seq.count(max(seq)) >= 2
    if "accessions" in c:
        by_acc = {}
        for _, ln in lines:
            f = ln.split(b"\t")
            by_acc.setdefault(f[1], set()).add(f[0])
        assert len(by_acc) == c["accessions"] and all(len(v) >= 2 for v in by_acc.values())


def test_name_families_have_their_properties():
    fam, acc = E.FAMILY, E.ACC_FAMILY
    assert len(set(fam)) == len(fam) and len(set(acc)) == len(acc)
    assert not any(b"\t" in x or b"\n" in x or b'"' in x or b"\0" in x or x.endswith(b"\r") for x in acc)
    for n in (11, 12, 13, 16, 17):                       # two names of n bytes that differ only in the last one
        assert any(len(a) == len(b) == n and a[:-1] == b[:-1] and a != b for a in fam for b in fam)
    for n, m in ((11, 12), (12, 13), (15, 16), (16, 17)):   # one a prefix of another
        assert any(len(a) == n and len(b) == m and b.startswith(a) for a in fam for b in fam)
    for x in (b"", b"\x01", b"\x7f", b"\x80", b"\xff", b" "):
        assert x in fam
    assert any(b"\r" in x[1:-1] for x in fam) and {300, 5000} <= {len(x) for x in fam}

    def first_difference(a, b):
        return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    diffs = {first_difference(a, b) for a in acc for b in acc if a != b}
    assert {8, 16, 39} <= diffs                          # byte 9, 17 and 40
    # a longer string that sorts before a shorter one with the same 8, 16 and 39 first bytes
    for n in (8, 16, 39):
        assert any(len(a) > len(b) and a < b and first_difference(a, b) == n for a in acc for b in acc)
    assert any(len(a) == 16 and b == a + b"\x01" for a in acc for b in acc)
    assert any(a[:1] >= b"\x80" for a in acc) and sorted(acc)[-1][:1] == b"\xff"


# ---- the spellings: each has the grammar verdict its prediction needs -------------------------------------------------------------
def _verdict(column, spelling):
    s = spelling.encode()
    return E.plain_for_gpu(s) if column == "e_value" else E.accepted_by_gpu(s, E.INTEGER[column])


@pytest.mark.parametrize("column", sorted(E.BOUNDARY))
def test_boundary_spellings_match_their_predictions(column):
    seen = set()
    for t in E.BOUNDARY[column]:
        assert t[0] not in seen, t
        seen.add(t[0])
        if not (t[1] == "refused" and t[2] == E.RANGE):     # (a range refusal is by the value, inside the grammar or not)
            assert _verdict(column, t[0]) == (t[1] == "gpu"), t
        assert t[1] in ("gpu", "cpu") or (t[1] == "refused" and t[2] in (E.NUMERIC, E.RANGE)), t
    # both sides of every limit are there
    verdicts = {t[0]: t[1] for t in E.BOUNDARY[column]}
    if not E.INTEGER[column]:
        assert verdicts["0." + "0" * 14 + "1"] == "gpu" and verdicts["0." + "0" * 15 + "1"] == "cpu"
        assert verdicts["+1"] == "cpu" and verdicts["1e5e5"] == "refused"
    if column == "perc_identity":
        assert [verdicts[s] for s in ("1e22", "1e23", "1e-22", "1e-23", "1e007", "1e0007")] == ["gpu", "cpu"] * 3
        assert verdicts["123456789012345"] == "gpu" and verdicts["1234567890123456"] == "cpu"


def test_the_grammar_restatement_on_its_limits():
    ok = lambda s, integer=False: E.accepted_by_gpu(s.encode(), integer)
    assert ok("1" * 15) and not ok("1" * 16)
    assert ok("0" * 40 + "1" * 15) and not ok("0" * 40 + "1" * 16)                   # leading zeros do not count
    assert ok("0." + "0" * 14 + "1") and not ok("0." + "0" * 15 + "1")              # zeros behind the point do
    assert ok("0." + "0" * 15) and not ok("0." + "0" * 16)
    assert ok("1e22") and not ok("1e23") and ok("1e-22") and not ok("1e-23")
    assert ok("0.5e23") and not ok("0.5e24") and ok("5000e19") and ok("50e22") and not ok("5e23") and not ok("0.05e-21") and ok("0.05e-20")
    assert ok("1e007") and not ok("1e0007") and not ok("1e") and not ok("e1") and not ok(".") and not ok("-") and not ok("")
    assert ok("1.") and ok(".1") and ok("-.1") and not ok("+1") and not ok("1 ") and not ok("--1") and not ok("1e+-1")
    assert ok("12", True) and ok("-12", True) and not ok("12.", True) and not ok("1e1", True)
    for s in ("nan", "inf", "infinity", "1_0", " 1", "0x10"):
        assert not ok(s)


def test_double_rounding_literals_differ_under_two_roundings():
    assert len(E.DOUBLE_ROUNDING) >= 6 and len(E.DOUBLE_ROUNDING_BIT_SCORE) >= 4
    for s in E.DOUBLE_ROUNDING:
        neg, mant, e, counted, _, _ = E.decompose(s.encode())
        assert counted in (16, 17) and e != 0 and mant > 2 ** 53 and not E.accepted_by_gpu(s.encode(), False)
        assert E.two_roundings(s.encode()) != float(s), s


# ---- the CPU parser on every case ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(E.ACCEPTED))
def test_cpu_parser_on_accepted_cases(tmp_path, name):
    check_case(tmp_path, E.accepted_case(name), -1, E.expected_of(name))


@pytest.mark.parametrize("name", E.DECLINED)
def test_cpu_parser_on_declined_and_refused_cases(tmp_path, name):
    case = E.declined_cases()[name]
    assert case.predict in ("cpu", "refused")
    check_case(tmp_path, case, -1)


def test_blank_lines_are_no_rows(tmp_path):
    """The reading with blank lines equals the reading of the file without them."""
    d = E.declined_cases()
    plain = E.expected(b"".join(ln + b"\n" for ln in d["blank_line_in_the_middle"].blob.split(b"\n") if ln), E.db_json())
    for name in ("blank_line_in_the_middle", "blank_line_at_the_end", "crlf_only_line_in_the_middle", "crlf_only_line_at_the_end"):
        assert E.expected(d[name].blob, E.db_json())[1] == plain[1], name


@pytest.mark.parametrize("column", [c for c in sorted(E.BOUNDARY) if c != "e_value"])
def test_cpu_parser_on_boundary_spellings(tmp_path, column):
    blob = E.spelling_blob(column, E.accepted_spellings(column))
    t, ck = E.expected(blob, E.db_json())
    if column == "subject_taxid":                  # the 15-digit taxid, taxid 0 spelled -0 and a negative one: joined, joined, unmatched
        assert (t["tax_desc_row"] != ref.UNMATCHED).sum() >= 6 and (t["tax_desc_row"] == ref.UNMATCHED).sum() >= 2
    bt, tj = write(tmp_path, blob)
    check_table(bt, tj, t, ck, -1, "cpu", builds=False)
    for spelling, predict, message in E.other_spellings(column):
        case = E.Case(E.spelling_blob(column, [spelling]), predict, message=message, builds=False)
        check_case(tmp_path, case, -1)


def check_e_value_spellings(tmp_path, spellings, device, path):
    blob = E.spelling_blob("e_value", spellings)
    kept = E.kept_by_e_value(blob)
    t, _ = E.expected(kept, E.db_json())
    bt, tj = write(tmp_path, blob)
    got = pipeline.ingest_columns(bt, tj, device=device, hit_filter={"max_e_value": E.MAX_E})
    assert pipeline.last_ingest_path() == path
    assert (got["n_lines"], got["n_kept"]) == (len(spellings) + 1, kept.count(b"\n"))
    assert_columns_equal(got, t)


def test_cpu_parser_on_e_value_spellings(tmp_path):
    acc = E.accepted_spellings("e_value")
    check_e_value_spellings(tmp_path, acc, -1, "cpu")
    assert 0 < E.kept_by_e_value(E.spelling_blob("e_value", acc)).count(b"\n") < len(acc)       # some dropped, some kept
    for spelling, predict, message in E.other_spellings("e_value"):
        if predict == "cpu":
            check_e_value_spellings(tmp_path, [spelling], -1, "cpu")
        else:
            bt, tj = write(tmp_path, E.spelling_blob("e_value", [spelling]))
            with pytest.raises(N.BluError, match=message):
                pipeline.ingest_columns(bt, tj, device=-1, hit_filter={"max_e_value": E.MAX_E})


@pytest.mark.parametrize("column", ["perc_identity", "bit_score"])
def test_cpu_parser_on_double_rounding_mantissas(tmp_path, column):
    spellings = E.DOUBLE_ROUNDING if column == "perc_identity" else E.DOUBLE_ROUNDING_BIT_SCORE
    check_case(tmp_path, E.Case(E.spelling_blob(column, spellings), "cpu"), -1)


@pytest.fixture(scope="module")
def random_cases():
    cache = {}

    def get(column, form):
        if (column, form) not in cache:
            case = E.random_case(column, form)
            cache[column, form] = (case, E.expected(case.blob, E.db_json()))
        return cache[column, form]
    return get


@pytest.mark.parametrize("form", ["staged", "general"])
@pytest.mark.parametrize("column", ["perc_identity", "bit_score"])
def test_random_spellings_are_inside_the_grammar_and_read_by_the_cpu_parser(tmp_path, random_cases, column, form):
    case, exp = random_cases(column, form)
    sp = case.claims["spellings"]
    outside = [s for s in sp if not E.accepted_by_gpu(s.encode(), False)]
    assert len(sp) == E.N_RANDOM and not outside, outside[:5]
    forms = [f for _, f in E.block_forms(case.blob)]
    assert set(forms[:-1]) == {form} and len(forms) > 70           # (the short last block fits the stage either way)
    # the generator reaches what it is weighted toward
    d = [E.decompose(s.encode()) for s in sp]
    assert sum(x[3] >= 14 for x in d) > 5000 and sum(x[2] <= -20 for x in d) > 3000
    assert any(x[1] == 10 ** 15 - 1 for x in d) and any(x[1] == 5 * 10 ** 14 for x in d)
    assert {len(s.lower().split("e")[1].lstrip("+-")) for s in sp if "e" in s.lower()} == {1, 2, 3}
    if column == "perc_identity":
        assert sum(x[2] >= 20 for x in d) > 3000
    else:
        assert all(abs(float(s)) < 2 ** 31 for s in sp)
    check_case(tmp_path, case, -1, exp)


def test_cpu_parser_on_a_name_holding_a_nul(tmp_path):
    case = E.nul_name_case()
    t, ck = E.expected(case.blob, E.db_json())
    assert any(b"\0" in q for q in t["query_names"]) and any(b"\0" in a for a in t["accessions"])
    check_nul_case(tmp_path, case, t, ck, -1, "cpu")


def check_nul_case(tmp_path, case, t, ck, device, path):
    bt, tj = write(tmp_path, case.blob)
    got = pipeline.ingest_columns(bt, tj, device=device)
    assert pipeline.last_ingest_path() == path
    for k in ("seg_off", "bitscore", "align_len", "tax_desc_row", "acc_rank"):
        assert np.array_equal(got[k], t[k]), k
    for k in ("query_names", "accessions"):             # the tables' bytes; the split lists cut the name at its NUL
        assert b"".join(s + b"\0" for s in got[k]) == b"".join(s + b"\0" for s in t[k]), k
        assert len(got[k]) > len(t[k])
    st, got_ck = pipeline.ingest_only(bt, tj, False, device=device)
    assert pipeline.last_ingest_path() == path and got_ck == ck
    assert st["n_queries"] == len(t["query_names"]) and st["n_hits"] == len(t["bitscore"])


def check_bs_as_written(tmp_path, device, path):
    case = E.bs_as_written_case()
    t, _ = E.expected(case.blob, E.db_json())
    assert min(float(ln.split(b"\t")[12]) for ln in case.blob.split(b"\n") if ln) == 0.5 and (t["bitscore"] == 0).any()
    bt, tj = write(tmp_path, case.blob)
    got = pipeline.ingest_columns(bt, tj, device=device, hit_filter={"min_bit_score": case.claims["min_bit_score"]})
    assert pipeline.last_ingest_path() == path and got["n_kept"] == got["n_lines"] == 300
    assert_columns_equal(got, t)


def test_cpu_parser_compares_the_bit_score_as_written(tmp_path):
    check_bs_as_written(tmp_path, -1, "cpu")
