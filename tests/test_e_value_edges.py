"""The e-value threshold cases (tests/e_value_edges.py) without a GPU: the restatement of the device's ladder decides as float()
does wherever it decides, the generator covers what it claims (every tier, the step and bracket boundaries, the net exponents
at which the device changes path), and the host parser (device=-1) gives `float(field) <= E` on every table.
tests/test_gpu_e_value_edges.py runs the same tables through the GPU parser."""
import collections
import math
import random

import pytest

from blutils_amd import pipeline
from tests import e_value_edges as V
from tests import hit_filter_reference as hf
from tests import ingest_edges as IE
from tests import ingest_reference as ref


# ---- shared with the GPU module -------------------------------------------------------------------------------------------------
def check_table(tmp_path, blob, texts, flt, device, passes=None, **kw):
    """One table under `flt` on `device`: the kept queries are those float() keeps, the columns are the independent reading of
    filter_text's copy, the counts are its counts, and the parser is the one §14.3 names: the GPU parser whenever a line is
    kept, the host parser with the empty table when none is."""
    src, dst = tmp_path / "e_values.tsv", tmp_path / "e_values_kept.tsv"
    src.write_bytes(blob)
    tj = IE.write_db(tmp_path)
    n_lines, n_kept = hf.filter_text(str(src), str(dst), flt)
    want = V.kept_queries(texts, flt["max_e_value"], passes)
    assert (n_lines, n_kept) == (len(texts), len(want))
    got = pipeline.ingest_columns(str(src), tj, device=device, hit_filter=flt, **kw)
    assert got["query_names"] == want
    assert pipeline.last_ingest_path() == ("gpu" if device >= 0 and want else "cpu")
    hf.assert_columns_equal(got, ref.read_table(str(dst), tj))
    assert (got["n_lines"], got["n_kept"]) == (n_lines, n_kept)
    return got


def texts_of(fields):
    return [f.text for f in fields]


def tables_of(name):
    """[(which, field texts)] of a threshold: the decided and the asked table, those that have a line."""
    decided, asked = V.split(name)
    return [(which, texts_of(fs)) for which, fs in (("decided", decided), ("asked", asked)) if fs]


# ---- the generator ---------------------------------------------------------------------------------------------------------------------
def test_the_thresholds_are_the_families_stated():
    assert [len(v) for v in V.FAMILIES.values()] == [19, 19, 19, 8, 7, 6] and len(V.THRESHOLDS) == 78
    for k in V.POWERS:
        p = float(f"1e{k}")
        lo, hi = V.THRESHOLDS[f"below_1e{k}"], V.THRESHOLDS[f"above_1e{k}"]
        assert lo < p < hi and math.nextafter(lo, math.inf) == p == math.nextafter(hi, 0.0)
        assert V.decade(p) == k == V.decade(hi) and V.decade(lo) == k - 1
    band = [E for E in V.THRESHOLDS.values() if V.finite_positive(E) and V.constants(E).band]
    assert min(band) == 1e-280 and max(band) == 1e280                    # both band edges, and a double beyond each
    assert not V.constants(V.THRESHOLDS["below_1e-280"]).band and not V.constants(V.THRESHOLDS["above_1e280"]).band
    assert set(V.ALSO_GENERAL) == set(V.FAMILIES) and all(V.FAMILY_OF[n] == f for f, n in V.ALSO_GENERAL.items())


def test_every_field_is_in_the_plain_grammar_and_is_the_case_it_claims():
    respelled = collections.Counter()
    n_own = 0
    for name in V.THRESHOLDS:
        fields = V.fields_for(name)
        own = [(f.neg, f.mant, f.e) for f in fields if f.origin != "common" or f.mant]
        assert len({f.text for f in fields}) == len(fields) and len(set(own)) == len(own)
        for f in fields:
            b = f.text.encode()
            neg, mant, e, counted, dot, has_exp = IE.decompose(b)
            assert IE.plain_for_gpu(b) and (neg, mant, e) == (f.neg, f.mant, f.e) and mant < 10 ** 15, (name, f)
            if has_exp:
                assert len(f.text.lower().split("e")[1].lstrip("+-")) <= 3, f
            if f.origin in ("neighbour", "magnitude"):
                n_own += 1
                if f.text != V.spell(f.mant, f.e):
                    respelled["any"] += 1
                    respelled["E"] += "E" in f.text
                    respelled["plus"] += "+" in f.text
                    respelled["leading_point"] += f.text.startswith(".")
                    respelled["leading_zeros"] += f.text.startswith("00")
                    respelled["zeros_behind_the_point"] += f.text.startswith(("0.0", ".0"))
                    if has_exp:
                        digits = f.text.lower().split("e")[1].lstrip("+-")
                        respelled[f"exp{len(digits)}"] += 1
                        respelled["padded"] += digits.startswith("0") and len(digits) > 1
        common = [f for f in fields if f.origin == "common"]
        assert [f.text for f in common] == list(V.COMMON)              # every threshold has them all
        assert 40 <= len(fields) <= 350
    assert 0.07 * n_own < respelled["any"] < 0.13 * n_own                 # a tenth
    for k in ("E", "plus", "leading_point", "leading_zeros", "zeros_behind_the_point", "exp1", "exp2", "exp3", "padded"):
        assert respelled[k] >= 50, (k, respelled)


def test_the_restatement_decides_as_float_does():
    """Wherever `tier` decides, it decides as float() does: over every generated case, and over 200 000 seeded random ones, a
    mantissa of 1 to 15 digits and a value within four decades of a threshold drawn from the list."""
    n = 0
    for name, E in V.THRESHOLDS.items():
        for f in V.fields_for(name):
            decision = V.tier(f.mant, f.e, f.neg, E)[1]
            assert decision is None or decision == V.expected_keep(f.text, E), (name, f)
            n += 1
    assert n > 19000
    rng = random.Random(2024)
    names = list(V.THRESHOLDS)
    seen = collections.Counter()
    for _ in range(200000):
        name = rng.choice(names)
        E = V.THRESHOLDS[name]
        d = rng.randrange(1, 16)
        mant = rng.randrange(10 ** (d - 1), 10 ** d)
        t = V.decade(E) if V.finite_positive(E) else rng.choice((-324, -323, -300, 0, 300, 308))
        e = t + rng.randrange(-4, 5) - (d - 1)
        which, decision = V.tier(mant, e, False, E)
        seen[which] += 1
        assert decision is None or decision == V.expected_keep(f"{mant}e{e}", E), (name, mant, e)
    # (a random value falls into the 2^-46 bracket about once in 3000 draws; the generated cases place fields there)
    assert all(seen[k] > 10000 for k in V.TIERS if k not in ("zero", "negative", "band_ask")) and seen["band_ask"] > 20, seen


def _counts(name):
    E = V.THRESHOLDS[name]
    c = collections.Counter()
    for f in V.fields_for(name):
        which, decision = V.tier(f.mant, f.e, f.neg, E)
        c[which] += 1
        c[which, decision] += 1
    return c


def test_coverage():
    """Every tier at least 100 times over the suite; the band tiers at least 10 times each in every powers-of-ten and
    band-edge table that can reach them; the net exponents on both sides of every 22-decade step.

    A table can reach the band tiers when its threshold lies in the band and the neighbours of every width from 2 to 15
    digits have a net exponent beyond +-22: t - (d - 1) < -22 for d >= 2, that is t <= -22, or t - 14 > 22, that is t >= 37.
    A value of 10^t with t in -21 .. 36 written in 15 digits has a net exponent within +-22, so between those bounds the
    device decides near fields in one operation and those tables must show that instead: one-operation keeps and drops."""
    total = collections.Counter()
    for name in V.THRESHOLDS:
        total.update({k: v for k, v in _counts(name).items() if isinstance(k, str)})
    assert set(total) == set(V.TIERS) and all(total[k] >= 100 for k in V.TIERS), total
    for fam in ("powers_of_ten", "below_powers_of_ten", "above_powers_of_ten", "band_edges"):
        for name, E in V.FAMILIES[fam]:
            c, t = _counts(name), V.decade(E)
            if not V.constants(E).band:
                assert c["ask_outside"] >= 100 and not any(c[k] for k in ("one_op", "band_keep", "band_drop", "band_ask")), name
            elif t <= -22 or t >= 37:
                assert all(c[k] >= 10 for k in ("band_keep", "band_drop", "band_ask")), (name, c)
            else:
                assert c["one_op", True] >= 10 and c["one_op", False] >= 10 and c["one_op"] >= 100, (name, c)
            assert c["mag_keep"] >= 10 and c["mag_drop"] >= 10, (name, c)       # on and beyond both magnitude tests
    # fields exactly on k_keep, one above it, one below k_drop and on it, in every finite positive threshold's table
    for name, E in V.THRESHOLDS.items():
        if V.finite_positive(E):
            k = V.constants(E)
            sums = {(len(str(f.mant)) + f.e) for f in V.fields_for(name) if f.origin == "magnitude"}
            tops = {(len(str(f.mant)) - 1 + f.e) for f in V.fields_for(name) if f.origin == "magnitude"}
            assert {k.k_keep - 1, k.k_keep, k.k_keep + 1} <= sums and {k.k_drop - 1, k.k_drop, k.k_drop + 1} <= tops, name
    # the steps of tiers 3 and 4: net exponents on both sides of 22 and 44
    reached = collections.defaultdict(set)
    for name, E in V.THRESHOLDS.items():
        for f in V.fields_for(name):
            which = V.tier(f.mant, f.e, f.neg, E)[0]
            if which in ("one_op", "band_keep", "band_drop", "band_ask"):
                reached[f.e].add(which)
    for e in (-45, -44, -23, -22, -21, 21, 22, 23, 44, 45):
        assert reached[e], e
        assert ("one_op" in reached[e]) == (abs(e) <= 22), e
    # inside and outside the bracket on both sides, at 15 digits
    for name in ("1e-30", "below_1e44", "3.7e-51", "4e279", "2.5e-280"):
        E = V.THRESHOLDS[name]
        near = [(f, V.tier(f.mant, f.e, f.neg, E)[0]) for f in V.fields_for(name) if f.origin == "neighbour" and len(str(f.mant)) == 15]
        for which in ("band_keep", "band_drop"):
            assert sum(w == which for _, w in near) >= 3, (name, which)
        asked = [f for f, w in near if w == "band_ask"]
        assert any(V.expected_keep(f.text, E) for f in asked) and any(not V.expected_keep(f.text, E) for f in asked), name
    # a decided table holds no undecided case, an asked table nothing else; every threshold has both
    for name, E in V.THRESHOLDS.items():
        decided, asked = V.split(name)
        assert decided and asked and len(decided) + len(asked) == len(V.fields_for(name))
        assert all(V.tier(f.mant, f.e, f.neg, E)[0] not in V.UNDECIDED for f in decided)
        assert all(V.tier(f.mant, f.e, f.neg, E)[0] in V.UNDECIDED for f in asked)
    # a table spans two 256-line parse blocks wherever the recipe gives that many fields
    assert sum(len(V.fields_for(n)) > 256 for n in V.THRESHOLDS) >= 50


def test_the_undecided_list_cases_are_what_they_claim():
    E = V.LIST_E
    undecided = lambda t: V.tier(*_mant_e(t), False, E)[1] is None
    for t in V.ASK_KEPT + (V.ASK_DROPPED,):
        assert V.tier(*_mant_e(t), False, E)[0] == "band_ask" and V.expected_keep(t, E) == (t != V.ASK_DROPPED)
    assert V.tier(*_mant_e(V.DECIDED_KEPT), False, E) == ("mag_keep", True) and V.expected_keep(V.DECIDED_KEPT, E)
    assert V.tier(*_mant_e(V.DECIDED_DROPPED), False, E) == ("mag_drop", False) and not V.expected_keep(V.DECIDED_DROPPED, E)
    for name, (n, where, which) in V.LIST_CASES.items():
        texts = V.list_case(name)
        at = [i for i, t in enumerate(texts) if undecided(t)]
        assert len(texts) == V.LIST_LINES and len(at) == n
        if where == "first":
            assert at == [0]
        if where == "last":
            assert at == [V.LIST_LINES - 1]
        kept = [V.expected_keep(texts[i], E) for i in at]
        if which == "dropped":
            assert not any(V.expected_keep(t, E) for t in texts) or n < V.LIST_LINES
            assert not any(kept)
        elif n > 1:
            assert any(kept) and not all(kept)
        if n == V.LIST_LINES:
            assert (which == "dropped") == (not any(V.expected_keep(t, E) for t in texts))
    texts, pid, passes = V.failing_pid_case()
    assert all(undecided(t) == (not p) for t, p in zip(texts, passes)) and 0 < sum(passes) < len(passes)
    assert all((float(x) >= V.PID_MIN) == p for x, p in zip(pid, passes))
    assert {t for t, p in zip(texts, passes) if not p} == set(V.ASK_KEPT + (V.ASK_DROPPED,))
    # the general form: no parse block of the padded lines (256, 256 and 88 of them) fits the parse kernel's stage
    assert {f for _, f in IE.block_forms(V.table(V.list_case(V.LIST_GENERAL), pad=V.LIST_PAD))} == {"general"}
    assert {f for _, f in IE.block_forms(V.table(V.list_case(V.LIST_GENERAL)))} == {"staged"}


def _mant_e(text):
    neg, mant, e, _, _, _ = IE.decompose(text.encode())
    assert not neg
    return mant, e


# ---- the host parser on every table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(V.FAMILIES))
def test_host_parser_on_every_table(tmp_path, family):
    for name, E in V.FAMILIES[family]:
        for which, texts in tables_of(name):
            check_table(tmp_path, V.table(texts), texts, {"max_e_value": E}, -1)
        if V.ALSO_GENERAL[family] == name:
            for which, texts in tables_of(name):
                blob = V.table(texts, pad=V.general_pad(len(texts)))
                assert IE.block_forms(blob)[0][1] == "general" and min(map(len, blob.split(b"\n")[:-1])) >= 128
                check_table(tmp_path, blob, texts, {"max_e_value": E}, -1)
                check_table(tmp_path, V.table(texts), texts, {"max_e_value": E}, -1, taxon_filter=IE.TAXON_FILTER_UNHIT)


@pytest.mark.parametrize("layout", list(V.LIST_LAYOUTS))
def test_host_parser_on_the_undecided_list_cases(tmp_path, layout):
    eol, open_tail = V.LIST_LAYOUTS[layout]
    for name in V.LIST_CASES:
        texts = V.list_case(name)
        check_table(tmp_path, V.table(texts, eol=eol, open_tail=open_tail), texts, {"max_e_value": V.LIST_E}, -1)
    texts, pid, passes = V.failing_pid_case()
    check_table(tmp_path, V.table(texts, eol=eol, open_tail=open_tail, pid=pid), texts,
                {"min_perc_identity": V.PID_MIN, "max_e_value": V.LIST_E}, -1, passes=passes)
