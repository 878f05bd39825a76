"""The table of tests/pass_chain_cases.py holds what it claims — counted here from the bytes of the table and of the
chain's copies, never from the generator's bookkeeping, and without a GPU.  The lengths of a query after each stage are line
counts of the copies; the class a pass sees is computed from them: S (<= 64 rows, a wave), M (65 .. 512, the long lists of the
passes, still the stream kernel of the engine) and L (> 512, the worklist kernel).  An empty class fails.

What cannot exist: the cover taking a segment from 600 to 64 rows, or from L to S at all — it keeps at
least need(n) > n / 2 rows of a top group.  600 -> 301 = need(600) stands in for it, and the L -> S class of the cover is
asserted empty."""
import collections
import re

import numpy as np
import pytest

from blutils_amd import pipeline
from tests import hit_filter_reference as hf
from tests import min_cover_reference as mc
from tests import outfmt_reference as R
from tests import pass_chain_cases as C
from tests import score_band_reference as band_ref


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    return str(tmp_path_factory.mktemp("pass_chain"))


@pytest.fixture(scope="module")
def main():
    return C.main_table()


@pytest.fixture(scope="module")
def full(directory, main):
    """the chain with every option on, grouped: {stage name: {query: lines}} and the stages"""
    stages = C.chain(directory, main, "grouped", "all", C.PASSES)
    per = {s.step: C.by_query(s.path) for s in stages}
    return stages, per


def _lengths(per, q):
    """n0, n1, n2, n3 of a query (0: erased)"""
    return tuple(len(per[s].get(q, ())) for s in ("table", "columns", "subject", "min_cover"))


def test_the_three_writings_are_one_table(directory, main):
    for order in ("grouped", "scrambled"):
        f = C.write(directory, main, order)
        base, ext, perm = (open(f[k], "rb").read() for k in ("base", "ext", "perm"))
        assert R.to_reference(ext, C.EXT_SPEC) == base and R.to_reference(perm, C.PERM_SPEC) == base
        at = R.columns_of(C.PERM_SPEC).index("qcovhsp")
        assert [l.split(b"\t")[13] for l in ext.splitlines()] == [l.split(b"\t")[at] for l in perm.splitlines()]
        assert not R.is_reference(R.parse_spec(C.PERM_SPEC))
    n = base.count(b"\n")
    assert 20000 < n < 35000, n
    names = list(C.by_query(f["base"]))
    assert len(names) > 1024 and {q[:3] for q in names} == {"s0.", "s1.", "s2."}
    assert set(names) < set(main.headers) and len(main.headers) == len(names) + 1
    labels = [h.split(";")[0] for h in main.headers]
    assert all(re.fullmatch(r"s[0-2]\.[0-9]+", l) for l in labels) and len(set(labels)) == len(labels)     # a sample and a count-table key each
    grouped, scrambled = C.by_query(C.write(directory, main, "grouped")["base"]), C.by_query(f["base"])
    assert {q: sorted(v) for q, v in grouped.items()} == {q: sorted(v) for q, v in scrambled.items()}     # the same lines,
    assert list(grouped) != list(scrambled) and grouped != scrambled          # in another numbering and another order inside a query
    lines = open(f["base"], "rb").read().splitlines()
    runs = sum(1 for a, b in zip(lines, lines[1:]) if a.split(b"\t")[0] != b.split(b"\t")[0])
    assert runs > 3 * len(names)                                              # not contiguous


def test_the_stage_counts_chain(directory, main):
    for order, parser in [("grouped", p) for p in C.PARSERS] + [("scrambled", "all")]:
        stages = C.chain(directory, main, order, parser, C.PASSES)
        assert [s.step for s in stages] == ["table"] + list(C.PARSERS[parser]) + ["columns"] + list(C.PASSES)
        for prev, s in zip(stages, stages[1:]):
            assert s.n_in == prev.n_out == C.n_lines(prev.path), (order, parser, s.step)
            assert s.n_out == C.n_lines(s.path)
            if s.step != "band" and s.step != "columns":
                assert s.n_out < s.n_in, (order, parser, s.step)              # every stage takes something
        band = stages[-2]
        assert band.counts["n_raised"] > 500 and band.counts["n_widened"] > 50
        cover = stages[-1].counts
        assert cover["n_narrowed"] > 100 and cover["n_unresolved"] >= 6
    g, s = (C.chain(directory, main, o, "all", C.PASSES) for o in ("grouped", "scrambled"))
    assert [x.counts for x in g] == [x.counts for x in s]                     # the file order changes no count


def test_the_six_seam_queries(full):
    _, per = full
    for tag, want in C.SEAM_TABLE.items():
        q = next(q for q in per["table"] if q.endswith(";" + tag))
        assert _lengths(per, q) == want, tag
    q = next(q for q in per["table"] if q.endswith(";t127_need"))
    assert C.top_size(per["band"][q]) == 127 and mc.need_rows(127, C.MIN_COVER_MILLI) == 64 and mc.need_rows(600, C.MIN_COVER_MILLI) == 301


def test_every_step_has_its_pairs_and_no_class_is_empty(full):
    """keyed by (step, class before, class after) and by the exact (before, after) pairs; for the pairs the other steps leave the
    length alone.  The engine's classes are those of the last lengths."""
    _, per = full
    classes, pairs = collections.Counter(), {"parser": set(), "subject": set(), "min_cover": set()}
    for q in per["table"]:
        n0, n1, n2, n3 = _lengths(per, q)
        if n1 == 0:
            classes["parser", C.klass(n0), "erased"] += 1
            continue
        for step, before, after in (("parser", n0, n1), ("subject", n1, n2), ("band", n2, n2), ("min_cover", n2, n3)):
            classes[step, C.klass(before), C.klass(after)] += 1
        classes["engine", "stream" if n3 <= C.STREAM else "worklist", C.klass(n2)] += 1
        changed = [(step, b, a) for step, b, a in (("parser", n0, n1), ("subject", n1, n2), ("min_cover", n2, n3)) if b != a]
        if len(changed) == 1:
            pairs[changed[0][0]].add(changed[0][1:])
        if not changed:
            for step in pairs:
                pairs[step].add((n0, n0))
    print("[pass chain] classes", sorted(classes.items()))
    want = [(a, b) for a in "SML" for b in "SML" if "SML".index(b) <= "SML".index(a)]
    for step in ("parser", "subject", "min_cover"):
        for a, b in want:
            if (step, a, b) == ("min_cover", "L", "S"):
                assert classes[step, a, b] == 0                               # (more than half of a top group stays)
            else:
                assert classes[step, a, b] > 0, (step, a, b)
    for a in "SML":
        assert classes["band", a, a] > 0
    assert classes["parser", "S", "erased"] > 70 and classes["parser", "M", "erased"] >= 1
    for key in (("engine", "stream", "S"), ("engine", "stream", "M"), ("engine", "stream", "L"), ("engine", "worklist", "L")):
        assert classes[key] > 0, key                                           # (stream, L): the cover handed the engine a segment of its stream kernel
    assert set(C.PAIRS) <= pairs["parser"], set(C.PAIRS) - pairs["parser"]
    assert set(C.PAIRS) | {(513, 64)} <= pairs["subject"], set(C.PAIRS) - pairs["subject"]
    assert set(C.COVER_PAIRS) <= pairs["min_cover"], set(C.COVER_PAIRS) - pairs["min_cover"]
    # (513, 64) of the subject step: one subject carries the 449 extra lines
    q = next(q for q in per["table"] if q.endswith(";subject_513_64"))
    subjects = collections.Counter(f[1] for f in per["columns"][q])
    assert sorted(subjects.values())[-2:] == [1, 450]


def test_the_band_cases(full):
    """T before -> after of (1, 64), (1, 65), (63, 65) and (1, n) on 65, 129 and 513 rows, the raised rows at rows 63 and 64 and
    in the last sweep of 64"""
    _, per = full
    seen = set()
    for q, before in per["subject"].items():
        after, last = per["band"][q], per["min_cover"][q]
        n = len(before)
        assert len(after) == n
        raised = [i for i in range(n) if before[i][12] != after[i][12]]
        if n in C.BAND_SEGMENTS and len(per["table"][q]) == n == len(last) and raised:
            seen.add((n, C.top_size(before), C.top_size(after)))
            if ";band_" in q:
                assert {63, 64} <= set(raised) and (len(raised) < 3 or max(raised) >= 64 * ((n - 1) // 64)), q
    want = {(n, t0, n if t1 is None else t1) for n in C.BAND_SEGMENTS for t0, t1 in C.BAND_TOPS}
    assert want <= seen, want - seen


def test_the_cascades(full):
    _, per = full
    lengths = {q: _lengths(per, q) for q in per["table"]}
    shrinking = [q for q, (n0, n1, n2, n3) in lengths.items() if n0 > n1 > n2 > n3 > 0]
    assert len(shrinking) >= 4 and any(lengths[q] == (600, 513, 512, 401) for q in shrinking)
    assert any(n3 > C.STREAM for q, (n0, n1, n2, n3) in lengths.items() if q in shrinking)      # long for every pass and for the engine
    crossing = [q for q in shrinking if len({C.klass(n) for n in lengths[q]}) == 3]
    assert crossing                                                          # one query: L, M and S in one run


def test_the_queries_the_parser_erases(directory, main):
    names = list(C.by_query(C.write(directory, main, "grouped")["base"]))
    gone = {}
    for parser in ("hit", "taxon", "cover", "all"):
        left = C.by_query(C.chain(directory, main, "grouped", parser, ())[-1].path)
        gone[parser] = [q not in left for q in names]
        g = gone[parser]
        assert g[0] and g[-1] and any(g[i] and not g[i - 1] and not g[i + 1] for i in range(10, len(g) - 10)), parser
        run = best = 0
        for x in g:
            run = run + 1 if x else 0
            best = max(best, run)
        assert best >= 70, (parser, best)
        assert all(q in main.headers for q in names)
    for parser in ("hit", "taxon", "cover"):                                  # reached by each option alone: queries only it erases
        others = [p for p in ("hit", "taxon", "cover") if p != parser]
        assert any(a and not b and not c for a, b, c in zip(gone[parser], gone[others[0]], gone[others[1]])), parser
    assert all(a >= b for p in ("hit", "taxon", "cover") for a, b in zip(gone["all"], gone[p]))


def test_the_table_every_line_of_which_goes(directory):
    t = C.erased_table()
    for parser in ("hit", "taxon", "cover", "all"):
        stages = C.chain(directory, t, "grouped", parser, C.PASSES)
        assert stages[0].n_out > 100 and all(s.n_out == 0 for s in stages[len(C.PARSERS[parser]):])
        assert open(stages[-1].path, "rb").read() == b""


def test_rows_without_a_usable_lineage(directory, main, full):
    stages, per = full
    usable = lambda taxid: mc.FIRST_TAXID <= taxid < mc.FIRST_TAXID + mc.N_TAXIDS and taxid not in (mc.BAD_TAXID, mc.EMPTY_TAXID)

    def top(lines):
        scores = [band_ref.truncated(f[12]) for f in lines]
        return [int(f[2]) for f, b in zip(lines, scores) if b == max(scores)]

    found = collections.Counter()
    for q, lines in per["band"].items():
        before, after = top(per["subject"][q]), top(lines)
        bad = [t for t in after if not usable(t)]
        if bad and all(usable(t) for t in before) and len(before) > 1:
            assert len(per["min_cover"][q]) == len(lines)                     # left alone
            kind = "bad" if mc.BAD_TAXID in bad else "empty" if mc.EMPTY_TAXID in bad else "lacking"
            found[kind, C.klass(len(lines))] += 1
    assert all(found[kind, k] >= 1 for kind in ("lacking", "bad", "empty") for k in "SM"), found
    # without the band the cover narrows these very queries: the band is why they are left alone
    alone = C.by_query(C.chain(directory, main, "grouped", "all", ("subject", "min_cover"))[-1].path)
    assert all(len(alone[q]) < len(per["min_cover"][q]) for q in per["table"] if ";unusable_" in q)
    # an unmatched row as the best and as the worse line of its subject
    best = worse = 0
    for q, lines in per["columns"].items():
        pairs = collections.defaultdict(list)
        for f in lines:
            pairs[f[1]].append(f)
        for fs in pairs.values():
            if len(fs) == 2 and {usable(int(f[2])) for f in fs} == {True, False}:
                top_line = max(fs, key=lambda f: band_ref.truncated(f[12]))
                best += not usable(int(top_line[2]))
                worse += usable(int(top_line[2]))
    assert best >= 2 and worse >= 2
    n_unmatched = lambda lines: sum(int(f[2]) >= mc.LACKING_TAXID for fs in lines.values() for f in fs)
    assert n_unmatched(per["subject"]) < n_unmatched(per["columns"])           # the count has to follow the subject pass


def test_a_subjects_worse_line_inside_the_band_and_first_in_the_file(full):
    """the order of the subject pass and the band shows on it: tied by the band first, the worse line would be the one kept"""
    _, per = full
    found = collections.Counter()
    for q, lines in per["columns"].items():
        t = max(band_ref.truncated(f[12]) for f in lines)
        first = {}
        for f in lines:
            if f[1] in first:
                a, b = first[f[1]], f
                sa, sb = band_ref.truncated(a[12]), band_ref.truncated(b[12])
                if sb == t and band_ref.in_band(sa, t, D=C.TOP_BITS) and (a[2], a[3]) != (b[2], b[3]):
                    assert [g for g in per["subject"][q] if g[1] == f[1]] == [b]
                    found[C.klass(len(lines))] += 1
            first.setdefault(f[1], f)
    assert found["S"] >= 1 and found["M"] >= 1, found


def test_the_neighbours(directory, main):
    """in the head of the grouped table, under every parser setting: a long query stands second or third of its four, between two
    short ones; once two long ones are adjacent; the table ends in a long query"""
    for parser in C.PARSERS:
        per = C.by_query(C.chain(directory, main, "grouped", parser, ())[-1].path)
        names = list(per)
        n = [len(per[q]) for q in names]
        head = next(i for i, q in enumerate(names) if q.endswith(";f"))       # (the first filler)
        longs = [i for i in range(head) if n[i] > C.SHORT]
        assert len(longs) > 40
        adjacent = 0
        for i in longs:
            assert i % 4 in (1, 2), (parser, names[i], i)
            group = range(i - i % 4, i - i % 4 + 4)
            others = [j for j in group if j != i and n[j] > C.SHORT]
            adjacent += len(others)
            assert n[group[0]] <= C.SHORT and n[group[-1]] <= C.SHORT and len(others) <= 1, (parser, names[i])
        assert adjacent == 2
        assert n[-1] > C.SHORT, (parser, names[-1])


def test_the_identity_tables(directory):
    for value, text in C.IDENTITY_VALUES.items():
        for variant in C.IDENTITY_VARIANTS:
            stages = C.chain(directory, C.identity_table(value, variant), "grouped", "none", C.PASSES)
            has = {s.step: text.encode() in {f[3] for fs in C.by_query(s.path).values() for f in fs} for s in stages}
            want = {"subject": (True, False, False, False), "min_cover": (True, True, True, False), "kept": (True, True, True, True)}[variant]
            assert (has["columns"], has["subject"], has["band"], has["min_cover"]) == want, (value, variant)
            others = {f[3] for s in stages for fs in C.by_query(s.path).values() for f in fs} - {text.encode()}
            for p in others:                                                  # every other identity: exact thousandths below the limit
                k = round(float(p) * 1000)
                assert k / 1000.0 == float(p) and k < 131071, p
    assert float("131.071") * 1000 == 131071 and round(98.1234 * 1000) / 1000.0 != 98.1234


SETTINGS = ["hit", "taxon", "cover", "all"]


@pytest.mark.parametrize("order", ["grouped", "scrambled"])
@pytest.mark.parametrize("parser", SETTINGS)
def test_the_host_parser_under_the_parser_options_gives_the_columns_of_the_copy(directory, main, parser, order):
    """pipeline.ingest_columns(device=-1): each parser option alone, and all together under the permuted layout"""
    f = C.write(directory, main, order)
    kw = C.options(parser, ())
    stages = C.chain(directory, main, order, parser, ())
    got = pipeline.ingest_columns(f["perm"] if "blast_outfmt" in kw else f["base"], f["db"], device=-1, **kw)
    assert pipeline.last_ingest_path() == "cpu"
    exp = pipeline.ingest_columns(stages[-1].path, f["db"], device=-1)
    hf.assert_columns_equal(got, exp)
    assert (got["n_lines"], got["n_kept"]) == (stages[0].n_out, stages[-1].n_out) and len(exp["bitscore"]) == stages[-1].n_out
    whole = C.whole_table_counts(directory, main, order)
    if "taxon_filter" in kw:
        assert (got["taxon_filter"]["n_excluded"], got["taxon_filter"]["excluded_by"]) == (whole["n_excluded"], whole["excluded_by"])
    if "query_cover" in kw:
        assert got["query_cover"]["n_below"] == whole["n_below"] and got["query_cover"]["source"] == "qcovhsp"
    assert np.array_equal(np.diff(exp["seg_off"].astype(np.int64)), [len(v) for v in C.by_query(stages[-1].path).values()])
