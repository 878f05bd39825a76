"""tests/document_edges.py kept honest, without a GPU: every claim a case makes about itself is recomputed from the bytes it
wrote and from the faithful oracle's output on the independent reading of those bytes.  The use-case itself has no route
without a device (the engine runs on the GPU under BLU_INGEST=cpu too), so this module checks the generator and the oracle
only; tests/test_gpu_document_edges.py holds the library to them."""
import json

import pytest

from oracle import oracle as orc
from tests import document_edges as E

PARAMS, IDS = E.case_params()


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    return str(tmp_path_factory.mktemp("document_edges"))


def read_table(path):
    """{name: [columns]} in file order, and the names in file order — from the bytes, not from the generator"""
    per_q = {}
    with open(path, "rb") as f:
        for line in f.read().split(b"\n")[:-1]:
            c = line.split(b"\t")
            assert len(c) == 13, line
            per_q.setdefault(c[0].decode(), []).append(c)
    return per_q


def lineages_of(tj):
    out = {}
    for t in json.load(open(tj, encoding="utf-8"))["taxonomies"]:
        out.setdefault(int(t["taxid"]), []).append(t["textLineage"].split(";"))
    return out


def test_taxonomies_document():
    base, dup = (json.loads(E.taxonomy_document(d))["taxonomies"] for d in (False, True))
    assert 200 <= len(base) <= 400 and len(dup) == len(base) + 3
    lins = [t["textLineage"] for t in base]
    assert len(set(lins)) == len(lins) and len({t["taxid"] for t in base}) == len(base)
    depth = [len(l.split(";")) for l in lins if "broken" not in l]
    assert set(depth) == {2, 3, 4, 5, 6, 7}
    have = set(lins)
    prefixes = [l for l in lins if any(o.startswith(l + ";") for o in have)]
    assert len(prefixes) >= 60 and {len(l.split(";")) for l in prefixes} == {2, 3, 4, 5, 6}
    # the last row of the lineage table is a short lineage that longer ones continue
    assert base[-1]["textLineage"] == dup[-1]["textLineage"] == "d__Bacteria;p__Ph5" and base[-1]["textLineage"] in prefixes
    twice = {t["taxid"] for t in dup if sum(u["taxid"] == t["taxid"] for u in dup) == 2}
    assert twice == {E.tid(*E.DUP_PLAIN), E.tid(*E.DUP_CROSS), E.tid(*E.DUP_SHORT)}
    assert sum("__" not in e for t in base for e in t["textLineage"].split(";")) == 1      # the one bad lineage


def test_sizes():
    for c in E.cases():
        assert 0 < c.n_lines() <= 60000, c.id
        assert [q.name for q in c.queries] == sorted((q.name for q in c.queries), key=str.encode), c.id


@pytest.mark.parametrize("case, strategy", PARAMS, ids=IDS)
def test_claims_hold_in_the_bytes_and_in_the_oracle(directory, case, strategy):
    bt, tj = E.write(case, directory)
    table = read_table(bt)
    exp = E.expected(case, strategy, directory)
    names = list(table)
    assert names == sorted(names, key=str.encode) == [q.name for q in case.queries]      # name order = file order = the engine's q
    lin = lineages_of(tj)
    for i, q in enumerate(case.queries):
        cols = table[q.name]
        scores = [int(float(c[12])) for c in cols]
        top = [k for k, s in enumerate(scores) if s == max(scores)]
        cl = q.claim
        assert (len(cols), top, len(top), i % 8, i % 32) == (cl["seg_len"], cl["top"], cl["n_top"], cl["slot8"], cl["slot32"]), (case.id, q.name)
        o = exp[q.name]
        if cl["kind"] == E.RENDERED:
            assert o["status"] == orc.ST_CONSENSUS and o["taxon"] is not None, (case.id, q.name, o)
            assert o["taxon"]["bitScore"] == max(scores)
            joined = sum(len(lin.get(int(cols[k][2]), [None])) for k in top)
            assert sum(b["occurrences"] for b in o["taxon"]["consensusBeans"]) == (1 if joined == 1 else joined), (case.id, q.name)
            assert joined == cl.get("joined_top", cl["n_top"])
            assert o["taxon"]["singleMatch"] is (joined == 1)
        else:
            assert o["status"] == E.NOT_RENDERED[cl["kind"]] and o["taxon"] is None, (case.id, q.name, o)


def by_family(family):
    return [c for c in E.cases() if c.family == family]


def test_sweeps_reach_every_length_and_placement():
    (case,) = by_family("sweeps")
    have = {q.claim["sweep"]: q.claim for q in case.queries}
    for n in E.SWEEP_LENGTHS:
        want = {"whole", "row0", "last"} if n > 2 else ({"whole"} if n == 1 else {"whole", "row0", "last"})
        if n >= 65:
            want.add("r63_64")
        if n > 64 and n % 64:
            want.add("last_partial")
        placed = {p for (m, p) in have if m == n}
        # (placements that select the same rows are one query: at 65 rows the last row alone IS the last partial sweep)
        rows = lambda p: {"whole": list(range(n)), "row0": [0], "last": [n - 1], "r63_64": [63, 64], "last_partial": list(range(n - n % 64, n))}[p]
        assert all(any(have[n, g]["top"] == rows(p) for g in placed) for p in want), n
        assert have[n, "whole"]["n_top"] == n
    for n_top in (64, 65):
        c = have[200, f"scattered{n_top}"]
        assert c["n_top"] == n_top and c["seg_len"] == 200 and {r // 64 for r in c["top"]} == {0, 1, 2, 3}
    claims = list(have.values())
    assert any(c["seg_len"] > 64 for c in claims)                                            # a second sweep
    assert any(min(c["top"]) > 63 for c in claims)                                           # a top row behind row 63 only
    assert any(c["top"] == [63, 64] for c in claims)                                         # one group across two sweeps
    assert any(c["n_top"] > 64 for c in claims) and any(c["n_top"] == 4097 for c in claims)  # a group larger than one sweep
    assert {512, 513} <= {c["seg_len"] for c in claims}                                      # the stream / worklist boundary
    assert set(case.strategies) == set(E.STRATEGIES)


def test_slots_reach_every_named_slot_with_every_kind(directory):
    tables = by_family("slots")
    assert {c.name for c in tables} == {f"{nq}-{k}" for nq in E.SLOT_COUNTS for k in E.NOT_RENDERED}
    assert {c.strategies[0] for c in tables} == set(E.STRATEGIES)
    for c in tables:
        nq, kind = c.name.split("-")
        nq = int(nq)
        assert len(c.queries) == nq and c.headers == tuple(E.HEADERS)
        assert all(h not in {q.name for q in c.queries} for h in c.headers)
        at = [i for i, q in enumerate(c.queries) if q.claim["kind"] != E.RENDERED]
        assert all(c.queries[i].claim["kind"] == kind for i in at)
        assert at == sorted(p for p in {0, 7, 8, nq - 1, *range(16, 24)} if p < nq), c.id
        assert 0 in at and nq - 1 in at                                                      # the first and the last query
        if nq > 23:
            assert {c.queries[i].claim["slot8"] for i in range(16, 24)} == set(range(8))     # one wave's eight, all of them
            assert {7, 8} <= set(at)
        if nq > E.BIG_AT:
            big = c.queries[E.BIG_AT].claim
            assert big["big"] and big["n_top"] == 130 and big["kind"] == E.RENDERED
        if nq > 32:
            rendered = [q.claim for q in c.queries if q.claim["kind"] == E.RENDERED]
            assert len({cl["n_top"] for cl in rendered}) >= 5 and len({cl["seg_len"] for cl in rendered}) >= 5      # no constant stride
    # n_queries + 1 on either side of the scan's 4096-element block
    assert {nq + 1 for nq in E.SLOT_COUNTS} >= {4096, 4097, 4098}


def test_scores_claims(directory):
    (case,) = by_family("scores")
    tops = {q.name: q.claim["score"] for q in case.queries}
    assert {2147483647, -2147483648, -5, 0, 700} == set(tops.values())
    table = read_table(E.write(case, directory)[0])
    assert [c[12] for c in table["sc_truncated"]][:2] == [b"700.9", b"700"]
    for strategy in case.strategies:
        exp = E.expected(case, strategy, directory)
        for q in case.queries:
            assert exp[q.name]["taxon"]["bitScore"] == tops[q.name]
        assert exp["sc_truncated"]["taxon"]["consensusBeans"][0]["occurrences"] + len(exp["sc_truncated"]["taxon"]["consensusBeans"]) >= 2


def test_routes_claims(directory):
    tables = {c.name: c for c in by_family("routes")}
    assert list(tables) == list(E.ROUTE_VARIANTS) and {c.route for c in tables.values()} == {"packed", "f64"}
    texts = {k: [c[3] for cols in read_table(E.write(c, directory)[0]).values() for c in cols] for k, c in tables.items()}
    milli = lambda t: len(t.split(b".")[1]) == 3
    assert all(len(v) == 1200 for v in texts.values())
    assert all(milli(t) and float(t) < 131.071 for t in texts["exact"]) and tables["exact"].route == "packed"
    assert [t for t in texts["four_decimals"] if not milli(t)] == [b"98.1234"] and texts["four_decimals"].index(b"98.1234") >= 1196
    assert [t for t in texts["at_limit"] if float(t) >= 131.071] == [b"131.071"] and all(milli(t) for t in texts["at_limit"])
    assert max(texts["below_limit"], key=float) == b"131.070" and all(milli(t) for t in texts["below_limit"])
    assert tables["four_decimals"].route == tables["at_limit"].route == "f64" and tables["below_limit"].route == "packed"
    for k, c in tables.items():                              # the odd value sits on a top row
        if k != "exact":
            q = c.queries[299 if k == "four_decimals" else 150]
            odd = [i for i, r in enumerate(q.rows) if r[2] in ("98.1234", "131.071", "131.070")]
            assert len(odd) == 1 and odd[0] in q.claim["top"]


def test_ragged_groups_are_ragged(directory):
    (case,) = by_family("ragged")
    bt, tj = E.write(case, directory)
    lin, table = lineages_of(tj), read_table(bt)
    last_row = json.load(open(tj))["taxonomies"][-1]
    seen = set()
    for q in case.queries:
        r = q.claim["ragged"]
        group = [lin[int(c[2])][0] for c in table[q.name]]
        lens = [len(l) for l in group]
        short = group[r["at"]]
        assert lens[r["at"]] == r["short_len"] == min(lens) and lens.count(min(lens)) == 1 and max(lens) == 4, q.name
        others = [l for i, l in enumerate(group) if i != r["at"]]
        if r["agree"]:
            assert all(l[:len(short)] == short for l in others), q.name                     # a proper prefix of every other
        else:
            assert all(l[:len(short) - 1] == short[:-1] and l[len(short) - 1] != short[-1] for l in others), q.name
        ids = {c[3] for c in table[q.name]}
        assert (len(ids) == 1) == r["tied"]
        assert r["last_db_row"] == (";".join(short) == last_row["textLineage"])
        seen.add((r["short_len"], ("first", "middle", "last")[(r["at"] > 0) + (r["at"] == len(group) - 1)], r["tied"], r["agree"], len(group), r["last_db_row"]))
        for strategy in case.strategies:       # the oracle never reads a level the short lineage lacks: the beans are above its end
            t = E.expected(case, strategy, directory)[q.name]["taxon"]
            assert sum(b["occurrences"] for b in t["consensusBeans"]) == len(group)
            assert all(b["rank"] in ("domain", "phylum", "class")[:r["short_len"]] for b in t["consensusBeans"]), (q.name, t)
    want = {(sl, pos, tied, agree, n) for sl in (2, 3) for pos in ("first", "middle", "last") for tied in (True, False)
            for agree in (True, False) for n in (4, 65)}
    assert {s[:5] for s in seen} == want
    assert any(s[5] for s in seen) and any(not s[5] for s in seen)
    assert set(case.strategies) == set(E.STRATEGIES)


def test_beans_claims(directory):
    case, dup = by_family("beans")
    assert dup.dup and not case.dup
    for strategy in E.STRATEGIES:
        exp = E.expected(case, strategy, directory)
        for q in case.queries:
            beans = exp[q.name]["taxon"]["consensusBeans"]
            assert len(beans) == q.claim["beans"], q.name
            if "accessions" in q.claim:
                assert beans[0]["accessions"] == q.claim["accessions"], q.name
            if "n_accessions" in q.claim:
                assert len(beans[0]["accessions"]) == q.claim["n_accessions"], q.name
        assert {b["rank"] for n in (65, 130) for b in exp[f"bn_one_lineage_{n}"]["taxon"]["consensusBeans"]} == {"species"}   # the last level
        eq = exp["bn_equal_occurrences"]["taxon"]["consensusBeans"]
        assert [b["occurrences"] for b in eq] == [2, 2, 2] and [b["identifier"] for b in eq] == sorted(b["identifier"] for b in eq)
        assert [b["occurrences"] for b in exp["bn_unequal_occurrences"]["taxon"]["consensusBeans"]] == [3, 2, 1]
        rev = exp["bn_file_order_against_accession_order"]["taxon"]["consensusBeans"]
        assert all(b["accessions"] == sorted(b["accessions"]) and len(b["accessions"]) == 5 for b in rev)
        forty = exp["bn_forty_beans"]["taxon"]["consensusBeans"]
        assert {b["occurrences"] for b in forty} == {1, 2}
        d = E.expected(dup, strategy, directory)
        assert d["bd_single_hit_twice"]["taxon"]["singleMatch"] is False
        assert [b["occurrences"] for b in d["bd_single_hit_twice"]["taxon"]["consensusBeans"]] == [2]
        assert sum(b["occurrences"] for b in d["bd_65_lines_130_rows"]["taxon"]["consensusBeans"]) == 130
    table = read_table(E.write(case, directory)[0])
    hi = [c[1] for c in table["bn_accession_bytes_above_0x7f"]]
    assert sum(max(a) >= 0x80 for a in hi) >= 4
    x = [c[1] for c in table["bn_same_accession_rows_63_64"]]
    assert x[63] == x[64] and len(set(x[:70])) == 69
