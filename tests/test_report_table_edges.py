"""Keeps tests/report_table_edges.py honest without a GPU: every claim of a case is recomputed from the case's own
lineages and records with the Python-integer hashes (the cases are found with numpy's), the predicted table sizes from the
restated host arithmetic, and the expected value is held to blutils_amd.report's host restatement and to the numpy aggregates
of the existing GPU tests."""
import numpy as np
import pytest

from blutils_amd import report
from tests import report_table_edges as E


def _keys_of_queries(case, slots):
    """the first-level path keys a case's queries reach (a case whose paths all sit at home), and nothing else"""
    keys = set()
    for q in range(len(case.recs)):
        if case.recs["status"][q] < 2:
            p = E.selected(case.lineages[int(case.desc[q])], int(case.recs["level_mask"][q]))
            if p:
                keys.add((E.NONE << 32) | p[0])
    return keys


# ---- the hashes ---------------------------------------------------------------------------------------------------------------------

def test_integer_and_numpy_hashes_agree():
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 1 << 64, 2000, dtype=np.uint64, endpoint=False)
    keys[:4] = [0, 1, E.U64_MAX, (E.NONE << 32) | 5]
    assert E._fmix64_np(keys).tolist() == [E.fmix64(int(k)) for k in keys]
    assert E._lds_cell_home_np(keys).tolist() == [E.lds_cell_home(int(k)) for k in keys]
    assert E._home_np(keys, 1024).tolist() == [E.home(int(k), 1024) for k in keys]
    assert E.fmix64(0) == 0 and E.fmix64(E.U64_MAX) != E.U64_MAX              # (the empty word is a key like any other to the hash)
    assert max(E.lds_cell_home(int(k)) for k in keys) < E.LDS_SLOTS and {E.lds_path_home(p) for p in range(1 << 16)} == set(range(E.LDS_SLOTS))


def test_sizes_follow_the_host_arithmetic():
    assert [E.next_pow2(x) for x in (0, 1, 2, 3, 1024, 1025)] == [1, 1, 2, 4, 1024, 2048]
    assert E.first_sizes("report", 512, 1, 300) == (1024, None) and E.first_sizes("report", 513, 1, 300)[0] == 2048
    assert E.first_sizes("sample", 256, 2, 300) == (1024, 1024) and E.first_sizes("sample", 300, 2, 300) == (2048, 2048)
    assert E.first_sizes("sample", 100_000, 7, 3000) == (32768, 262144)     # guess 10 096, cells guess + n_queries
    assert E.first_sizes("count", 100, 2, 300, 5, 513) == (1024, 2048) and E.first_sizes("count", 100, 2, 300, 0, 10 ** 9)[1] == 1024
    assert E.retry_sizes("report", 600) == (2048, None) and E.retry_sizes("sample", 600) == (2048, 2048)
    assert E.retry_sizes("count", 600, 5000) == (2048, 16384)


# ---- family 1 -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", E.CHAIN_KINDS)
def test_global_chains_lie_where_they_claim(kind):
    lengths = E.ACROSS_LENGTHS if kind == "second_across_parent" else E.CHAIN_LENGTHS
    cases = E.global_chains(kind)
    assert [len(c.claims["chain_keys"]) for c in cases] == list(lengths)
    for case, n in zip(cases, lengths):
        cl, S = case.claims, 1024
        assert len(set(cl["chain_keys"])) == n and {E.home(k, S) for k in cl["chain_keys"]} == {cl["home"]}
        probe = n + 1 if kind == "second_across_parent" else n
        assert cl["probe"] == probe and cl["span"] == {(cl["home"] + i) % S for i in range(probe)}
        wraps = cl["home"] + probe > S
        assert wraps == (kind.endswith("-1") or (kind.endswith("-2") and probe > 2)) or kind.startswith("second")
        others = [E.home(k, S) for k in cl["other_keys"]]
        assert len(set(others)) == len(others)                               # isolated: each at its home
        if kind == "second_across_parent":
            assert cl["parent_slot"] in cl["span"] and cl["parent_slot"] == others[-1] == (cl["home"] + 1) % S
            others = others[:-1]
        assert not set(others) & cl["span"]
        # the keys are the ones the queries make, and there are no more
        if cl["table"] == "path":
            first = _keys_of_queries(case, S)
            if kind.startswith("second"):
                assert first == set(cl["other_keys"])
                a = cl["parent_slot"]
                second = {(a << 32) | p[1] for p in case.expected("report")["direct"] if len(p) == 2}
                assert second == set(cl["chain_keys"]) and all(p[0] == cl["other_keys"][-1] & E.U32_MAX for p in case.expected("report")["direct"] if len(p) == 2)
            else:
                assert first == set(cl["chain_keys"]) | set(cl["other_keys"])
            over = probe > E.PROBE_FIRST
            assert case.attempts == dict.fromkeys(E.ENTRIES, 2 if over else 1)
        else:
            assert _keys_of_queries(case, S) == set(cl["path_keys"])
            slots = [E.home(k, S) for k in cl["path_keys"]]
            assert len(set(slots)) == len(slots)                             # the path table: seven keys at home, uncrowded
            slot_of = {k & E.U32_MAX: s for k, s in zip(cl["path_keys"], slots)}
            cells = {(slot_of[p[0]] << 32) | s for (p, s) in case.expected("sample")["cells"]}
            assert cells == set(cl["chain_keys"]) | set(cl["other_keys"])
            assert case.attempts == {"report": 1, "sample": 2 if n > 128 else 1, "count": 2 if n > 128 else 1}
        # 1 024 slots in every table of every entry point, before and after the retry
        for entry in E.ENTRIES:
            for attempts in (1, 2):
                assert case.sizes(entry, attempts) == (1024, None if entry == "report" else 1024), (case.name, entry, attempts)
        want = case.expected("sample")
        assert sum(want["unclassified"]) > 0 and sum(want["unplaced"]) > 0 and len(case.recs) <= 512
        assert case.expected("count") == want                               # one non-zero a query: the sibling's table


# ---- family 2 -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,target", E.LDS_PATH_CASES)
def test_lds_path_chains_lie_where_they_claim(n, target):
    case = E.lds_path_chain(n, target)
    cl, S = case.claims, E.LDS_PATH_SLOTS
    assert cl["found"] == n >= 8 and (n == 8 or cl["found"] >= 9)
    assert case.sizes("report", 1) == (S, None) and case.sizes("sample", 1)[0] == S and case.sizes("count", 1)[0] == S
    ids = [E.home(k, S) for k in cl["chain_keys"]]
    assert ids == cl["path_ids"] and len(set(ids)) == n                      # each alone at its home: the slot is the path id
    assert {E.lds_path_home(p) for p in ids} == {target}
    assert _keys_of_queries(case, S) == set(cl["chain_keys"])
    block = case.recs[:E.WALK_BLOCK]
    assert (block["status"] < 2).all() and (case.recs["level_mask"][E.WALK_BLOCK:][case.recs["status"][E.WALK_BLOCK:] < 2] == 0).all()
    assert set(block["ref_row"].tolist()) == set(range(n)) and (block["ref_row"][::2] == 0).all()
    assert target + min(n, E.LDS_PROBE) > E.LDS_SLOTS or target == 1000     # the two at the end wrap
    # smaller tables do not hold 40 slots under one LDS home
    assert sum(1 for s in range(S // 2) if E.lds_path_home(s) == target) < 40 <= sum(1 for s in range(S) if E.lds_path_home(s) == target)


@pytest.mark.parametrize("n,target,hi", E.LDS_CELL_CASES)
def test_lds_cell_chains_lie_where_they_claim(n, target, hi):
    case = E.lds_cell_chain(n, target, hi)
    cl = case.claims
    assert cl["found"] == n and len(set(cl["chain_keys"])) == n and {E.lds_cell_home(k) for k in cl["chain_keys"]} == {target}
    assert len(case.recs) <= E.COUNT_BLOCK                                   # one block of either kernel
    want = case.expected("sample")
    samples = {k & E.U32_MAX for k in cl["chain_keys"]}
    if hi == "path":
        node = case.lineages[0][0]
        assert {k >> 32 for k in cl["chain_keys"]} == {E.home((E.NONE << 32) | node, 1024)}
        assert {s for (p, s) in want["cells"] if p == (node,)} == samples
        homes = [E.home((E.NONE << 32) | l[0], 1024) for l in case.lineages]
        assert len(set(homes)) == len(homes)
    else:
        assert {k >> 32 for k in cl["chain_keys"]} == {E.CELL_UNCLASSIFIED if hi == "unclassified" else E.CELL_UNPLACED}
        assert {s for s, v in enumerate(want[hi]) if v} == samples
    assert case.sample_of[0] == case.sample_of[2] == case.sample_of[2 * n - 2]    # the hot key in between


def test_fixed_rows_fall_out_of_the_lds_table():
    case = E.long_fixed_rows()
    ptr, sample, count = case.csr
    for q, key in ((3, "unclassified"), (70, "unplaced")):
        row = sample[int(ptr[q]):int(ptr[q + 1])]
        assert len(set(row.tolist())) == 5000 > E.LDS_SLOTS and q < E.COUNT_BLOCK
        assert sum(1 for x in case.expected("count")[key] if x) == 5000
    assert case.recs["status"][3] >= 2 and case.recs["status"][70] < 2 and case.recs["level_mask"][70] == 0
    assert len(case.recs) % E.COUNT_BLOCK
    case = E.crowded_block()
    want = case.expected("sample")
    assert len(case.recs) == E.WALK_BLOCK and len(want["cells"]) > E.LDS_SLOTS
    assert sum(1 for x in want["unclassified"] if x) == sum(1 for x in want["unplaced"] if x) == 162


# ---- family 3 -----------------------------------------------------------------------------------------------------------------------

def test_lane_mapping_covers_every_level_count_and_row_kind():
    case = E.lane_mapping()
    plan = case.claims["plan"]
    ptr, sample, count = case.csr
    nq = len(plan)
    assert nq == len(case.recs) and nq % E.COUNT_BLOCK and nq > 4 * E.COUNT_BLOCK
    assert {(L, rk) for L, rk, _ in plan[:512]} == {(L, rk) for L in range(1, 65) for rk in E.ROW_KINDS}
    assert {(q % E.COUNT_Q, rk) for q, (_, rk, _) in enumerate(plan[:512])} == {(s, rk) for s in range(E.COUNT_Q) for rk in E.ROW_KINDS}
    assert {mk for _, _, mk in plan} == set(E.MASK_KINDS) | {"bit63", "no_taxon", "no_level"}
    for mk in E.MASK_KINDS:                                                  # each way to L levels at small and large L, dividing 64 or not
        Ls = {L for L, _, m in plan if m == mk}
        assert Ls & {1, 2, 4, 8, 16, 32, 64} and Ls & {3, 5, 6, 7, 9, 21, 22, 33, 63} and min(Ls) <= 3 and max(Ls) >= 60
    primes = set(E.PRIMES)
    for q, (L, rk, mk) in enumerate(plan):
        per = 64 // L
        want = {"0": 0, "1": 1, "per-1": per - 1, "per": per, "per+1": per + 1, "2per": 2 * per, "2per+1": 2 * per + 1, "3x64+1": 3 * 64 + 1}[rk]
        lo, hi = int(ptr[q]), int(ptr[q + 1])
        assert hi - lo == want, (q, L, rk)
        rec = case.recs[q]
        if mk == "no_taxon":
            assert rec["status"] >= 2
        else:
            levels = E.selected(case.lineages[int(rec["ref_row"])], int(rec["level_mask"]))
            assert rec["status"] < 2 and len(levels) == (0 if mk == "no_level" else L), (q, L, mk)
            if mk == "bit63":
                assert int(rec["level_mask"]) == 1 << 63 and L == 1
            if mk == "short":
                assert len(case.lineages[int(rec["ref_row"])]) == L and int(rec["level_mask"]) == E.U64_MAX
        s, c = sample[lo:hi].tolist(), count[lo:hi].tolist()
        assert len(set(s)) == len(s)                                         # a cell of this query is one non-zero
        nz = [x for x in c if x]
        assert len(set(nz)) == len(nz) and all(x & (x - 1) == 0 or x in primes for x in nz)
        assert (0 in c) == (hi - lo >= 3)
    assert sum(1 for L, rk, _ in plan if 64 % L and row_longer_than_per(L, rk)) > 100


def row_longer_than_per(L, rk):
    return E.row_length(rk, L) > 64 // L


# ---- the refusal cases ----------------------------------------------------------------------------------------------------------------

def test_refusal_cases_hold_one_bad_record():
    assert sorted(q % 32 for q in E.BAD_PLACES) == [0, 4, 7, 31] and E.BAD_PLACES[2] == E.REFUSAL_QUERIES - 1
    for how in E.BAD_RECORDS:
        for bad in E.BAD_PLACES:
            case = E.refusal_case(how, bad)
            n_rows = len(case.lineages) + len(case.extra_rows)
            named = case.recs["ref_row"].astype(np.int64)
            good = (case.recs["status"] >= 2) | (named < len(case.lineages))
            assert np.nonzero(~good)[0].tolist() == [bad]
            if how == "ref_row_past_n_rows":
                assert named[bad] >= n_rows
            else:
                row = case.extra_rows[named[bad] - len(case.lineages)]
                assert (row == E.UNMATCHED) if how == "unmatched_row" else (row != E.UNMATCHED and row & ((1 << E.ROW_BITS) - 1) >= len(case.lineages))
            ok = E.refusal_case(how, bad, status=2)
            assert ok.recs["status"][bad] == 2 and ok.recs["ref_row"][bad] == case.recs["ref_row"][bad]
            assert ok.expected("sample")["total"] == E.REFUSAL_QUERIES


# ---- the expected value against the host restatement and the numpy aggregates ---------------------------------------------------------

def _as_results(case, entry):
    """the case as a document's results: the taxonomy of a query spells its node tuple, its name carries sample and size"""
    out = []
    for q in range(len(case.recs)):
        name = f"q{q};sample=S{int(case.sample_of[q]):07d};size={case.weight(q)}" if entry != "count" else f"q{q}"
        taxon = None
        if case.recs["status"][q] < 2:
            p = E.selected(case.lineages[int(case.desc[q])], int(case.recs["level_mask"][q]))
            taxon = {"taxonomy": ";".join(f"clade__{x}" for x in p)}
        out.append({"query": name, "taxon": taxon})
    return out


def _spell(p):
    return tuple(f"clade__{x}" for x in p)


def _table_of_text(text):
    """sample_table_from_results' text -> ({(taxonomy, column): value > 0}, the listed taxonomies)"""
    lines = text.splitlines()
    cols = lines[0].split("\t")[4:]
    cells, listed = {}, []
    for line in lines[1:]:
        f = line.split("\t")
        key = f[2] if f[2] else f[1]
        listed.append(key)
        assert int(f[3]) == sum(int(x) for x in f[4:])
        for c, x in zip(cols, f[4:]):
            if int(x):
                cells[(key, c)] = int(x)
    return cells, listed


def _held_to_the_host_restatement(case, tmp_path=None):
    want = case.expected("report")
    clade = {}
    for (p, _), v in want["cells"].items():
        clade[p] = clade.get(p, 0) + v
    text = report.render(want["unclassified"][0], want["unplaced"][0], {_spell(p): [d, clade.get(p, 0)] for p, d in want["direct"].items()})
    assert text == report.report_from_results(_as_results(case, "report"), "size")
    for entry in ("sample", "count"):
        want = case.expected(entry)
        if entry == "count":
            if tmp_path is None:
                continue
            ptr, s, c = case.count_rows()
            lines = ["#OTU ID\t" + "\t".join(f"S{k:07d}" for k in range(case.n_samples))]
            for q in range(len(case.recs)):
                row = [0] * case.n_samples
                for k in range(int(ptr[q]), int(ptr[q + 1])):
                    row[int(s[k])] += int(c[k])
                lines.append(f"q{q}\t" + "\t".join(map(str, row)))
            (tmp_path / "counts.tsv").write_text("\n".join(lines) + "\n")
            got, listed = _table_of_text(report.sample_table_from_results(_as_results(case, entry), "one", str(tmp_path / "counts.tsv")))
        else:
            got, listed = _table_of_text(report.sample_table_from_results(_as_results(case, entry), "size"))
        mine = {(";".join(_spell(p)), f"S{s:07d}"): v for (p, s), v in want["cells"].items()}
        mine.update({("unclassified", f"S{s:07d}"): v for s, v in enumerate(want["unclassified"]) if v})
        mine.update({("unplaced", f"S{s:07d}"): v for s, v in enumerate(want["unplaced"]) if v})
        assert got == mine, (case.name, entry, E.first_difference(got, mine))
        assert set(listed) - {"unclassified", "unplaced"} == {";".join(_spell(p)) for p in want["direct"]}, (case.name, entry)


def _random_case(seed, nq=400, ns=9, distinct_rows=False):
    rng = np.random.default_rng(seed)
    lineages = [[1, 10 + i // 8, 100 + i // 2, 1000 + i][:1 + i % 4] for i in range(40)] + [[2] + [3000 + j for j in range(63)]]
    st = rng.choice([0, 1, 2, 16], nq, p=[0.5, 0.3, 0.1, 0.1]).tolist()
    desc = [-1 if s >= 2 else int(d) for s, d in zip(st, rng.integers(0, len(lineages), nq))]
    mask = [int(m) for m in rng.integers(0, 32, nq)]
    mask[::17] = [E.U64_MAX] * len(mask[::17])
    mask[5::19] = [1 << 63] * len(mask[5::19])
    lengths = rng.integers(0, 7, nq)
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    sample = np.concatenate([rng.permutation(ns)[:n] for n in lengths] + [np.zeros(0, np.int64)]).astype(np.uint32) if distinct_rows else \
        rng.integers(0, ns, int(ptr[-1])).astype(np.uint32)
    csr = (ptr, sample, rng.integers(0, 40, int(ptr[-1])).astype(np.uint32))
    w = rng.integers(0, 50, nq).astype(np.uint32)
    return E.small(0, f"random_{seed}", lineages, desc, st, mask, np.sort(rng.integers(0, ns, nq)), ns, w, csr=csr)


def test_expected_value_against_the_host_restatement(tmp_path):
    for case in (E.global_chain("second", 2), E.global_chain("cells", 127), E.crowded_block(), E.lds_cell_chain(9, 77, "unplaced")):
        _held_to_the_host_restatement(case)
    _held_to_the_host_restatement(_random_case(3, distinct_rows=True), tmp_path)
    # the lane mapping's rows as a count table
    _held_to_the_host_restatement(E.lane_mapping(), tmp_path)


def test_expected_value_against_the_numpy_aggregates_of_the_gpu_tests():
    from tests.test_gpu_count_table import _expect
    from tests.test_gpu_report import _int_aggregate
    from tests.test_gpu_sample_table import _cells, _HandPaths
    for seed in range(4):
        case = _random_case(10 + seed)
        recs = case.recs.copy()
        recs["ref_row"] = np.where(recs["status"] < 2, recs["ref_row"], 0)      # (the aggregates index with it)
        recs["status"] = case.recs["status"]
        paths, u, n = _int_aggregate(case.lineages, recs, case.weights)
        want = case.expected("report")
        assert {p: v[0] for p, v in paths.items()} == want["direct"] and (u, n) == (want["unclassified"][0], want["unplaced"][0])
        cells, unc, unp = _cells(_HandPaths(case.lineages, recs), recs, case.sample_of, case.weights)
        want = case.expected("sample")
        assert cells == want["cells"] and unc == want["unclassified"][:len(unc)] and unp == want["unplaced"][:len(unp)]
        assert not any(want["unclassified"][len(unc):]) and not any(want["unplaced"][len(unp):])
        cells, direct, unc, unp = _expect(_HandPaths(case.lineages, recs), recs, *case.count_rows(), case.n_samples)
        want = case.expected("count")
        assert (cells, direct, unc, unp) == (want["cells"], want["direct"], want["unclassified"], want["unplaced"])


def test_compare_names_the_first_difference():
    case = _random_case(20)
    for entry in E.ENTRIES:
        want = case.expected(entry)
        got = {k: (dict(v) if isinstance(v, dict) else list(v) if isinstance(v, list) else v) for k, v in want.items()}
        clade = {p: 0 for p in want["direct"]}
        for (p, _), v in want["cells"].items():
            clade[p] += v
        got["clade"] = clade
        assert E.compare(got, want, entry) is None
        p = min(want["direct"])
        got["direct"][p] += 1
        assert f"direct of path {p}" in E.compare(got, want, entry)
        got["direct"][p] -= 1
        got["unplaced"][0] += 1
        assert "unplaced" in E.compare(got, want, entry)
    key = min(want["cells"])
    got["unplaced"][0] -= 1
    del got["cells"][key]
    assert f"cell (path {key[0]}, sample {key[1]})" in E.compare(got, want, "count")
