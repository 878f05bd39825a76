"""The report, sample-table and count-table kernels (csrc/report_kernel.hip) on the cases of tests/report_table_edges.py
(DESIGN.md §9): every case through device pointers and host pointers and through each entry point that has the structure, the
result equal to the plain-Python expected value, `attempts` as an aimed case claims it and `table_slots` as the restated host
arithmetic gives it.  A failure names the family, the case, the entry point, the route and the first key that differs."""
import numpy as np
import pytest
import torch

from blutils_amd import _native as N
from blutils_amd import engine, report, synth
from tests import report_table_edges as E

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def _dev_recs(recs):
    return torch.from_numpy(recs.view(np.uint8)).to("cuda:0")


def _dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def _taxonomy(case):
    """the handle of a case's lineages (every level ranked `clade`) and its tax_row column: the engine row of every desc row,
    then the case's extra rows"""
    lin = case.lineages
    lin_off = np.concatenate([[0], np.cumsum([len(l) for l in lin])]).astype(np.uint64)
    lin_node = np.concatenate([np.asarray(l, np.uint32) for l in lin])
    lin_rank = np.full(len(lin_node), synth.RANK_NAMES.index("clade"), np.uint16)
    t = engine.Taxonomy(lin_off, lin_node, lin_rank, synth.RANK_NAMES, taxon="bacteria", device=0)
    assert t.n_tax == len(lin) and t.max_depth == case.depth
    return t, np.concatenate([t.row_map()[0], np.asarray(case.extra_rows, np.uint32)]).astype(np.uint32)


def _call(case, t, tax_row, entry, route, recs_dev=None, packed=None, n_hits=None):
    """one entry point on one route; tax_row: the plain column, or the side records with `packed`"""
    dev = route == "device"
    n_hits = len(tax_row) if n_hits is None else n_hits
    recs = case.recs
    if dev:
        recs = _dev_recs(case.recs) if recs_dev is None else recs_dev
        tax_row = tax_row if hasattr(tax_row, "data_ptr") else _dev(tax_row)
    w = case.weights
    if entry == "report":
        return report.consensus_report(t, tax_row, recs, n_hits, weights=None if w is None else _dev(w) if dev else w,
                                       on_device=dev, packed=packed)
    if entry == "sample":
        return report.consensus_sample_table(t, tax_row, recs, n_hits, _dev(case.sample_of) if dev else case.sample_of, case.n_samples,
                                             weights=None if w is None else _dev(w) if dev else w, on_device=dev, packed=packed)
    ptr, s, c = case.count_rows()
    if dev:
        ptr, s, c = _dev64(ptr), _dev(s), _dev(c)
    return report.consensus_sample_table_counts(t, tax_row, recs, n_hits, ptr, s, c, case.n_samples, on_device=dev, packed=packed)


def _hold(case, result, entry, route):
    """a result to the expected value, the claimed attempts and the restated table size"""
    where = case.where(entry, route)
    diff = E.compare(E.decode(result, entry), case.expected(entry), entry)
    assert diff is None, f"{where}: {diff}"
    want = case.attempts.get(entry)
    assert result["attempts"] == want if want else result["attempts"] in (1, 2), f"{where}: {result['attempts']} attempts for {want}"
    slots = case.table_slots(entry, result["attempts"])
    assert result["table_slots"] == slots, f"{where}: {result['table_slots']} slots for {slots} after {result['attempts']} attempts"


def _check(case, entries=None):
    t, tax_row = _taxonomy(case)
    out = {}
    for entry in entries or case.entries:
        for route in ("device", "host"):
            out[entry, route] = _call(case, t, tax_row, entry, route)
            _hold(case, out[entry, route], entry, route)
    return t, tax_row, out


def _refused(case, t, tax_row, entry, word, **kw):
    for route in kw.pop("routes", ("device", "host")):
        with pytest.raises(N.BluError, match=word) as e:
            _call(case, t, tax_row, entry, route, **kw)
        assert e.value.code == N.BLU_ERR_INVALID_ARG, f"{case.where(entry, route)}: code {e.value.code}"


# ---- family 1: chains in the global tables ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", E.CHAIN_KINDS)
def test_global_chains_at_the_probe_limit_and_the_table_end(kind):
    """chains of 2, 127 and 128 slots are one attempt, 129 start again from the bound (every case holds queries without a
    taxon and without a level, so a counter that survived the first attempt would show); the cell chains overflow the cell table
    alone, and the report of the same records, which has none, takes one attempt"""
    for case in E.global_chains(kind):
        _, _, out = _check(case)
        assert sum(case.expected("sample")["unclassified"]) > 0 and sum(case.expected("sample")["unplaced"]) > 0
        if case.claims["probe"] > E.PROBE_FIRST:
            assert out["sample", "device"]["attempts"] == out["count", "host"]["attempts"] == 2


# ---- family 2: chains in the blocks' LDS tables -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n,target", E.LDS_PATH_CASES)
def test_lds_chains_of_leaf_paths(n, target):
    case = E.lds_path_chain(n, target)
    assert case.claims["found"] == n
    _check(case)


@pytest.mark.parametrize("n,target,hi", E.LDS_CELL_CASES)
def test_lds_chains_of_cells_and_of_the_fixed_rows(n, target, hi):
    """beyond eight keys of one LDS home a block adds to global memory at once: to the cell table, or (the unclassified and the
    unplaced row) to the per-sample counters"""
    case = E.lds_cell_chain(n, target, hi)
    assert case.claims["found"] == n
    _check(case, ("sample", "count"))


def test_fixed_rows_longer_than_the_lds_table():
    case = E.long_fixed_rows()
    _check(case)
    want = case.expected("count")
    assert sum(1 for x in want["unclassified"] if x) == 5000 and sum(1 for x in want["unplaced"] if x) == 5000


def test_a_block_crowded_by_classified_cells_keeps_its_fixed_rows():
    case = E.crowded_block()
    _check(case)
    want = case.expected("sample")
    assert len(want["cells"]) == 2101 and sum(1 for x in want["unclassified"] if x) == 162 == sum(1 for x in want["unplaced"] if x)


# ---- family 3: the lane mapping of count_cells ------------------------------------------------------------------------------------

def test_every_level_count_against_rows_either_side_of_the_lane_stride():
    case = E.lane_mapping()
    _check(case)
    assert max(len(p) for p in case.expected("count")["direct"]) == 64


# ---- family 4: refusals -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", E.BAD_RECORDS)
def test_a_bad_record_is_refused_naming_the_query(how):
    """by report_paths, sample_cells and count_cells alike, wherever the query sits in a wave's run of 32; the same junk on a
    record without a taxon is no error"""
    for bad in E.BAD_PLACES:
        case = E.refusal_case(how, bad)
        t, tax_row = _taxonomy(case)
        for entry in E.ENTRIES:
            _refused(case, t, tax_row, entry, f"record {bad} has a taxon")
        _check(E.refusal_case(how, bad, status=2 + bad % 3))


def test_device_records_off_a_16_byte_boundary_are_refused():
    case = E.refusal_case()
    t, tax_row = _taxonomy(case)
    buf = torch.zeros(32 * len(case.recs) + 16, dtype=torch.uint8, device="cuda:0")
    off = buf[8:8 + 32 * len(case.recs)]
    off.copy_(_dev_recs(case.recs))
    assert off.data_ptr() % 16 == 8
    for entry in E.ENTRIES:
        _refused(case, t, tax_row, entry, "aligned", routes=("device",), recs_dev=off)


def test_which_error_wins_is_the_host_codes_order():
    """a bad row before a bad sample before a bad record before a reserved node; each in a query of its own"""
    lineages = E.REFUSAL_LINEAGES + [[E.NONE, 9]]
    nq = E.REFUSAL_QUERIES
    desc, st = [q % 2 for q in range(nq)], [0] * nq
    desc[40], desc[80] = 3, 2                                              # the unmatched extra row; the reserved node
    sample_of = [q % 4 for q in range(nq)]
    sample_of[120] = 4
    row_ptr = np.arange(nq + 1, dtype=np.uint64)
    for drop in range(4):
        ptr = row_ptr.copy()
        d, s = list(desc), list(sample_of)
        if drop == 0:
            ptr[161] = ptr[160] - 1                                        # row 160 ends before it begins
        if drop > 1:
            s[120] = 0
        if drop > 2:
            d[40] = 0
        csr = (ptr, np.array(s, np.uint32), np.ones(nq, np.uint32))
        case = E.small(4, f"precedence_{drop}", lineages, d, st, [0b111] * nq, s, 4, csr=csr, extra_rows=(E.UNMATCHED,))
        t, tax_row = _taxonomy(case)
        _refused(case, t, tax_row, "count", ("query 16[01] has a row_ptr", "query 120 has a sample id", "record 40 has a taxon", "record 80 has a path")[drop])
        _refused(case, t, tax_row, "sample", ("query 120 has a sample id", "query 120 has a sample id", "record 40 has a taxon", "record 80 has a path")[drop])
        _refused(case, t, tax_row, "report", "record 80 has a path" if drop == 3 else "record 40 has a taxon")


# ---- family 5: strides and shapes -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("packed", ["packed", "packed64"])
def test_rows_read_from_the_packed_side_records(packed):
    rng = np.random.default_rng(4)
    lineages = [[1, 10 + i // 8, 100 + i] for i in range(40)]
    nq = 300
    desc = rng.integers(0, 40, nq).tolist()
    st = rng.choice([0, 1, 2], nq, p=[0.6, 0.3, 0.1]).tolist()
    desc = [-1 if s == 2 else d for d, s in zip(desc, st)]
    lengths = rng.integers(0, 6, nq)
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    csr = (ptr, rng.integers(0, 7, int(ptr[-1])).astype(np.uint32), rng.integers(0, 50, int(ptr[-1])).astype(np.uint32))
    case = E.small(5, packed, lineages, desc, st, rng.integers(0, 8, nq).tolist(), rng.integers(0, 7, nq), 7, E._weights(nq, 1), csr=csr)
    t, tax_row, plain = _check(case)
    zeros = torch.zeros(len(tax_row), dtype=torch.int32, device="cuda:0")
    cols = {"tax_row": _dev(tax_row), "align_len": zeros + 400, "acc_rank": zeros, "pident_milli": zeros + 99000}
    side = engine.pack_hits_device(t, cols, wide=packed == "packed64")
    words = 6 if packed == "packed64" else 4
    assert side.numel() == words * len(tax_row)
    host_side = side.cpu().numpy().view(np.uint32)
    assert (host_side[::words] == tax_row).all()
    for entry in E.ENTRIES:
        for route, col in (("device", side), ("host", host_side)):
            got = _call(case, t, col, entry, route, packed=packed, n_hits=len(tax_row))
            _hold(case, got, entry, f"{route} {packed}")
            assert got["table_slots"] == plain[entry, route]["table_slots"]


def _shapes():
    L = [[1, 2, 3], [1, 2, 4], [5]]
    yield E.small(5, "no_queries", L, [], [], [], [], 3, np.zeros(0, np.uint32))
    yield E.small(5, "no_queries_no_samples", L, [], [], [], [], 0, np.zeros(0, np.uint32))
    yield E.small(5, "no_record_with_a_taxon", L, [-1] * 70, [2 + q % 3 for q in range(70)], [0b111] * 70, [q % 3 for q in range(70)], 3,
                  E._weights(70, 2))
    yield E.small(5, "no_record_with_a_level", L, [q % 3 for q in range(70)], [q % 2 for q in range(70)], [0 if q % 2 else 0b1000 for q in range(70)],
                  [q % 3 for q in range(70)], 3, E._weights(70, 3))
    yield E.small(5, "one_sample", L, [q % 3 for q in range(70)], [q % 3 for q in range(70)], [q % 8 for q in range(70)], [0] * 70, 1,
                  E._weights(70, 4))
    w = np.array([0, E.U32_MAX] * 35, np.uint32)
    yield E.small(5, "weights_0_and_2^32-1", L, [(q // 2) % 3 for q in range(70)], [(q // 7) % 3 for q in range(70)], [0b111] * 70,
                  [(q // 4) % 3 for q in range(70)], 3, w)
    # count rows made of zeros only (queries 0 and 1: the only ones on lineage [5]), beside rows with counts
    desc = [2, 2] + [q % 2 for q in range(68)]
    lengths = [4, 0] + [3] * 68
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    count = np.array([0] * 4 + [1 + k for k in range(3 * 68)], np.uint32)
    yield E.small(5, "a_row_of_zeros", L, desc, [0] * 70, [0b111] * 70, None, 3, None,
                  csr=(ptr, (np.arange(len(count)) % 3).astype(np.uint32), count), entries=("count",))


@pytest.mark.parametrize("case", list(_shapes()), ids=lambda c: c.name)
def test_degenerate_shapes(case):
    _check(case)
    if case.name == "a_row_of_zeros":
        want = case.expected("count")
        assert want["direct"][(5,)] == 0 and not any(p == (5,) for p, _ in want["cells"])


# ---- family 6: node id 0xFFFFFFFF -------------------------------------------------------------------------------------------------

RESERVED_LINEAGES = [[E.NONE], [5, E.NONE, 7], [5, E.NONE], [6, 8]]


def _reserved_case(name, bad=None):
    """40 queries that meet 0xFFFFFFFF as a second element, under a mask without a level, or without a taxon; `bad`: (query, desc
    row, mask) of one whose path begins with it"""
    nq = 40
    desc = [1 + q % 3 for q in range(nq)]
    st = [q % 2 for q in range(nq)]
    mask = [(0b001, 0b011, 0b111, 0b101)[q % 4] for q in range(nq)]
    desc[7], mask[7] = 0, 0b10                                             # row [0xFFFFFFFF] under a mask beyond it: unplaced
    desc[9], st[9] = 0, 2                                                  # ... and without a taxon
    if bad:
        desc[bad[0]], mask[bad[0]], st[bad[0]] = bad[1], bad[2], 0
    return E.small(6, name, RESERVED_LINEAGES, desc, st, mask, [q % 3 for q in range(nq)], 3, E._weights(nq, 6))


def test_node_id_all_ones_behind_a_first_element_is_an_id_like_any_other():
    case = _reserved_case("later_element")
    _check(case)
    assert (5, E.NONE, 7) in case.expected("sample")["direct"]


@pytest.mark.parametrize("bad", [(0, 0, 0b1), (39, 0, 0b1), (31, 2, 0b10), (20, 1, 0b110)], ids=lambda b: f"query_{b[0]}_row_{b[1]}_mask_{b[2]}")
def test_a_path_that_begins_with_node_id_all_ones_is_refused(bad):
    """its key would be the table's empty word: the three kernels flag the record and nothing is counted"""
    case = _reserved_case("first_element", bad)
    t, tax_row = _taxonomy(case)
    for entry in E.ENTRIES:
        _refused(case, t, tax_row, entry, f"record {bad[0]} has a path that begins with node id 0xFFFFFFFF")
