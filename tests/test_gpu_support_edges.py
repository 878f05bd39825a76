"""The support kernel (csrc/support_kernel.hip) at the edges of its clade range search and its segment scan:
every family of tests/support_edges.py through engine.support_device and engine.support_host, all eight fields against the
independent expected value, device and host bytes identical, the invariants of §15.1, the packed strides with 0xFFFFFFFF
and noise behind word 0.  The taxonomy's own row map has to equal the independent sort first: the hits are built from
the latter."""
import numpy as np
import pytest
import torch

from blutils_amd import engine, synth
from tests import support_edges as E
from tests import support_reference as ref

pytestmark = pytest.mark.gpu


def _taxonomy(t):
    lin_off, lin_node = t.lin_arrays()
    lin_rank = np.full(len(lin_node), synth.RANK_NAMES.index("clade"), np.uint16)
    tax = engine.Taxonomy(lin_off, lin_node, lin_rank, synth.RANK_NAMES, taxon="bacteria", device=0, bad=t.bad)
    fwd = tax.row_map()[0]
    diff = np.nonzero(fwd != t.eng)[0]
    assert len(diff) == 0, (t.name, "row map differs from the independent sort at row", diff[:5], fwd[diff[:5]], t.eng[diff[:5]])
    return tax


def _assert_fields(t, got, exp, route):
    assert len(got) == len(exp), (t.name, route)
    bad = np.zeros(len(exp), bool)
    for f in ref.SUPPORT_FIELDS:
        bad |= got[f].astype(np.int64) != exp[f]
    if bad.any():
        q = int(np.nonzero(bad)[0][0])
        f = next(f for f in ref.SUPPORT_FIELDS if int(got[f][q]) != int(exp[f][q]))
        raise AssertionError(f"{route}: {t.where(q)}: {f} = {int(got[f][q])}, expected {int(exp[f][q])} "
                             f"(got {got[q]}, expected {exp[q]}; {int(bad.sum())} queries differ)")


def _cuda(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to("cuda:0")


def _device(tax, t, eng, layout="tax_row", fill="ones"):
    hits = {"seg_off": _cuda(t.seg, np.int64), "bitscore": _cuda(t.bs, np.int32)}
    if layout == "tax_row":
        hits["tax_row"] = _cuda(eng, np.int32)
    else:
        words = {"packed": 4, "packed64": 6}[layout]
        hits[layout] = _cuda(E.packed_rows(eng, words, fill, seed=words), np.int32).reshape(-1)
    return engine.support_device(tax, hits, _cuda(t.recs.view(np.uint8), np.uint8))


def _all_routes(tax, t, strides):
    """Device and host, and with `strides` the 4- and 6-word records on both; returns the device counts."""
    exp, eng = t.expected(), t.eng_rows()
    dev = _device(tax, t, eng)
    _assert_fields(t, dev, exp, "device, tax_row")
    E.assert_invariants(dev, t)
    host = engine.support_host(tax, t.seg, t.bs, eng, t.recs)
    _assert_fields(t, host, exp, "host, tax_row")
    assert host.tobytes() == dev.tobytes()
    if strides:
        for layout, words in (("packed", 4), ("packed64", 6)):
            for fill in ("ones", "noise"):
                got = _device(tax, t, eng, layout, fill)
                _assert_fields(t, got, exp, f"device, {layout} ({words} words, {fill} behind word 0)")
                assert got.tobytes() == dev.tobytes()
            host = engine.support_host(tax, t.seg, t.bs, None, t.recs, **{layout: E.packed_rows(eng, words, "noise", seed=9)})
            _assert_fields(t, host, exp, f"host, {layout}")
            assert host.tobytes() == dev.tobytes()
    return dev


@pytest.mark.parametrize("name", E.SMALL_TABLES)
def test_range_search_edges_every_stride_both_routes(name):
    """Families 1 (near sweep), 2 (skip path), 4 (table ends) and 5 (levels), each through stride 1, 4 and 6 (family 8)."""
    t = E.table(name)
    tax = _taxonomy(t)
    dev = _all_routes(tax, t, strides=True)
    clade = t.q_lo >= 0
    assert (dev["n_support"][clade] >= 1).all() and not dev["n_support"][~clade].any()
    tax.close()


@pytest.fixture(scope="module")
def large():
    t = E.table("high_levels")
    tax = _taxonomy(t)
    yield tax, t
    tax.close()


def test_high_levels_of_the_sparse_table(large):
    """Family 3: 2^20 + 40 rows, 17 levels; clades of 2^k - 1, 2^k, 2^k + 1 blocks up to k = 16, the whole table under
    level_mask = 1, clades that touch either end of the table."""
    tax, t = large
    assert tax.n_tax == E.LARGE_ROWS
    dev = _all_routes(tax, t, strides=False)
    whole = (t.q_lo == 0) & (t.q_hi == tax.n_tax - 1)
    assert whole.sum() == 3 and (dev["n_support"][whole] == dev["n_matched"][whole]).all()


def test_high_levels_packed_strides(large):
    tax, t = large
    exp, eng = t.expected(), t.eng_rows()
    for layout in ("packed", "packed64"):
        _assert_fields(t, _device(tax, t, eng, layout, "noise"), exp, f"device, {layout}")


def test_segment_scan_edges():
    """Family 6: lengths 0 ... 4 097, where the maximum sits, ties, INT32_MIN / INT32_MAX, sums beyond 2^32."""
    t = E.table("segment_scan")
    tax = _taxonomy(t)
    dev = _all_routes(tax, t, strides=True)
    assert (dev["bits"] > 1 << 32).any() and (dev["support_bits"] < -(1 << 32)).any()
    tax.close()


def test_hostile_offsets_are_clamped():
    """Family 7 (§15.2 "Offsets are clamped"): s1 = min(s1, n_hits), s0 = min(s0, s1); records without a taxon."""
    t = E.hostile_offsets()
    tax = _taxonomy(t)
    dev = _all_routes(tax, t, strides=True)
    assert dev["n_hits"].sum() < 2 * E.HOSTILE_HITS and (dev["n_hits"] == 0).sum() >= 5
    tax.close()


def test_hostile_offsets_read_nothing_behind_n_hits():
    """The columns are the first n_hits elements of larger buffers whose tail holds valid row ids and a large score, and no
    offset leaves the buffers: the tail is memory the kernel could read and must not count."""
    t = E.hostile_offsets_inside_allocation()
    tax = _taxonomy(t)
    n, room = E.HOSTILE_HITS, E.HOSTILE_ALLOC
    assert int(t.seg.max()) <= room
    bs = torch.full((room,), 7777, dtype=torch.int32, device="cuda:0")
    rows = torch.full((room,), int(t.eng[3]), dtype=torch.int32, device="cuda:0")
    bs[:n] = _cuda(t.bs, np.int32)
    rows[:n] = _cuda(t.eng_rows(), np.int32)
    hits = {"seg_off": _cuda(t.seg, np.int64), "bitscore": bs[:n], "tax_row": rows[:n]}
    got = engine.support_device(tax, hits, _cuda(t.recs.view(np.uint8), np.uint8))
    _assert_fields(t, got, t.expected(), "device, columns inside larger buffers")
    assert got.tobytes() == engine.support_host(tax, t.seg, t.bs, t.eng_rows(), t.recs).tobytes()
    tax.close()
