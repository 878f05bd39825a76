"""The shared-level lookups at their table edges, on the device (tests/shared_level_edges.py).

The device code of these lookups is not the host mirror that tests/test_shared_level_edges.py pins: packed byte subtraction on
the reference row's run lengths, `exclude_mask` and 16-bit element minima in the block reader of `shared_levels()`, `uint4`
chain compares.  Only end-to-end records can check it: one query per case, laid out in three segment forms so that the stream
kernel (the top rows alone), the long pass (among 200 lower-scoring rows) and the worklist / long kernel (among 600) each see
every (lo, hi); four layouts, both strategies; every record equal to the columnar oracle's, and `bean_index`, the root
disagreement and the reference row equal to what the restatement says."""
import numpy as np
import pytest

from blutils_amd import _native as N
from blutils_amd import engine
from oracle import oracle as orc
from tests import helpers as H
from tests import shared_level_edges as E

pytestmark = pytest.mark.gpu

LAYOUTS = ("f64", "milli", "packed", "wide")


def _taxonomy(t):
    x = t.tax
    return engine.Taxonomy(x.lin_off, x.lin_node, x.lin_rank, x.rank_names, taxon="custom", custom=E.ZERO_CUTS, device=0)


def _run(tx, hits, strategy, layout):
    rows = tx.engine_rows(hits["tax_row"])
    f64 = layout in ("f64", "wide")
    return engine.run_consensus_host(tx, hits["seg_off"], hits["bitscore"], rows, hits["pident"] if f64 else None, hits["align_len"], hits["acc_rank"],
                                     strategy=strategy, pident_milli=None if f64 else hits["pident_milli"],
                                     packed={"packed": True, "wide": "wide"}.get(layout, False))


def _assert_restatement(t, cs, meta, got, where):
    for q, (s, root, agree, bean) in enumerate(E.expected(t, cs, meta)):
        at = where + (cs[meta["case"][q]], int(meta["form"][q]), s)
        assert got["ref_row"][q] == meta["ref_row"][q], at
        if root:
            assert got["status"][q] == N.ST_ERR_ROOT, at
        else:
            assert got["status"][q] == N.ST_MULTI and got["bean_index"][q] == bean, at
            assert bool(got["flags"][q] & N.FLAG_AGREE) == agree, at


@pytest.mark.parametrize("inst", E.SMALL, ids=E.instance_id)
def test_every_case_in_three_segment_forms_four_layouts_both_strategies(inst):
    t, cs = E.table(inst), E.cases(inst)
    tx = _taxonomy(t)
    inv = tx.row_map()[1]
    for strategy in ("cautious", "relaxed"):
        for form in E.FORMS:
            hits, meta = E.build_hits(t, cs, strategy, inv, forms=(form,))
            exp = H.columnar(t.tax, hits, "custom", strategy, E.ZERO_CUTS)
            for layout in LAYOUTS:
                got = _run(tx, hits, strategy, layout)
                H.assert_records_equal(got, exp)
                _assert_restatement(t, cs, meta, got, (t.name, strategy, layout))
    tx.close()


@pytest.mark.parametrize("n_wide", E.LIMITS)
def test_the_wide_node_limit(n_wide):
    """65 534 wide nodes: the highest node id is reached through a chain; 65 535: no wide tables.  The top rows alone, packed."""
    inst = ("limit", n_wide)
    t, cs = E.table(inst), E.cases(inst)[::2]
    tx = _taxonomy(t)
    inv = tx.row_map()[1]
    for strategy in ("cautious", "relaxed"):
        hits, meta = E.build_hits(t, cs, strategy, inv, forms=(0,))
        got = _run(tx, hits, strategy, "packed")
        H.assert_records_equal(got, H.columnar(t.tax, hits, "custom", strategy, E.ZERO_CUTS))
        _assert_restatement(t, cs, meta, got, (t.name, strategy, "packed"))
    tx.close()


@pytest.mark.parametrize("inst", [("chain", 17, 9, 21, False, 150), ("chain", 17, 70, 64, False, 32)], ids=E.instance_id)
def test_one_call_with_the_three_forms_interleaved(inst):
    """A wave whose lanes take different paths (the deeper chain entries are asked for per lane) gives the records of the
    per-form runs: the whole case list in one call, a case's three forms next to each other."""
    t, cs = E.table(inst), E.cases(inst)
    tx = _taxonomy(t)
    inv = tx.row_map()[1]
    fields = [f for f in orc.RESULT_DTYPE.names if f != "ref_row"]
    for strategy in ("cautious", "relaxed"):
        hits, meta = E.build_hits(t, cs, strategy, inv, interleave=True)
        exp = H.columnar(t.tax, hits, "custom", strategy, E.ZERO_CUTS)
        apart = {}
        for form in E.FORMS:
            h1, m1 = E.build_hits(t, cs, strategy, inv, forms=(form,))
            apart[form] = (_run(tx, h1, strategy, "packed"), h1["seg_off"], m1)
        for layout in LAYOUTS:
            got = _run(tx, hits, strategy, layout)
            H.assert_records_equal(got, exp)
            _assert_restatement(t, cs, meta, got, (t.name, strategy, layout))
            for form in E.FORMS:
                one, seg1, m1 = apart[form]
                mine = np.nonzero(meta["form"] == form)[0]
                assert (meta["case"][mine] == m1["case"]).all()
                for f in fields:
                    a, b = got[f][mine], one[f]
                    if f == "ident_used":
                        a, b = a.view(np.uint64), b.view(np.uint64)
                    assert (a == b).all(), (t.name, strategy, layout, form, f)
                # the reference row, counted from the query's first row (the lower-scoring rows differ between the two tables)
                assert (got["ref_row"][mine] - hits["seg_off"][:-1][mine] == one["ref_row"] - seg1[:-1]).all(), (t.name, strategy, layout, form)
    tx.close()
