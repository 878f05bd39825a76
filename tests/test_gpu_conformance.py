"""Conformance matrix of the consensus engine: every hit-table layout through every host entry path, both strategies, and
the automatic and both forced builds of the stream kernel, on boundary tables (tests/conformance_tables.py) whose top
groups sit one milli-percent or one ulp from a level's cutoff.  Every field of every record against the columnar oracle.

Layouts: f64 columns, milli-percent columns, 16-byte packed records, 24-byte packed64 records (layouts 0..3 of
launch_consensus).  Tables off the milli-percent grid go to the f64 layouts only; the milli-percent layouts get the
on-grid variant of the same tables.  Paths: host pointers in one chunk; host pointers cut into chunks (BLU_STAGE_ROWS,
one size below the longest query); device pointers, three calls on the same buffers (the per-table kind cache and its
"skip the worklist kernel" bit), then the offsets rewritten in place, with short and then with long segments, and three
calls on each; blu_consensus_run_multi over two and three handles."""
import functools

import numpy as np
import pytest

from blutils_amd import engine
from tests import conformance_tables as CT
from tests import helpers as H

pytestmark = pytest.mark.gpu

LAYOUTS = ("f64", "milli", "packed", "packed64")
PATHS = ("host", "chunked", "device", "multi")
STRATEGIES = ("relaxed", "cautious")
BUILDS = (None, "ring", "noring")                 # BLU_STREAM_KIND unset: the device classifies the table
STAGE_ROWS = (40000, 5000, 1000)                  # the longest query has 1500 rows
# (seed, taxon, custom, deep): built-in backbones on deep taxonomies (lineages past 16 levels, many interpolated cutoffs),
# the custom backbone on both depths
CONFIGS = ((31, "bacteria", None, True), (32, "fungi", None, True), (33, "custom", H.CUSTOM_16S, False),
           (34, "custom", H.CUSTOM_16S, True), (35, "bacteria", None, True), (36, "fungi", None, True))


@functools.lru_cache(maxsize=None)
def _table(i: int, grid: bool) -> CT.BoundaryTable:
    seed, taxon, custom, deep = CONFIGS[i]
    return CT.build(seed, taxon, custom, deep=deep, grid=grid)


@functools.lru_cache(maxsize=None)
def _recut(i: int, grid: bool):
    """The table's rows cut into even short segments (an empty worklist queue), and into long ones (the worklist kernel)."""
    t = _table(i, grid)
    return t.with_segments(CT.even_segments(t.hits["seg_off"])), t.with_segments(CT.long_segments(t.hits["seg_off"], 100 + i))


def _handle(T: CT.BoundaryTable) -> engine.Taxonomy:
    return engine.Taxonomy(T.tax.lin_off, T.tax.lin_node, T.tax.lin_rank, T.tax.rank_names, taxon=T.taxon, custom=T.custom,
                           device=0, taxid=T.tax.taxid)


def _host_args(layout, T):
    """(pident, pident_milli, packed) of run_consensus_host / run_consensus_multi for a layout."""
    h = T.hits
    if layout in ("f64", "packed64"):
        return h["pident"], None, "wide" if layout == "packed64" else False
    return None, h["pident_milli"], layout == "packed"


def _run_host(t, T, layout, strategy):
    h = T.hits
    pid, pm, packed = _host_args(layout, T)
    return engine.run_consensus_host(t, h["seg_off"], h["bitscore"], t.engine_rows(h["tax_row"]), pid, h["align_len"], h["acc_rank"],
                                     strategy, pident_milli=pm, packed=packed)


def _device_buffers(t, T, layout):
    import torch
    h = T.hits
    cols = {"seg_off": torch.from_numpy(h["seg_off"]).cuda(), "bitscore": torch.from_numpy(h["bitscore"]).cuda(),
            "tax_row": torch.from_numpy(t.engine_rows(h["tax_row"]).view(np.int32)).cuda(),
            "align_len": torch.from_numpy(h["align_len"]).cuda(), "acc_rank": torch.from_numpy(h["acc_rank"]).cuda()}
    if layout in ("f64", "packed64"):
        cols["pident"] = torch.from_numpy(h["pident"]).cuda()
    else:
        cols["pident_milli"] = torch.from_numpy(h["pident_milli"].view(np.int32)).cuda()
    if layout in ("packed", "packed64"):
        rec = engine.pack_hits_device(t, cols, wide=layout == "packed64")
        torch.cuda.synchronize()
        return {"seg_off": cols["seg_off"], "bitscore": cols["bitscore"], layout: rec}
    return cols


def _check_device(t, T, recut, layout, strategy):
    """Three calls on one set of buffers; then the offsets rewritten in place (same pointers and counts: the kind cache
    takes it for the same table) with even short segments, three calls (the queue the device reports is short: the
    worklist kernel is no longer launched); then with long segments, three calls (the first one still without the
    worklist kernel: the stream kernel's last block works the queue off)."""
    import torch
    bufs = _device_buffers(t, T, layout)
    out = torch.empty(32 * T.n_queries, dtype=torch.uint8, device="cuda")
    for table in (T,) + recut:
        if table is not T:
            bufs["seg_off"].copy_(torch.from_numpy(table.hits["seg_off"]))
            torch.cuda.synchronize()
        exp = table.expected(strategy)
        for call in range(3):
            out.fill_(0xA5)
            engine.run_consensus_device(t, bufs, out, strategy=strategy)
            torch.cuda.synchronize()
            got = engine.records_from_tensor(out)
            try:
                H.assert_records_equal(got, exp)
            except AssertionError as e:
                raise AssertionError(("device", "table" if table is T else ("even" if table is recut[0] else "long"), "call", call,
                                      str(e)[:3000])) from None


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_layout_and_path_against_the_oracle(layout, path, monkeypatch):
    grid = layout in ("milli", "packed")
    monkeypatch.delenv("BLU_STAGE_ROWS", raising=False)
    for i in range(len(CONFIGS)):
        T = _table(i, grid)
        multi = [_handle(T) for _ in range(3)] if path == "multi" else None
        for strategy in STRATEGIES:
            exp = T.expected(strategy)
            for build in BUILDS:
                if build is None:
                    monkeypatch.delenv("BLU_STREAM_KIND", raising=False)
                else:
                    monkeypatch.setenv("BLU_STREAM_KIND", build)
                where = (T.taxon, strategy, build)
                if path == "device":
                    t = _handle(T)         # a fresh handle: its first call classifies the table
                    try:
                        _check_device(t, T, _recut(i, grid), layout, strategy)
                    except AssertionError as e:
                        raise AssertionError((where, str(e))) from None
                    t.close()
                elif path == "host":
                    t = _handle(T)
                    try:
                        H.assert_records_equal(_run_host(t, T, layout, strategy), exp)
                    except AssertionError as e:
                        raise AssertionError((where, str(e)[:3000])) from None
                    t.close()
                elif path == "chunked":
                    t = _handle(T)
                    for stage_rows in STAGE_ROWS:
                        monkeypatch.setenv("BLU_STAGE_ROWS", str(stage_rows))
                        try:
                            H.assert_records_equal(_run_host(t, T, layout, strategy), exp)
                        except AssertionError as e:
                            raise AssertionError((where, stage_rows, str(e)[:3000])) from None
                    monkeypatch.delenv("BLU_STAGE_ROWS")
                    t.close()
                else:
                    h = T.hits
                    rows = multi[0].engine_rows(h["tax_row"])
                    pid, pm, packed = _host_args(layout, T)
                    for n in (2, 3):
                        got = engine.run_consensus_multi(multi[:n], h["seg_off"], h["bitscore"], rows, pid, h["align_len"],
                                                         h["acc_rank"], strategy, pident_milli=pm, packed=packed)
                        try:
                            H.assert_records_equal(got, exp)
                        except AssertionError as e:
                            raise AssertionError((where, n, str(e)[:3000])) from None
        if multi:
            for t in multi:
                t.close()
    monkeypatch.delenv("BLU_STREAM_KIND", raising=False)

