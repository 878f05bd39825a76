"""The e-value threshold cases (tests/e_value_edges.py) through the GPU parser (csrc/ingest_gpu.hip: e_value_verdict under
device_filter's constants, list_undecided, apply_decisions).  The expected value of every line is `float(field) <= E`; every
table is also held to the independent reading of filter_text's copy, to the counts and to the parser §14.3 names.

What the value checks alone cannot see is who decided.  Each threshold's cases come as two tables, split by the restatement of
the ladder in tests/e_value_edges.py: a *decided* table must leave no `e-values decided on the host` line in the trace — a
kernel that asked the host about a field it can decide fails here — and an *asked* table must leave one.
tests/test_e_value_edges.py keeps the generator and the restatement honest without a GPU."""
import contextlib
import os

import pytest

from tests import e_value_edges as V
from tests import ingest_edges as IE
from tests import test_e_value_edges as T

pytestmark = pytest.mark.gpu

HOST_LINE = "e-values decided on the host"
PARSED_LINE = "parse (filtered)"
NOTHING_KEPT = "GPU parser declined (no rows kept by the filters)"


@pytest.fixture(autouse=True)
def force_gpu():
    old = os.environ.get("BLU_INGEST")
    os.environ["BLU_INGEST"] = "gpu"
    yield
    if old is None:
        os.environ.pop("BLU_INGEST", None)
    else:
        os.environ["BLU_INGEST"] = old


@contextlib.contextmanager
def tracing():
    old = os.environ.get("BLU_INGEST_TRACE")
    os.environ["BLU_INGEST_TRACE"] = "1"
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("BLU_INGEST_TRACE", None)
        else:
            os.environ["BLU_INGEST_TRACE"] = old


def run(tmp_path, capfd, blob, texts, flt, asked, passes=None, **kw):
    """One table on the device with the trace on: the expected table on the expected path (T.check_table), the filtered parse
    ran, and the host was asked exactly when `asked` says so.  A table that keeps nothing ends on the host parser, for that
    reason and no other."""
    with tracing():
        capfd.readouterr()
        got = T.check_table(tmp_path, blob, texts, flt, 0, passes=passes, **kw)
        err = capfd.readouterr().err
    assert PARSED_LINE in err, err
    assert (HOST_LINE in err) == asked, err
    assert (NOTHING_KEPT in err) == (got["n_kept"] == 0) and ("declined" in err) == (got["n_kept"] == 0), err
    return got


@pytest.mark.parametrize("family", list(V.FAMILIES))
def test_decided_tables_cause_no_host_round_trip(tmp_path, capfd, family):
    for name, E in V.FAMILIES[family]:
        texts = T.texts_of(V.split(name)[0])
        try:
            run(tmp_path, capfd, V.table(texts), texts, {"max_e_value": E}, asked=False)
        except AssertionError as e:
            raise AssertionError(f"threshold {name}: {_table_of(texts, E)}") from e


@pytest.mark.parametrize("family", list(V.FAMILIES))
def test_asked_tables_are_decided_on_the_host(tmp_path, capfd, family):
    for name, E in V.FAMILIES[family]:
        texts = T.texts_of(V.split(name)[1])
        try:
            run(tmp_path, capfd, V.table(texts), texts, {"max_e_value": E}, asked=True)
        except AssertionError as e:
            raise AssertionError(f"threshold {name}: {_table_of(texts, E)}") from e


def _table_of(texts, E):
    """For a failure's message: which table it was, for reading e_value_verdict against its fields."""
    return f"E = {E!r}, {len(texts)} fields, the first: {texts[:6]}"


@pytest.mark.parametrize("family", list(V.FAMILIES))
def test_general_form_and_taxon_filter_build(tmp_path, capfd, family):
    """One threshold per family through the parse kernel's general form (no parse block fits the stage) and through the third
    build of the parse kernels, under a taxon filter that names a taxon no line hits."""
    name = V.ALSO_GENERAL[family]
    E = V.THRESHOLDS[name]
    for texts, asked in zip(map(T.texts_of, V.split(name)), (False, True)):
        blob = V.table(texts, pad=V.general_pad(len(texts)))
        assert IE.block_forms(blob)[0][1] == "general"
        run(tmp_path, capfd, blob, texts, {"max_e_value": E}, asked)
        got = run(tmp_path, capfd, V.table(texts), texts, {"max_e_value": E}, asked, taxon_filter=IE.TAXON_FILTER_UNHIT)
        assert got["taxon_filter"]["n_excluded"] == 0 and got["taxon_filter"]["excluded_by"] == [0]
        got = run(tmp_path, capfd, blob, texts, {"max_e_value": E}, asked, taxon_filter=IE.TAXON_FILTER_UNHIT)
        assert got["taxon_filter"]["n_excluded"] == 0


@pytest.mark.parametrize("name", list(V.LIST_CASES))
def test_the_undecided_list(tmp_path, capfd, name):
    """list_undecided and apply_decisions at their 256-thread grid edges: 1 (first line, last line), 255, 256, 257 and all 600
    lines undecided, with a mixed outcome and with every one dropped; LF, CRLF and an open last line."""
    texts = V.list_case(name)
    flt = {"max_e_value": V.LIST_E}
    for layout, (eol, open_tail) in V.LIST_LAYOUTS.items():
        run(tmp_path, capfd, V.table(texts, eol=eol, open_tail=open_tail), texts, flt, asked=True)
    if name == V.LIST_GENERAL:
        blob = V.table(texts, pad=V.LIST_PAD)
        assert {f for _, f in IE.block_forms(blob)} == {"general"}
        run(tmp_path, capfd, blob, texts, flt, asked=True)


def test_lines_that_fail_another_threshold_are_never_asked_about(tmp_path, capfd):
    """Every line spelled like the e-value threshold fails min_perc_identity: no round trip.  Without that threshold the same
    table causes one."""
    texts, pid, passes = V.failing_pid_case()
    blob = V.table(texts, pid=pid)
    run(tmp_path, capfd, blob, texts, {"min_perc_identity": V.PID_MIN, "max_e_value": V.LIST_E}, asked=False, passes=passes)
    run(tmp_path, capfd, blob, texts, {"max_e_value": V.LIST_E}, asked=True)
