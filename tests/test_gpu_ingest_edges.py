"""The byte-level edge cases of the BLAST table ingest (tests/ingest_edges.py) through the GPU parser (csrc/ingest_gpu.hip): the
columns of the independent reading (tests/ingest_reference.py) on the path every case predicts.  An accepted case is read by
the GPU parser itself (`last_ingest_path() == "gpu"`: a wrong tab mask or digit count that merely hands the file to the CPU
parser fails here) by each of its three builds: plain, under a hit filter that drops nothing and turns every threshold on, and
under a taxon filter that names a taxon no row hits.  tests/test_ingest_edges.py keeps the generator honest without a GPU."""
import os

import pytest

from blutils_amd import _native as N
from blutils_amd import pipeline
from tests import ingest_edges as E
from tests import test_ingest_edges as T

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def force_gpu():
    old = os.environ.get("BLU_INGEST")
    os.environ["BLU_INGEST"] = "gpu"
    yield
    if old is None:
        os.environ.pop("BLU_INGEST", None)
    else:
        os.environ["BLU_INGEST"] = old


@pytest.mark.parametrize("name", sorted(E.ACCEPTED))
def test_accepted(tmp_path, name):
    case = E.accepted_case(name)
    assert case.predict == "gpu"
    T.check_case(tmp_path, case, 0, E.expected_of(name))


@pytest.mark.parametrize("name", E.DECLINED)
def test_declined_and_refused(tmp_path, name):
    case = E.declined_cases()[name]
    code = T.check_case(tmp_path, case, 0)
    if case.predict == "refused":
        assert code == T.check_case(tmp_path, case, -1)


@pytest.mark.parametrize("column", [c for c in sorted(E.BOUNDARY) if c != "e_value"])
def test_accepted_boundary_spellings(tmp_path, column):
    blob = E.spelling_blob(column, E.accepted_spellings(column))
    t, ck = E.expected(blob, E.db_json())
    bt, tj = T.write(tmp_path, blob)
    T.check_table(bt, tj, t, ck, 0, "gpu", builds=True)


def _other(column):
    return [pytest.param(column, s, p, m, id=f"{column}-{s!r}") for s, p, m in E.other_spellings(column)]


@pytest.mark.parametrize("column,spelling,predict,message", [p for c in sorted(E.BOUNDARY) if c != "e_value" for p in _other(c)])
def test_spellings_outside_the_gpu_grammar(tmp_path, column, spelling, predict, message):
    """One spelling per table: the GPU parser declines it, and the CPU parser reads it as float() / int() do or refuses it."""
    case = E.Case(E.spelling_blob(column, [spelling]), predict, message=message, builds=False)
    code = T.check_case(tmp_path, case, 0)
    assert pipeline.last_ingest_path() == "cpu"
    if predict == "refused":
        assert code == T.check_case(tmp_path, case, -1)


def test_accepted_e_value_spellings(tmp_path):
    T.check_e_value_spellings(tmp_path, E.accepted_spellings("e_value"), 0, "gpu")


@pytest.mark.parametrize("column,spelling,predict,message", _other("e_value"))
def test_e_value_spellings_outside_the_plain_grammar(tmp_path, column, spelling, predict, message):
    if predict == "cpu":
        T.check_e_value_spellings(tmp_path, [spelling], 0, "cpu")
        return
    bt, tj = T.write(tmp_path, E.spelling_blob("e_value", [spelling]))
    codes = []
    for device in (0, -1):
        with pytest.raises(N.BluError, match=message) as e:
            pipeline.ingest_columns(bt, tj, device=device, hit_filter={"max_e_value": E.MAX_E})
        codes.append(e.value.code)
    assert codes[0] == codes[1]


@pytest.mark.parametrize("column", ["perc_identity", "bit_score"])
def test_double_rounding_mantissas_are_left_to_the_cpu_parser(tmp_path, column):
    spellings = E.DOUBLE_ROUNDING if column == "perc_identity" else E.DOUBLE_ROUNDING_BIT_SCORE
    T.check_case(tmp_path, E.Case(E.spelling_blob(column, spellings), "cpu"), 0)


@pytest.mark.parametrize("form", ["staged", "general"])
@pytest.mark.parametrize("column", ["perc_identity", "bit_score"])
def test_random_spellings(tmp_path, column, form):
    """20 000 spellings of the accepted grammar: the device's one f64 multiplication or division gives float()'s bits."""
    case = E.random_case(column, form)
    T.check_case(tmp_path, case, 0)


def test_a_name_holding_a_nul(tmp_path):
    case = E.nul_name_case()
    t, ck = E.expected(case.blob, E.db_json())
    T.check_nul_case(tmp_path, case, t, ck, 0, "gpu")


def test_the_bit_score_threshold_reads_the_score_as_written(tmp_path):
    T.check_bs_as_written(tmp_path, 0, "gpu")
