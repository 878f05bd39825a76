"""The stream kernel's builds keep what their launch bounds promise (scripts/tools/resource_gate.py): compile only, no GPU.
Skipped where there is no hipcc."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("resource_gate", os.path.join(ROOT, "scripts", "tools", "resource_gate.py"))
gate = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gate)


@pytest.fixture(scope="module")
def rows():
    hipcc = gate.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    return gate.resource_usage(hipcc)


def test_every_stream_build_fits_its_launch_bounds(rows):
    lines, failures = gate.check(rows)
    print("\n".join(lines))
    assert len(lines) == 16, lines          # 2 strategies x 4 layouts x with / without the ring
    assert not failures, failures


def test_the_packed_ring_builds(rows):
    """The builds of the headline workload: three waves per SIMD, nothing in scratch, inside the CU's LDS."""
    seen = 0
    for r in rows:
        m = gate.STREAM.search(r["name"])
        if m and m.group(2) == "2" and m.group(3) == "1":
            seen += 1
            assert int(r["Occupancy [waves/SIMD]"]) == 3, r
            assert int(r["ScratchSize [bytes/lane]"]) == 0, r
            assert int(r["LDS Size [bytes/block]"]) <= 163840, r
    assert seen == 2


def test_the_gate_catches_a_build_that_misses():
    name = "_ZN3blu27blu_consensus_stream_kernelILi1ELi2ELb1EEEvNS_7HitsDevE"
    good = {"name": name, "VGPRs": "162", "ScratchSize [bytes/lane]": "0", "LDS Size [bytes/block]": "163400", "Occupancy [waves/SIMD]": "3"}
    assert gate.check([good])[1] == []
    for key, value in (("LDS Size [bytes/block]", "165120"), ("Occupancy [waves/SIMD]", "2"), ("ScratchSize [bytes/lane]", "8")):
        assert len(gate.check([dict(good, **{key: value})])[1]) == 1, key
    noring = dict(good, name=name.replace("Lb1E", "Lb0E"), **{"Occupancy [waves/SIMD]": "4", "ScratchSize [bytes/lane]": "12"})
    assert gate.check([noring])[1] == []
