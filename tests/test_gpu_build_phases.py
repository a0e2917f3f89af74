"""The path every build takes through the driver (run_build and the stages it calls), pinned: the fixed matrix
of tiny builds of tools/build_phases.py — every plain golden input x test_gpu_diff.MODES x float64 / int8 on
each front-end and dictionary route, the partition's declining cases (the no-group retry), the entry points
that set a context flag around the build, and the decimal range builds of the sharded protocol — must report
the status, n_nodes, nnz, format and ordered phase names recorded in tests/golden/expected/build_phases.json,
which is that tool's output at the commit before the driver was split into stages."""
import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def _tool():
    spec = importlib.util.spec_from_file_location("build_phases", ROOT / "tools" / "build_phases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BP = _tool()


@pytest.fixture(scope="module")
def expected():
    return json.loads((ROOT / "tests" / "golden" / "expected" / "build_phases.json").read_text())


def test_fixture_covers_every_group(expected):
    assert sorted(expected["cases"]) == sorted(BP.GROUPS)
    inputs = sorted(p.name for p in BP.golden_inputs())
    for route in BP.ROUTES:  # no case left out of any route
        assert sorted(expected["cases"][f"route-{route}"]) == inputs, route


@pytest.mark.parametrize("group", BP.GROUPS)
def test_build_phases(gpu, expected, group):
    want = BP.unpack(expected, group)
    got = BP.run_group(group)
    assert sorted(got) == sorted(want), group
    bad = [(case, k, got[case][k], want[case][k]) for case in want for k in range(len(want[case]))
           if len(got[case]) != len(want[case]) or got[case][k] != want[case][k]]
    assert not bad, (group, len(bad), bad[:3])
