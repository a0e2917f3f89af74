"""What the CSR distance searches report about themselves, pinned: for the cases of
tools/dist_info_table.py (a chain in the narrow regime, a star whose hub overflows the narrow queue,
two batches, the empty inputs) and each of the calls (hop min / mean, weighted min / mean-fold, pair
sums / table, the weighted pair table), the deterministic g2n_dist_info / g2n_wdist_info fields equal
that tool's output at the commit before the host code around the searches was folded onto shared batch
drivers.  Recorded twice there; both runs agreed in every field, so none is left out."""
import importlib.util
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def _tool():
    spec = importlib.util.spec_from_file_location("dist_info_table", ROOT / "tools" / "dist_info_table.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


DI = _tool()

EXPECTED = {
    "chain": {
        "hop min": {"levels": 69, "launches": 3, "batches": 1},
        "hop mean": {"levels": 69, "launches": 3, "batches": 1},
        "weighted min": {"rounds": 69, "launches": 5, "batches": 1, "batch_paths": 2},
        "weighted mean-fold": {"rounds": 69, "launches": 6, "batches": 1, "batch_paths": 2},
        "pair sums": {"levels": 69, "launches": 3, "batches": 1},
        "pair table": {"levels": 69, "launches": 3, "batches": 1},
        "weighted pair table": {"rounds": 69, "launches": 5, "batches": 1, "batch_paths": 3},
    },
    "star": {
        "hop min": {"levels": 4, "launches": 16, "batches": 1},
        "hop mean": {"levels": 4, "launches": 16, "batches": 1},
        "weighted min": {"rounds": 4, "launches": 18, "batches": 1, "batch_paths": 2},
        "weighted mean-fold": {"rounds": 4, "launches": 19, "batches": 1, "batch_paths": 2},
        "pair sums": {"levels": 4, "launches": 16, "batches": 1},
        "pair table": {"levels": 4, "launches": 16, "batches": 1},
        "weighted pair table": {"rounds": 4, "launches": 18, "batches": 1, "batch_paths": 2},
    },
    "two-batches": {
        "hop min": {"levels": 69, "launches": 6, "batches": 2},
        "hop mean": {"levels": 69, "launches": 6, "batches": 2},
        "weighted min": {"rounds": 69, "launches": 10, "batches": 2, "batch_paths": 64},
        "weighted mean-fold": {"rounds": 69, "launches": 12, "batches": 2, "batch_paths": 64},
        "pair sums": {"levels": 69, "launches": 6, "batches": 2},
        "pair table": {"levels": 69, "launches": 6, "batches": 2},
        "weighted pair table": {"rounds": 69, "launches": 10, "batches": 2, "batch_paths": 64},
    },
    "empty-K0-nsrc0": {
        "hop min": {"levels": 0, "launches": 0, "batches": 0},
        "hop mean": {"levels": 0, "launches": 0, "batches": 0},
        "weighted min": {"rounds": 0, "launches": 0, "batches": 0, "batch_paths": 1},
        "weighted mean-fold": {"rounds": 0, "launches": 0, "batches": 0, "batch_paths": 1},
        "pair sums": {"levels": 0, "launches": 0, "batches": 0},
        "pair table": {"levels": 0, "launches": 0, "batches": 0},
        "weighted pair table": {"rounds": 0, "launches": 0, "batches": 0, "batch_paths": 1},
    },
    "empty-ntgt0": {
        "hop min": {"levels": 0, "launches": 0, "batches": 1},
        "hop mean": {"levels": 0, "launches": 0, "batches": 1},
        "weighted min": {"rounds": 0, "launches": 2, "batches": 1, "batch_paths": 2},
        "weighted mean-fold": {"rounds": 0, "launches": 3, "batches": 1, "batch_paths": 2},
        "pair sums": {"levels": 69, "launches": 3, "batches": 1},
        "pair table": {"levels": 69, "launches": 3, "batches": 1},
        "weighted pair table": {"rounds": 0, "launches": 0, "batches": 0, "batch_paths": 3},
    },
    "empty-no-entries": {
        "hop min": {"levels": 0, "launches": 3, "batches": 1},
        "hop mean": {"levels": 0, "launches": 3, "batches": 1},
        "weighted min": {"rounds": 0, "launches": 5, "batches": 1, "batch_paths": 2},
        "weighted mean-fold": {"rounds": 0, "launches": 6, "batches": 1, "batch_paths": 2},
        "pair sums": {"levels": 0, "launches": 3, "batches": 1},
        "pair table": {"levels": 0, "launches": 3, "batches": 1},
        "weighted pair table": {"rounds": 0, "launches": 5, "batches": 1, "batch_paths": 1},
    },
}


def test_every_case_is_pinned():
    assert sorted(EXPECTED) == sorted(DI.cases())


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_dist_info(gpu, case):
    assert DI.run_case(case) == EXPECTED[case]
