"""GPU: ``graph_stats`` (g2n_csr_stats_host -> the kernels of g2n_stats.hip) on hand-made CSR
structures, against scipy's connected_components and numpy degree / edge counts.  Each shape runs
with int32 and with int64 indptr / indices, directed and undirected, and twice (the union-find's
races must not change the answer).  The shapes are the smallest that reach each way the kernels can
go wrong: sizes around the block (64, 65, 257), empty rows, a row longer than a block (the queued
long-row walk), every hook and column count on one address, chains (the diameter case) in three id
orders, many tiny components, self-loops, reciprocal and duplicate entries."""
import numpy as np
import pytest
import scipy.sparse as sp

from stats_util import checker, csr_of

pytestmark = pytest.mark.gpu

CHAIN = 100_003
STAR = 100_000


def matrix(indptr, indices, n, idt):
    A = sp.csr_matrix((np.ones(len(indices), dtype=np.float64), indices.astype(np.int32), indptr.astype(np.int32)),
                      shape=(n, n))
    A.indptr, A.indices = indptr.astype(idt), indices.astype(idt)  # (the constructor narrows int64)
    assert A.indptr.dtype == idt and A.indices.dtype == idt
    return A


def run_all(indptr, indices, n, components=None):
    from gfa2network_amd import graph_stats

    for directed in (True, False):
        want = checker(indptr, indices, n, directed)
        if components is not None:
            assert want["components"] == components
        for idt in (np.int32, np.int64):
            A = matrix(indptr, indices, n, idt)
            first = graph_stats(A, directed=directed)
            assert first == want, (directed, idt)
            assert list(first) == ["nodes", "edges", "components", "max_degree", "density"]
            assert all(type(first[k]) is int for k in ("nodes", "edges", "components", "max_degree"))
            assert graph_stats(A, directed=directed) == first, (directed, idt)


@pytest.mark.parametrize("n", [0, 1, 64, 65, 257])
def test_small_sizes(gpu, n):
    rng = np.random.default_rng(n)
    m = 2 * n
    rows, cols = rng.integers(0, max(n, 1), m), rng.integers(0, max(n, 1), m)
    if n == 0:
        rows = cols = np.zeros(0, dtype=np.int64)
    pairs = np.unique(np.stack([rows, cols], axis=1), axis=0) if n else np.zeros((0, 2), dtype=np.int64)
    run_all(*csr_of(pairs[:, 0], pairs[:, 1], n), n)


def test_one_node_with_a_self_loop(gpu):
    run_all(*csr_of([0], [0], 1), 1, components=1)


@pytest.mark.parametrize("n", [1, 65, 1000])
def test_isolated_nodes(gpu, n):
    run_all(np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), n, components=n)


@pytest.fixture(scope="module")
def chain_orders():
    k = np.arange(CHAIN, dtype=np.int64)
    return {"in_order": k, "reversed": k[::-1].copy(), "permuted": np.random.default_rng(7).permutation(CHAIN)}


@pytest.mark.parametrize("order", ["in_order", "reversed", "permuted"])
def test_chain(gpu, chain_orders, order):
    ids = chain_orders[order]  # chain position k has node id ids[k]
    run_all(*csr_of(ids[:-1], ids[1:], CHAIN), CHAIN, components=1)


def test_two_chains_joined_by_the_last_entry(gpu):
    n = 2 * CHAIN
    k = np.arange(CHAIN - 1, dtype=np.int64)
    rows = np.concatenate([k, CHAIN + k])
    cols = np.concatenate([k + 1, CHAIN + k + 1])
    ip, ix = csr_of(rows, cols, n)
    run_all(ip, ix, n, components=2)
    # one more entry, stored last (the last row's): the far end of the second chain to the first's start
    ip2, ix2 = csr_of(np.concatenate([rows, [n - 1]]), np.concatenate([cols, [0]]), n)
    assert ix2[-1] == 0 and ip2[-1] == len(ix) + 1
    run_all(ip2, ix2, n, components=1)


def test_star_as_the_hubs_row(gpu):
    n = STAR + 1
    for hub in (0, n - 1, 12345):
        leaves = np.delete(np.arange(n, dtype=np.int64), hub)
        run_all(*csr_of(np.full(STAR, hub), leaves, n), n, components=1)


def test_star_as_rows_pointing_at_the_hub(gpu):
    n = STAR + 1
    for hub in (0, n - 1):
        leaves = np.delete(np.arange(n, dtype=np.int64), hub)
        run_all(*csr_of(leaves, np.full(STAR, hub), n), n, components=1)


def test_disjoint_triangles(gpu):
    t = 3 * np.arange(10_000, dtype=np.int64)
    rows = np.concatenate([t, t + 1, t + 2])
    cols = np.concatenate([t + 1, t + 2, t])
    run_all(*csr_of(rows, cols, 30_000), 30_000, components=10_000)


def test_self_loops_only(gpu):
    k = np.arange(1000, dtype=np.int64)
    run_all(*csr_of(k, k, 1000), 1000, components=1000)


def test_long_and_short_rows_mixed(gpu):
    """Rows of 64 and 65 entries side by side (the walk's one-thread / queued threshold), plus empties."""
    n = 300
    rows = np.concatenate([np.full(64, 3), np.full(65, 4), np.full(299, 200), [299]])
    cols = np.concatenate([np.arange(64) + 10, np.arange(65) + 100, np.delete(np.arange(300), 200), [299]])
    run_all(*csr_of(rows, cols, n), n)


def test_reciprocal_and_duplicate_entries(gpu):
    """A COO with reciprocal and repeated entries: graph_stats converts it, duplicates summed."""
    from gfa2network_amd import graph_stats

    rows = np.array([0, 1, 0, 0, 2, 3, 3, 5, 5, 4])
    cols = np.array([1, 0, 1, 1, 2, 4, 4, 5, 5, 3])
    C = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(7, 7))
    S = C.tocsr()
    S.sum_duplicates()
    assert S.nnz == 6
    for directed in (True, False):
        want = checker(S.indptr.astype(np.int64), S.indices.astype(np.int64), 7, directed)
        assert want["components"] == 5
        for A in (C, S, C.tocsc(), C.todok()):
            assert graph_stats(A, directed=directed) == want
    run_all(S.indptr.astype(np.int64), S.indices.astype(np.int64), 7)


def test_out_of_range_structure_is_refused(gpu):
    """An index one past the last node, an indptr past the entries: ValueError, never addressed."""
    from gfa2network_amd import _native

    ip = np.array([0, 1, 2], dtype=np.int32)
    with pytest.raises(ValueError):
        _native.csr_stats_host(ip, np.array([1, 2], dtype=np.int32), 2, True)
    with pytest.raises(ValueError):
        _native.csr_stats_host(ip, np.array([1, -1], dtype=np.int32), 2, False)
    with pytest.raises(ValueError):
        _native.csr_stats_host(np.array([0, 3, 2], dtype=np.int32), np.array([1, 0], dtype=np.int32), 2, True)
    # and the context still answers
    assert _native.csr_stats_host(ip, np.array([1, 0], dtype=np.int32), 2, True)["n_components"] == 1
