"""GPU: ``graph_components`` and ``split_components`` (g2n_csr_components_host /
g2n_csr_split_components_host -> the kernels of g2n_stats.hip and g2n_components.hip) on hand-made
CSR structures, against the checker of tests/components_util.py (scipy's labels, numpy's stable
argsort, ``A[idx][:, idx]``, a numpy restatement of "stored order kept").  All comparisons are exact.
Each shape runs with int32 and with int64 indptr / indices, and twice (the union-find's races must
not change the answer).  The shapes are the smallest that reach each way the kernels can go wrong:
sizes around the block, isolated nodes (k = n), chains in three id orders, a star (one row of many
blocks of entries, every hook on one address), 255 / 256 / 257 / 65 537 components (1, 2 and 3
passes of the sort), interleaved components (perm is no identity), rows of 0, 1, 64 and 65 entries
(the one-thread / one-block boundary of the copy), unsorted rows and duplicates, all five dtypes."""
import numpy as np
import pytest
import scipy.sparse as sp

import components_util as cu

pytestmark = pytest.mark.gpu

CHAIN = 100_003
STAR = 100_000


def split_arrays(S):
    return [S.labels, S.perm, S.offsets, S.sizes, S.indptr, S.indices, S.data]


def run_all(indptr, indices, n, components=None, dtype="float64"):
    """Labels and the split of this structure, both index widths, each twice; returns the last split."""
    from gfa2network_amd import graph_components, split_components

    k, lab = cu.want_labels(indptr, indices, n)
    if components is not None:
        assert k == components
    S = None
    for idt in (np.int32, np.int64):
        A = cu.matrix(indptr, indices, n, idt, cu.telling_values(len(indices), dtype))
        for _ in range(2):
            gk, glab = graph_components(A)
            assert type(gk) is int and gk == k, idt
            assert cu.same_bits(glab, lab), idt
        S = split_components(A)
        assert cu.check_split(S, A) == k
        again = split_components(A)
        assert all(cu.same_bits(np.asarray(a), np.asarray(b)) for a, b in zip(split_arrays(S), split_arrays(again)))
    return S


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_random_graphs(gpu, n):
    rng = np.random.default_rng(n)
    m = n // 2 + 1  # sparse enough for several components
    pairs = np.unique(np.stack([rng.integers(0, n, m), rng.integers(0, n, m)], axis=1), axis=0)
    run_all(*cu.csr_of(pairs[:, 0], pairs[:, 1], n), n)


def test_one_node_without_entries(gpu):
    run_all(np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.int64), 1, components=1)


def test_isolated_nodes(gpu):
    S = run_all(np.zeros(1001, dtype=np.int64), np.zeros(0, dtype=np.int64), 1000, components=1000)
    A0, nodes = S.component(999)
    assert A0.shape == (1, 1) and A0.nnz == 0 and nodes.tolist() == [999]


@pytest.fixture(scope="module")
def chain_orders():
    k = np.arange(CHAIN, dtype=np.int64)
    return {"in_order": k, "reversed": k[::-1].copy(), "permuted": np.random.default_rng(7).permutation(CHAIN)}


@pytest.mark.parametrize("order", ["in_order", "reversed", "permuted"])
def test_chain(gpu, chain_orders, order):
    ids = chain_orders[order]  # chain position k has node id ids[k]; each link stored one way only
    run_all(*cu.csr_of(ids[:-1], ids[1:], CHAIN), CHAIN, components=1)


@pytest.mark.parametrize("hub", [0, STAR, 12345])
def test_star_as_the_hubs_row(gpu, hub):
    """One row of 100 000 entries: the block-per-row copy over many blocks of entries."""
    n = STAR + 1
    leaves = np.delete(np.arange(n, dtype=np.int64), hub)
    run_all(*cu.csr_of(np.full(STAR, hub), leaves, n), n, components=1)


def test_hub_row_longer_than_one_pass_of_the_grid(gpu):
    """A row of more entries than the grid's threads (1024 blocks of 256): every thread of the grid-wide
    copy takes a second stripe; unsorted, so a misplaced stripe shows."""
    n = 1024 * 256 + 1500
    leaves = np.random.default_rng(2).permutation(np.arange(1, n, dtype=np.int64))
    run_all(*cu.csr_of(np.zeros(n - 1, dtype=np.int64), leaves, n), n, components=1, dtype="int32")


def test_star_as_rows_pointing_at_the_hub(gpu):
    n = STAR + 1
    leaves = np.arange(n - 1, dtype=np.int64)
    run_all(*cu.csr_of(leaves, np.full(STAR, n - 1), n), n, components=1)


def test_self_loops_reciprocal_and_duplicate_entries(gpu):
    rows = np.array([0, 1, 0, 0, 2, 3, 3, 5, 5, 4, 6, 6])
    cols = np.array([1, 0, 1, 1, 2, 4, 4, 5, 5, 3, 6, 6])
    ip, ix = cu.csr_of(rows, cols, 8)
    assert not cu.is_canonical(ip, ix)
    run_all(ip, ix, 8, components=6)
    k = np.arange(1000, dtype=np.int64)
    run_all(*cu.csr_of(k, k, 1000), 1000, components=1000)


def test_other_formats_are_converted(gpu):
    from gfa2network_amd import graph_components, split_components

    rows = np.array([0, 1, 0, 0, 2, 3, 3, 5, 5, 4])
    cols = np.array([1, 0, 1, 1, 2, 4, 4, 5, 5, 3])
    C = sp.coo_matrix((np.arange(1.0, 11.0), (rows, cols)), shape=(7, 7))
    R = C.tocsr()
    k, lab = cu.want_labels(R.indptr, R.indices, 7)
    assert k == 5
    for A in (C, R, C.tocsc(), C.todok(), C.tolil()):
        gk, glab = graph_components(A)
        assert gk == k and cu.same_bits(glab, lab)
        T = A.tocsr()
        assert cu.check_split(split_components(A), T) == k


def test_directed_structures_stored_one_way(gpu):
    """A tree whose links are stored child -> parent only, one whose links are stored parent -> child
    only, and a cycle stored in descending direction: direction never matters."""
    n = 3000
    rng = np.random.default_rng(11)
    child = np.arange(1, 1000, dtype=np.int64)
    parent = (rng.random(999) * child).astype(np.int64)  # a parent below the child
    rows = np.concatenate([child, 1000 + parent, 2000 + np.arange(1, 1000), [2000]])
    cols = np.concatenate([parent, 1000 + child, 2000 + np.arange(0, 999), [2999]])
    run_all(*cu.csr_of(rows, cols, n), n, components=3)


@pytest.mark.parametrize("k", [255, 256, 257, 65_537])
def test_sort_passes_and_interleaved_components(gpu, k):
    """k components {i, i + k, i + 2k}: their nodes interleave, so perm is no identity; 255 and 256
    labels sort in one pass, 257 in two, 65 537 in three."""
    n = 3 * k
    i = np.arange(k, dtype=np.int64)
    rows = np.concatenate([i + 2 * k, i + k])  # stored from the higher index down, one way only
    cols = np.concatenate([i, i + 2 * k])
    S = run_all(*cu.csr_of(rows, cols, n), n, components=k)
    assert not np.array_equal(S.perm, np.arange(n))
    assert S.perm[:6].tolist() == [0, k, 2 * k, 1, k + 1, 2 * k + 1]


def test_halves_linked(gpu):
    """i linked to i + n / 2, n / 2 components of two."""
    n = 5000
    i = np.arange(n // 2, dtype=np.int64)
    run_all(*cu.csr_of(i, i + n // 2, n), n, components=n // 2)


@pytest.mark.parametrize("dtype", cu.DTYPES)
def test_row_lengths_around_the_copy_boundary(gpu, dtype):
    """Rows of 0, 1, 63, 64 (the last one-thread row), 65 (the first queued one), 256, 257 and 600
    entries (more than one block of entries), 4096 (the last one-block row) and 4097 (the first the
    whole grid copies), in two components, one row unsorted with duplicates — with values that tell a
    misplaced item from a right one, in every dtype."""
    from gfa2network_amd import _native

    B, H = _native.SPLIT_SHORT_ROW, _native.SPLIT_HUGE_ROW
    assert (B, H) == (64, 4096)
    n = 10_400
    rng = np.random.default_rng(5)
    rows, cols = [], []
    for r, ln in ((2, 1), (3, B - 1), (5, B), (7, B + 1), (11, 256), (13, 257), (17, 600), (19, H), (29, H + 1)):
        c = rng.choice(5200, ln, replace=False) * 2  # even nodes: the first component
        rows.append(np.full(ln, r * 2))
        cols.append(c)
    for r, ln in ((1, B), (9, B + 1), (21, 1), (23, 2 * B + 3), (25, H + 1), (27, H)):
        c = rng.choice(5200, ln, replace=False) * 2 + 1  # odd nodes: the second
        rows.append(np.full(ln, r * 2 + 1))
        cols.append(c)
    rows.append(np.full(6, 100))
    cols.append(np.array([44, 8, 44, 2, 1000, 8]))  # unsorted, duplicates
    ip, ix = cu.csr_of(np.concatenate(rows), np.concatenate(cols), n)
    assert not cu.is_canonical(ip, ix)
    lens = np.diff(ip)
    assert {0, 1, B - 1, B, B + 1, 256, 257, 600, H, H + 1} <= set(lens.tolist())
    S = run_all(ip, ix, n, dtype=dtype)
    assert S.n_components > 2 and S.data.dtype == np.dtype(dtype)
    # and the canonical form of the same matrix against scipy's own slices
    A = cu.matrix(ip, ix, n, np.int32, cu.telling_values(len(ix), "float64"))
    A.sum_duplicates()
    A.sort_indices()
    run_all(A.indptr.astype(np.int64), A.indices.astype(np.int64), n, dtype=dtype)


def test_largest_takes_the_lowest_label_on_ties(gpu):
    ip, ix = cu.csr_of([0, 2, 4, 7, 8], [1, 3, 5, 8, 9], 10)  # {0,1} {2,3} {4,5} {6} {7,8,9}
    S = run_all(ip, ix, 10, components=5)
    L, nodes = S.largest()
    assert nodes.tolist() == [7, 8, 9] and L.nnz == 2
    ip, ix = cu.csr_of([0, 2, 4], [1, 3, 5], 7)
    S = run_all(ip, ix, 7, components=4)
    assert S.sizes.tolist() == [2, 2, 2, 1]
    L, nodes = S.largest()
    assert nodes.tolist() == [0, 1] and L.toarray().tolist() == [[0.0, cu.telling_values(3, "float64")[0]], [0.0, 0.0]]


def test_out_of_range_structure_is_refused(gpu):
    """An index one past the last node, a negative one, a decreasing indptr, an indptr past the
    entries: ValueError (G2N_E_ARG), never addressed — and the context still answers."""
    from gfa2network_amd import _native

    one = np.ones(2, dtype=np.float32)
    for idt in (np.int32, np.int64):
        ip = np.array([0, 1, 2], dtype=idt)
        bad = [(ip, np.array([1, 2], dtype=idt)), (ip, np.array([1, -1], dtype=idt)),
               (np.array([0, 3, 2], dtype=idt), np.array([1, 0], dtype=idt)),
               (np.array([0, 2, 1], dtype=idt), np.array([1, 0], dtype=idt)),
               (np.array([-1, 1, 2], dtype=idt), np.array([1, 0], dtype=idt))]
        for bip, bix in bad:
            with pytest.raises(ValueError, match="out of range"):
                _native.csr_components_host(bip, bix, 2)
            with pytest.raises(ValueError, match="out of range"):
                _native.csr_split_components_host(bip, bix, one, 2)
            with pytest.raises(ValueError, match="out of range"):
                _native.csr_split_components_host(bip, bix, None, 2)
        labels, info = _native.csr_components_host(ip, np.array([1, 0], dtype=idt), 2)
        assert labels.tolist() == [0, 0] and info["n_components"] == 1
        out = _native.csr_split_components_host(ip, np.array([1, 0], dtype=idt), None, 2)
        assert out[0].tolist() == [0, 0] and out[2].tolist() == [0, 2] and out[4].tolist() == [1, 0] and out[5] is None
    with pytest.raises(ValueError):
        _native.csr_split_components_host(np.array([0, 1, 2], dtype=np.int32), np.array([1, 0], dtype=np.int32),
                                          np.ones(2, dtype=np.int16), 2)
