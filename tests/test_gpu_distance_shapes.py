"""GPU: ``path_distances`` (g2n_csr_path_distances_host -> the kernels of g2n_dist.hip) on hand-made
CSR structures, against scipy's unweighted Dijkstra (dist_util).  Each shape runs with int32 and with
int64 indptr / indices, with both methods, and twice (the atomics' races must not change a value).
The shapes are the smallest that reach each way the kernels can go wrong: path counts around the
mask word and the batch (63, 64, 65, 129), sizes around the block, empty rows, chains (a level per
node: the narrow regime), a star (a long row, a queue overflow, narrow -> wide), a grid (the
frontier passes the narrow cap and comes back), one node in 65 paths, a step repeated 1000 times,
rows of 64 and 65 entries."""
import numpy as np
import pytest
import scipy.sparse as sp

from dist_util import mean_matrix, min_matrix, same, tables
from stats_util import csr_of

pytestmark = pytest.mark.gpu

CHAIN = 100_003
STAR = 100_000


def matrix(indptr, indices, n, idt):
    A = sp.csr_matrix((np.ones(len(indices), dtype=np.float64), indices.astype(np.int32), indptr.astype(np.int32)),
                      shape=(n, n))
    A.indptr, A.indices = indptr.astype(idt), indices.astype(idt)  # (the constructor narrows int64)
    assert A.indptr.dtype == idt and A.indices.dtype == idt
    return A


def run_all(indptr, indices, n, paths):
    """Both methods x both index widths x two runs against the checker; the int32 runs' info."""
    from gfa2network_amd import path_distances

    D, S, C = tables(indptr, indices, n, paths)
    want = {"min": min_matrix(D), "mean": mean_matrix(S, C)}
    infos = {}
    for method in ("min", "mean"):
        for idt in (np.int32, np.int64):
            A = matrix(indptr, indices, n, idt)
            first, info = path_distances(A, paths, method=method, return_info=True)
            assert first.dtype == np.float64 and first.shape == (len(paths), len(paths))
            assert same(first, want[method]), (method, idt)
            assert same(path_distances(A, paths, method=method), first), (method, idt)
            assert info["batches"] == (len(paths) + 63) // 64
            infos[method] = info
    return D, infos


def undirected(rows, cols):
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    return np.concatenate([rows, cols]), np.concatenate([cols, rows])


@pytest.mark.parametrize("K", [0, 1, 2, 63, 64, 65, 129])
def test_path_counts(gpu, K):
    """The mask-word and batch boundaries on a 257-node random graph: single-node paths, ragged
    ones with repeats, and one path that covers every node."""
    n = 257
    rng = np.random.default_rng(K)
    pairs = np.unique(np.stack([rng.integers(0, n, 400), rng.integers(0, n, 400)], axis=1), axis=0)
    paths = [[int(rng.integers(0, n))] if k % 3 == 0 else rng.integers(0, n, int(rng.integers(2, 9))).tolist()
             for k in range(K)]
    if K > 1:
        paths[K // 2] = list(range(n))
    run_all(*csr_of(pairs[:, 0], pairs[:, 1], n), n, paths)


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_small_sizes(gpu, n):
    rng = np.random.default_rng(n)
    pairs = np.unique(np.stack([rng.integers(0, n, 2 * n), rng.integers(0, n, 2 * n)], axis=1), axis=0)
    paths = [[0], [n - 1], rng.integers(0, n, 5).tolist(), []]
    run_all(*csr_of(pairs[:, 0], pairs[:, 1], n), n, paths)


def test_empty_rows_and_no_entries(gpu):
    n = 300
    D, _ = run_all(*csr_of([5, 5, 200], [6, 299, 5], n), n, [[200], [299, 6], [0], [5]])
    assert D[0, 1] == 2 and D[1, 0] == 0xFFFFFFFF
    paths = [[0, 1], [2], [299]]
    D, infos = run_all(np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), n, paths)
    assert (D == 0xFFFFFFFF).sum() == 6 and infos["min"]["levels"] == 0


@pytest.fixture(scope="module")
def chain_orders():
    k = np.arange(CHAIN, dtype=np.int64)
    return {"in_order": k, "reversed": k[::-1].copy(), "permuted": np.random.default_rng(7).permutation(CHAIN)}


@pytest.mark.parametrize("order", ["in_order", "reversed", "permuted"])
def test_chain_depth(gpu, chain_orders, order):
    """A level per node.  launches * 16 < levels holds only when the narrow regime carried the
    search: a launch per level (or per few levels) cannot meet it."""
    ids = chain_orders[order]  # chain position k has node id ids[k]
    rows, cols = undirected(ids[:-1], ids[1:])
    paths = [[int(ids[0])], [int(ids[CHAIN // 2])], [int(ids[-1])]]
    D, infos = run_all(*csr_of(rows, cols, CHAIN), CHAIN, paths)
    assert D[0, 2] == CHAIN - 1 and D[1, 0] == CHAIN // 2
    for info in infos.values():
        assert info["levels"] == CHAIN - 1 == 100_002
        assert info["launches"] * 16 < info["levels"]


def test_chain_direction(gpu, chain_orders):
    ids = chain_orders["permuted"]
    paths = [[int(ids[0])], [int(ids[CHAIN // 2])], [int(ids[-1])]]
    D, _ = run_all(*csr_of(ids[:-1], ids[1:], CHAIN), CHAIN, paths)
    assert D[0, 2] == CHAIN - 1 and list(D[2, :2]) == [0xFFFFFFFF] * 2 and D[1, 0] == 0xFFFFFFFF


def test_star_as_the_hubs_row(gpu):
    """The hub's row is walked by a block; the frontier jumps from 1 node to 100 000 (the narrow
    queue overflows, the wide pass rebuilds it)."""
    n = STAR + 1
    for hub in (0, 12345):
        leaves = np.delete(np.arange(n, dtype=np.int64), hub)
        paths = [[hub], [int(leaves[0]), int(leaves[77]), int(leaves[-1])]]
        D, _ = run_all(*csr_of(np.full(STAR, hub), leaves, n), n, paths)
        assert D[0, 1] == 1 and D[1, 0] == 0xFFFFFFFF


def test_star_as_rows_pointing_at_the_hub(gpu):
    n = STAR + 1
    hub = n - 1
    leaves = np.arange(STAR, dtype=np.int64)
    paths = [[hub], [3, 50_000, STAR - 1]]
    D, _ = run_all(*csr_of(leaves, np.full(STAR, hub), n), n, paths)
    assert D[1, 0] == 1 and D[0, 1] == 0xFFFFFFFF
    # both ways: leaf -> hub -> every leaf
    rows, cols = undirected(leaves, np.full(STAR, hub))
    D, infos = run_all(*csr_of(rows, cols, n), n, paths + [[7]])
    assert D[2, 1] == 2 and infos["min"]["levels"] == 2


def test_grid(gpu):
    """300 x 300, undirected, paths at a corner and at the centre (an anti-diagonal of at most 300
    nodes and a diamond of at most 600: narrow) and one of four whole grid rows: its 1200 sources fit
    one workgroup's queue, level 1's eight rows (2400 nodes) do not, and after 40 levels the rows
    have met and the frontier is narrow again until the corner's search ends at level 598."""
    w = 300
    idx = np.arange(w * w, dtype=np.int64).reshape(w, w)
    rows, cols = undirected(np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()]),
                            np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()]))
    bars = idx[[30, 110, 190, 270], :].ravel().tolist()
    paths = [[0], [int(idx[w // 2, w // 2])], bars]
    D, infos = run_all(*csr_of(rows, cols, w * w), w * w, paths)
    assert D[0, 1] == w and D[1, 0] == w and D[2, 1] == 40 and D[0, 2] == 30
    for info in infos.values():
        assert info["levels"] == 2 * (w - 1)
        assert info["launches"] < info["levels"] // 2  # (some 40 wide levels of 3 launches, the rest narrow)


def test_shared_hub(gpu):
    """65 paths that all hold node 0 plus a private node: every accumulation of the hub lands on
    one node's membership entries, across two batches."""
    n = 200
    rows, cols = undirected(np.zeros(n - 1, dtype=np.int64), np.arange(1, n))
    paths = [[0, k + 1] for k in range(65)]
    D, _ = run_all(*csr_of(rows, cols, n), n, paths)
    assert (D == 0).all()
    paths = [[k + 1] for k in range(65)] + [[0]]
    D, _ = run_all(*csr_of(rows, cols, n), n, paths)
    assert D[0, 1] == 2 and D[0, 65] == 1


def test_duplicate_steps(gpu):
    """The same step 1000 times counts 1000 times in the mean."""
    n = 10
    k = np.arange(n - 1)
    rows, cols = undirected(k, k + 1)
    paths = [[0], [3] * 1000 + [5], [9, 9]]
    from gfa2network_amd import _native

    ip, ix = csr_of(rows, cols, n)
    run_all(ip, ix, n, paths)
    ptr = np.cumsum([0] + [len(p) for p in paths])
    (S, C), _ = _native.csr_path_distances_host(ip, ix, n, ptr, np.concatenate(paths), True)
    assert C[0, 1] == 1001 and S[0, 1] == 3005 and C[1, 0] == 1 and S[1, 0] == 3 and C[2, 1] == 1001


def test_self_loops_and_other_formats(gpu):
    """Self-loops; reciprocal and repeated entries through COO / CSC / DOK inputs (converted,
    duplicates summed)."""
    from gfa2network_amd import path_distances

    k = np.arange(50, dtype=np.int64)
    run_all(*csr_of(k, k, 50), 50, [[0], [1, 2], [49]])
    rows = np.array([0, 1, 0, 0, 2, 3, 3, 5, 5, 4])
    cols = np.array([1, 0, 1, 1, 2, 4, 4, 5, 5, 3])
    Cm = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(7, 7))
    Sm = Cm.tocsr()
    Sm.sum_duplicates()
    paths = [[0], [1], [3, 3], [4], [6]]
    D, S, C = tables(Sm.indptr, Sm.indices, 7, paths)
    for A in (Cm, Sm, Cm.tocsc(), Cm.todok()):
        assert same(path_distances(A, paths), min_matrix(D))
        assert same(path_distances(A, paths, method="mean"), mean_matrix(S, C))
    run_all(Sm.indptr.astype(np.int64), Sm.indices.astype(np.int64), 7, paths)


def test_long_and_short_rows_mixed(gpu):
    """Rows of 64 and 65 entries side by side (one thread / a block), plus empties."""
    n = 300
    rows = np.concatenate([np.full(64, 3), np.full(65, 4), np.full(299, 200), [299]])
    cols = np.concatenate([np.arange(64) + 10, np.arange(65) + 100, np.delete(np.arange(300), 200), [299]])
    run_all(*csr_of(rows, cols, n), n, [[3], [4], [200], [73, 164], [299], [3, 4]])


def test_out_of_range_input_is_refused(gpu):
    """An index one past the last node, an indptr past the entries, a step past the nodes or below
    -1, a path offset that runs backwards: ValueError, never addressed."""
    from gfa2network_amd import _native

    ip = np.array([0, 1, 2], dtype=np.int32)
    ok = np.array([1, 0], dtype=np.int32)
    ptr, steps = np.array([0, 1, 2]), np.array([0, 1])

    def call(ip_, ix_, ptr_=ptr, steps_=steps, mean=False):
        return _native.csr_path_distances_host(ip_, ix_, 2, ptr_, steps_, mean)

    for mean in (False, True):
        with pytest.raises(ValueError):
            call(ip, np.array([1, 2], dtype=np.int32), mean=mean)
        with pytest.raises(ValueError):
            call(ip, np.array([1, -1], dtype=np.int32), mean=mean)
        with pytest.raises(ValueError):
            call(np.array([0, 3, 2], dtype=np.int32), ok, mean=mean)
        with pytest.raises(ValueError):
            call(ip, ok, steps_=np.array([0, 2]), mean=mean)
        with pytest.raises(ValueError):
            call(ip, ok, steps_=np.array([-2, 1]), mean=mean)
        with pytest.raises(ValueError):
            call(ip, ok, ptr_=np.array([0, 3, 2]), mean=mean)
    # and the context still answers
    (D,), info = call(ip, ok)
    assert D.tolist() == [[0, 1], [1, 0]] and info["levels"] == 1
    # a step of -1 is no node: no source, never reached
    (D,), _ = call(ip, ok, ptr_=np.array([0, 2, 4]), steps_=np.array([-1, 0, 1, -1]))
    assert D.tolist() == [[0, 1], [1, 0]]
    (S, C), _ = call(ip, ok, ptr_=np.array([0, 2, 4]), steps_=np.array([-1, 0, 1, -1]), mean=True)
    assert S.tolist() == [[0, 1], [1, 0]] and C.tolist() == [[1, 1], [1, 1]]
    (D,), _ = call(ip, ok, steps_=np.array([-1, 1]))
    assert D.tolist() == [[0xFFFFFFFF] * 2, [0xFFFFFFFF, 0]]  # (path 0 has no node left: nothing to reach)


def test_device_pointer_entry(gpu):
    """g2n_csr_path_distances itself: device arrays in, device tables out, on a context of the
    caller's — the same tables as the host entry, and its refusals."""
    import ctypes

    from gfa2network_amd import _native as nat

    lib, hip = nat.load(), nat.hip_runtime()
    n = 500
    rng = np.random.default_rng(9)
    pairs = np.unique(np.stack([np.append(rng.integers(0, n, 900), 0), np.append(rng.integers(0, n, 900), n - 1)],
                               axis=1), axis=0)  # (0, n - 1) is stored
    ip, ix = csr_of(pairs[:, 0], pairs[:, 1], n)
    paths = [rng.integers(0, n, int(rng.integers(1, 6))).tolist() for _ in range(70)]
    ptr = np.cumsum([0] + [len(p) for p in paths]).astype(np.int64)
    steps = np.concatenate(paths).astype(np.int64)
    K = len(paths)
    D, S, C = tables(ip, ix, n, paths)
    ctx = lib.g2n_context_create(0)
    bufs = []

    def dev(a):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), max(a.nbytes, 16)) == 0
        bufs.append(p)
        assert hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p

    try:
        for idt in (np.int32, np.int64):
            d_ip, d_ix, d_pp, d_pn = dev(ip.astype(idt)), dev(ix.astype(idt)), dev(ptr), dev(steps)
            for mean in (False, True):
                out = np.zeros((2, K, K), np.uint64) if mean else np.zeros((1, K, K), np.uint32)
                d_out = dev(out)
                info = nat.DistInfo()
                rc = lib.g2n_csr_path_distances(ctx, d_ip, d_ix, np.dtype(idt).itemsize, n, len(ix), d_pp, d_pn, K,
                                                int(mean), d_out, ctypes.byref(info))
                assert rc == nat.OK, nat.last_error()
                assert hip.hipMemcpy(out.ctypes.data, d_out, out.nbytes, 2) == 0
                assert info.batches == 2 and info.launches > 0
                if mean:
                    assert np.array_equal(out[0], S) and np.array_equal(out[1], C)
                else:
                    assert np.array_equal(out[0], D)
            info = nat.DistInfo()
            assert lib.g2n_csr_path_distances(ctx, d_ip, d_ix, 2, n, len(ix), d_pp, d_pn, K, 0, d_out,
                                              ctypes.byref(info)) == nat.E_ARG  # index_width
            assert lib.g2n_csr_path_distances(ctx, d_ip, d_ix, np.dtype(idt).itemsize, n, len(ix), d_pp, d_pn, K, 7,
                                              d_out, ctypes.byref(info)) == nat.E_ARG  # mode
            assert lib.g2n_csr_path_distances(ctx, d_ip, d_ix, np.dtype(idt).itemsize, n - 1, len(ix), d_pp, d_pn, K, 0,
                                              d_out, ctypes.byref(info)) == nat.E_ARG  # indices past n - 1
    finally:
        lib.g2n_context_destroy(ctx)
        for p in bufs:
            hip.hipFree(p)
