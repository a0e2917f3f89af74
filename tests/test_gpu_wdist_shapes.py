"""GPU: ``path_distances(..., weighted=True)`` (g2n_csr_path_distances_weighted_host -> the kernels of
g2n_wdist.hip) on hand-made float64 CSRs, bit for bit against scipy's Dijkstra (wdist_util).  Each
shape runs with int32 and with int64 indptr / indices, with both methods, and twice (the order in
which the relaxations race must not show in any output).  The shapes are the smallest that reach each
way the kernels can go wrong: path counts around the mask word and the batch, sizes around the block,
nodes that are improved after their first discovery, zero lengths and zero-length cycles, sums that
differ in the last bit, a chain (a round per node: the narrow regime), a star (a long row, a queue
overflow, narrow -> wide), a grid (wide and back), multiplicities, parallel entries, value dtypes,
the device-pointer entry and a matrix built from a file with a weight tag."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from stats_util import csr_of
from wdist_util import mean_matrix, min_matrix, same, tables

pytestmark = pytest.mark.gpu

CHAIN = 100_003
STAR = 100_000


def matrix(indptr, indices, values, n, idt):
    A = sp.csr_matrix((np.asarray(values), indices.astype(np.int32), indptr.astype(np.int32)), shape=(n, n))
    A.indptr, A.indices = indptr.astype(idt), indices.astype(idt)  # (the constructor narrows int64)
    assert A.indptr.dtype == idt and A.indices.dtype == idt and A.nnz == len(values)
    return A


def check_info(info, K, n):
    assert 1 <= info["batch_paths"] <= 64
    assert info["batches"] == -(-K // info["batch_paths"])
    assert 0 <= info["rounds"] <= n


def run_all(indptr, indices, values, n, paths, expect=None):
    """Both methods x both index widths x two runs against the checker; (D, S, C) and the int32
    runs' info.  ``expect``: the checker's tables when they come from another matrix."""
    from gfa2network_amd import path_distances

    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    D, S, C = expect if expect is not None else tables(indptr, indices, values, n, paths)
    want = {"min": min_matrix(D), "mean": mean_matrix(S, C)}
    infos = {}
    for method in ("min", "mean"):
        for idt in (np.int64, np.int32):
            A = matrix(indptr, indices, values, n, idt)
            first, info = path_distances(A, paths, method=method, weighted=True, return_info=True)
            assert first.dtype == np.float64 and first.shape == (len(paths), len(paths))
            assert same(first, want[method]), (method, idt)
            again, info2 = path_distances(A, paths, method=method, weighted=True, return_info=True)
            assert same(again, first), (method, idt)
            check_info(info, len(paths), n)
            check_info(info2, len(paths), n)
            infos[method] = info
    return (D, S, C), infos


def weighted_csr(rows, cols, w, n):
    """csr_of with the values carried along (stable within each row)."""
    rows = np.asarray(rows, dtype=np.int64)
    order = np.argsort(rows, kind="stable")
    indptr, indices = csr_of(rows, cols, n)
    return indptr, indices, np.asarray(w, dtype=np.float64)[order]


def undirected(rows, cols, w):
    rows, cols, w = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), np.asarray(w, dtype=np.float64)
    return np.concatenate([rows, cols]), np.concatenate([cols, rows]), np.concatenate([w, w])


def scaled_uniform(rng, m):
    """U(0, 1) * 10^k, k in -3 .. 3."""
    return rng.random(m) * 10.0 ** rng.integers(-3, 4, m)


@pytest.mark.parametrize("K", [0, 1, 2, 63, 64, 65, 129])
def test_path_counts(gpu, K):
    """The mask-word and batch boundaries on a 257-node random graph: single-node paths, ragged
    ones with repeats, and one path that covers every node."""
    n = 257
    rng = np.random.default_rng(K)
    pairs = np.unique(np.stack([rng.integers(0, n, 600), rng.integers(0, n, 600)], axis=1), axis=0)
    paths = [[int(rng.integers(0, n))] if k % 3 == 0 else rng.integers(0, n, int(rng.integers(2, 9))).tolist()
             for k in range(K)]
    if K > 1:
        paths[K // 2] = list(range(n))
    _, infos = run_all(*weighted_csr(pairs[:, 0], pairs[:, 1], scaled_uniform(rng, len(pairs)), n), n, paths)
    assert infos["min"]["batch_paths"] == max(1, min(K, 64))


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_small_sizes(gpu, n):
    rng = np.random.default_rng(n)
    pairs = np.unique(np.stack([rng.integers(0, n, 2 * n), rng.integers(0, n, 2 * n)], axis=1), axis=0)
    paths = [[0], [n - 1], rng.integers(0, n, 5).tolist(), []]
    run_all(*weighted_csr(pairs[:, 0], pairs[:, 1], scaled_uniform(rng, len(pairs)), n), n, paths)


def test_empty_rows_and_no_entries(gpu):
    n = 300
    (D, _, _), _ = run_all(*weighted_csr([5, 5, 200], [6, 299, 5], [0.25, 3.0, 1.5], n), n, [[200], [299, 6], [0], [5]])
    assert D[0, 1] == 1.75 and D[1, 0] == np.inf
    paths = [[0, 1], [2], [299]]
    (D, _, C), infos = run_all(np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0), n, paths)
    assert np.isinf(D).sum() == 6 and C.sum() == 4 and infos["min"]["rounds"] == 0


def test_triangle_is_improved_after_its_first_discovery(gpu):
    (D, _, _), infos = run_all(*weighted_csr([0, 0, 1], [2, 1, 2], [10.0, 1.0, 1.0], 3), 3, [[0], [2], [1]])
    assert D[0, 1] == 2.0 and D[0, 2] == 1.0 and D[1, 0] == np.inf
    assert infos["min"]["rounds"] == 2


@pytest.mark.parametrize("direct", ["falling", "rising"])
def test_staircase(gpu, direct):
    """1000 nodes, k -> k + 1 of 1 and 0 -> k (0's long row) of 2 (n - k) ("falling") or of 2 k
    ("rising").  Every node is reached directly in round 1.  With the falling steps the chain then
    improves nothing for path 0 (2 (n - k) + 1 > 2 (n - k - 1)).  With the rising ones node k's
    distance falls from 2 k to k + 1 along the chain, after its first discovery — the re-relaxation
    this shape is for; a node may read a distance that fell in the same round, so the rounds are
    at most the chain's n - 1, not exactly that."""
    n = 1000
    k = np.arange(1, n)
    rows = np.concatenate([np.zeros(n - 1, dtype=np.int64), k[:-1]])
    cols = np.concatenate([k, k[1:]])
    w = np.concatenate([2.0 * (n - k) if direct == "falling" else 2.0 * k, np.ones(n - 2)])
    (D, _, _), infos = run_all(*weighted_csr(rows, cols, w, n), n, [[0], [n - 1], [n // 2, 3]])
    if direct == "falling":
        assert D[0, 1] == 2.0 and D[0, 2] == 2.0 * (n - n // 2)
    else:
        assert D[0, 1] == float(n) and D[0, 2] == 4.0
    assert infos["min"]["rounds"] <= n - 1 and infos["mean"]["rounds"] <= n - 1


def test_zero_lengths(gpu):
    """A zero-length 3-cycle reachable from the source is not requeued forever; an all-zero graph
    gives 0.0 wherever anything is reached."""
    rows, cols = [0, 1, 2, 3, 3, 4], [1, 2, 3, 1, 4, 0]
    (D, _, _), infos = run_all(*weighted_csr(rows, cols, [1.0, 0.0, 0.0, 0.0, 2.0, 0.0], 6), 6, [[0], [3], [4], [5]])
    assert D[0, 1] == 1.0 and D[0, 2] == 3.0 and D[1, 0] == 2.0 and D[0, 3] == np.inf
    assert infos["min"]["rounds"] <= 5
    n = 257
    rng = np.random.default_rng(3)
    pairs = np.unique(np.stack([rng.integers(0, n, 500), rng.integers(0, n, 500)], axis=1), axis=0)
    paths = [[0], [7, 9], list(range(100, 140)), [256]]
    (D, S, _), _ = run_all(*weighted_csr(pairs[:, 0], pairs[:, 1], np.zeros(len(pairs)), n), n, paths)
    assert not D[np.isfinite(D)].any() and not S.any()
    # -0.0 counts as 0
    (D, _, _), _ = run_all(*weighted_csr([0, 1], [1, 2], [-0.0, 0.5], 3), 3, [[0], [2]])
    assert same(D[0, 1], 0.5)


def test_rounding(gpu):
    """Multiples of 0.1; two routes to one node whose sums differ in the last bit; 1e16 + 1 + 1
    against 1 + 1 + 1e16."""
    n = 257
    rng = np.random.default_rng(11)
    pairs = np.unique(np.stack([rng.integers(0, n, 700), rng.integers(0, n, 700)], axis=1), axis=0)
    w = rng.integers(0, 60, len(pairs)) * 0.1
    run_all(*weighted_csr(pairs[:, 0], pairs[:, 1], w, n), n, [[0], [1, 2, 3], list(range(50, 120)), [256, 256]])
    # 0.1 + 0.2 = 0.30000000000000004 against 0.3
    (D, _, _), _ = run_all(*weighted_csr([0, 1, 0, 2], [1, 3, 2, 3], [0.1, 0.2, 0.3, 0.0], 4), 4, [[0], [3]])
    assert same(D[0, 1], 0.3)
    (D, _, _), _ = run_all(*weighted_csr([0, 1, 0, 2], [1, 3, 2, 3], [0.1, 0.2, 0.30000000000000004, 0.0], 4), 4,
                           [[0], [3]])
    assert same(D[0, 1], 0.1 + 0.2)
    rows, cols = [0, 1, 2, 0, 3, 4], [1, 2, 5, 3, 4, 5]
    (D, _, _), _ = run_all(*weighted_csr(rows, cols, [1e16, 1.0, 1.0, 1.0, 1.0, 1e16], 6), 6, [[0], [5]])
    assert same(D[0, 1], 1e16) and (1.0 + 1.0) + 1e16 > 1e16
    # a sum that overflows is "not reached"
    (D, _, C), _ = run_all(*weighted_csr([0, 1], [1, 2], [1.7e308, 1.7e308], 3), 3, [[0], [2], [1]])
    assert D[0, 1] == np.inf and C[0, 1] == 0 and D[0, 2] == 1.7e308


def test_unit_weights_are_hops(gpu):
    from gfa2network_amd import path_distances

    n = 257
    rng = np.random.default_rng(5)
    pairs = np.unique(np.stack([rng.integers(0, n, 500), rng.integers(0, n, 500)], axis=1), axis=0)
    indptr, indices = csr_of(pairs[:, 0], pairs[:, 1], n)
    A = matrix(indptr, indices, np.ones(len(indices)), n, np.int32)
    paths = [[0], [7, 9, 9], list(range(100, 140)), [256], [1, 2]]
    for method in ("min", "mean"):
        assert same(path_distances(A, paths, method=method, weighted=True), path_distances(A, paths, method=method))


@pytest.fixture(scope="module")
def chain_orders():
    k = np.arange(CHAIN, dtype=np.int64)
    return {"in_order": k, "reversed": k[::-1].copy(), "permuted": np.random.default_rng(7).permutation(CHAIN)}


@pytest.mark.parametrize("order", ["in_order", "reversed", "permuted"])
def test_chain_depth(gpu, chain_orders, order):
    """A round per node.  launches * 16 < rounds holds only when the narrow regime carried the
    search: a launch per round (or per few rounds) cannot meet it."""
    ids = chain_orders[order]  # chain position k has node id ids[k]
    rng = np.random.default_rng(13)
    rows, cols, w = undirected(ids[:-1], ids[1:], rng.random(CHAIN - 1))
    paths = [[int(ids[0])], [int(ids[CHAIN // 2])], [int(ids[-1])]]
    (D, _, _), infos = run_all(*weighted_csr(rows, cols, w, CHAIN), CHAIN, paths)
    assert np.isfinite(D).all() and D[0, 2] > D[0, 1] > 0.0  # (D[2][0] adds the same lengths in the other order)
    for info in infos.values():
        assert info["rounds"] == CHAIN - 1 == 100_002
        assert info["launches"] * 16 < info["rounds"]


def test_star_as_the_hubs_row(gpu):
    """The hub's row is walked by a block; the frontier jumps from 1 node to 100 000 (the narrow
    queue overflows, the wide pass rebuilds it)."""
    n = STAR + 1
    rng = np.random.default_rng(17)
    for hub in (0, 12345):
        leaves = np.delete(np.arange(n, dtype=np.int64), hub)
        w = rng.random(STAR)
        paths = [[hub], [int(leaves[0]), int(leaves[77]), int(leaves[-1])], [int(leaves[5])]]
        (D, _, _), _ = run_all(*weighted_csr(np.full(STAR, hub), leaves, w, n), n, paths)
        assert same(D[0, 1], min(w[0], w[77], w[-1])) and D[1, 0] == np.inf
        # both ways: leaf -> hub -> every leaf
        rows, cols, w2 = undirected(np.full(STAR, hub), leaves, w)
        (D, _, _), infos = run_all(*weighted_csr(rows, cols, w2, n), n, paths)
        assert same(D[2, 1], min(w[5] + w[0], w[5] + w[77], w[5] + w[-1])) and infos["min"]["rounds"] == 2


@pytest.mark.parametrize("kind", ["uniform", "integer"])
def test_grid(gpu, kind):
    """300 x 300, undirected: a corner, the centre and four whole grid rows (their 1200 sources fit
    one workgroup's queue, what they improve does not: wide, and narrow again near the end)."""
    w_ = 300
    idx = np.arange(w_ * w_, dtype=np.int64).reshape(w_, w_)
    a = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    b = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    rng = np.random.default_rng(19)
    w = rng.random(len(a)) if kind == "uniform" else rng.integers(1, 10, len(a)).astype(np.float64)
    rows, cols, w = undirected(a, b, w)
    bars = idx[[30, 110, 190, 270], :].ravel().tolist()
    paths = [[0], [int(idx[w_ // 2, w_ // 2])], bars]
    _, infos = run_all(*weighted_csr(rows, cols, w, w_ * w_), w_ * w_, paths)
    for info in infos.values():
        # a node h hops away is discovered in round h exactly (a node improved in a round is expanded
        # in the next); above, no more rounds than synchronous Bellman-Ford's, itself below n
        assert 2 * (w_ - 1) <= info["rounds"] < w_ * w_


def test_shared_hub(gpu):
    """65 paths that all hold node 0 plus a private node, across two batches."""
    n = 200
    rng = np.random.default_rng(23)
    rows, cols, w = undirected(np.zeros(n - 1, dtype=np.int64), np.arange(1, n), rng.random(n - 1))
    ip, ix, val = weighted_csr(rows, cols, w, n)
    (D, _, _), _ = run_all(ip, ix, val, n, [[0, k + 1] for k in range(65)])
    assert not D.any()
    (D, _, _), _ = run_all(ip, ix, val, n, [[k + 1] for k in range(65)] + [[0]])
    assert same(D[0, 1], w[0] + w[1]) and same(D[0, 65], w[0])


def test_duplicate_steps(gpu):
    """The same step 1000 times counts 1000 times in the mean, added one after the other."""
    from gfa2network_amd import _native

    n = 10
    k = np.arange(n - 1)
    rows, cols, w = undirected(k, k + 1, np.full(n - 1, 0.1))
    ip, ix, val = weighted_csr(rows, cols, w, n)
    paths = [[0], [3] * 1000 + [5], [9, 9]]
    run_all(ip, ix, val, n, paths)
    ptr = np.cumsum([0] + [len(p) for p in paths])
    (S, C), _ = _native.csr_path_distances_weighted_host(ip, ix, val, n, ptr, np.concatenate(paths), True)
    d3 = (0.0 + 0.1 + 0.1) + 0.1
    total = 0.0
    for _ in range(1000):
        total += d3
    total += ((d3 + 0.1) + 0.1)
    assert C[0, 1] == 1001 and same(S[0, 1], total)
    assert C[1, 0] == 1 and same(S[1, 0], d3) and C[2, 1] == 1001 and S.dtype == np.float64 and C.dtype == np.uint64


def test_long_and_short_rows_mixed(gpu):
    """Rows of 64 and 65 entries side by side (one thread / a block), plus empties."""
    n = 300
    rng = np.random.default_rng(29)
    rows = np.concatenate([np.full(64, 3), np.full(65, 4), np.full(299, 200), [299]])
    cols = np.concatenate([np.arange(64) + 10, np.arange(65) + 100, np.delete(np.arange(300), 200), [299]])
    run_all(*weighted_csr(rows, cols, scaled_uniform(rng, len(rows)), n), n, [[3], [4], [200], [73, 164], [299], [3, 4]])


def test_parallel_entries(gpu):
    """A non-canonical CSR: the stored entries of one (u, v) are parallel edges — the shortest counts."""
    n = 40
    rng = np.random.default_rng(31)
    rows, cols = rng.integers(0, n, 400), rng.integers(0, n, 400)  # (400 draws of 1600 pairs: many repeats)
    w = scaled_uniform(rng, 400)
    assert len(np.unique(rows * n + cols)) < 400
    best = {}
    for r, c, x in zip(rows.tolist(), cols.tolist(), w.tolist()):
        best[(r, c)] = min(x, best.get((r, c), np.inf))
    keys = sorted(best)
    paths = [[0], [5, 6], list(range(20, 30)), [39]]
    canon = weighted_csr([k[0] for k in keys], [k[1] for k in keys], [best[k] for k in keys], n)
    expect = tables(*canon, n, paths)
    run_all(*weighted_csr(rows, cols, w, n), n, paths, expect=expect)


@pytest.mark.parametrize("dt", [np.bool_, np.int8, np.int32, np.float32])
def test_value_dtypes(gpu, dt):
    from gfa2network_amd import path_distances

    n = 100
    rng = np.random.default_rng(37)
    pairs = np.unique(np.stack([rng.integers(0, n, 300), rng.integers(0, n, 300)], axis=1), axis=0)
    indptr, indices = csr_of(pairs[:, 0], pairs[:, 1], n)
    if dt is np.bool_:
        vals = rng.integers(0, 2, len(indices)).astype(dt)
    elif dt is np.float32:
        vals = rng.random(len(indices)).astype(dt)
    else:
        vals = rng.integers(0, 100, len(indices)).astype(dt)
    A = matrix(indptr, indices, vals, n, np.int32)
    assert A.dtype == dt
    paths = [[0], [1, 2], list(range(40, 60))]
    D, S, C = tables(indptr, indices, vals.astype(np.float64), n, paths)
    assert same(path_distances(A, paths, weighted=True), min_matrix(D))
    assert same(path_distances(A, paths, method="mean", weighted=True), mean_matrix(S, C))
    assert same(path_distances(A.astype(np.float64), paths, weighted=True), min_matrix(D))
    assert same(path_distances(A.tocoo(), paths, weighted=True), min_matrix(D))  # (no repeats: tocsr() sums nothing)


def test_bad_values_are_refused_on_the_device(gpu):
    """The native entry checks the values itself (the Python surface never lets them through), and
    out-of-range structure is refused as by the unweighted entry; the context still answers."""
    from gfa2network_amd import _native

    ip, ix = np.array([0, 1, 2], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    ptr, steps = np.array([0, 1, 2]), np.array([0, 1])

    def call(val, ix_=ix, ptr_=ptr, steps_=steps, mean=False):
        return _native.csr_path_distances_weighted_host(ip, ix_, np.asarray(val, dtype=np.float64), 2, ptr_, steps_,
                                                        mean)

    for mean in (False, True):
        for bad in (-1.0, float("nan"), float("inf"), -float("inf"), -5e-324):
            with pytest.raises(ValueError):
                call([0.5, bad], mean=mean)
        with pytest.raises(ValueError):
            call([0.5, 0.5], ix_=np.array([1, 2], dtype=np.int32), mean=mean)
        with pytest.raises(ValueError):
            call([0.5, 0.5], steps_=np.array([0, 2]), mean=mean)
        with pytest.raises(ValueError):
            call([0.5, 0.5], ptr_=np.array([0, 3, 2]), mean=mean)
    (D,), info = call([0.5, 0.25])
    assert D.tolist() == [[0.0, 0.5], [0.25, 0.0]] and info["rounds"] == 1
    (S, C), _ = call([0.5, 0.25], ptr_=np.array([0, 2, 4]), steps_=np.array([-1, 0, 1, -1]), mean=True)
    assert S.tolist() == [[0.0, 0.5], [0.25, 0.0]] and C.tolist() == [[1, 1], [1, 1]]


def test_device_pointer_entry(gpu):
    """g2n_csr_path_distances_weighted itself: device arrays in, device tables out, on a context of
    the test's own — the checker's tables, its refusals, and an output buffer a refused call leaves
    as it was."""
    from gfa2network_amd import _native as nat

    lib, hip = nat.load(), nat.hip_runtime()
    n = 500
    rng = np.random.default_rng(9)
    pairs = np.unique(np.stack([np.append(rng.integers(0, n, 900), 0), np.append(rng.integers(0, n, 900), n - 1)],
                               axis=1), axis=0)  # (0, n - 1) is stored
    ip, ix, val = weighted_csr(pairs[:, 0], pairs[:, 1], scaled_uniform(rng, len(pairs)), n)
    paths = [rng.integers(0, n, int(rng.integers(1, 6))).tolist() for _ in range(70)]
    ptr = np.cumsum([0] + [len(p) for p in paths]).astype(np.int64)
    steps = np.concatenate(paths).astype(np.int64)
    K = len(paths)
    D, S, C = tables(ip, ix, val, n, paths)
    ctx = lib.g2n_context_create(0)
    bufs = []

    def dev(a):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), max(a.nbytes, 16)) == 0
        bufs.append(p)
        assert hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p

    try:
        d_val, d_pp, d_pn = dev(val), dev(ptr), dev(steps)
        neg = val.copy()
        neg[len(neg) // 2] = -neg[len(neg) // 2] - 1.0
        d_neg = dev(neg)
        for idt in (np.int32, np.int64):
            d_ip, d_ix = dev(ip.astype(idt)), dev(ix.astype(idt))
            iw = np.dtype(idt).itemsize
            for mean in (False, True):
                out = np.zeros((2 if mean else 1, K, K), np.float64)
                d_out = dev(out)
                info = nat.WDistInfo()
                rc = lib.g2n_csr_path_distances_weighted(ctx, d_ip, d_ix, iw, d_val, n, len(ix), d_pp, d_pn, K,
                                                         int(mean), d_out, ctypes.byref(info))
                assert rc == nat.OK, nat.last_error()
                assert hip.hipMemcpy(out.ctypes.data, d_out, out.nbytes, 2) == 0
                assert info.batch_paths == 64 and info.batches == 2 and info.launches > 0 and info.rounds <= n
                if mean:
                    assert same(out[0], S) and np.array_equal(out[1].view(np.uint64), C)
                else:
                    assert same(out[0], D)
                # refusals leave the tables as they were
                mark = np.full(out.shape, 123.25)
                assert hip.hipMemcpy(d_out, mark.ctypes.data, mark.nbytes, 1) == 0
                info = nat.WDistInfo()
                refused = [
                    lib.g2n_csr_path_distances_weighted(ctx, d_ip, d_ix, 2, d_val, n, len(ix), d_pp, d_pn, K, int(mean),
                                                        d_out, ctypes.byref(info)),  # index_width
                    lib.g2n_csr_path_distances_weighted(ctx, d_ip, d_ix, iw, d_val, n, len(ix), d_pp, d_pn, K, 7, d_out,
                                                        ctypes.byref(info)),  # mode
                    lib.g2n_csr_path_distances_weighted(ctx, d_ip, d_ix, iw, d_val, n - 1, len(ix), d_pp, d_pn, K,
                                                        int(mean), d_out, ctypes.byref(info)),  # indices past n - 1
                    lib.g2n_csr_path_distances_weighted(ctx, d_ip, d_ix, iw, d_neg, n, len(ix), d_pp, d_pn, K, int(mean),
                                                        d_out, ctypes.byref(info)),  # a negative value
                ]
                assert refused == [nat.E_ARG] * 4
                back = np.empty_like(mark)
                assert hip.hipMemcpy(back.ctypes.data, d_out, back.nbytes, 2) == 0
                assert same(back, mark)
    finally:
        lib.g2n_context_destroy(ctx)
        for p in bufs:
            hip.hipFree(p)


def test_from_a_file_with_a_weight_tag(gpu, tmp_path):
    """A 20-segment GFA with RC:i: and RC:f: tags and three P lines: the weighted matrix built on the
    GPU, the paths' steps through the node list, and the weighted distances over that same matrix."""
    from gfa2network_amd import convert_format, load_paths, parse_gfa, path_distances

    rng = np.random.default_rng(41)
    names = [f"s{k}" for k in range(20)]
    lines = ["H\tVN:Z:1.0"] + [f"S\t{nm}\tACGT" for nm in names]
    pairs = {(k, k + 1) for k in range(19)} | {(int(a), int(b)) for a, b in rng.integers(0, 20, (25, 2)) if a != b}
    for q, (a, b) in enumerate(sorted(pairs)):
        tag = f"RC:i:{int(rng.integers(0, 40))}" if q % 2 else f"RC:f:{float(rng.integers(1, 400)) / 8.0}"
        lines.append(f"L\t{names[a]}\t+\t{names[b]}\t+\t0M\t{tag}")
    lines += ["P\tp1\ts0+,s1+,s2+\t*", "P\tp2\ts19+\t*", "P\tp3\ts7+,s7+,s12-,s3+\t*"]
    path = tmp_path / "weighted.gfa"
    path.write_text("\n".join(lines) + "\n")
    A, nodes = parse_gfa(str(path), build_graph=False, build_matrix=True, weight_tag="RC", asymmetric=True,
                         return_node_list=True)
    A = convert_format(A, "csr")
    assert A.format == "csr" and A.shape == (20, 20) and A.dtype == np.float64 and (A.data != 1.0).any()
    index = {nm: k for k, nm in enumerate(nodes)}
    paths = [[index[s] for s in steps] for steps in load_paths(str(path)).values()]
    assert [len(p) for p in paths] == [3, 1, 4]
    D, S, C = tables(A.indptr, A.indices, A.data, 20, paths)
    assert np.isfinite(D[0]).all()
    assert same(path_distances(A, paths, weighted=True), min_matrix(D))
    assert same(path_distances(A, paths, method="mean", weighted=True), mean_matrix(S, C))
