"""GPU: ``pair_sums`` and ``node_distances`` (g2n_csr_pair_distances_host / _weighted_host -> the
kernels of g2n_pairs.hip) on hand-made CSRs, against scipy's Dijkstra per distinct source
(pair_util).  Each shape runs with int32 and with int64 indptr / indices, and twice (the atomics'
races must not move a value); the sums also against the S / C column the singleton-path emulation
through g2n_csr_path_distances gives.  The shapes are the smallest that reach each way the kernels
can go wrong — source counts around the mask word and the batch, sizes around the block, a chain
past one narrow launch's level budget (the LDS sums are flushed and start again), a star (a long
row, a queue overflow, narrow -> wide, a collect whose targets lie in many blocks), a grid whose
frontier passes the narrow cap and comes back, repeated targets and sources, -1, unreachable parts,
empty rows — and ``info`` tells that the intended regime ran: per batch one launch sets the sources,
every wide level costs three (collect, two expansions), a narrow launch one."""
import numpy as np
import pytest
import scipy.sparse as sp

import pair_util
from pair_util import same
from stats_util import csr_of

pytestmark = pytest.mark.gpu

LEVEL_BUDGET = 8192  # kDistLevelBudget
NARROW_CAP = 2048    # kDistNarrowCap
WEIGHTS = np.array([0.1, 0.2, 0.7, 0.3, 1.5, 0.0])


def matrix(indptr, indices, values, n, idt):
    data = np.ones(len(indices), dtype=np.float64) if values is None else np.asarray(values, dtype=np.float64)
    A = sp.csr_matrix((data, indices.astype(np.int32), indptr.astype(np.int32)), shape=(n, n))
    A.indptr, A.indices = indptr.astype(idt), indices.astype(idt)  # (the constructor narrows int64)
    assert A.indptr.dtype == idt and A.indices.dtype == idt
    return A


def weights_for(indices, seed=3):
    return WEIGHTS[np.random.default_rng(seed).integers(0, len(WEIGHTS), len(indices))]


def emulated_sums(indptr, indices, n, sources, targets):
    """S / C of the last column of path_distances(singletons + [targets], "mean")'s tables"""
    from gfa2network_amd import _native

    paths = [[int(s)] for s in sources] + [[int(t) for t in targets]]
    ptr = np.cumsum([0] + [len(p) for p in paths])
    steps = np.concatenate([np.asarray(p, dtype=np.int64) for p in paths]) if ptr[-1] else np.zeros(0, dtype=np.int64)
    (S, C), _ = _native.csr_path_distances_host(indptr.astype(np.int32), indices.astype(np.int32), n, ptr, steps, True)
    k = len(sources)
    return S[:k, k].copy(), C[:k, k].copy()


def run_all(indptr, indices, n, sources, targets, values=None, emulate=True):
    """pair_sums and node_distances (hops; weighted too when values are given) x both index widths x
    two runs against the checker.  Returns (the hop table, {"sums" / "table" / "weighted": info})."""
    from gfa2network_amd import node_distances, pair_sums

    T = pair_util.table(indptr, indices, None, n, sources, targets)
    S, C = pair_util.sums(T)
    W = None if values is None else pair_util.table(indptr, indices, values, n, sources, targets)
    infos = {}
    for idt in (np.int32, np.int64):
        A = matrix(indptr, indices, values, n, idt)
        for _again in range(2):
            gs, gc, infos["sums"] = pair_sums(A, sources, targets, return_info=True)
            assert gs.dtype == np.uint64 == gc.dtype
            assert same(gs, S) and same(gc, C), (idt, gs, S, gc, C)
            got, infos["table"] = node_distances(A, sources, targets, return_info=True)
            assert same(got, T), idt
            if W is not None:
                got, infos["weighted"] = node_distances(A, sources, targets, weighted=True, return_info=True)
                assert same(got, W), idt
        for k in ("sums", "table"):
            assert infos[k]["batches"] == (len(sources) + 63) // 64
    if emulate:
        es, ec = emulated_sums(indptr, indices, n, sources, targets)
        assert same(es, S) and same(ec, C)
    return T, infos


def undirected(rows, cols):
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    return np.concatenate([rows, cols]), np.concatenate([cols, rows])


@pytest.fixture(scope="module")
def random257():
    n = 257
    rng = np.random.default_rng(1)
    pairs = np.unique(np.stack([rng.integers(0, n, 400), rng.integers(0, n, 400)], axis=1), axis=0)
    ip, ix = csr_of(pairs[:, 0], pairs[:, 1], n)
    return n, ip, ix, weights_for(ix)


@pytest.mark.parametrize("n_src", [0, 1, 63, 64, 65, 129])
def test_source_counts(gpu, random257, n_src):
    """The mask-word and batch boundaries: bit b of batch k is source occurrence 64 k + b."""
    n, ip, ix, val = random257
    rng = np.random.default_rng(n_src)
    sources = rng.integers(0, n, n_src)
    targets = np.concatenate([rng.integers(0, n, 70), sources[:5]])  # (targets that are sources)
    _T, infos = run_all(ip, ix, n, sources, targets, val)
    if n_src:
        assert infos["weighted"]["batches"] == (n_src + 63) // 64 and infos["weighted"]["batch_paths"] == min(64, n_src)


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_small_sizes(gpu, n):
    rng = np.random.default_rng(n)
    pairs = np.unique(np.stack([rng.integers(0, n, 2 * n), rng.integers(0, n, 2 * n)], axis=1), axis=0)
    ip, ix = csr_of(pairs[:, 0], pairs[:, 1], n)
    run_all(ip, ix, n, [0, n - 1, int(rng.integers(0, n))], np.arange(n), weights_for(ix))
    run_all(ip, ix, n, np.arange(n), [], weights_for(ix))
    run_all(ip, ix, n, [], [0], weights_for(ix))


def test_chain_past_the_level_budget(gpu):
    """8200 nodes in a row, one source at the head: the first narrow launch runs its 8192 levels and
    hands the frontier back, the second finishes — targets on both sides of that boundary, so the
    sums held in LDS are flushed by the first launch and continue from zero in the second."""
    n = 8200
    k = np.arange(n - 1, dtype=np.int64)
    ip, ix = csr_of(k, k + 1, n)
    targets = [0, 5, LEVEL_BUDGET - 1, LEVEL_BUDGET, LEVEL_BUDGET + 1, n - 1, n - 1, 5]
    T, infos = run_all(ip, ix, n, [0, LEVEL_BUDGET - 3], targets, np.full(len(ix), 0.1))
    assert T[0].tolist() == [float(t) for t in targets] and T[1, 1] == np.inf and T[1, 3] == 3
    for key in ("sums", "table"):
        assert infos[key]["levels"] == n - 1
        # the sources, one collect, a narrow launch of 8192 levels and one of the last 8
        assert infos[key]["launches"] == 4, infos[key]
    assert infos["weighted"]["rounds"] == n - 1 and infos["weighted"]["launches"] < 10


def test_star_overflows_the_narrow_queue(gpu):
    """A hub with 2100 leaves, both ways.  From the hub: its row (past kStatsShortRow, walked by the
    block) pushes 2100 nodes at the one workgroup's queue of 2048 — the launch ends, the wide
    collect takes level 1 in nine blocks, each flushing its own LDS counts."""
    leaves = 2100
    assert leaves > NARROW_CAP
    n = leaves + 1
    hub = 0
    rows, cols = undirected(np.full(leaves, hub), np.arange(1, n))
    ip, ix = csr_of(rows, cols, n)
    targets = np.arange(n)
    T, infos = run_all(ip, ix, n, [hub], targets, weights_for(ix))
    assert T[0, 0] == 0 and (T[0, 1:] == 1).all()
    for key in ("sums", "table"):
        assert infos[key]["levels"] == 1
        # sources, collect 0, narrow (overflow), collect 1, two wide expansions, collect 2 (empty)
        assert infos[key]["launches"] == 7, infos[key]
    # from a leaf too: level 2 is wide again, seen from another bit of the same batch
    T, infos = run_all(ip, ix, n, [hub, 7, hub], np.concatenate([targets, targets[-300:]]), emulate=False)
    assert T[1, 7] == 0 and T[1, 0] == 1 and T[1, 8] == 2
    for key in ("sums", "table"):
        assert infos[key]["levels"] == 2 and infos[key]["launches"] == 10, infos[key]


def test_rows_of_64_and_65(gpu):
    """Rows of exactly 64 and 65 entries side by side (one thread / the block), plus empty rows."""
    n = 300
    rows = np.concatenate([np.full(64, 3), np.full(65, 4), np.full(299, 200), [299]])
    cols = np.concatenate([np.arange(64) + 10, np.arange(65) + 100, np.delete(np.arange(300), 200), [299]])
    ip, ix = csr_of(rows, cols, n)
    run_all(ip, ix, n, [3, 4, 200, 73, 299, 0], np.arange(n), weights_for(ix))


def test_grid_passes_the_cap_and_comes_back(gpu):
    """64 x 64, undirected, one whole grid row as the 64 sources of one batch: the union of their
    diamonds' rims passes 2048 nodes from level 16 on and thins out again before the far corners
    (level 32 + 63) — narrow, wide, narrow."""
    w = 64
    idx = np.arange(w * w, dtype=np.int64).reshape(w, w)
    rows, cols = undirected(np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()]),
                            np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()]))
    ip, ix = csr_of(rows, cols, w * w)
    sources = idx[32, :]
    targets = np.concatenate([idx[0, :], idx[63, ::7], idx[32, :5]])
    T, infos = run_all(ip, ix, w * w, sources, targets, emulate=False)
    assert T[0, 63] == 32 + 63 and T[5, 5] == 32
    for key in ("sums", "table"):
        levels, launches = infos[key]["levels"], infos[key]["launches"]
        assert levels == 32 + 63
        all_wide = 1 + 3 * (levels + 1) + 1
        assert 1 + 3 * 8 < launches < all_wide - 3 * 8, infos[key]  # (several wide levels, several narrow ones)


def test_repeated_targets_and_sources(gpu):
    """One node 1000 times in the targets counts 1000 times; one node 65 times in the sources is 65
    bits over two batches with the same row."""
    n = 10
    k = np.arange(n - 1)
    rows, cols = undirected(k, k + 1)
    ip, ix = csr_of(rows, cols, n)
    from gfa2network_amd import pair_sums

    sources = [0] + [3] * 65 + [9]
    targets = [3] * 1000 + [5, 0]
    T, _ = run_all(ip, ix, n, sources, targets, weights_for(ix))
    S, C = pair_sums(matrix(ip, ix, None, n, np.int32), sources, targets)
    assert C.tolist() == [1002] * 67 and S[0] == 3005 and S[1] == 2 + 3 and (S[1:66] == S[1]).all()
    assert (T[1:66] == T[1]).all()


def test_no_node_unreachable_and_empty(gpu):
    """-1 in both lists, components that do not meet, empty rows, and a matrix without entries."""
    n = 300
    ip, ix = csr_of([5, 5, 200], [6, 299, 5], n)
    sources = [200, -1, 299, 5, -1, 0]
    targets = [-1, 299, 6, 200, 5, 0, -1, 299]
    T, _ = run_all(ip, ix, n, sources, targets, np.array([0.2, 0.7, 0.1]))
    assert T[0].tolist() == [np.inf, 2, 2, 0, 1, np.inf, np.inf, 2]
    assert np.isinf(T[1]).all() and np.isinf(T[:, 0]).all() and T[5, 5] == 0 and np.isinf(T[2, 2])
    run_all(ip, ix, n, [-1, -1], [-1], np.array([0.2, 0.7, 0.1]))
    empty_ip, empty_ix = np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int64)
    T, infos = run_all(empty_ip, empty_ix, n, [0, 1, 299], [1, 299, 299, 7], np.zeros(0))
    assert np.isfinite(T).sum() == 3 and infos["sums"]["levels"] == 0


def test_other_formats_and_return_shapes(gpu):
    from gfa2network_amd import node_distances, pair_sums

    rows = np.array([0, 1, 0, 2, 3, 5, 4])
    cols = np.array([1, 0, 2, 2, 4, 5, 3])
    Cm = sp.coo_matrix((np.array([0.5, 0.1, 0.2, 0.7, 0.3, 1.0, 0.1]), (rows, cols)), shape=(7, 7))
    Sm = Cm.tocsr()
    src, tgt = [0, 3, 6], [2, 4, 1, 1]
    T = pair_util.table(Sm.indptr, Sm.indices, None, 7, src, tgt)
    W = pair_util.table(Sm.indptr, Sm.indices, Sm.data, 7, src, tgt)
    for A in (Cm, Sm, Cm.tocsc(), Cm.todok()):
        assert same(node_distances(A, src, tgt), T)
        assert same(node_distances(A, src, tgt, weighted=True), W)
        S, C = pair_sums(A, src, tgt)
        assert same(S, pair_util.sums(T)[0]) and same(C, pair_util.sums(T)[1])
    assert node_distances(Sm, [], []).shape == (0, 0) and node_distances(Sm, [1], [], weighted=True).shape == (1, 0)


def test_out_of_range_input_is_refused(gpu):
    """An id one past the last node or below -1 in either list, an index past the nodes, an indptr
    past the entries, a negative length: ValueError (G2N_E_ARG), nothing addressed, no table written;
    and the context still answers."""
    from gfa2network_amd import _native

    ip = np.array([0, 1, 2], dtype=np.int32)
    ok = np.array([1, 0], dtype=np.int32)
    one = np.ones(2)

    def call(ip_=ip, ix_=ok, src=(0, 1), tgt=(1, 0), table=True, val=None):
        return _native.csr_pair_distances_host(ip_, ix_, val, 2, np.array(src), np.array(tgt), table)

    for table, val in ((False, None), (True, None), (True, one)):
        for bad in (dict(ix_=np.array([1, 2], dtype=np.int32)), dict(ix_=np.array([1, -1], dtype=np.int32)),
                    dict(ip_=np.array([0, 3, 2], dtype=np.int32)), dict(src=(0, 2)), dict(src=(-2, 1)),
                    dict(tgt=(2, 0)), dict(tgt=(0, -2))):
            with pytest.raises(ValueError, match="out of range"):
                call(table=table, val=val, **bad)
    with pytest.raises(ValueError, match="negative or not finite"):
        call(val=np.array([1.0, -0.5]))
    with pytest.raises(ValueError, match="negative or not finite"):
        call(val=np.array([np.nan, 1.0]))
    (D,), info = call()
    assert D.tolist() == [[1, 0], [0, 1]] and D.dtype == np.uint32 and info["levels"] == 1
    (S, C), _ = call(table=False)
    assert S.tolist() == [1, 1] and C.tolist() == [2, 2]
    (D,), info = call(val=np.array([0.1, 0.7]))
    assert D.tolist() == [[0.1, 0.0], [0.0, 0.7]] and info["rounds"] == 1
    (D,), _ = call(src=(-1, 1), tgt=(1, -1))
    assert D.tolist() == [[0xFFFFFFFF] * 2, [0, 0xFFFFFFFF]]


def test_device_entry_points(gpu):
    """g2n_csr_pair_distances(_weighted) themselves: device arrays in, device output out, on a context
    of the caller's; a refused call leaves the output as it was."""
    import ctypes

    from gfa2network_amd import _native as nat

    lib, hip = nat.load(), nat.hip_runtime()
    n = 257
    rng = np.random.default_rng(9)
    pairs = np.unique(np.stack([np.append(rng.integers(0, n, 500), 0), np.append(rng.integers(0, n, 500), n - 1)],
                               axis=1), axis=0)  # (0, n - 1) is stored
    ip, ix = csr_of(pairs[:, 0], pairs[:, 1], n)
    val = weights_for(ix)
    src, tgt = rng.integers(0, n, 70).astype(np.int64), rng.integers(-1, n, 90).astype(np.int64)
    T = pair_util.table(ip, ix, None, n, src, tgt)
    W = pair_util.table(ip, ix, val, n, src, tgt)
    S, C = pair_util.sums(T)
    ctx = lib.g2n_context_create(0)
    bufs = []

    def dev(a):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), max(a.nbytes, 16)) == 0
        bufs.append(p)
        assert hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p

    def back(d, like):
        out = np.empty_like(like)
        assert hip.hipMemcpy(out.ctypes.data, d, out.nbytes, 2) == 0
        return out

    try:
        d_src, d_tgt, d_val = dev(src), dev(tgt), dev(val)
        for idt in (np.int32, np.int64):
            d_ip, d_ix = dev(ip.astype(idt)), dev(ix.astype(idt))
            iw = np.dtype(idt).itemsize
            common = (n, len(ix), d_src, len(src), d_tgt, len(tgt))
            info, winfo = nat.DistInfo(), nat.WDistInfo()
            sevens = np.full((len(src), len(tgt)), 7, dtype=np.uint32)
            d_out = dev(sevens)
            assert lib.g2n_csr_pair_distances(ctx, d_ip, d_ix, iw, *common, nat.PAIR_TABLE, d_out,
                                              ctypes.byref(info)) == nat.OK, nat.last_error()
            got = back(d_out, sevens).astype(np.float64)
            got[got == 0xFFFFFFFF] = np.inf
            assert same(got, T) and info.batches == 2 and info.launches > 0
            d_sc = dev(np.full((2, len(src)), 7, dtype=np.uint64))
            assert lib.g2n_csr_pair_distances(ctx, d_ip, d_ix, iw, *common, nat.PAIR_SUMS, d_sc,
                                              ctypes.byref(info)) == nat.OK, nat.last_error()
            assert same(back(d_sc, np.stack([S, C])), np.stack([S, C]))
            minus = np.full((len(src), len(tgt)), -1.0)
            d_w = dev(minus)
            assert lib.g2n_csr_pair_distances_weighted(ctx, d_ip, d_ix, iw, d_val, *common, d_w,
                                                       ctypes.byref(winfo)) == nat.OK, nat.last_error()
            assert same(back(d_w, minus), W) and winfo.batches == 2
            # refused: an unknown mode, a width of 2, a node count below an index — the output is untouched
            d_out, d_w = dev(sevens), dev(minus)
            short = (n - 1,) + common[1:]
            assert lib.g2n_csr_pair_distances(ctx, d_ip, d_ix, iw, *common, 5, d_out, ctypes.byref(info)) == nat.E_ARG
            assert lib.g2n_csr_pair_distances(ctx, d_ip, d_ix, 2, *common, nat.PAIR_TABLE, d_out,
                                              ctypes.byref(info)) == nat.E_ARG
            assert lib.g2n_csr_pair_distances(ctx, d_ip, d_ix, iw, *short, nat.PAIR_TABLE, d_out,
                                              ctypes.byref(info)) == nat.E_ARG
            assert lib.g2n_csr_pair_distances_weighted(ctx, d_ip, d_ix, iw, d_val, *short, d_w,
                                                       ctypes.byref(winfo)) == nat.E_ARG
            assert same(back(d_out, sevens), sevens) and same(back(d_w, minus), minus)
    finally:
        lib.g2n_context_destroy(ctx)
        for p in bufs:
            hip.hipFree(p)
