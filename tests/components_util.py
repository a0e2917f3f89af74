"""The checker of the component tests: what ``graph_components`` / ``split_components`` must return,
from scipy and numpy alone (the reference itself is not needed for it).

  * labels: ``scipy.sparse.csgraph.connected_components(A, directed=False)``
  * perm / offsets / sizes: ``np.argsort(labels, kind="stable")``, ``np.bincount``
  * a component of a canonical CSR: ``A[idx][:, idx]``
  * a component of any CSR: a plain numpy restatement of "row p of component j is row nodes_j[p]
    of A, its entries in stored order, each column replaced by its position in nodes_j"
"""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

DTYPES = ("bool", "int8", "int32", "float32", "float64")


def csr_of(rows, cols, n):
    """The CSR structure of the entries (rows[k], cols[k]) in the given order within each row."""
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    order = np.argsort(rows, kind="stable")
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    return indptr, cols[order]


def matrix(indptr, indices, n, idt, data=None):
    """A scipy CSR over exactly these arrays (no sorting, no summing), its indices of dtype idt."""
    if data is None:
        data = np.ones(len(indices), dtype=np.float64)
    A = sp.csr_matrix((data, np.asarray(indices).astype(np.int32), np.asarray(indptr).astype(np.int32)), shape=(n, n))
    A.indptr, A.indices = np.asarray(indptr).astype(idt), np.asarray(indices).astype(idt)  # (the constructor narrows)
    assert A.indptr.dtype == idt and A.indices.dtype == idt and A.data.dtype == data.dtype
    return A


def telling_values(nnz, dtype, seed=0):
    """One value per entry that tells a misplaced item from a right one, as far as the dtype can: all
    distinct where it is wide enough, else a pseudo-random sequence."""
    dt = np.dtype(dtype)
    k = np.arange(nnz, dtype=np.int64)
    if dt == np.bool_:
        return np.random.default_rng(seed).integers(0, 2, nnz).astype(np.bool_)
    if dt == np.int8:
        return ((k * 37 + 11) % 251 - 125).astype(np.int8)
    if dt == np.int32:
        return (k * 7919 - 1_000_003).astype(np.int32)
    if dt == np.float32:
        return (k % 1_000_003).astype(np.float32) * np.float32(-1.25) + np.float32(0.5)
    return k.astype(np.float64) * 1.000000119 + 0.25


def want_labels(indptr, indices, n):
    """(k, int32 labels) as scipy numbers them."""
    if n == 0:
        return 0, np.zeros(0, dtype=np.int32)
    S = sp.csr_matrix((np.ones(len(indices), dtype=np.int8), np.asarray(indices, dtype=np.int64),
                       np.asarray(indptr, dtype=np.int64)), shape=(n, n))
    k, lab = connected_components(S, directed=False)
    return int(k), lab.astype(np.int32)


def want_grouping(labels, k):
    """(perm, offsets, sizes) of the labels."""
    perm = np.argsort(labels, kind="stable").astype(np.int64)
    sizes = np.bincount(labels, minlength=k).astype(np.int64)
    offsets = np.zeros(k + 1, dtype=np.int64)
    np.cumsum(sizes, out=offsets[1:])
    return perm, offsets, sizes


def want_component(indptr, indices, data, nodes, n):
    """(indptr, indices, data) of the component with these nodes (ascending), stored order kept: plain
    numpy, row by row."""
    pos = np.full(n, -1, dtype=np.int64)
    pos[nodes] = np.arange(len(nodes))
    lens = (indptr[nodes + 1] - indptr[nodes]).astype(np.int64)
    oip = np.zeros(len(nodes) + 1, dtype=np.int64)
    np.cumsum(lens, out=oip[1:])
    # entry q of the output comes from entry src[q] of the input
    src = np.repeat(indptr[nodes].astype(np.int64) - oip[:-1], lens) + np.arange(oip[-1])
    oix = pos[indices[src]]
    assert (oix >= 0).all()  # both ends of an entry are in one component
    return oip, oix, data[src]


def is_canonical(indptr, indices):
    lens = np.diff(indptr)
    rows = np.repeat(np.arange(len(lens)), lens)
    key = rows.astype(np.int64) * (int(indices.max()) + 1 if len(indices) else 1) + indices
    return bool((np.diff(key) > 0).all())


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_split(S, A):
    """Every field and every component of the result S of split_components(A) for the scipy CSR A
    (arrays as given: possibly unsorted rows, duplicates).  Returns the number of components."""
    n = A.shape[0]
    ip, ix, data = np.asarray(A.indptr), np.asarray(A.indices), np.asarray(A.data)
    k, lab = want_labels(ip, ix, n)
    perm, offsets, sizes = want_grouping(lab, k)
    assert S.n_components == k and type(S.n_components) is int
    assert same_bits(S.labels, lab)
    assert np.array_equal(S.perm, perm) and np.array_equal(S.offsets, offsets) and np.array_equal(S.sizes, sizes)
    canonical = is_canonical(ip, ix)
    for j in comps_to_check(k, sizes):
        Aj, nodes = S.component(j)
        want_nodes = np.flatnonzero(lab == j)
        assert np.array_equal(nodes, want_nodes), j
        wip, wix, wdata = want_component(ip, ix, data, want_nodes, n)
        assert Aj.shape == (len(nodes), len(nodes)) and Aj.dtype == A.dtype, j
        assert np.array_equal(Aj.indptr, wip) and np.array_equal(Aj.indices, wix), j
        assert same_bits(np.asarray(Aj.data), wdata), j
        if canonical and len(nodes) <= 5000:
            B = A[want_nodes][:, want_nodes]
            assert np.array_equal(Aj.indptr, B.indptr) and np.array_equal(Aj.indices, B.indices), j
            assert same_bits(np.asarray(Aj.data), np.asarray(B.data).astype(A.dtype)), j
    # the split is a permutation of the whole matrix: row p is row perm[p], stored order kept, each
    # column its node's position in perm minus its component's offset
    assert int(S.indptr[-1]) == int(ip[-1]) == len(S.indices) == len(S.data)
    assert int((S.indptr[offsets[1:]] - S.indptr[offsets[:-1]]).sum()) == int(ip[-1])  # component nnz add up to nnz
    lens = (ip[perm + 1] - ip[perm]).astype(np.int64)
    wip = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=wip[1:])
    src = np.repeat(ip[perm].astype(np.int64) - wip[:-1], lens) + np.arange(wip[-1])
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    cols = ix[src].astype(np.int64)
    assert np.array_equal(S.indptr, wip) and S.indptr.dtype == ip.dtype
    assert np.array_equal(S.indices, inv[cols] - offsets[lab[cols]]) and S.indices.dtype == ix.dtype
    assert same_bits(np.asarray(S.data), data[src])
    L, nodes = S.largest()
    jl = int(np.argmax(sizes))
    assert np.array_equal(nodes, np.flatnonzero(lab == jl)) and L.shape[0] == sizes[jl]
    return k


def comps_to_check(k, sizes):
    """Every component when there are few; else the first, the last, the largest and a spread."""
    if k <= 300:
        return range(k)
    pick = {0, 1, k - 1, k - 2, int(np.argmax(sizes)), int(np.argmin(sizes))}
    pick.update(int(x) for x in np.linspace(0, k - 1, 64).astype(np.int64))
    return sorted(pick)
