"""Checkers shared by the weighted path-distance tests: the directed tables D / S / C that
g2n_csr_path_distances_weighted defines, taken with scipy's multi-source Dijkstra over the float64
CSR (one search per path, as the reference runs NetworkX's with weight="weight"), and the matrices
path_distances(weighted=True) forms from them.  Comparisons are bit for bit.  The reference itself is
not needed."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import dijkstra


def graph(indptr, indices, values, n):
    """The float64 CSR as scipy's csgraph reads it: an explicit zero is an edge of length 0."""
    return sp.csr_matrix((np.asarray(values, dtype=np.float64), np.asarray(indices, dtype=np.int64),
                          np.asarray(indptr, dtype=np.int64)), shape=(n, n))


def tables(indptr, indices, values, n, paths):
    """(D, S, C) of K node lists: D[i][j] = min over the steps v of j of d_i(v) (float64, inf when no
    step is reached), S[i][j] = the sum of d_i(v) over the reached steps of j added in step order,
    left to right from 0.0 (a Python loop: np.sum is pairwise, another order), C[i][j] = how many
    those are (uint64).  A step of -1 is no node."""
    K = len(paths)
    D = np.full((K, K), np.inf, dtype=np.float64)
    S = np.zeros((K, K), dtype=np.float64)
    C = np.zeros((K, K), dtype=np.uint64)
    steps = [np.asarray(p, dtype=np.int64).reshape(-1) for p in paths]
    steps = [s[s >= 0] for s in steps]
    G = graph(indptr, indices, values, n)
    for i in range(K):
        if not len(steps[i]):
            continue
        d = dijkstra(G, directed=True, indices=np.unique(steps[i]), min_only=True)
        for j in range(K):
            total, count = 0.0, 0
            for x in d[steps[j]].tolist():
                if x != float("inf"):
                    total += x
                    count += 1
                    if x < D[i, j]:
                        D[i, j] = x
            S[i, j] = total
            C[i, j] = count
    return D, S, C


def min_matrix(D):
    """The directed min table with 0.0 on the diagonal."""
    M = np.array(D, dtype=np.float64)
    np.fill_diagonal(M, 0.0)
    return M


def mean_matrix(S, C):
    """(S[i][j] + S[j][i]) / float(C[i][j] + C[j][i]) in Python floats, inf without a reached term,
    0.0 on the diagonal."""
    K = len(S)
    M = np.zeros((K, K), dtype=np.float64)
    for i in range(K):
        for j in range(K):
            if i != j:
                c = int(C[i, j]) + int(C[j, i])
                M[i, j] = (float(S[i, j]) + float(S[j, i])) / float(c) if c else float("inf")
    return M


def same(a, b):
    """Bit-for-bit equality of two float64 arrays."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()
