"""Checkers shared by the path-distance tests: the directed tables D / S / C that
g2n_csr_path_distances defines, taken with scipy's unweighted multi-source Dijkstra over a CSR
structure (one search per path, as the reference runs NetworkX's), and the matrices the reference
forms from them.  The reference itself is not needed."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import dijkstra

UNREACHED = np.uint32(0xFFFFFFFF)


def tables(indptr, indices, n, paths):
    """(D, S, C) of K node lists: D[i][j] = min over the steps v of j of d_i(v) (uint32, 0xFFFFFFFF
    when no step is reached), S[i][j] / C[i][j] = the sum / count of d_i(v) over the reached steps
    of j, duplicates counted each time (uint64)."""
    K = len(paths)
    D = np.full((K, K), UNREACHED, dtype=np.uint32)
    S = np.zeros((K, K), dtype=np.uint64)
    C = np.zeros((K, K), dtype=np.uint64)
    steps = [np.asarray(p, dtype=np.int64).reshape(-1) for p in paths]
    G = sp.csr_matrix((np.ones(len(indices), dtype=np.int8), np.asarray(indices, dtype=np.int64),
                       np.asarray(indptr, dtype=np.int64)), shape=(n, n))
    for i in range(K):
        if not len(steps[i]):
            continue
        d = dijkstra(G, directed=True, unweighted=True, indices=np.unique(steps[i]), min_only=True)
        for j in range(K):
            dj = d[steps[j]]
            dj = dj[np.isfinite(dj)]
            if len(dj):
                D[i, j] = np.uint32(dj.min())
                S[i, j] = np.uint64(dj.sum())
                C[i, j] = np.uint64(len(dj))
    return D, S, C


def level_sizes(indptr, indices, n, paths):
    """How many nodes enter the frontier at each level when all the paths (at most 64: one batch) are
    searched together: the nodes v with d_i(v) == L for some path i."""
    G = sp.csr_matrix((np.ones(len(indices), dtype=np.int8), np.asarray(indices, dtype=np.int64),
                       np.asarray(indptr, dtype=np.int64)), shape=(n, n))
    codes = []
    for p in paths:
        d = dijkstra(G, directed=True, unweighted=True, indices=np.unique(np.asarray(p, dtype=np.int64)), min_only=True)
        v = np.nonzero(np.isfinite(d))[0]
        codes.append(d[v].astype(np.int64) * n + v)
    return np.bincount(np.unique(np.concatenate(codes)) // n)


def min_matrix(D):
    """The directed min table as float64: inf where unreached, 0.0 on the diagonal."""
    M = D.astype(np.float64)
    M[D == UNREACHED] = np.inf
    np.fill_diagonal(M, 0.0)
    return M


def mean_matrix(S, C):
    """genome_distance_matrix's mean: (S[i][j] + S[j][i]) / (C[i][j] + C[j][i]) as one division of
    Python ints, inf without a reached term, 0.0 on the diagonal."""
    K = len(S)
    M = np.zeros((K, K), dtype=np.float64)
    for i in range(K):
        for j in range(K):
            if i != j:
                c = int(C[i, j]) + int(C[j, i])
                M[i, j] = (int(S[i, j]) + int(S[j, i])) / c if c else float("inf")
    return M


def reference_matrix(D, S, C, method):
    """What genome_distance_matrix returns: min holds D[i][j] (i < j) in both triangles."""
    if method != "min":
        return mean_matrix(S, C)
    M = min_matrix(D)
    iu = np.triu_indices(len(M), 1)
    M.T[iu] = M[iu]
    return M


def same(a, b):
    """Bit-for-bit equality of two float64 arrays."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()
