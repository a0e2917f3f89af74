"""Checkers shared by the node-to-node distance tests: the table g2n_csr_pair_distances(_weighted)
defines, taken with scipy's Dijkstra — one search per distinct source, unweighted or over the float64
values —, the sums and counts G2N_PAIR_SUMS forms from it, and the reference's ordered fold of
genome_distance(method="mean").  Comparisons are bit for bit.  The reference itself is not needed."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import dijkstra


def graph(indptr, indices, values, n):
    """The CSR as scipy's csgraph reads it (values None: every entry an edge of length 1; an explicit
    zero is an edge of length 0)."""
    data = np.ones(len(indices), dtype=np.float64) if values is None else np.asarray(values, dtype=np.float64)
    return sp.csr_matrix((data, np.asarray(indices, dtype=np.int64), np.asarray(indptr, dtype=np.int64)), shape=(n, n))


def table(indptr, indices, values, n, sources, targets):
    """T[i][t] = the distance from sources[i] to targets[t] as float64: 0.0 for the same node, inf
    without a path or where either id is -1.  Lists in order, duplicates kept."""
    src = np.asarray(sources, dtype=np.int64).reshape(-1)
    tgt = np.asarray(targets, dtype=np.int64).reshape(-1)
    T = np.full((len(src), len(tgt)), np.inf, dtype=np.float64)
    distinct = np.unique(src[src >= 0])
    if not len(distinct) or not len(tgt) or n == 0:
        return T
    d = dijkstra(graph(indptr, indices, values, n), directed=True, unweighted=values is None, indices=distinct)
    d = np.concatenate([d, np.full((len(distinct), 1), np.inf)], axis=1)  # (column n: a target of -1)
    row = {int(v): k for k, v in enumerate(distinct)}
    col = np.where(tgt >= 0, tgt, n)
    for i, v in enumerate(src.tolist()):
        if v >= 0:
            T[i] = d[row[v]][col]
    return T


def sums(T):
    """(S, C) of a hop table: the sum and the count of each row's finite cells, uint64."""
    T = np.asarray(T, dtype=np.float64)
    reached = np.isfinite(T)
    S = np.where(reached, T, 0.0).sum(axis=1).astype(np.uint64)  # (integers far below 2^53: exact)
    return S.reshape(-1), reached.sum(axis=1).astype(np.uint64).reshape(-1)


def fold(T):
    """genome_distance(method="mean") over the table, in the reference's order of additions: u outer,
    v inner, ``total = 0.0; total += d`` for every pair with a path; (total / count, count), or
    (None, 0) when no pair has one (the reference raises NetworkXNoPath)."""
    total, count = 0.0, 0
    for row in np.asarray(T, dtype=np.float64).tolist():
        for d in row:
            if d != float("inf"):
                total += d
                count += 1
    return (total / count if count else None), count


def same(a, b):
    """Bit-for-bit equality of two arrays of one dtype."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
