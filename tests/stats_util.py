"""Checkers shared by the GPU statistics tests: scipy's connected_components and numpy degree /
edge counts over a CSR structure (the reference itself is not needed for them)."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components


def csr_of(rows, cols, n):
    """The CSR structure of the entries (rows[k], cols[k]) in the given order within each row."""
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    order = np.argsort(rows, kind="stable")
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    return indptr, cols[order]


def checker(indptr, indices, n, directed):
    nnz = len(indices)
    lens = np.diff(indptr)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    diag = np.zeros(n, dtype=np.int64)
    diag[rows[rows == indices]] = 1
    nd = int(diag.sum())
    if directed:
        edges, deg = nnz, lens + np.bincount(indices, minlength=n)
    else:
        edges, deg = (nnz + nd) // 2, lens + diag
    comps = 0
    if n:
        comps = int(connected_components(sp.csr_matrix((np.ones(nnz, dtype=np.int8), indices, indptr), shape=(n, n)),
                                         directed=False, return_labels=False))
    dens = 0 if edges == 0 or n <= 1 else (edges / (n * (n - 1))) * (1 if directed else 2)
    return {"nodes": n, "edges": edges, "components": comps, "max_degree": int(deg.max()) if n else 0,
            "density": dens}
