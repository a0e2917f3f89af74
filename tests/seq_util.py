"""The CPU checker of the sequence-distance tests: the reference's rules for a node's sequence
(parser.py:135-163, builders.py:164-189) restated over the file's bytes, and the search as scipy's
unweighted multi-source Dijkstra over the CPU oracle's CSR.  The reference itself is not needed."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import dijkstra


def node_sequences(data: bytes) -> dict:
    """name -> sequence: the last S record of the name that has one wins."""
    out = {}
    for line in data.split(b"\n"):
        f = line.split(b"\t")
        if f[0] != b"S" or len(f) < 3:
            continue
        try:
            int(f[2])
        except ValueError:
            out[f[1]] = f[2]
            continue
        if len(f) > 3:
            p = f[3].split(b":", 2)
            if not (len(p) == 3 and len(p[0]) == 2 and len(p[1]) == 1):
                out[f[1]] = f[3]
    return out


def seq_nodes(data: bytes, names: list, seq: bytes) -> list:
    """The ids (ascending = node order) of the nodes, named names[id], whose sequence is seq."""
    seqs = node_sequences(data)
    return [i for i, n in enumerate(names) if seqs.get(n) == seq]


def distance(indptr, indices, n: int, ids_a, ids_b, directed: bool):
    """Fewest hops from a node of ids_a to a node of ids_b over the CSR structure (an edge u -> v per
    stored entry; both ways when not directed); None when none is reached."""
    G = sp.csr_matrix((np.ones(len(indices), dtype=np.int8), np.asarray(indices, dtype=np.int64),
                       np.asarray(indptr, dtype=np.int64)), shape=(n, n))
    d = dijkstra(G, directed=directed, unweighted=True, indices=np.unique(np.asarray(ids_a, dtype=np.int64)),
                 min_only=True)[np.asarray(ids_b, dtype=np.int64)]
    return int(d.min()) if np.isfinite(d).any() else None


def oracle_names(o) -> list:
    blob, offs = o.names_blob.tobytes(), o.names_offsets
    return [blob[offs[i]:offs[i + 1]] for i in range(o.n_nodes)]
