"""Host checkers for the weighted graph matrix (``graph_matrix``, the LAST finish) and for the
reference's order of additions in ``genome_distance_matrix(method="mean")``.

The matrix is a dict-overwrite loop over the records, as ``G.add_edge`` behaves in the reference's
builder: a record with a numeric weight sets the edge's value, a record without one leaves an
existing value alone and creates the edge with 1.0.  Distances come from scipy's Dijkstra
(``wdist_util``)."""
import numpy as np
from scipy.sparse.csgraph import dijkstra

import wdist_util


def last_cells(records, directed: bool) -> dict:
    """{(u, v): value} after the records (u, v, w) in order; w None = no numeric weight tag."""
    cells: dict = {}
    for u, v, w in records:
        for key in ((u, v),) if directed else ((u, v), (v, u)):
            if w is not None:
                cells[key] = float(w)
            else:
                cells.setdefault(key, 1.0)
    return cells


def cells_csr(cells: dict, n: int):
    """(indptr int32, indices int32, data float64): columns ascending within a row."""
    keys = sorted(cells)
    indptr = np.zeros(n + 1, dtype=np.int32)
    for u, _v in keys:
        indptr[u + 1] += 1
    np.cumsum(indptr, out=indptr)
    return (indptr, np.array([v for _u, v in keys], dtype=np.int32),
            np.array([cells[k] for k in keys], dtype=np.float64))


def last_csr(records, n: int, directed: bool):
    return cells_csr(last_cells(records, directed), n)


def same_csr(A, want) -> bool:
    """A scipy CSR against (indptr, indices, data): dtypes and bytes."""
    ip, ix, d = want
    return (A.format == "csr" and A.dtype == np.float64 and A.data.dtype == np.float64 and
            A.shape == (len(ip) - 1,) * 2 and
            np.asarray(A.indptr, dtype=np.int32).tobytes() == ip.tobytes() and
            np.asarray(A.indices, dtype=np.int32).tobytes() == ix.tobytes() and A.data.tobytes() == d.tobytes())


def tag_value(fields, tag: bytes):
    """The numeric value of a record's last ``tag`` field (``i`` / ``f`` typed), or None."""
    w = None
    for f in fields:
        parts = f.split(b":", 2)
        if len(parts) == 3 and parts[0] == tag:
            w = None
            try:
                if parts[1] == b"i":
                    w = float(int(parts[2]))
                elif parts[1] == b"f":
                    w = float(parts[2])
            except ValueError:
                w = None
    return w


def link_records(data: bytes, tag: bytes):
    """(node names in first-touch order, records (u, v, w)) of a file of plain S and L lines — the
    shape of tests/golden/wdist_inputs and of the generators here; other record kinds are skipped."""
    ids: dict = {}
    records = []
    for line in data.split(b"\n"):
        f = line.split(b"\t")
        if f[0] == b"S" and len(f) > 1:
            ids.setdefault(f[1], len(ids))
        elif f[0] == b"L" and len(f) >= 6:
            u = ids.setdefault(f[1], len(ids))
            v = ids.setdefault(f[3], len(ids))
            records.append((u, v, tag_value(f[6:], tag)))
    return list(ids), records


def node_distances(csr, n: int, paths):
    """d[i][v]: the distance from path i's steps to node v (inf: not reached; None for an empty path)."""
    G = wdist_util.graph(*csr, n)
    out = []
    for p in paths:
        p = np.asarray(p, dtype=np.int64).reshape(-1)
        out.append(dijkstra(G, directed=True, indices=np.unique(p), min_only=True) if len(p) else None)
    return out


def reference_mean(csr, n: int, paths) -> np.ndarray:
    """genome_distance_matrix(method="mean") in the reference's order of additions: one running total
    per cell i < j from 0.0 — path i's steps against path j's distances, then path j's steps against
    path i's —, divided by the count; both triangles, inf without a reached step, 0.0 on the diagonal."""
    d = node_distances(csr, n, paths)
    K = len(paths)
    M = np.zeros((K, K), dtype=np.float64)
    inf = float("inf")
    for i in range(K):
        for j in range(i + 1, K):
            total, count = 0.0, 0
            for steps, lengths in ((paths[i], d[j]), (paths[j], d[i])):
                if lengths is None:
                    continue
                for x in lengths[np.asarray(steps, dtype=np.int64)].tolist():
                    if x != inf:
                        total += x
                        count += 1
            M[i, j] = M[j, i] = total / count if count else inf
    return M


# ------------------------------------------------------------------ shape generators ------
def _cell(rng, col, copies):
    """`copies` records of one cell: untagged and tagged interleaved, the last tagged one neither the
    cell's first nor its last record when there are three or more."""
    if copies == 1:
        return [(col, int(rng.integers(0, 1000)) if rng.random() < 0.7 else None)]
    if copies == 2:
        return [(col, int(rng.integers(0, 1000))), (col, None)]
    ws = [int(rng.integers(0, 1000)) if rng.random() < 0.5 else None for _ in range(copies)]
    ws[0] = None
    ws[-1] = None
    ws[copies - 2] = int(rng.integers(0, 1000))
    return [(col, w) for w in ws]


def _row(rng, n, length, distinct):
    """`length` records over `distinct` columns, shuffled (each cell keeps its own order)."""
    cols = rng.choice(n, size=distinct, replace=False).tolist()
    counts = [1] * distinct
    for _ in range(length - distinct):
        counts[int(rng.integers(0, distinct))] += 1
    cells = [_cell(rng, c, k) for c, k in zip(cols, counts)]
    out = []
    while cells:
        k = int(rng.integers(0, len(cells)))
        out.append(cells[k].pop(0))
        if not cells[k]:
            cells.pop(k)
    return out


def shape_records(scale: int = 1, seed: int = 7):
    """(n, records (u, v, w)) holding every row shape of the LAST finish (g2n_kernels.hip k_row_finish<RowLast>):
    rows of 1, 2, 8, 9, 16, 17 and 33 triplets (both sides of the 8-wide network and of kRegRow = 16),
    rows whose columns arrive descending (12: the network sorts, 20: the merge runs), one cell 40 times
    inside a 60-entry row, a cell of untagged records only, a 256-row block of 9-entry rows (2304
    entries: past kStageSumW = 2048, unstaged) beside block 0 (staged), and a hub row of 5000 / scale
    triplets over 50 columns.  The rows' records are interleaved at random, each row's order kept."""
    rng = np.random.default_rng(seed)
    n = 600
    rows = {}
    for r, length in enumerate((1, 2, 8, 9, 16, 17, 33)):
        rows[r] = _row(rng, n, length, max(1, length - length // 3))
    rows[7] = [(c, int(rng.integers(0, 1000))) for c in range(420, 400, -1)]
    rows[8] = [(c, None if c % 3 == 0 else int(rng.integers(0, 1000))) for c in range(312, 300, -1)]
    rows[9] = _cell(rng, 77, 40) + _row(rng, 70, 20, 20)
    rng.shuffle(rows[9])
    rows[10] = [(5, None), (6, None), (5, None)]  # cells without any numeric tag: 1.0
    rows[11] = [(11, 0), (11, None), (12, None), (12, 0), (12, None)]  # an explicit zero stays stored
    per = 9 if scale == 1 else 2
    for r in range(256, 512):
        rows[r] = _row(rng, n, per, per - 2 if per > 2 else per)
    rows[520] = _row(rng, n, 5000 // scale, 50)
    queues = {r: list(v) for r, v in rows.items()}
    order = [r for r, v in queues.items() for _ in v]
    rng.shuffle(order)
    records = [(r, *queues[r].pop(0)) for r in order]
    return n, records


def dec_names(n):
    return [str(k + 1).encode() for k in range(n)]


def hashed_names(n):
    """Names no decimal or prefix + decimal pattern describes: letters only."""
    out = []
    for k in range(n):
        s, k = b"", k + 26
        while k:
            s = bytes([97 + k % 26]) + s
            k //= 26
        out.append(b"n" + s)
    return out


def gfa_bytes(names, records, tag=b"RC", float_at=None, paths=()):
    """S lines in order, then one L line a record (``tag:i:w`` when it has a weight; record
    ``float_at`` spelled ``tag:f:w.0``: a spelling only the general weight parse takes), then P lines."""
    out = [b"S\t" + nm + b"\t*\n" for nm in names]
    for k, (u, v, w) in enumerate(records):
        line = b"L\t" + names[u] + b"\t+\t" + names[v] + b"\t+\t0M"
        if w is not None:
            line += b"\t" + tag + (b":f:%d.0" % w if k == float_at else b":i:%d" % w)
        out.append(line + b"\n")
    for name, steps in paths:
        out.append(b"P\t" + name + b"\t" + b",".join(names[s] + b"+" for s in steps) + b"\t*\n")
    return b"".join(out)
