"""CPU: the count rule of the MAX-SYM finish in place (k_sym_count, g2n_sym.hip), restated in numpy,
against scipy's A.maximum(A.T).

The finish partitions the entries of an unweighted COO by the high bits of their row into buckets
of 2^low rows.  An entry (a, b) whose two rows share a bucket travels as ONE pair word and gives the
cells (a, b) and (b, a); any other entry gives the element (a, b) to a's bucket and (b, a) to b's.
The count pass must know a bucket's merged cells without sorting it:

  * pair words: one bit per key (min << low | max) of the rows inside the bucket, in a map of
    2^(2 low) bits; a new key counts two cells, one when a == b;
  * the other elements have their column outside the bucket, so they never meet a pair word's
    cell: counted as distinct (row, column).

For dtypes whose sums of ones never reach zero (every one but int8) that is the bucket's nnz.
"""
import numpy as np
import pytest
import scipy.sparse as sp

LOWS = (1, 4, 6, 7, 8)


def count_rule(rows, cols, n, low):
    """per-bucket cell counts by the device's rule (buckets holding rows: ceil(n / 2^low))"""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    n_bk = (n + (1 << low) - 1) >> low
    out = np.zeros(n_bk, np.int64)
    m = (1 << low) - 1
    pair = (rows >> low) == (cols >> low)
    # pair words: the key map of each bucket
    pa, pb, bk = rows[pair] & m, cols[pair] & m, rows[pair] >> low
    lo, hi = np.minimum(pa, pb), np.maximum(pa, pb)
    key = (lo << low) | hi
    assert key.size == 0 or key.max() < 1 << (2 * low)
    maps = np.zeros((n_bk, 1 << (2 * low)), bool) if n_bk << (2 * low) <= 1 << 26 else None
    if maps is not None:
        for b, k, l, h in zip(bk, key, lo, hi):  # in stream order, as the atomics see them
            if not maps[b, k]:
                maps[b, k] = True
                out[b] += 2 if l != h else 1
    else:
        u = np.unique(np.stack([bk, key]), axis=1)
        l, h = u[1] >> low, u[1] & m
        np.add.at(out, u[0], np.where(l != h, 2, 1))
    # the elements that leave: (row, column) in the row's bucket, both directions
    r = np.concatenate([rows[~pair], cols[~pair]])
    c = np.concatenate([cols[~pair], rows[~pair]])
    if r.size:
        assert np.all((r >> low) != (c >> low))  # never a pair word's cell
        u = np.unique(np.stack([r, c]), axis=1)
        np.add.at(out, u[0] >> low, 1)
    return out


def scipy_counts(rows, cols, n, low):
    A = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n)).tocsr()
    M = A.maximum(A.T).tocsr()
    M.eliminate_zeros()
    per_row = np.diff(M.indptr)
    n_bk = (n + (1 << low) - 1) >> low
    pad = np.zeros(n_bk << low, np.int64)
    pad[:n] = per_row
    return pad.reshape(n_bk, 1 << low).sum(axis=1)


def _random_coo(rng, n, n_e, local):
    a = rng.integers(0, n, n_e)
    b = np.where(rng.random(n_e) < local, np.clip(a + rng.integers(-3, 4, n_e), 0, n - 1), rng.integers(0, n, n_e))
    return a, b


@pytest.mark.parametrize("low", LOWS)
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000, 1003])
def test_random_coos(low, n):
    rng = np.random.default_rng(1000 * low + n)
    for n_e, local in ((0, 1.0), (1, 1.0), (3 * n, 0.95), (3 * n, 0.0), (8 * n, 0.5)):
        a, b = _random_coo(rng, n, n_e, local)
        assert np.array_equal(count_rule(a, b, n, low), scipy_counts(a, b, n, low)), (n_e, local)


@pytest.mark.parametrize("low", LOWS)
def test_adversarial_coos(low):
    n = 3 * (1 << low) + 5  # not a multiple of the bucket: a partial last bucket
    w = 1 << low
    last = n - 1
    rows, cols = [], []

    def add(a, b, k=1):
        rows.extend([a] * k)
        cols.extend([b] * k)

    add(0, 0)                 # a self-loop alone
    add(1 % n, 1 % n, 7)      # ... and repeated
    add(last, last, 2)        # in the partial bucket
    add(w, w + 1)             # (a, b) with (b, a), inside one bucket
    add(w + 1, w)
    add(w, w + 1, 3)          # repeated links, the reverse fewer times
    add(w - 1, w)             # neighbours across a bucket boundary, both directions
    add(w, w - 1, 2)
    add(0, last, 300)         # a far link repeated, its reverse once
    add(last, 0)
    add(2 * w, last)          # two rows of one bucket to the same far column
    add(2 * w + 1, last)
    add(last, 2 * w)          # ... whose A.T entry is already a cell
    for a in range(n):        # every row's first and last in-bucket neighbour
        add(a, (a >> low) << low)
        add(a, min(((a >> low) << low) + w - 1, last))
    assert np.array_equal(count_rule(rows, cols, n, low), scipy_counts(rows, cols, n, low))


def test_key_map_is_exact_at_its_width():
    """every key of a full bucket is its own bit: 2^low rows, all pairs once"""
    for low in (1, 4, 6):
        w = 1 << low
        a, b = np.divmod(np.arange(w * w), w)
        got = count_rule(a + w, b + w, 3 * w, low)  # the middle bucket
        assert got.tolist() == [0, w * w, 0]
        assert np.array_equal(got, scipy_counts(a + w, b + w, 3 * w, low))
