"""The sharded build's device primitives (HipEngine in gfa2network_amd/shard.py: g2n_dedup_keys,
g2n_partition_keys, g2n_gather_keys, g2n_order_keys, g2n_rank_keys, g2n_remap_pairs,
g2n_route_triplets, g2n_route_group_slots, g2n_csr_from_coo_pair), each driven directly with small
adversarial inputs and compared EXACTLY with its host restatement (tests/shard_cpu_engine.py
CpuEngine: dict, numpy, scipy) — the inputs the whole-file builds of tests/test_gpu_shard.py never
produce: keys past the dictionary's 16-byte inline head that differ in their tails only, empty keys
and keys holding NUL / tab / newline, heavy duplication inside one wave, unaligned coordinate
arrays, empty sources and owners, tile-edge sizes, slices with one empty stream.

The owner of a key (g2n_partition_keys) is pinned as fmix64(FNV-1a 64(bytes)) mod n_ranks: ranks on
different GPUs must agree on it.  No process is spawned and no file is read; the one CPU test checks
the key pool and the host references against plain dict / list restatements.
"""
import ctypes
import random

import numpy as np
import pytest
import scipy.sparse as sp

from shard_cpu_engine import CpuEngine
from shard_prim_util import (COLLIDING, build_pool, check_pool, distinct_keys, fnv1a64, key_hash, key_owner, pack,
                             row_bounds, stable_partition, tail_groups, unpack)

SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 5000, 70_000)
CPU = CpuEngine(None)
_POOL = []


def pool():
    if not _POOL:
        _POOL.extend(build_pool())
    return _POOL


def _t(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr))


def _dev(eng, arr):
    return _t(arr).to(eng.device)


def _np(x):
    return x.cpu().numpy()


# ------------------------------------------------------------------ the host half --
def test_key_pool_and_host_references():
    """The pool has the properties the key tests rely on; CpuEngine.dedup_keys / gather_keys agree with
    a plain dict / list (an empty blob and n = 0 included); the Python owner function leaves none of
    3 ranks empty and is the documented function of the bytes."""
    p = pool()
    check_pool(p)
    assert 1000 <= len(p) <= 2000
    assert len(tail_groups(p)) >= 50
    r = random.Random(1)
    for keys in ([], [b""], [b"", b""], p, [r.choice(p) for _ in range(4000)], [p[0]] * 70):
        blob, offs = pack(keys)
        assert unpack(blob, offs) == keys
        ids, first, nd = CPU.dedup_keys(_t(blob), _t(offs))
        seen = {}
        for i, k in enumerate(keys):
            seen.setdefault(k, (len(seen), i))
        assert ids.numpy().tolist() == [seen[k][0] for k in keys]
        assert first.numpy().tolist() == [i for _, i in seen.values()] and nd == len(seen)
        index = [r.randrange(len(keys)) for _ in range(len(keys) // 2)] if keys else []
        want = [keys[i] for i in index]
        gb, go = CPU.gather_keys(_t(blob), _t(offs), _t(np.array(index, dtype=np.int32)), sum(len(k) for k in want))
        assert unpack(gb.numpy(), go.numpy()) == want
    owners = [key_owner(k, 3) for k in p]
    assert set(owners) == {0, 1, 2}
    # pinned: FNV-1a 64 (0xaf63dc4c8601ec8c for "a") and then the finaliser, not FNV-1a alone
    assert fnv1a64(b"") == 0xCBF29CE484222325 and fnv1a64(b"a") == 0xAF63DC4C8601EC8C
    assert key_hash(b"") == 0xEFD01F60BA992926 and key_hash(b"a") == 0x82A2A958A9BECE5B
    assert key_hash(b"GRCh38#0#chr1:12x") == 0xD7F3CDE0A335AAF4
    assert [key_owner(b"a", n) for n in (1, 2, 3, 7)] == [0x82A2A958A9BECE5B % n for n in (1, 2, 3, 7)]


# ------------------------------------------------------------------------- dedup --
def _check_dedup(eng, keys, what):
    blob, offs = pack(keys)
    ids, first, nd = eng.dedup_keys(_dev(eng, blob), _dev(eng, offs))
    wi, wf, wn = CPU.dedup_keys(_t(blob), _t(offs))
    assert nd == wn, what
    assert ids.numel() == len(keys) and np.array_equal(_np(ids), wi.numpy()), what
    assert np.array_equal(_np(first), wf.numpy()), what


def _pattern(name, n, r):
    p = pool()
    if name.startswith("adjacent"):  # every key k times in adjacent positions: duplicates share a wave
        k = int(name[8:])
        return [key for key in distinct_keys(p, (n + k - 1) // k) for _ in range(k)][:n]
    if name == "then_reversed":
        seq = distinct_keys(p, (n + 1) // 2)
        r.shuffle(seq)
        return seq + seq[::-1][:n - len(seq)]
    if name == "last_is_first":
        seq = distinct_keys(p, max(n - 1, 1))
        r.shuffle(seq)
        return (seq + seq[:1])[:n]
    assert name == "random_draws"
    return [r.choice(p) for _ in range(n)]


@pytest.mark.gpu
def test_gpu_dedup_all_distinct(gpu):
    """(a) every key distinct: the S-prefix identity path (no lookup round), ids = arange."""
    from gfa2network_amd.shard import HipEngine

    eng = HipEngine(0)
    try:
        r = random.Random(2)
        for n in SIZES:
            keys = distinct_keys(pool(), n)
            r.shuffle(keys)
            _check_dedup(eng, keys, n)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("key", [b"a", b"\0", b"pan#genome#chr22" + bytes(range(56, 240))], ids=["short", "nul", "200"])
def test_gpu_dedup_one_key_repeated(gpu, key):
    """(b) one key n times (a short key, and a 200-byte key compared through tail_eq by every touch)."""
    from gfa2network_amd.shard import HipEngine

    assert len(key) in (1, 200)
    eng = HipEngine(0)
    try:
        for n in SIZES:
            _check_dedup(eng, [key] * n, n)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["adjacent2", "adjacent3", "adjacent64", "adjacent65", "then_reversed",
                                  "last_is_first", "random_draws"])
def test_gpu_dedup_duplicate_patterns(gpu, name):
    """(c) - (f): duplicates inside one wave, a sequence then its reverse, one late duplicate of the very
    first key, random draws from the pool — the first occurrence must be reported, in order."""
    from gfa2network_amd.shard import HipEngine

    eng = HipEngine(0)
    try:
        r = random.Random(name)
        for n in SIZES:
            _check_dedup(eng, _pattern(name, n, r), (name, n))
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_dedup_pool_tail_groups(gpu):
    """Keys of equal length and equal first 16 bytes that differ at or after byte 16 only (tail_eq, and
    key_hash's byte loop): every group on its own, twice over and interleaved, then all groups at once."""
    from gfa2network_amd.shard import HipEngine

    groups = list(tail_groups(pool()).values())
    eng = HipEngine(0)
    try:
        for g in groups:
            _check_dedup(eng, g + g[::-1] + g, (len(g[0]), g[0][:16]))
        allk = [k for g in groups for k in g]
        random.Random(3).shuffle(allk)
        _check_dedup(eng, allk + allk, "all groups")
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_dedup_keys_colliding_in_tag_and_slot(gpu):
    """Two keys of one 16-byte head and one length that differ at byte 16 only AND hash to the same
    tag and the same slot (shard_prim_util.COLLIDING): the second one meets the first one's entry with
    everything but the tail equal, so a tail_eq that skipped byte 16 would merge them (different hashes
    keep every other such pair apart before tail_eq runs).  Alone, both ways round, repeated, and
    among other keys, in tables of 1024 .. 4096 entries."""
    from gfa2network_amd.shard import HipEngine

    p = pool()
    others = [k for k in p if not k.startswith(b"tagcoll#")]
    eng = HipEngine(0)
    try:
        for a, b in COLLIDING:
            for keys in ([a, b], [b, a], [a, b, b, a], [a, a, b], others[:300] + [a] + others[300:600] + [b, a],
                         [b] + others[:1300] + [a], [a] * 40 + [b] * 40 + [a, b] * 40):
                assert len(keys) <= 2730  # a table of at most 4096 entries: one slot for both
                _check_dedup(eng, keys, (a, len(keys)))
        _check_dedup(eng, [k for pair in COLLIDING for k in pair] * 2, "all pairs")
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_dedup_empty_keys_and_blob_end(gpu):
    """(g) a blob whose last key is empty (its offset == the blob's length), and blobs of empty keys
    only (no blob bytes at all, n > 0)."""
    from gfa2network_amd.shard import HipEngine

    eng = HipEngine(0)
    try:
        p = pool()
        for n in (1, 2, 65, 1025):
            _check_dedup(eng, distinct_keys([k for k in p if k], n - 1) + [b""], ("last empty", n))
            _check_dedup(eng, [b""] * n, ("all empty", n))
        _check_dedup(eng, [b"", b"ab", b"", b"ab", b""], "mixed")
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_dedup_after_a_larger_call(gpu):
    """The context's arena is grow-only: after a 70 000-key call, the small ones (2, 0, 65 keys) on the
    same engine must not read what the large one left behind."""
    from gfa2network_amd.shard import HipEngine

    eng = HipEngine(0)
    try:
        r = random.Random(4)
        p = pool()
        big = distinct_keys(p, 30_000)
        _check_dedup(eng, [r.choice(big) for _ in range(70_000)], 70_000)
        _check_dedup(eng, [p[5], p[5]], 2)
        _check_dedup(eng, [], 0)
        _check_dedup(eng, [r.choice(p[:40]) for _ in range(65)], 65)
        _check_dedup(eng, distinct_keys(p, 2), "2 distinct")
    finally:
        eng.close()


# --------------------------------------------------------------------- partition --
@pytest.mark.gpu
def test_gpu_partition_keys_owner_and_order(gpu):
    """g2n_partition_keys equals the stable partition by owner = fmix64(FNV-1a 64(key)) mod n_ranks
    (Python ints), for 1 .. 4096 ranks (the limit), duplicates, empty keys and an empty input."""
    from gfa2network_amd.shard import HipEngine

    p = pool()
    r = random.Random(5)
    hashes = {k: key_hash(k) for k in p}
    inputs = {0: [], 1: [p[7]], 65: [r.choice(p) for _ in range(65)], 5000: [r.choice(p) for _ in range(5000)],
              "empty keys": [b""] * 5}
    eng = HipEngine(0)
    try:
        for n_ranks in (1, 2, 3, 7, 64, 255, 256, 257, 4096):
            for name, keys in inputs.items():
                blob, offs = pack(keys)
                oblob, ooffs, oidx, starts = eng.partition_keys(_dev(eng, blob), _dev(eng, offs), n_ranks)
                order, want_starts = stable_partition([hashes[k] % n_ranks for k in keys], n_ranks)
                what = (n_ranks, name)
                assert np.array_equal(_np(starts), want_starts), what
                assert np.array_equal(_np(oidx), order), what
                wb, wo = pack([keys[i] for i in order])
                assert np.array_equal(_np(ooffs), wo), what
                assert _np(oblob).tobytes() == wb.tobytes(), what
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_ranks", [0, 4097])
def test_gpu_partition_keys_refuses_ranks_out_of_range(gpu, n_ranks):
    from gfa2network_amd.shard import HipEngine

    eng = HipEngine(0)
    try:
        blob, offs = pack(pool()[:10])
        with pytest.raises(RuntimeError, match="G2N_E_ARG"):
            eng.partition_keys(_dev(eng, blob), _dev(eng, offs), n_ranks)
        got = eng.partition_keys(_dev(eng, blob), _dev(eng, offs), 1)  # the engine still works
        assert _np(got[0]).tobytes() == blob.tobytes() and _np(got[3]).tolist() == [0, 10]
    finally:
        eng.close()


# ------------------------------------------------------------------------ gather --
@pytest.mark.gpu
def test_gpu_gather_keys(gpu):
    """g2n_gather_keys against CpuEngine.gather_keys: the identity, reversed, repeats, nothing, and
    empty keys only (0 bytes gathered)."""
    from gfa2network_amd.shard import HipEngine

    p = pool()
    r = random.Random(6)
    keys = p[:600] + [b""]  # the blob ends with an empty key
    blob, offs = pack(keys)
    n = len(keys)
    empties = [i for i, k in enumerate(keys) if not k]
    assert len(empties) == 2
    cases = {"identity": np.arange(n), "reversed": np.arange(n)[::-1],
             "repeats": np.array([r.randrange(n) for _ in range(2 * n)] + [3, 3, 3]), "nothing": np.zeros(0),
             "empty keys": np.array(empties * 3), "one": np.array([n - 2])}
    eng = HipEngine(0)
    try:
        db, do = _dev(eng, blob), _dev(eng, offs)
        for name, index in cases.items():
            index = index.astype(np.int32)
            nbytes = int(sum(len(keys[i]) for i in index))
            assert (nbytes == 0) == (name in ("nothing", "empty keys"))
            gb, go = eng.gather_keys(db, do, _dev(eng, index), nbytes)
            wb, wo = CPU.gather_keys(_t(blob), _t(offs), _t(index), nbytes)
            assert np.array_equal(_np(go), wo.numpy()), name
            assert gb.numel() == nbytes and _np(gb).tobytes() == wb.numpy().tobytes(), name
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_gather_keys_short_buffer_is_refused_and_untouched(gpu):
    """out_cap one byte short: G2N_E_ARG, and nothing written to the output blob (include/g2n.h)."""
    import torch

    from gfa2network_amd import _native as nat
    from gfa2network_amd.shard import HipEngine

    keys = pool()[:300]
    blob, offs = pack(keys)
    index = np.arange(len(keys), dtype=np.int32)[::-1].copy()
    nbytes = len(blob)
    eng = HipEngine(0)
    try:
        db, do, di = _dev(eng, blob), _dev(eng, offs), _dev(eng, index)
        out = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=eng.device)
        ooffs = torch.empty(len(keys) + 1, dtype=torch.int64, device=eng.device)
        got = ctypes.c_uint64(0)
        eng._sync()
        rc = eng.lib.g2n_gather_keys(eng.ctx, db.data_ptr(), do.data_ptr(), di.data_ptr(), len(keys), out.data_ptr(),
                                     nbytes - 1, ooffs.data_ptr(), ctypes.byref(got))
        assert rc == nat.E_ARG and nat.status_name(rc) == "G2N_E_ARG"
        assert np.all(_np(out) == 0xA5)
        gb, go = eng.gather_keys(db, do, di, nbytes)  # the exact size is accepted
        assert _np(gb).tobytes() == b"".join(keys[::-1])
    finally:
        eng.close()


# ------------------------------------------------------------ order / rank keys --
def _order_case(counts, r, dense=False):
    """(first_of, src_idx) over sum(counts) arrivals: ascending arrivals holding the first and the last
    arrival of every non-empty source."""
    ends = np.cumsum(counts)
    total = int(ends[-1])
    must = set()
    for s, c in enumerate(counts):
        if c:
            must |= {int(ends[s]) - c, int(ends[s]) - 1}
    f = set(range(total)) if dense else must | {r.randrange(total) for _ in range(min(total, 300))}
    first_of = np.array(sorted(f), dtype=np.int32)
    src_idx = np.random.default_rng(total).integers(0, 2**32 - 1, total)  # local ids: 32 bits
    src_idx[::5] = np.resize([0, 1, 2**31 - 1, 2**31, 2**32 - 2], len(src_idx[::5]))
    return first_of, src_idx.astype(np.int64)


@pytest.mark.gpu
def test_gpu_order_keys_sources(gpu):
    """g2n_order_keys against CpuEngine.order_keys: one source, empty sources (equal ends) at the front,
    in the middle and at the end, 4096 sources (the limit) most of them empty; 0 and 4097 refused."""
    from gfa2network_amd.shard import HipEngine

    r = random.Random(7)
    many = [0] * 4096
    for s in (0, 1, 2, 77, 2047, 2048, 4000, 4095):
        many[s] = r.choice([1, 2, 300])
    many2 = list(many)
    many2[0] = many2[4095] = 0
    cases = {"one": [1], "one long": [70_000], "front": [0, 0, 3, 1, 5], "middle": [4, 0, 0, 1, 600],
             "end": [2, 9, 1, 0, 0], "all three": [0, 1, 0, 300, 0], "4096": many, "4096 empty ends": many2}
    eng = HipEngine(0)
    try:
        for name, counts in cases.items():
            for dense in (False, True):
                first_of, src_idx = _order_case(counts, r, dense)
                got = eng.order_keys(_dev(eng, first_of), _dev(eng, src_idx), counts)
                want = CPU.order_keys(_t(first_of), _t(src_idx), counts)
                assert np.array_equal(_np(got), want.numpy()), (name, dense)
                src = _np(got) >> 32
                assert set(src.tolist()) == {s for s, c in enumerate(counts) if c}, (name, dense)
        none = eng.order_keys(_dev(eng, np.zeros(0, np.int32)), _dev(eng, np.zeros(0, np.int64)), [0, 0])
        assert none.numel() == 0
        first_of, src_idx = _order_case([3], r)
        for counts in ([], [0] * 4096 + [3]):
            with pytest.raises(RuntimeError, match="G2N_E_ARG"):
                eng.order_keys(_dev(eng, first_of), _dev(eng, src_idx), counts)
    finally:
        eng.close()


def _runs(sizes, r, layout):
    """Sorted, mutually distinct int64 order keys (source << 32 | id) per owner; layout: how owner 0's
    keys lie against the others' (below all, above all, interleaved)."""
    total = sum(sizes)
    vals = sorted(r.sample(range(1, 4095 << 32), total))
    if layout == "interleaved":
        idx = list(range(total))
        r.shuffle(idx)
    else:
        rest = list(range(sizes[0], total))
        r.shuffle(rest)
        idx = list(range(sizes[0])) + rest  # owner 0 takes the smallest keys
        if layout == "above":
            idx = [total - 1 - i for i in idx]
    out, pos = [], 0
    for n in sizes:
        out.append(np.array(sorted(vals[i] for i in idx[pos:pos + n]), dtype=np.int64))
        pos += n
    return out


@pytest.mark.gpu
def test_gpu_rank_keys_owner_runs(gpu):
    """g2n_rank_keys against CpuEngine.rank_keys: one owner (arange), empty owner runs, self first / in
    the middle / last, keys below, above and between the other owners', 4096 owners (the limit)."""
    from gfa2network_amd.shard import HipEngine

    r = random.Random(8)
    wide = [0] * 4096
    for o in (0, 5, 2048, 4095):
        wide[o] = 50
    shapes = [[1], [700], [5, 0, 9, 300], [300, 0, 0, 7], [0, 40, 0, 2], [1, 1, 1, 1], [257, 256, 255, 1], wide]
    eng = HipEngine(0)
    try:
        for sizes in shapes:
            for layout in ("interleaved", "below", "above") if len(sizes) <= 4 else ("interleaved",):
                runs = _runs(sizes, r, layout)
                druns = [_dev(eng, x) for x in runs]
                selfs = range(len(sizes)) if len(sizes) <= 4 else (0, 5, 6, 4095)
                for me in selfs:
                    got = eng.rank_keys(druns[me], druns, me)
                    want = CPU.rank_keys(_t(runs[me]), [_t(x) for x in runs], me)
                    what = (sizes[:4], layout, me)
                    assert np.array_equal(_np(got), want.numpy()), what
                    if len(sizes) == 1:
                        assert np.array_equal(_np(got), np.arange(sizes[0])), what
                if len(sizes) <= 4:  # every owner's ids together: a permutation of 0 .. total - 1
                    ids = np.concatenate([_np(eng.rank_keys(druns[o], druns, o)) for o in range(len(sizes))])
                    assert np.array_equal(np.sort(ids), np.arange(sum(sizes))), (sizes, layout)
        for n_ranks, me in ((4097, 0), (4, 4)):
            runs = [np.array([o + 1], dtype=np.int64) for o in range(n_ranks)]
            with pytest.raises(RuntimeError, match="G2N_E_ARG"):
                eng.rank_keys(_dev(eng, runs[0]), [_dev(eng, x) for x in runs], me)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_src", [2, 3, 5])
def test_gpu_global_ids_composed(gpu, n_src):
    """Steps 2 - 4 of the protocol without processes: n_src sources with overlapping distinct-key lists,
    keys routed by the Python owner, GPU dedup_keys per owner on the arrivals in source order, GPU
    order_keys, GPU rank_keys over all owners' order keys — the global ids are a permutation and equal
    the first-touch order of a dict fed source 0's keys, then source 1's, ..."""
    from gfa2network_amd.shard import HipEngine

    p = pool()
    r = random.Random(n_src)
    sources = [r.sample(p, r.choice([300, 700, 1100])) for _ in range(n_src)]
    sources[-1] = sources[-1] + [k for k in sources[0][:50] if k not in set(sources[-1])]
    want = {}
    for keys in sources:
        for k in keys:
            want.setdefault(k, len(want))
    n_own = n_src
    eng = HipEngine(0)
    try:
        arrivals, okeys, firsts = [], [], []
        for o in range(n_own):
            arr, idx, counts = [], [], []
            for keys in sources:  # a source's keys arrive in its local-id order
                mine = [(k, i) for i, k in enumerate(keys) if key_owner(k, n_own) == o]
                arr += [k for k, _ in mine]
                idx += [i for _, i in mine]
                counts.append(len(mine))
            blob, offs = pack(arr)
            ids, first, nd = eng.dedup_keys(_dev(eng, blob), _dev(eng, offs))
            assert nd == len(set(arr))
            ok = eng.order_keys(first, _dev(eng, np.array(idx, dtype=np.int64)), counts)
            arrivals.append(arr)
            firsts.append(_np(first))
            okeys.append(ok.clone())
        got = {}
        for o in range(n_own):
            gids = _np(eng.rank_keys(okeys[o], okeys, o))
            for j, g in zip(firsts[o], gids):
                assert arrivals[o][j] not in got
                got[arrivals[o][j]] = int(g)
        assert sorted(got.values()) == list(range(len(want)))
        assert got == want
    finally:
        eng.close()


# ------------------------------------------------------------------------- remap --
REMAP_SIZES = (0, 1, 3, 4, 5, 7, 8, 1023, 1024, 1025, 3072, 3073, 3074, 3075)  # 4 * 256 * 3 + k
SENTINEL = -7


def _views(eng, n, o_rows, o_cols, rows, cols):
    """rows / cols as views big[o : o + n] of sentinel-filled arrays (element offset o)."""
    import torch

    bigs = [torch.full((n + 12,), SENTINEL, dtype=torch.int32, device=eng.device) for _ in range(2)]
    vr, vc = bigs[0][o_rows:o_rows + n], bigs[1][o_cols:o_cols + n]
    vr.copy_(_t(rows))
    vc.copy_(_t(cols))
    return bigs, vr, vc


def _outside_untouched(bigs, n, o_rows, o_cols):
    for big, o in zip(bigs, (o_rows, o_cols)):
        h = _np(big)
        assert np.all(h[:o] == SENTINEL) and np.all(h[o + n:] == SENTINEL)


@pytest.mark.gpu
def test_gpu_remap_pairs_aligned_and_unaligned(gpu):
    """g2n_remap_pairs against CpuEngine.remap_pairs at the vector variant's edges (n % 4 tails, one
    block and more), on 16-byte-aligned arrays (k_remap_pairs<true>) and on views at element offsets
    1 - 3 of rows, of cols and of both (k_remap_pairs<false>); nothing outside the view is written."""
    from gfa2network_amd.shard import HipEngine

    rng = np.random.default_rng(9)
    n_map = 1000
    gmap = rng.integers(0, 2**31, n_map).astype(np.int32)
    eng = HipEngine(0)
    try:
        dmap = _dev(eng, gmap)
        for n in REMAP_SIZES:
            rows = rng.integers(0, n_map, n).astype(np.int32)
            cols = rng.integers(0, n_map, n).astype(np.int32)
            if n:
                rows[-1], cols[-1] = n_map - 1, 0
            wr, wc = CPU.remap_pairs(_t(rows), _t(cols), _t(gmap))
            dr, dc = _dev(eng, rows), _dev(eng, cols)  # fresh tensors
            assert dr.data_ptr() % 16 == 0 and dc.data_ptr() % 16 == 0
            eng.remap_pairs(dr, dc, dmap)
            assert np.array_equal(_np(dr), wr.numpy()) and np.array_equal(_np(dc), wc.numpy()), n
            offsets = [(4, 8)] + [(o, 0) for o in (1, 2, 3)] + [(0, o) for o in (1, 2, 3)] + [(o, o) for o in (1, 2, 3)] \
                + [(1, 3)]
            for o_rows, o_cols in offsets:
                bigs, vr, vc = _views(eng, n, o_rows, o_cols, rows, cols)
                if n:
                    assert ((vr.data_ptr() | vc.data_ptr()) % 16 == 0) == ((o_rows, o_cols) == (4, 8))
                eng.remap_pairs(vr, vc, dmap)
                what = (n, o_rows, o_cols)
                assert np.array_equal(_np(vr), wr.numpy()) and np.array_equal(_np(vc), wc.numpy()), what
                _outside_untouched(bigs, n, o_rows, o_cols)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_remap_pairs_bad_id_contract(gpu):
    """An id equal to n_map — in the vector body, in the last n % 4 elements, and the same two places in
    the scalar variant — is refused with G2N_E_ARG; exactly the offending entries are -1, all others
    mapped; the next valid call on the same engine succeeds (the counter is per call)."""
    from gfa2network_amd.shard import HipEngine

    rng = np.random.default_rng(10)
    n_map, n = 500, 4 * 256 * 3 + 3
    gmap = rng.integers(0, 2**31, n_map).astype(np.int32)
    eng = HipEngine(0)
    try:
        dmap = _dev(eng, gmap)
        for o_rows, o_cols in ((4, 8), (1, 0), (0, 3), (2, 2)):
            for place, in_rows in ((1031, True), (n - 1, False), (n - 3, True)):  # the body; the n % 4 tail
                rows = rng.integers(0, n_map, n).astype(np.int32)
                cols = rng.integers(0, n_map, n).astype(np.int32)
                wr, wc = (x.numpy().copy() for x in CPU.remap_pairs(_t(rows), _t(cols), _t(gmap)))
                (rows if in_rows else cols)[place] = n_map
                (wr if in_rows else wc)[place] = -1
                bigs, vr, vc = _views(eng, n, o_rows, o_cols, rows, cols)
                what = (o_rows, o_cols, place)
                with pytest.raises(RuntimeError, match="G2N_E_ARG"):
                    eng.remap_pairs(vr, vc, dmap)
                assert np.array_equal(_np(vr), wr) and np.array_equal(_np(vc), wc), what
                _outside_untouched(bigs, n, o_rows, o_cols)
                rows[place] = cols[place] = n_map - 1  # a valid call next
                wr, wc = CPU.remap_pairs(_t(rows), _t(cols), _t(gmap))
                bigs, vr, vc = _views(eng, n, o_rows, o_cols, rows, cols)
                eng.remap_pairs(vr, vc, dmap)
                assert np.array_equal(_np(vr), wr.numpy()) and np.array_equal(_np(vc), wc.numpy()), what
    finally:
        eng.close()


# ------------------------------------------------------------------------- route --
ROUTE_N = (1, 63, 64, 65, 1023, 1024, 1025, 16383, 16384, 16385, 32769)


def _route_rows(dist, n, n_global, n_ranks, rng):
    """The routed rows of a distribution (ids below n_global)."""
    b = row_bounds(n_global, n_ranks)
    if dist == "uniform":
        return rng.integers(0, n_global, n)
    if dist == "rank 0":
        return rng.integers(0, max(b[1], 1), n)
    if dist == "last rank":
        return rng.integers(min(b[n_ranks - 1], n_global - 1), n_global, n)
    assert dist == "last row"
    return np.full(n, n_global - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("n_ranks", [1, 2, 3, 255, 256, 257])
def test_gpu_route_triplets_small_shapes(gpu, n_ranks):
    """g2n_route_triplets at the ballot and tile edges (n of 1, 63 .. 65, 1023 .. 1025, 16383 .. 16385,
    32769), with every row owned by rank 0 / by the last rank, n_global below n_ranks (owners without
    rows, repeated bounds), rows equal to n_global - 1; map, transposition and the value width rotate
    over the cases.  Reference: numpy's stable partition by floor(row * R / n_global)."""
    from gfa2network_amd.shard import HipEngine

    rng = np.random.default_rng(n_ranks)
    shapes = [("uniform", 100_003), ("rank 0", 100_003), ("last rank", 100_003), ("last row", 100_003),
              ("uniform", 1), ("uniform", 2), ("uniform", max(n_ranks - 1, 1)), ("last row", max(n_ranks - 1, 1)),
              ("uniform", n_ranks)]
    combos = [(m, t, dt) for dt in ("float64", "int8", None) for t in (False, True) for m in (False, True)]
    eng = HipEngine(0)
    maps = {}
    try:
        count = 0
        for n in ROUTE_N:
            for dist, n_global in shapes:
                use_map, transposed, dt = combos[count % len(combos)]
                count += 1
                r = _route_rows(dist, n, n_global, n_ranks, rng).astype(np.int64)
                c = rng.integers(0, n_global, n).astype(np.int64)
                assert r.min() >= 0 and r.max() < n_global
                data = None if dt is None else rng.integers(-100, 100, n).astype(dt)
                a, b = (c, r) if transposed else (r, c)  # what the kernel reads as rows / cols
                dmap = None
                if use_map:
                    if n_global not in maps:
                        perm = rng.permutation(n_global).astype(np.int32)
                        inv = np.empty(n_global, dtype=np.int64)
                        inv[perm] = np.arange(n_global)
                        maps[n_global] = (_dev(eng, perm), inv)
                    dmap, inv = maps[n_global]
                    a, b = inv[a], inv[b]
                order, starts = stable_partition(r * n_ranks // n_global, n_ranks)
                rr, cc, dd, st = eng.route_triplets(_dev(eng, a.astype(np.int32)), _dev(eng, b.astype(np.int32)),
                                                    None if data is None else _dev(eng, data), dt or "float64", dmap,
                                                    n_global, n_ranks, transposed)
                what = (n, dist, n_global, use_map, transposed, dt)
                assert np.array_equal(_np(st), starts), what
                assert np.array_equal(_np(rr), r[order]) and np.array_equal(_np(cc), c[order]), what
                if data is None:
                    assert dd is None
                else:
                    assert _np(dd).tobytes() == data[order].tobytes(), what
            count += 2  # 11 per n: every shape meets 11 of the 12 combinations
        assert count >= 8 * len(combos)
    finally:
        eng.close()


def _slot_shard(rows, cols, n_trip, gcount, n_groups, gcap):
    from gfa2network_amd.shard import LocalShard

    return LocalShard(status=0, err_line=-1, err_index=-1, err_value=0.0, err_detail=b"", warn_line=-1,
                      has_warning=False, warn_byte=0, n_lines=0, n_records=0, n_records_before_error=0, n_edges=0,
                      n_local_nodes=0, rows=rows, cols=cols, slots=(gcount.data_ptr(), n_groups, gcap), n_trip=n_trip)


@pytest.mark.gpu
@pytest.mark.parametrize("n_ranks", [1, 3, 256])
def test_gpu_route_group_slots_synthetic_layout(gpu, n_ranks):
    """g2n_route_group_slots on slots built here: group counts of 0, 1, gcap - 1 and gcap, a gcap of 1,
    below, at and across the 16384-element tile, all counts zero; every slot's unused tail holds the
    valid id 0 (no live entry does), so a read past a group's count shows as a wrong count, never as an
    out-of-range access.  Expected: the stable partition of the live entries in group order."""
    from gfa2network_amd.shard import HipEngine

    rng = np.random.default_rng(100 + n_ranks)
    n_global = 1000
    eng = HipEngine(0)
    try:
        for n_groups in (1, 3, 17):
            for gcap in (1, 100, 16384, 16385, 40000):
                choices = [0, 1, gcap - 1, gcap]
                for variant, transposed in (("mixed", False), ("mixed", True), ("full", False), ("zero", True)):
                    if variant == "mixed":
                        gcount = np.array([choices[(g + n_groups + transposed) % 4] for g in range(n_groups)])
                        if n_groups > 4:
                            gcount = rng.permutation(gcount)
                    else:
                        gcount = np.full(n_groups, gcap if variant == "full" else 0)
                    rows = np.zeros(n_groups * gcap, dtype=np.int32)  # dead tails: row 0, column 0
                    cols = np.zeros(n_groups * gcap, dtype=np.int32)
                    live = np.concatenate([np.arange(g * gcap, g * gcap + gcount[g]) for g in range(n_groups)])
                    live = live.astype(np.int64)
                    rows[live] = rng.integers(1, n_global, len(live))
                    cols[live] = rng.integers(1, n_global, len(live))
                    r, c = rows[live].astype(np.int64), cols[live].astype(np.int64)
                    if transposed:
                        r, c = c, r
                    order, starts = stable_partition(r * n_ranks // n_global, n_ranks)
                    dg = _dev(eng, gcount.astype(np.int32))
                    sh = _slot_shard(_dev(eng, rows), _dev(eng, cols), len(live), dg, n_groups, gcap)
                    rr, cc, dd, st = eng.route_slots(sh, n_global, n_ranks, transposed)
                    what = (n_groups, gcap, variant, transposed, gcount.tolist())
                    assert dd is None and rr.numel() == len(live) and cc.numel() == len(live), what
                    assert np.array_equal(_np(st), starts), what
                    assert np.array_equal(_np(rr), r[order]) and np.array_equal(_np(cc), c[order]), what
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_route_group_slots_refuses_the_sort_path(gpu):
    """Group slots route to at most 256 ranks (include/g2n.h): 257 is G2N_E_ARG."""
    from gfa2network_amd.shard import HipEngine

    eng = HipEngine(0)
    try:
        z = _dev(eng, np.ones(8, dtype=np.int32))
        sh = _slot_shard(z, z, 2, _dev(eng, np.array([1, 1], dtype=np.int32)), 2, 4)
        with pytest.raises(RuntimeError, match="G2N_E_ARG"):
            eng.route_slots(sh, 10, 257, False)
    finally:
        eng.close()


# ---------------------------------------------------------------------- csr_pair --
def _coo_cases():
    """name -> (n_global, rows, cols): small global COOs in stream order."""
    rng = np.random.default_rng(11)
    out = {}
    n = 3000
    r = rng.integers(0, n, 20_000)
    c = rng.integers(0, n, 20_000)
    r[r % 7 == 3] += 1  # rows = 3 mod 7 have no entries (nor those columns for MAX-SYM's transpose: kept)
    r = np.minimum(r, n - 2)
    r[:400], c[:400] = 17, rng.integers(0, n, 400)  # a hub row
    r[400:800], c[400:800] = c[1000:1400], r[1000:1400]  # (r, c) and (c, r)
    r[800:1000] = c[800:1000]  # the diagonal
    r[1400:1500], c[1400:1500] = 5, 9  # one (r, c) a hundred times
    r[1500:1510], c[1500:1510] = 9, 5
    perm = rng.permutation(20_000)
    out["random 3000"] = (n, r[perm], c[perm])
    n = 50
    hub = np.concatenate([np.full(20, 3), rng.integers(0, n, 20)])
    hc = np.concatenate([np.arange(20) * 2, rng.integers(0, n, 20)])
    out["hub 50"] = (n, hub, hc)
    out["first row 50"] = (n, np.zeros(40, dtype=np.int64), rng.integers(40, 50, 40))
    out["last row 50"] = (n, np.full(40, 49), np.concatenate([rng.integers(0, 10, 39), [49]]))
    out["one entry 50"] = (n, np.array([20]), np.array([31]))
    out["empty 50"] = (n, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    out["diagonal 2"] = (2, np.array([0, 1, 1, 0] * 10), np.array([0, 1, 0, 0] * 10))
    out["one entry 2"] = (2, np.array([1]), np.array([0]))
    out["empty 2"] = (2, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    out["forty 1"] = (1, np.zeros(40, dtype=np.int64), np.zeros(40, dtype=np.int64))
    out["one entry 1"] = (1, np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64))
    out["empty 1"] = (1, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    for n, r, c in out.values():
        assert len(r) in (0, 1, 40, 20_000) and n in (1, 2, 50, 3000)
    n, r, c = out["random 3000"]
    assert np.bincount(r, minlength=n).max() > 16 and (np.bincount(r, minlength=n) == 0).any() and (r == c).any()
    return out


def _check_csr_slices(eng, dtype, uniform, seen):
    NP = {"bool": np.bool_, "int8": np.int8, "int32": np.int32, "float32": np.float32, "float64": np.float64}[dtype]
    rng = np.random.default_rng(12)
    for name, (n, r, c) in _coo_cases().items():
        vals = np.ones(len(r), dtype=NP) if uniform else rng.integers(-3, 4, len(r)).astype(NP)
        M = sp.coo_matrix((vals, (r, c)), shape=(n, n)).tocsr()
        for maxsym in (0, 1):
            W = M.maximum(M.T).tocsr() if maxsym else M
            assert W.has_sorted_indices
            for n_ranks in (1, 2, 3, 5):
                b = row_bounds(n, n_ranks)
                for k in range(n_ranks):
                    base, n_rows = b[k], b[k + 1] - b[k]
                    ina = (r >= base) & (r < b[k + 1])  # the slice's A stream, and A.T's: numpy's stable partition
                    inT = (c >= base) & (c < b[k + 1])

                    def stream(x, y, m):
                        return (_dev(eng, x[m].astype(np.int32)), _dev(eng, y[m].astype(np.int32)),
                                None if uniform else _dev(eng, vals[m]))

                    a = stream(r, c, ina)
                    ways = [stream(c, r, inT)] if maxsym else [None]
                    if maxsym and n_ranks == 1:  # one rank that routed nothing: A's own arrays, swapped
                        ways.append((a[1], a[0], a[2]))
                    an, tn = int(ina.sum()), int(inT.sum()) if maxsym else 0
                    rows_in = np.concatenate([r[ina], c[inT]] if maxsym else [r[ina]])
                    if n_rows == 0:
                        seen.add("no rows")
                    elif an + tn == 0:
                        seen.add("empty slice")
                    elif an == 0:
                        seen.add("only A.T")
                    if n_rows > 1 and len(rows_in) and (rows_in == base).all():
                        seen.add("first row only")
                    if n_rows > 1 and len(rows_in) and (rows_in == base + n_rows - 1).all():
                        seen.add("last row only")
                    lo, hi = W.indptr[base], W.indptr[base + n_rows]
                    for j, t in enumerate(ways):
                        if j:
                            seen.add("self_t")
                        indptr, indices, data, _, _ = eng.csr_pair(a, t, bool(maxsym), base, n_rows, n, dtype,
                                                                   uniform, -1)
                        what = (name, dtype, uniform, maxsym, n_ranks, k, j)
                        assert np.array_equal(_np(indptr), W.indptr[base:base + n_rows + 1] - lo), what
                        assert np.array_equal(_np(indices), W.indices[lo:hi]), what
                        want = W.data[lo:hi].astype(np.uint8 if dtype == "bool" else NP)
                        assert _np(data).dtype == want.dtype and _np(data).tobytes() == want.tobytes(), what


CSR_BRANCHES = {"no rows", "empty slice", "only A.T", "first row only", "last row only", "self_t"}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bool", "int8", "int32", "float32", "float64"])
def test_gpu_csr_pair_uniform_slices(gpu, dtype):
    """g2n_csr_from_coo_pair without values (every value dtype(1)): for 1, 2, 3 and 5 row slices of small
    global COOs (duplicates, the diagonal, (r, c) with (c, r), a hub row, empty rows, n_global below
    the slice count), each slice's CSR equals rows [base, base + n_rows) of scipy's coo.tocsr() and of
    M.maximum(M.T) bit for bit.  The slices include an empty one, one with A.T entries only, one
    without rows, entries in the first / the last row only, and one rank's swapped-arrays A.T."""
    from gfa2network_amd.shard import HipEngine

    eng = HipEngine(0)
    seen = set()
    try:
        _check_csr_slices(eng, dtype, True, seen)
        assert seen == CSR_BRANCHES
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int32", "float32", "float64"])
def test_gpu_csr_pair_weighted_slices(gpu, dtype):
    """The same slices with values in [-3, 3] (zero included): the sums are exact in any order, so the
    slice's own sort verdict (force_unsorted = -1) is enough and the comparison stays bit-exact."""
    from gfa2network_amd.shard import HipEngine

    eng = HipEngine(0)
    seen = set()
    try:
        _check_csr_slices(eng, dtype, False, seen)
        assert seen == CSR_BRANCHES
    finally:
        eng.close()
