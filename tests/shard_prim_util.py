"""Inputs and host references for tests/test_gpu_shard_primitives.py — TEST INFRASTRUCTURE.

The adversarial key pool the key primitives share (g2n_dedup_keys, g2n_partition_keys,
g2n_gather_keys), the owner function of g2n_partition_keys in Python ints, and numpy stable
partitions.  Nothing here needs a GPU; only tests import it.
"""
from __future__ import annotations

import random

import numpy as np

M64 = (1 << 64) - 1
TAIL_LENS = (1, 7, 8, 9, 31, 32, 33, 200)  # bytes past the 16-byte inline head of a dictionary entry
GROUPS_PER_TAIL = 7
SPECIALS = (b"", b"\0", b"\0\0", b"a", b"a\0")  # one zero-padded 16-byte head, different lengths
PREFIX16 = b"GRCh38#0#chr1:12"  # 16 bytes; the pool holds its first 15, all 16, and 17 bytes
MARKED = (b"a\tb", b"a\nb", b"S\t1\n", b"x:+", b"\t", b"\n", b":", b"\xff", b"\x80\xfe\xc3\xa9",
          b"HG002#1#chr6\t:\n\x80", b"HG002#1#chr6:2997\t+\n\xe2\x82\xac", b"CHM13#0#chrX:1-2\xff\n\t:tail")


# Pairs of 17-byte keys with one 16-byte head that differ at byte 16 only and whose dictionary hashes
# (dict_key_hash) agree in the 32-bit tag and in the low 12 bits, i.e. in the slot of any table of up
# to 4096 entries: the second key of a pair probes the first one's entry with an equal tag, an equal
# head and an equal length, so tail_eq alone tells them apart.  Found by search (2^44 pairs each);
# check_pool asserts the property.
COLLIDING = tuple(
    (b"tagcoll#" + hi.to_bytes(8, "little") + bytes([b1]), b"tagcoll#" + hi.to_bytes(8, "little") + bytes([b2]))
    for hi, b1, b2 in ((0x1E1E02352D0C3AA3, 141, 150), (0xAAAA8BF2B125EF9C, 30, 172), (0xF6F6CCB91FA3B3BF, 115, 116)))


def dict_key_hash(key: bytes) -> int:
    """The device dictionary's hash of a key (key_hash in g2n_kernels.hip, not bidirected): the
    zero-padded 16-byte head and the length mixed, FNV-1a steps over the bytes past 16, fmix64.  An
    entry's tag is its high 32 bits, its slot the low bits."""
    head = key[:16].ljust(16, b"\0")
    lo, hi = int.from_bytes(head[:8], "little"), int.from_bytes(head[8:], "little")
    h = (lo * 0x9E3779B97F4A7C15) & M64
    m = (hi * 0xC2B2AE3D27D4EB4F) & M64
    h ^= ((m << 31) & M64) | (m >> 33)
    h ^= (len(key) * 0x165667B19E3779F9) & M64
    for b in key[16:]:
        h = ((h ^ b) * 0x100000001B3) & M64
    return fmix64(h)


def fnv1a64(key: bytes) -> int:
    h = 0xCBF29CE484222325
    for b in key:
        h = ((h ^ b) * 0x100000001B3) & M64
    return h


def fmix64(k: int) -> int:
    """MurmurHash3's 64-bit finaliser."""
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & M64
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & M64
    k ^= k >> 33
    return k


def key_hash(key: bytes) -> int:
    """What g2n_partition_keys reduces mod n_ranks (k_key_owner): fmix64(FNV-1a 64 of the bytes)."""
    return fmix64(fnv1a64(key))


def key_owner(key: bytes, n_ranks: int) -> int:
    return key_hash(key) % n_ranks


def tail_groups(pool):
    """Groups of >= 2 pool keys of equal length > 16 and equal first 16 bytes: {(head, len): [keys]}."""
    g = {}
    for k in pool:
        if len(k) > 16:
            g.setdefault((k[:16], len(k)), []).append(k)
    return {h: v for h, v in g.items() if len(v) >= 2}


def check_pool(pool) -> None:
    """The properties the key tests rely on (the issue's list), asserted."""
    s = set(pool)
    assert len(s) == len(pool), "pool keys are distinct"
    assert all(k in s for k in SPECIALS)
    assert {PREFIX16[:15], PREFIX16, PREFIX16 + b"x"} <= s
    for a, b in COLLIDING:
        assert a in s and b in s and len(a) == len(b) == 17 and a[:16] == b[:16] and a[16] != b[16]
        ha, hb = dict_key_hash(a), dict_key_hash(b)
        assert ha != hb and ha >> 32 == hb >> 32 and ha & 0xFFF == hb & 0xFFF
    groups = tail_groups(pool)
    assert len(groups) >= 50, len(groups)
    for tl in TAIL_LENS:
        mine = [v for (h, n), v in groups.items() if n == 16 + tl]
        assert len(mine) >= GROUPS_PER_TAIL, tl
        # members differing at byte 16 only, and at the last byte only
        assert any(any(a[:16] == b[:16] and a[17:] == b[17:] and a[16] != b[16] for a in v for b in v) for v in mine)
        assert any(any(a[:-1] == b[:-1] and a[-1] != b[-1] for a in v for b in v) for v in mine), tl
    for v in groups.values():
        assert all(a[:16] == b[:16] and len(a) == len(b) and a[16:] != b[16:] for a in v for b in v if a is not b)
    for ch in (b"\t", b"\n", b":"):
        assert any(ch in k for k in pool)
        assert any(ch in k[16:] for k in pool), "also past the inline head"
    assert any(max(k) >= 0x80 for k in pool if k) and any(k[16:] and max(k[16:]) >= 0x80 for k in pool)
    assert {len(k) for k in pool} >= set(range(40))


def build_pool(seed: int = 20260) -> list:
    """About 1500 distinct byte keys at the edges of the device dictionary (module docstring)."""
    r = random.Random(seed)
    rb = lambda n: bytes(r.randrange(256) for _ in range(n))  # noqa: E731
    keys = list(SPECIALS) + [PREFIX16[:15], PREFIX16, PREFIX16 + b"x"] + list(MARKED) + [k for p in COLLIDING for k in p]
    for tl in TAIL_LENS:
        for g in range(GROUPS_PER_TAIL):
            head = (b"grp%02d#%03d#chr" % (g, tl) + rb(16))[:16]
            tail = bytearray(rb(tl))
            group = [bytes(tail)]
            for pos in {0, tl // 2, tl - 1}:  # byte 16, the middle, the last byte
                t2 = bytearray(tail)
                t2[pos] ^= 1 + r.randrange(255)
                group.append(bytes(t2))
            if tl > 1:  # two places at once
                t2 = bytearray(tail)
                t2[0] ^= 0x20
                t2[-1] ^= 0x01
                group.append(bytes(t2))
            keys += [head + t for t in group]
    for n in range(40):
        keys += [rb(n) for _ in range(28)]
    pool = list(dict.fromkeys(keys))
    r.shuffle(pool)
    check_pool(pool)
    return pool


_HEAD = b"pan#genome#chr22"  # 16 bytes


def distinct_keys(pool, n: int) -> list:
    """n distinct keys: the pool, then short names, keys sharing one 16-byte head whose tails differ
    in 4 bytes, and 39-byte keys of that head that differ in their last 3 bytes only."""
    out = list(pool[:n])
    for i in range(len(out), n):
        if i % 3 == 0:
            out.append(b"n%d" % i)
        elif i % 3 == 1:
            out.append(_HEAD + i.to_bytes(4, "little"))
        else:
            out.append(_HEAD + bytes(20) + i.to_bytes(3, "big"))
    assert len(set(out)) == n
    return out


def pack(keys):
    """(blob uint8, offsets int64 of len(keys) + 1): the keys back to back, no separator."""
    offs = np.zeros(len(keys) + 1, dtype=np.int64)
    if keys:
        np.cumsum([len(k) for k in keys], out=offs[1:])
    return np.frombuffer(b"".join(keys), dtype=np.uint8).copy(), offs


def unpack(blob, offs) -> list:
    b = np.asarray(blob, dtype=np.uint8).tobytes()
    return [b[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


def stable_partition(owner, n_ranks: int):
    """(order, starts) of numpy's stable partition by owner: order[j] = the input index of output j,
    starts[k] = the first output of owner k (starts[n_ranks] = n)."""
    owner = np.asarray(owner, dtype=np.int64)
    order = np.argsort(owner, kind="stable")
    starts = np.searchsorted(owner[order], np.arange(n_ranks + 1))
    return order, starts


def row_bounds(n_global: int, n_ranks: int) -> list:
    """The protocol's row bounds: rank k owns rows [ceil(k n / R), ceil((k + 1) n / R))."""
    return [(k * n_global + n_ranks - 1) // n_ranks for k in range(n_ranks + 1)]
