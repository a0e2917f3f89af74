"""Cases for the hash dictionary tiers at their thresholds — TEST INFRASTRUCTURE, CPU only.

The three open-addressing tables that turn names into first-touch node ids (the lean S-first hash,
the classic tiers of build_dictionary, the chunked build's key set) are driven by
tests/test_gpu_dict_edges.py with the inputs built here; tests/test_dict_cases.py shows on the CPU
that every input sits where its name says.  This module restates, in plain Python, what the device
computes and what the host decides:

* the hashes (dict_key_hash of shard_prim_util for the dictionary, ks_hash for the key set) and
  numpy forms of both, used to search names with a wanted tag and home slot;
* first_touch(): builders.py's dict semantics — the reference every case is compared with;
* the geometry: lean_cap, classic_caps, ks_cap, in_lean_shape, the lean premises and the tier a
  build must end in (expected_tier), the number of tables it must initialise (expected_table_inits).

The constants are read from g2n_pipeline.hip / g2n_kernels.hip / g2n_keyset.hip and restated, not
imported.  Importing the module costs nothing; cases() and keyset_scripts() are cached and cost about
8 s of CPU the first time (three searches of 2^23 hashes, a pool of 2^17 names, one bisection), which
the two test modules pay once each at collection.  Every searched name is made of letters only: no
tab, newline, ':' or digit (the host's first-line guesses then choose neither the decimal nor the
direct tier).
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from shard_prim_util import COLLIDING, M64, dict_key_hash, fnv1a64

ROUTES = ("lean", "classic", "general")  # TEST_DICT_HASH; TEST_DICT_HASH | TEST_NO_HASH_LEAN; TEST_DICT_GENERAL
Case = namedtuple("Case", "name lines tiers expect_retry family")

_U = np.uint64
_ALPHA = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEF", dtype=np.uint8)
MIN_CAP = 1024       # the smallest table of every tier
PROBE_BOUND = 4096   # build_dictionary's probe bound below full_cap
LEAN_LINE = 48       # lean_edge_names: bytes of an edge line before its newline
INLINE = 16          # key bytes held in a DictEntry


# ------------------------------------------------------------------ hashes ------
def bidir_key(name: bytes, ori: bytes) -> bytes:
    """key_head / touch_byte with bidir: the name's bytes, ':' at byte len(name), then the orientation."""
    return name + b":" + ori


def ks_hash(key: bytes) -> int:
    """g2n_keyset.hip ks_hash: FNV-1a 64, then h ^ h >> 29; tag = high 32 bits, slot = h & mask."""
    h = fnv1a64(key)
    return h ^ (h >> 29)


def tag_slot(h: int, cap: int):
    return h >> 32, h & (cap - 1)


def fmix64_np(k):
    k = k.astype(_U, copy=True)
    k ^= k >> _U(33)
    k *= _U(0xFF51AFD7ED558CCD)
    k ^= k >> _U(33)
    k *= _U(0xC4CEB9FE1A85EC53)
    k ^= k >> _U(33)
    return k


def dict_hash_np(lo, hi, length: int):
    """dict_key_hash of keys of at most 16 bytes, given as their two little-endian words."""
    lo, hi = np.asarray(lo, dtype=_U), np.asarray(hi, dtype=_U)
    h = lo * _U(0x9E3779B97F4A7C15)
    m = hi * _U(0xC2B2AE3D27D4EB4F)
    h = h ^ ((m << _U(31)) | (m >> _U(33)))
    h = h ^ _U((length * 0x165667B19E3779F9) & M64)
    return fmix64_np(np.broadcast_to(h, np.broadcast(lo, hi).shape))


def ks_hash_np(words, length: int = 8):
    """ks_hash of keys of `length` <= 8 bytes, given as little-endian words."""
    words = np.asarray(words, dtype=_U)
    h = np.full(words.shape, 0xCBF29CE484222325, dtype=_U)
    for j in range(length):
        h = (h ^ ((words >> _U(8 * j)) & _U(0xFF))) * _U(0x100000001B3)
    return h ^ (h >> _U(29))


def words8(prefix3: bytes, n: int):
    """n eight-byte names as little-endian words: a 3-letter prefix, then 5 letters spelling the index."""
    assert len(prefix3) == 3 and n <= 1 << 25
    i = np.arange(n, dtype=np.int64)
    w = np.full(n, int.from_bytes(prefix3, "little"), dtype=_U)
    for k in range(5):
        w |= _ALPHA[(i >> (5 * k)) & 31].astype(_U) << _U(8 * (3 + k))
    return w


def _name(w) -> bytes:
    return int(w).to_bytes(8, "little")


def _equal_tag_slot(h, slot_bits: int = 10):
    """Index pairs of h that agree in the 32-bit tag and the low slot_bits bits, in index order."""
    key = ((h >> _U(32)) << _U(slot_bits)) | (h & _U((1 << slot_bits) - 1))
    order = np.argsort(key, kind="stable")
    ks = key[order]
    at = np.nonzero(ks[1:] == ks[:-1])[0]
    return sorted((int(min(order[j], order[j + 1])), int(max(order[j], order[j + 1]))) for j in at)


FIXED_HI = b"#fixedHI"  # the other half of the 16-byte names of tag_pairs("lo") / ("hi")
FIXED_LO = b"fixedLO#"
SEARCH = 1 << 23


@functools.lru_cache(maxsize=None)
def tag_pairs(kind: str):
    """Pairs of names with equal dictionary tag and equal home slot in a table of 1024:
    "lo": 16-byte names that differ in their low word only; "hi": in their high word only;
    "byte16": 17-byte names with one 16-byte head (COLLIDING, its pairs free of ':', 12 slot bits)."""
    if kind == "byte16":
        return tuple(p for p in COLLIDING if not any(c in k for k in p for c in b"\t\n:"))
    w = words8(b"seg", SEARCH)
    if kind == "lo":
        h = dict_hash_np(w, _U(int.from_bytes(FIXED_HI, "little")), 16)
        return tuple((_name(w[a]) + FIXED_HI, _name(w[b]) + FIXED_HI) for a, b in _equal_tag_slot(h))
    assert kind == "hi"
    h = dict_hash_np(_U(int.from_bytes(FIXED_LO, "little")), w, 16)
    return tuple((FIXED_LO + _name(w[a]), FIXED_LO + _name(w[b])) for a, b in _equal_tag_slot(h))


# One name whose zero-padded forms of 10 and of 13 bytes share the dictionary tag: equal tag and equal 16-byte
# head, so the entry's length is all that tells them apart.  (The length is hashed: found by a search of 2^31
# eight-letter names x the 36 pairs of lengths 8 .. 16, about a minute — kept as a constant, asserted in
# tests/test_dict_cases.py.)  Their home slots differ; padded_chain() lays S names on every slot between.
PADDED = (b"lysqlcaa" + b"\0" * 2, b"lysqlcaa" + b"\0" * 5)


def padded_chain():
    """(the S name, the absent name, filler S names): the absent name's walk from its home slot in a table of
    1024 passes one filler per slot and then meets the S name's entry."""
    absent, s_name = PADDED
    a, b = dict_key_hash(absent) & (MIN_CAP - 1), dict_key_hash(s_name) & (MIN_CAP - 1)
    return s_name, absent, [homed((a + j) % MIN_CAP, 1)[0] for j in range((b - a) % MIN_CAP)]


@functools.lru_cache(maxsize=None)
def ks_tag_pairs():
    """Pairs of 8-byte keys with equal key-set tag, length and home slot in a table of 1024.  (Random bytes:
    FNV-1a sends names that differ by a few letters to a lattice whose points share no tag.)"""
    w = np.unique(np.random.default_rng(20261).integers(0, 1 << 63, SEARCH, dtype=np.int64).astype(_U))
    return tuple((_name(w[a]), _name(w[b])) for a, b in _equal_tag_slot(ks_hash_np(w)))


@functools.lru_cache(maxsize=None)
def _pool(which: str):
    """2^17 eight-byte names, grouped by their home slot in a table of 1024: {slot: [names]}."""
    w = words8(b"chn" if which == "dict" else b"ksp", 1 << 17)
    h = dict_hash_np(w, _U(0), 8) if which == "dict" else ks_hash_np(w)
    slot = (h & _U(MIN_CAP - 1)).astype(np.int64)
    order = np.argsort(slot, kind="stable")
    starts = np.searchsorted(slot[order], np.arange(MIN_CAP + 1))
    return [[_name(w[j]) for j in order[starts[s]:starts[s + 1]]] for s in range(MIN_CAP)], [_name(x) for x in w]


def homed(slot: int, k: int, which: str = "dict", skip: int = 0) -> list:
    """k names whose home slot in a table of 1024 is `slot` (dictionary hash, or the key set's)."""
    names = _pool(which)[0][slot % MIN_CAP][skip:skip + k]
    assert len(names) == k, (slot, k)
    return names


def plain_names(n: int, which: str = "dict", start: int = 0) -> list:
    """n distinct pool names in index order (homes as they fall)."""
    return _pool(which)[1][start:start + n]


# ------------------------------------------------------------------ the first-touch model ------
def _fields(line: bytes):
    return line.rstrip(b"\n").split(b"\t")


def _link(f):
    """(u, ori_u, v, ori_v) of an L line's fields, as the reference reads them: a third field of "+" or "-" makes
    fields 1 - 4 the two names and orientations; otherwise fields 1 and 2 each carry their orientation as a last
    byte ("+" when it is neither), and every trailing '+' / '-' is stripped from the name."""
    if f[2] in (b"+", b"-"):
        return f[1], f[2], f[3], f[4]
    ou = f[1][-1:] if f[1][-1:] in (b"+", b"-") else b"+"
    ov = f[2][-1:] if f[2][-1:] in (b"+", b"-") else b"+"
    return f[1].rstrip(b"+-"), ou, f[2].rstrip(b"+-"), ov


def touch_stream(lines, bidirected: bool, keep: bool = True):
    """[(key, is_s_touch)] in the order builders.py mints: an S line its name (bidirected:
    name:+ then name:-), an edge line u then v (bidirected without keep: then v:flip, u:flip)."""
    flip = {b"+": b"-", b"-": b"+"}
    out = []
    for line in lines:
        f = _fields(line)
        if f[0] == b"S":
            out += [(k, True) for k in ((f[1] + b":+", f[1] + b":-") if bidirected else (f[1],))]
        elif f[0] == b"L":
            u, ou, v, ov = _link(f)
            if not bidirected:
                out += [(u, False), (v, False)]
                continue
            out += [(bidir_key(u, ou), False), (bidir_key(v, ov), False)]
            if not keep:
                out += [(bidir_key(v, flip[ov]), False), (bidir_key(u, flip[ou]), False)]
    return out


def first_touch(lines, bidirected: bool, keep: bool = True):
    """(node keys in id order, [(id_u, id_v)] of every matrix entry pair minted in stream order): the id
    of a key is the rank of its first touch — a Python dict's insertion order."""
    ids: dict = {}
    edge_ids = []
    for key, is_s in touch_stream(lines, bidirected, keep):
        if key not in ids:
            ids[key] = len(ids)
        if not is_s:
            edge_ids.append(ids[key])
    return list(ids), list(zip(edge_ids[0::2], edge_ids[1::2]))


def blob_of(keys) -> bytes:
    return b"".join(keys)


# ------------------------------------------------------------------ geometry restated from the host ------
def lean_cap(n_s: int) -> int:
    """lean_tier_build (the hash tier): the smallest power of two >= 1024 with cap * 67 >= n_s * 100."""
    cap = MIN_CAP
    while cap * 67 < n_s * 100:
        cap *= 2
    return cap


def classic_caps(n_st: int, n_et: int):
    """build_dictionary's first table and its retry table, from the S and the edge touches."""
    full = MIN_CAP
    while full < 2 * (n_st + n_et):
        full *= 2
    est = n_st + (n_et // 2 if n_st * 32 < n_et else n_et // 16) + 1024
    cap = MIN_CAP
    while cap < est + est // 2:
        cap *= 2
    return min(cap, full), full


def ks_cap(n_before: int, n_call: int, cap_before: int) -> int:
    """keyset_rehash as keyset_add calls it: load <= 1/2 even if every key of the call is new."""
    if n_call == 0:
        return cap_before
    cap = cap_before or MIN_CAP
    while cap < 2 * (n_before + n_call):
        cap *= 2
    return cap


def n_touches(lines, bidirected: bool = False, keep: bool = True):
    ts = touch_stream(lines, bidirected, keep)
    n_st = sum(1 for _k, s in ts if s)
    return n_st, len(ts) - n_st


def in_lean_shape(line: bytes) -> bool:
    """lean_edge_names: at most 48 bytes before the newline, at least 5 tabs, one-byte +/- orientations."""
    body = line.rstrip(b"\n")
    f = body.split(b"\t")
    return len(body) <= LEAN_LINE and len(f) >= 6 and f[2] in (b"+", b"-") and f[4] in (b"+", b"-")


def _shared_tag_met(keys, cap: int) -> bool:
    """Distinct keys claimed in order into a table of cap slots: does a probe chain meet another key's
    equal tag?  (Keys sharing a home slot always meet, whichever claims first.)"""
    table = {}
    for k in dict.fromkeys(keys):
        tag, s = tag_slot(dict_key_hash(k), cap)
        while s in table:
            if table[s][0] == tag:
                return True
            s = (s + 1) % cap
        table[s] = (tag, k)
    return False


def table_layout(keys, cap: int) -> dict:
    """{slot: key} after claiming the distinct keys in order (the occupied SET does not depend on the order)."""
    table = {}
    for k in dict.fromkeys(keys):
        s = dict_key_hash(k) & (cap - 1)
        while s in table:
            s = (s + 1) % cap
        table[s] = k
    return table


def broken_premises(lines) -> list:
    """The lean S-first hash tier's premises that an input breaks (the tier hashes plain names in every mode)."""
    recs = [_fields(x) for x in lines]
    s_names = [f[1] for f in recs if f[0] == b"S"]
    if not s_names:
        return ["s_lines"]
    out = []
    seen_edge = False
    for f in recs:
        seen_edge |= f[0] == b"L"
        if f[0] == b"S" and seen_edge:
            out.append("s_first")
            break
    if len(set(s_names)) != len(s_names):
        out.append("unique_names")
    if _shared_tag_met(s_names, lean_cap(len(s_names))):  # (of the distinct names)
        out.append("unique_tags")
    edges = [f for f in recs if f[0] == b"L"]
    if not all(in_lean_shape(x) for x, f in zip(lines, recs) if f[0] == b"L"):
        out.append("shape")
    if not all(n in set(s_names) for f in edges for n in (_link(f)[0], _link(f)[2])):  # (whatever the line's shape)
        out.append("defined")
    if any(f[0] not in (b"H", b"S", b"L", b"P") or (f[0] == b"P" and len(f) < 3) for f in recs):
        out.append("records")
    return out


def _classic_tier(lines, bidirected: bool, keep: bool) -> str:
    """build_dictionary: the S-first fast path holds when every key an edge touches was first touched by an
    S line, and no S touch was deferred for good (a shared tag met: its loser walks to an empty slot)."""
    ts = touch_stream(lines, bidirected, keep)
    first = {}
    for j, (k, s) in enumerate(ts):
        first.setdefault(k, (j, s))
    if any(not first[k][1] for k, s in ts if not s):
        return "general"
    s_keys = [k for k, s in ts if s]
    n_st, n_et = n_touches(lines, bidirected, keep)
    if _shared_tag_met(s_keys, classic_caps(n_st, n_et)[0]):
        return "general"
    return "either" if len(set(s_keys)) != len(s_keys) else "fast"  # a repeated S name: the claim race decides


def expected_tier(lines, route: str, bidirected: bool = False, keep: bool = True) -> str:
    """lean | fast | general | either: where a build of `lines` must end on a route."""
    if route == "general":
        return "general"
    if route == "lean" and not broken_premises(lines):
        return "lean"
    return _classic_tier(lines, bidirected, keep)


def longest_run(table: dict, cap: int) -> int:
    """The longest run of occupied slots (cyclic) of a table_layout."""
    if len(table) >= cap:
        return cap
    start = next(s for s in range(cap) if s not in table)
    best = run = 0
    for j in range(1, cap + 1):
        run = run + 1 if (start + j) % cap in table else 0
        best = max(best, run)
    return best


def expect_retry(lines, bidirected: bool = False, keep: bool = True):
    """Do the general rounds overflow their first table?  True with more distinct keys than slots; False when
    every key finds a slot within the probe bound wherever the races put the others (the occupied slots do
    not depend on the order: no walk is longer than the longest run of them, plus one); None when the bound
    of 4096 may or may not trip — a table past 4096 slots filled to the brim."""
    n_st, n_et = n_touches(lines, bidirected, keep)
    cap, full = classic_caps(n_st, n_et)
    keys = first_touch(lines, bidirected, keep)[0]
    if cap >= full:
        return False
    if len(keys) > cap:
        return True
    return False if cap <= PROBE_BOUND or longest_run(table_layout(keys, cap), cap) < PROBE_BOUND else None


def expected_table_inits(lines, route: str, bidirected: bool = False, keep: bool = True):
    """How many table_init phases the build reports, or None where a race decides the tier."""
    tier = expected_tier(lines, route, bidirected, keep)
    if tier == "either":
        return None
    n = 1 if route == "lean" and any(_fields(x)[0] == b"S" for x in lines) else 0  # lean_tier_build's hash table
    if tier == "lean":
        return n
    n += 1 if route != "general" else 0  # the S-first attempt
    if tier == "general":
        retry = expect_retry(lines, bidirected, keep)
        if retry is None:
            return None
        n += 1 + int(retry)
    return n


# ------------------------------------------------------------------ the cases ------
def S(name: bytes, seq: bytes = b"*") -> bytes:
    return b"S\t" + name + b"\t" + seq + b"\n"


def L(a: bytes, oa: bytes, b: bytes, ob: bytes, ov: bytes = b"0M") -> bytes:
    return b"L\t" + a + b"\t" + oa + b"\t" + b + b"\t" + ob + b"\t" + ov + b"\n"


def L2(a: bytes, oa: bytes, b: bytes, ob: bytes) -> bytes:
    """A GFA2-style link: the orientation is the last byte of each name field (five fields: the reference rejects an L
    record of fewer)."""
    return b"L\t" + a + oa + b"\t" + b + ob + b"\t*\t*\n"


H = b"H\tVN:Z:1.0\n"
HEAD16 = b"pangenome#chrom_"  # 16 bytes
A_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 18, 31, 32, 33, 40)
A_GROUPS = (  # equal in their first 16 bytes
    (HEAD16 + b"x", HEAD16 + b"y"),                          # byte 16 is the last byte
    (HEAD16 + b"Pqrstuvw", HEAD16 + b"Qqrstuvw"),            # differ at byte 16 only
    (HEAD16 + b"tailtaiA", HEAD16 + b"tailtaiB"),            # differ at the last byte only
    (HEAD16[:15], HEAD16, HEAD16 + b"x"),                    # 16 bytes beside its 15-byte prefix and 17-byte extension
    (b"a", b"a\0", b"a\0\0"),                                # equal only after zero padding
)
BIDIR_LENGTHS = (13, 14, 15, 16, 17)  # ':' or the orientation byte on byte 15, 16 or 17 of the key


def _len_name(n: int) -> bytes:
    return (b"len" + bytes([ord("A") + n % 26]) * 40)[:n]


def _a_names():
    names = [b"first"] + [_len_name(n) for n in A_LENGTHS] + [k for g in A_GROUPS for k in g]
    return list(dict.fromkeys(names))


def _pair_edges(names, lo: int, hi: int):
    out, flip = [], 0
    for a in names:
        for b in names:
            if lo <= len(a) + len(b) <= hi:
                out.append(L(a, b"+-"[flip & 1:][:1], b, b"+-"[(flip >> 1) & 1:][:1]))
                flip += 1
    return out


def _family_a():
    names = _a_names()
    s = [H] + [S(n, b"ACGT") for n in names]
    path = [b"P\tpath\t" + names[1] + b"+," + names[2] + b"-\t*\n"]
    yield "A_lengths_0_to_40_links_la+lb<=38_lean", s + path + _pair_edges(names, 0, 38)
    yield "A_one_link_la+lb=39_past_the_lean_shape", s + _pair_edges(names, 0, 38)[:50] + [L(_len_name(31), b"+", _len_name(8), b"-")]
    yield "A_links_of_names_33_and_40_classic", s + _pair_edges(names, 66, 80)
    b = [b"first"] + [_len_name(n) for n in BIDIR_LENGTHS] + [b"ab", b"ab:+", b"x:y"]
    sb = [H] + [S(n) for n in b]
    both = [L(x, o1, y, o2) for x in b for y in b for o1 in (b"+", b"-") for o2 in (b"+", b"-")]
    yield "A_bidir_names_13_to_17_and_colon_names_lean", sb + both
    g = b[:-2]  # (a GFA2 field strips every trailing '+' / '-': names ending in one are another case's)
    yield "A_bidir_names_13_to_17_gfa2_style_classic", [H] + [S(n) for n in g] + [
        L2(x, o1, y, o2) for x in g for y in g for o1 in (b"+", b"-") for o2 in (b"+", b"-")]


CHAIN_SLOT = 500
FILLERS = tuple(range(100, 120))  # home slots far from every chain


def _fillers():
    return [b"first"] + [homed(s, 1)[0] for s in FILLERS]


def _family_b():
    for k in (2, 3, 64, 65):
        c = homed(CHAIN_SLOT, k)
        yield f"B_chain_of_{k}_on_slot_{CHAIN_SLOT}_cap_1024", [H] + [S(n) for n in _fillers() + c] + [
            L(c[0], b"+", c[-1], b"-"), L(c[-1], b"+", c[0], b"+"), L(c[-1], b"-", c[-1], b"-"), L(c[0], b"+", b"first", b"+")]
    c = homed(CHAIN_SLOT, 65)
    mid, past = homed(CHAIN_SLOT + 30, 1)[0], homed(CHAIN_SLOT, 1, skip=65)[0]
    base = [H] + [S(n) for n in _fillers() + c] + [L(c[0], b"+", c[-1], b"-")]
    yield "B_absent_key_homed_inside_the_chain_of_65", base + [L(mid, b"+", c[3], b"-"), L(c[-1], b"+", c[0], b"+")]
    yield "B_absent_key_walks_the_whole_chain_of_65", base + [L(c[5], b"+", past, b"-"), L(c[-1], b"+", c[0], b"+")]
    w = homed(MIN_CAP - 2, 3) + homed(MIN_CAP - 1, 2) + homed(0, 2)
    wrap = [H] + [S(n) for n in _fillers() + w]
    yield "B_chain_from_slot_cap-2_wraps_past_slot_0", wrap + [L(a, b"+", b, b"-") for a in w for b in (w[0], w[-1])]
    yield "B_absent_key_homed_at_cap-1_walks_across_the_end", wrap + [
        L(w[0], b"+", homed(MIN_CAP - 1, 1, skip=2)[0], b"-"), L(w[-1], b"+", w[0], b"+")]


def _family_c():
    for kind in ("lo", "hi", "byte16"):
        x, y = tag_pairs(kind)[0]
        f = [H] + [S(n) for n in _fillers()]
        yield f"C_two_S_names_share_tag_and_slot_{kind}", f + [S(x), S(y), L(x, b"+", y, b"-"), L(y, b"+", x, b"+"),
                                                              L(b"first", b"+", y, b"+")]
        yield f"C_edge_names_the_partner_of_an_S_name_{kind}", f + [S(x), L(x, b"+", y, b"-"), L(y, b"-", b"first", b"+"),
                                                                    L(x, b"+", x, b"+")]
        yield f"C_both_of_a_pair_named_by_one_edge_only_{kind}", f + [L(b"first", b"+", b"first", b"-"), L(x, b"+", y, b"-"),
                                                                      L(y, b"+", x, b"+")]
    s_name, absent, fill = padded_chain()
    yield "C_edge_names_an_S_name_zero_padded_to_another_length_equal_tag", [H, S(b"first")] + [S(n) for n in fill] + [
        S(s_name), L(absent, b"+", b"first", b"-"), L(s_name, b"-", absent, b"+")]
    x = tag_pairs("lo")[0][0]
    yield "C_repeated_S_name_the_claim_race_decides", [H] + [S(n) for n in _fillers()] + [S(x), S(x), L(x, b"+", b"first", b"-")]


def _edge_file(n_s: int, n_lines: int, n_new: int):
    """n_s S lines, then n_lines links whose 2 n_lines touches name n_new names no S line defines (each
    first named in turn), the S names otherwise."""
    names = plain_names(n_s + n_new)
    s, new = ([b"first"] + names[1:n_s]) if n_s else [], names[n_s:]
    touch = new + [(s or new)[j % len(s or new)] for j in range(2 * n_lines - n_new)]
    assert len(touch) == 2 * n_lines
    return [H] + [S(n) for n in s] + [L(touch[2 * j], b"+-"[j & 1:][:1], touch[2 * j + 1], b"+") for j in range(n_lines)]


D_C16 = (100, 1600)  # S lines, links: est = 100 + 3200 / 16 + 1024 -> cap 2048, full_cap 8192


def _family_d():
    for n_s in (686, 687, 1372, 1373):  # lean_cap flips after 686 and after 1372
        names = [b"first"] + plain_names(n_s)[1:]
        yield f"D_lean_{n_s}_S_lines_cap_{lean_cap(n_s)}", [H] + [S(n) for n in names] + [
            L(names[(7 * j) % n_s], b"+-"[j & 1:][:1], names[(13 * j + 5) % n_s], b"+") for j in range(300)]
    cap = classic_caps(D_C16[0], 2 * D_C16[1])[0]
    for d, what in ((-1, "cap-1"), (0, "cap_full_table"), (1, "cap+1_retry")):
        yield f"D_classic_16th_branch_keys_{what}", _edge_file(D_C16[0], D_C16[1], cap + d - D_C16[0])
    yield "D_classic_half_branch_100_S_3202_edge_touches_fits", _edge_file(100, 1601, cap + 1 - D_C16[0])
    yield "D_classic_half_branch_L_only_4200_lines_retry", _edge_file(0, 4200, 8400)
    n = half_branch_fit()  # the neighbour that just fits: the most lines whose every walk stays within the probe bound
    yield f"D_classic_half_branch_L_only_{n}_lines_longest_run_below_the_probe_bound", _edge_file(0, n, 2 * n)
    # 8192 keys in 8192 slots: a full table whose last claims may walk past the probe bound (retry or not: the races decide)
    yield "D_classic_half_branch_L_only_4096_lines_full_table", _edge_file(0, 4096, 8192)


def _l_only_run(n_lines: int) -> int:
    return longest_run(table_layout(plain_names(2 * n_lines), 8192), 8192)


@functools.lru_cache(maxsize=None)
def half_branch_fit() -> int:
    """The largest L-only file of distinct names (2 keys a line, cap 8192) in which no run of occupied slots
    reaches the probe bound: more keys only lengthen the runs, so a bisection finds it."""
    lo, hi = 3000, 4096  # (fits, does not)
    assert _l_only_run(lo) < PROBE_BOUND <= _l_only_run(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _l_only_run(mid) < PROBE_BOUND else (lo, mid)
    return lo


E_TAILS = (0, 1, 7, 8, 23, 24, 25)  # bytes between the last S name's end and the input's end


def _e_names(tag: bytes):
    return [(tag + b"abcdefghijklmnopqrstuvwxyz")[:n] if n else b"" for n in range(18)]


def _family_e():
    for pad in range(8):  # the H line's length moves every name through the 8 alignment phases
        names = [b"first"] + _e_names(bytes([ord("A") + pad]))
        head = [b"H\t" + b"x" * pad + b"\n"]
        yield f"E_names_0_to_17_bytes_H_pad_{pad}_S_only", head + [S(n) for n in names]
        yield f"E_names_0_to_17_bytes_H_pad_{pad}_L_before_S", head + [L(names[16], b"+", names[3], b"-")] + [S(n) for n in names]
    for nl in (5, 16, 17):
        for d in E_TAILS:
            last = (b"last_name_of_the_file")[:nl]
            end = b"S\t" + last + (b"" if d == 0 else b"\n" if d == 1 else b"\t" + b"A" * (d - 1))
            body = [S(b"first"), S(b"second_name")]
            yield f"E_last_S_name_of_{nl}_ends_{d}_before_the_end_S_only", [H] + body + [end]
            yield f"E_last_S_name_of_{nl}_ends_{d}_before_the_end_L_before_S", [H, L(last, b"+", b"first", b"-")] + body + [end]


@functools.lru_cache(maxsize=None)
def cases():
    """Every GFA case: (name, lines, {route: expected tier of the plain build}, expect_retry, family)."""
    out = []
    for fam, gen in (("A", _family_a), ("B", _family_b), ("C", _family_c), ("D", _family_d), ("E", _family_e)):
        for name, lines in gen():
            lines = tuple(lines)
            out.append(Case(name, lines, {r: expected_tier(lines, r) for r in ROUTES}, expect_retry(lines), fam))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


def name_spans(lines):
    """(offset, length) of every S name in the input."""
    out, at = [], 0
    for x in lines:
        if x[:2] == b"S\t":
            out.append((at + 2, len(_fields(x)[1])))
        at += len(x)
    return out


# ------------------------------------------------------------------ F. the key set ------
KS_CHAIN_SLOT = 300
KS_CAPS = {  # the table after each call of a script that sits on a growth threshold (ks_cap restates the rule)
    "F_512_keys_fill_the_first_table": [1024, 1024, 2048],  # (the last call: 512 + 212 known keys still grow it)
    "F_513_keys_grow_to_2048": [1024, 2048, 2048],
    "F_1024_then_1025_keys": [1024, 2048, 4096, 4096],
    "F_rehash_that_adds_no_key": [1024, 2048, 2048, 2048],
}


def ks_empty_slot(cap: int = MIN_CAP) -> int:
    return ks_hash(b"") & (cap - 1)


def keyset_scripts():
    """{name: [(label, keys of one call)]}: each script starts from an empty set; the keys of one call are
    distinct (the chunked build's contract)."""
    P = plain_names(2100, "ks")
    (a1, b1), (a2, b2) = ks_tag_pairs()[:2]
    e = ks_empty_slot()
    chain = homed(KS_CHAIN_SLOT, 40, "ks")
    wrap = homed(MIN_CAP - 2, 3, "ks") + homed(MIN_CAP - 1, 3, "ks") + homed(0, 2, "ks")
    around_empty = homed(e - 1, 2, "ks") + homed(e, 2, "ks")
    out = {}
    # growth exactly at 2 (n_set + n_call) > cap, at 1024 and at 2048
    out["F_512_keys_fill_the_first_table"] = [("300 new", P[:300]), ("212 new: 512 = cap / 2, no growth", P[300:512]),
                                              ("all 512 again", P[:512][::-1][:212])]
    out["F_513_keys_grow_to_2048"] = [("300 new", [b""] + P[:299]), ("213 new: 513, growth", P[299:512]),
                                      ("found after the growth", [b""] + P[:511][::-1][:100])]
    out["F_1024_then_1025_keys"] = [("512 new", P[:512]), ("512 new: 1024 = 2048 / 2", P[512:1024]),
                                    ("1 new: growth to 4096", [b""]), ("all found", P[:1024][::3] + [b""])]
    # a call of known keys only that still forces the rehash: 400 + 200 > 512 with nothing to add
    out["F_rehash_that_adds_no_key"] = [("400 new", [b""] + P[:399]), ("200 known keys: growth, no new key", P[:199] + [b""]),
                                        ("every earlier key, its id kept", [b""] + P[:399]), ("then new ones", P[399:420])]
    # equal tag + length + slot
    out["F_equal_tag_pair_in_one_call"] = [("both of two pairs", [a1, b1, b2, a2]), ("found", [b1, a1, a2, b2])]
    out["F_equal_tag_pair_in_two_calls"] = [("one of each", [a1, b2]), ("the partners are new", [b1, a2, a1]),
                                            ("all four", [a2, b2, b1, a1])]
    # chains: inside one, across the table's end, around the empty key's home
    out["F_chain_and_absent_key_inside_it"] = [("a chain of 40 on one slot", chain),
                                               ("absent keys homed inside it", homed(KS_CHAIN_SLOT + 20, 1, "ks") + homed(KS_CHAIN_SLOT, 1, "ks", skip=40) + chain[:3]),
                                               ("all found", chain[::-1])]
    out["F_chain_across_the_tables_end"] = [("homes cap-2, cap-1, 0", wrap), ("absent, homed at cap-1", homed(MIN_CAP - 1, 1, "ks", skip=3) + wrap[:2]),
                                            ("all found", wrap[::-1])]
    out["F_empty_key_inside_a_chain"] = [("keys homed on and before the empty key's slot", around_empty), ("the empty key, new", [b""] + around_empty[:1]),
                                         ("found", around_empty + [b""])]
    out["F_empty_key_first_then_its_chain"] = [("the empty key alone", [b""]), ("its neighbours", around_empty), ("found", [b""] + around_empty[::-1])]
    return out
