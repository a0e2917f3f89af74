"""CPU: the inputs of tests/test_gpu_dict_edges.py sit where their names say (tests/dict_util.py), and on
every one of them the oracle's node ids are the plain dict first-touch model's."""
import numpy as np
import pytest

import dict_util as D
from shard_prim_util import COLLIDING, dict_key_hash

CASES = D.cases()
BY_FAMILY = {f: [c for c in CASES if c.family == f] for f in "ABCDE"}


def _s_names(lines):
    return [D._fields(x)[1] for x in lines if x[:2] == b"S\t"]


def _edges(lines):
    return [x for x in lines if x[:2] == b"L\t"]


def _tag_slot(key, cap=D.MIN_CAP):
    return D.tag_slot(dict_key_hash(key), cap)


def test_hashes_restated_agree():
    """The numpy forms against the scalar ones; the bidirected key is name + ':' + orientation whatever byte
    of the 16-byte head the ':' lands on (key_head's three branches, touch_byte's two)."""
    r = np.random.default_rng(3)
    w = r.integers(0, 1 << 63, 200, dtype=np.int64).astype(np.uint64)
    v = r.integers(0, 1 << 63, 200, dtype=np.int64).astype(np.uint64)
    h16, h8, hk = D.dict_hash_np(w, v, 16), D.dict_hash_np(w, np.uint64(0), 8), D.ks_hash_np(w)
    for j in range(200):
        a, b = int(w[j]).to_bytes(8, "little"), int(v[j]).to_bytes(8, "little")
        assert int(h16[j]) == dict_key_hash(a + b) and int(h8[j]) == dict_key_hash(a) and int(hk[j]) == D.ks_hash(a)
    assert D.ks_hash(b"") == 0xCBF29CE484222325 ^ (0xCBF29CE484222325 >> 29)
    for n in (13, 14, 15, 16, 17):  # the same bytes hash alike as a plain name and as a bidirected key
        name = b"n" * n
        assert dict_key_hash(D.bidir_key(name, b"-")) == dict_key_hash(name + b":-")
        assert dict_key_hash(D.bidir_key(name, b"+")) != dict_key_hash(D.bidir_key(name, b"-"))


@pytest.mark.parametrize("kind", ["lo", "hi", "byte16"])
def test_searched_pairs_share_tag_and_slot(kind):
    pairs = D.tag_pairs(kind)
    assert len(pairs) >= 2
    for a, b in pairs:
        assert a != b and len(a) == len(b) and _tag_slot(a) == _tag_slot(b) and dict_key_hash(a) != dict_key_hash(b)
        assert not any(c in k for k in (a, b) for c in b"\t\n:")
        if kind == "lo":
            assert len(a) == 16 and a[8:] == b[8:] == D.FIXED_HI and a[:8] != b[:8]
        elif kind == "hi":
            assert len(a) == 16 and a[:8] == b[:8] == D.FIXED_LO and a[8:] != b[8:]
        else:  # one 16-byte head; byte 16 is the last byte; the slot agrees in tables of up to 4096
            assert (a, b) in COLLIDING and len(a) == 17 and a[:16] == b[:16] and a[16] != b[16]
            assert _tag_slot(a, 4096) == _tag_slot(b, 4096)


def test_searched_names_have_their_home_slots():
    for slot in (D.CHAIN_SLOT, D.MIN_CAP - 2, D.MIN_CAP - 1, 0) + D.FILLERS:
        for k in (2, 3, 64, 65):
            names = D.homed(slot, k)
            assert len(set(names)) == k and all(_tag_slot(n)[1] == slot and len(n) == 8 and n.isalpha() for n in names)
    for slot in (D.KS_CHAIN_SLOT, D.MIN_CAP - 2, D.MIN_CAP - 1, 0, D.ks_empty_slot(), D.ks_empty_slot() - 1):
        names = D.homed(slot, 40 if slot == D.KS_CHAIN_SLOT else 3, "ks")
        assert all(D.ks_hash(n) & (D.MIN_CAP - 1) == slot % D.MIN_CAP for n in names) and len(set(names)) == len(names)
    pairs = D.ks_tag_pairs()
    assert len(pairs) >= 2
    for a, b in pairs:
        assert a != b and len(a) == len(b) == 8 and D.tag_slot(D.ks_hash(a), 1024) == D.tag_slot(D.ks_hash(b), 1024)


def test_geometry_restated():
    assert [D.lean_cap(n) for n in (1, 686, 687, 1372, 1373)] == [1024, 1024, 2048, 2048, 4096]
    assert D.classic_caps(100, 3200) == (2048, 8192)          # n_st * 32 == n_et: the /16 branch
    assert D.classic_caps(100, 3202) == (4096, 8192)          # n_st * 32 < n_et: the /2 branch
    assert D.classic_caps(0, 8400) == (8192, 32768) and D.classic_caps(0, 8192) == (8192, 16384)
    assert D.classic_caps(86, 8) == (1024, 1024)              # at most 512 touches: the first table is the full one
    assert [D.ks_cap(a, b, c) for a, b, c in ((0, 512, 0), (0, 513, 0), (300, 212, 1024), (300, 213, 1024),
                                               (1024, 1, 2048), (400, 200, 1024), (5, 0, 1024))] == \
        [1024, 2048, 1024, 2048, 4096, 2048, 1024]
    ok = D.L(b"a" * 19, b"+", b"b" * 19, b"-")
    assert D.in_lean_shape(ok) and len(ok) == 49 and not D.in_lean_shape(D.L(b"a" * 20, b"+", b"b" * 19, b"-"))
    assert not D.in_lean_shape(D.L2(b"a", b"+", b"b", b"-")) and not D.in_lean_shape(b"L\ta\t+\tb\t-\n")


def test_every_case_breaks_at_most_one_lean_premise_and_names_are_clean():
    for c in CASES:
        broken = D.broken_premises(c.lines)
        assert (c.tiers["lean"] == "lean") == (not broken), c.name
        assert len(broken) <= 1, (c.name, broken)
        assert c.tiers["general"] == "general" and c.tiers["classic"] in ("fast", "general", "either"), c.name
        assert (c.tiers["classic"] == "either") == (c.name == "C_repeated_S_name_the_claim_race_decides"), c.name
        s = _s_names(c.lines)
        if s:  # the host's first-line guesses: no digit in the first S name
            assert not any(ch.isdigit() for ch in s[0].decode("latin-1")), c.name
        for n in s:
            assert b"\t" not in n and b"\n" not in n and (b":" not in n or c.name.startswith("A_bidir")), c.name
        assert all(x.endswith(b"\n") for x in c.lines[:-1]) and b"".join(c.lines).count(b"\n") >= len(c.lines) - 1


def test_family_a_sits_on_the_inline_head_and_the_lean_shape():
    a = {c.name: c for c in BY_FAMILY["A"]}
    lean = a["A_lengths_0_to_40_links_la+lb<=38_lean"]
    names = _s_names(lean.lines)
    assert {len(n) for n in names} >= set(D.A_LENGTHS) and b"" in names and {b"a", b"a\0", b"a\0\0"} <= set(names)
    heads = {}
    for n in names:
        if len(n) > 16:
            heads.setdefault((n[:16], len(n)), []).append(n)
    groups = [(x, y) for g in heads.values() for x in g for y in g if x < y]
    assert any(x[17:] == y[17:] and x[16] != y[16] and len(x) > 17 for x, y in groups)  # byte 16 only
    assert any(x[:-1] == y[:-1] and x[-1] != y[-1] and len(x) > 17 for x, y in groups)  # the last byte only
    assert {D.HEAD16[:15], D.HEAD16, D.HEAD16 + b"x", D.HEAD16 + b"y"} <= set(names)
    e = _edges(lean.lines)
    used = {n for x in e for n in (D._fields(x)[1], D._fields(x)[3])}
    assert all(D.in_lean_shape(x) for x in e) and max(len(x) for x in e) == 49 and used >= {n for n in names if len(n) <= 33}
    assert any(len(D._fields(x)[1]) + len(D._fields(x)[3]) == 38 for x in e)
    past = [x for x in _edges(a["A_one_link_la+lb=39_past_the_lean_shape"].lines) if not D.in_lean_shape(x)]
    assert len(past) == 1 and len(past[0]) == 50
    assert not any(D.in_lean_shape(x) for x in _edges(a["A_links_of_names_33_and_40_classic"].lines))
    b = a["A_bidir_names_13_to_17_and_colon_names_lean"]
    keys = D.first_touch(b.lines, True)[0]
    assert {len(n) for n in _s_names(b.lines)} >= set(D.BIDIR_LENGTHS)
    assert {b"ab:+", b"ab:-", b"ab:+:+", b"ab:+:-"} <= set(keys) and len(keys) == 2 * len(_s_names(b.lines))
    g = a["A_bidir_names_13_to_17_gfa2_style_classic"]
    assert not any(D.in_lean_shape(x) for x in _edges(g.lines)) and D.first_touch(g.lines, True)[0] == \
        [n + o for n in _s_names(g.lines) for o in (b":+", b":-")]
    for c in (b, g):  # both orientations of every name are used by an edge
        used = {k for k, s in D.touch_stream(c.lines, True) if not s}
        assert used == set(D.first_touch(c.lines, True)[0]), c.name


def test_family_b_builds_its_chains_in_a_table_of_1024():
    for c in BY_FAMILY["B"]:
        s = _s_names(c.lines)
        assert D.lean_cap(len(s)) == 1024 and D.classic_caps(*D.n_touches(c.lines))[0] == 1024, c.name
        t = D.table_layout(s, 1024)
        absent = [n for x in _edges(c.lines) for n in (D._fields(x)[1], D._fields(x)[3]) if n not in set(s)]
        assert bool(absent) == (c.tiers["lean"] == "general"), c.name
        if "slot_500" in c.name or "chain_of_65" in c.name:
            k = 65 if "chain_of_65" in c.name else int(c.name.split("_")[3])
            run = [t.get(D.CHAIN_SLOT + j) for j in range(k)]
            assert all(_tag_slot(n)[1] == D.CHAIN_SLOT for n in run) and D.CHAIN_SLOT - 1 not in t and D.CHAIN_SLOT + k not in t
            named = {n for x in _edges(c.lines) for n in (D._fields(x)[1], D._fields(x)[3])}
            assert {s[-k], s[-1]} <= named, "edges name the chain's first and last S name"
            for n in absent:  # homed inside the chain: the walk ends at the chain's empty slot
                assert D.CHAIN_SLOT <= _tag_slot(n)[1] < D.CHAIN_SLOT + k, c.name
            if "inside" in c.name:
                assert D.CHAIN_SLOT < _tag_slot(absent[0])[1] < D.CHAIN_SLOT + k - 1
        else:  # homes cap - 2, cap - 1 and 0: slots 1022, 1023, 0 .. 4
            assert set(t) >= {1022, 1023, 0, 1, 2, 3, 4} and 1021 not in t and 5 not in t, c.name
            assert _tag_slot(t[0])[1] == 1022 and _tag_slot(t[4])[1] == 0
            assert all(_tag_slot(n)[1] == 1023 for n in absent)


def test_family_c_pairs_meet_in_both_tables():
    for c in BY_FAMILY["C"]:
        if "repeated" in c.name:
            assert len(set(_s_names(c.lines))) == len(_s_names(c.lines)) - 1
            continue
        if "zero_padded" in c.name:  # equal tag and 16-byte head, another length; the absent name's walk meets the S name
            s_name, absent, fill = D.padded_chain()
            assert _tag_slot(s_name)[0] == _tag_slot(absent)[0] and len(s_name) != len(absent) <= 16
            assert s_name.ljust(16, b"\0") == absent.ljust(16, b"\0") and D.PADDED == (absent, s_name)
            assert D.classic_caps(*D.n_touches(c.lines))[0] == 1024 and D.lean_cap(len(_s_names(c.lines))) == 1024
            t, at = D.table_layout(_s_names(c.lines), 1024), _tag_slot(absent)[1]
            while t[at] != s_name:
                assert _tag_slot(t[at])[0] != _tag_slot(absent)[0]
                at = (at + 1) % 1024
            assert at == _tag_slot(s_name)[1] and (at + 1) % 1024 not in t and len(fill) > 100
            assert absent in D.first_touch(c.lines, False)[0] and c.tiers == {r: "general" for r in D.ROUTES}
            continue
        a, b = D.tag_pairs(c.name.rsplit("_", 1)[1])[0]
        s = set(_s_names(c.lines))
        assert D.classic_caps(*D.n_touches(c.lines))[0] == 1024 and D.lean_cap(len(s)) == 1024, c.name
        assert len(s & {a, b}) == (2 if "two_S" in c.name else 1 if "partner" in c.name else 0), c.name
        nodes = D.first_touch(c.lines, False)[0]
        assert a in nodes and b in nodes and c.tiers == {r: "general" for r in D.ROUTES}, c.name
        if "one_edge" in c.name:  # both claimed in one launch of the general rounds
            assert any({D._fields(x)[1], D._fields(x)[3]} == {a, b} for x in _edges(c.lines))


def test_family_d_sits_on_the_table_sizes():
    d = {c.name: c for c in BY_FAMILY["D"]}
    for n_s, cap in ((686, 1024), (687, 2048), (1372, 2048), (1373, 4096)):
        c = d[f"D_lean_{n_s}_S_lines_cap_{cap}"]
        assert len(_s_names(c.lines)) == len(set(_s_names(c.lines))) == n_s and c.tiers["lean"] == "lean"
    for what, keys, retry in (("cap-1", 2047, False), ("cap_full_table", 2048, False), ("cap+1_retry", 2049, True)):
        c = d[f"D_classic_16th_branch_keys_{what}"]
        assert D.n_touches(c.lines) == (100, 3200) and D.classic_caps(100, 3200) == (2048, 8192)
        assert len(D.first_touch(c.lines, False)[0]) == keys and c.expect_retry == retry, c.name
    c = d["D_classic_half_branch_100_S_3202_edge_touches_fits"]  # the same keys past 2048, the other branch
    assert D.n_touches(c.lines) == (100, 3202) and len(D.first_touch(c.lines, False)[0]) == 2049 and not c.expect_retry
    c = d["D_classic_half_branch_L_only_4200_lines_retry"]
    assert D.n_touches(c.lines) == (0, 8400) and len(D.first_touch(c.lines, False)[0]) == 8400 > 8192 and c.expect_retry
    n = D.half_branch_fit()  # the neighbour that just fits: one more line and a run of slots reaches the probe bound
    c = d[f"D_classic_half_branch_L_only_{n}_lines_longest_run_below_the_probe_bound"]
    assert D.n_touches(c.lines) == (0, 2 * n) and D.classic_caps(0, 2 * n) == (8192, 16384) and c.expect_retry is False
    assert D._l_only_run(n) < D.PROBE_BOUND <= D._l_only_run(n + 1) and 3000 < n < 4096
    assert D._l_only_run(n) == D.longest_run(D.table_layout(D.first_touch(c.lines, False)[0], 8192), 8192)
    c = d["D_classic_half_branch_L_only_4096_lines_full_table"]  # 8192 slots > the probe bound of 4096: undecided
    assert D.n_touches(c.lines) == (0, 8192) and len(D.first_touch(c.lines, False)[0]) == 8192 and c.expect_retry is None
    assert D.longest_run({0: b"", 1: b"", 3: b"", 6: b""}, 8) == 2 and D.longest_run({7: b"", 0: b"", 1: b""}, 8) == 3
    # the table_init phases a build must report: the lean attempt, the S-first attempt, the general rounds (+ retry)
    r = d["D_classic_16th_branch_keys_cap+1_retry"].lines
    assert [D.expected_table_inits(r, x) for x in D.ROUTES] == [4, 3, 2]
    f = d["D_classic_16th_branch_keys_cap_full_table"].lines
    assert [D.expected_table_inits(f, x) for x in D.ROUTES] == [3, 2, 1]
    assert [D.expected_table_inits(d["D_lean_686_S_lines_cap_1024"].lines, x) for x in D.ROUTES] == [1, 1, 1]
    assert [D.expected_table_inits(d["D_classic_half_branch_L_only_4200_lines_retry"].lines, x) for x in D.ROUTES] == [3, 3, 2]


def test_family_e_covers_every_length_phase_and_tail():
    seen, tails = set(), set()
    for c in BY_FAMILY["E"]:
        data = b"".join(c.lines)
        spans = D.name_spans(c.lines)
        if "H_pad" in c.name:
            seen |= {(ln, off & 7, "L_before" in c.name) for off, ln in spans}
        else:
            off, ln = spans[-1]
            d = len(data) - off - ln
            assert c.name.startswith(f"E_last_S_name_of_{ln}_ends_{d}_before"), c.name
            tails.add((ln, d, "L_before" in c.name, data.endswith(b"\n")))
        assert c.tiers["lean"] == ("general" if "L_before" in c.name else "lean"), c.name
    assert seen >= {(ln, p, f) for ln in range(18) for p in range(8) for f in (False, True)}
    assert {(ln, d, f) for ln, d, f, _nl in tails} == {(ln, d, f) for ln in (5, 16, 17) for d in D.E_TAILS for f in (False, True)}
    assert {nl for _l, d, _f, nl in tails if d != 1} == {False} and {nl for _l, d, _f, nl in tails if d == 1} == {True}


def _names_of(o):
    blob, offs = o.names_blob.tobytes(), o.names_offsets
    return [blob[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


@pytest.mark.parametrize("family", list("ABCDE"))
def test_oracle_equals_first_touch(oracle_lib, family):
    """The names in id order and the stream-order COO of the plain and the bidirected builds (asymmetric: one
    entry per edge, no A.maximum(A.T)), and the undirected bidirected build's four touches per edge."""
    for c in BY_FAMILY[family]:
        data = b"".join(c.lines)
        for mode, bidir, keep in (({"asymmetric": True}, False, True),
                                  ({"bidirected": True, "keep_directed_bidir": True, "asymmetric": True}, True, True),
                                  ({"bidirected": True}, True, False)):
            o = oracle_lib.run(data, **mode)
            nodes, edges = D.first_touch(c.lines, bidir, keep)
            assert o.status == 0 and _names_of(o) == nodes, (c.name, mode)
            rows = [u for u, _v in edges] if keep else [x for u, v in edges for x in (u, v)]
            cols = [v for _u, v in edges] if keep else [x for u, v in edges for x in (v, u)]
            assert o.rows.tolist() == rows and o.cols.tolist() == cols, (c.name, mode)


def test_keyset_scripts_sit_on_the_growth_thresholds():
    e = D.ks_empty_slot()
    for name, calls in D.keyset_scripts().items():
        ref, cap, caps = {}, 0, []
        for label, keys in calls:
            assert len(set(keys)) == len(keys) and keys, (name, label)
            cap = D.ks_cap(len(ref), len(keys), cap)
            for k in keys:
                ref.setdefault(k, len(ref))
            caps.append(cap)
            assert 2 * len(ref) <= cap
        if name in D.KS_CAPS:
            assert caps == D.KS_CAPS[name], (name, caps)
        else:
            assert caps[-1] == 1024, name  # the chains are laid out for the first table
    s = D.keyset_scripts()
    assert [len(k) for _l, k in s["F_512_keys_fill_the_first_table"][:2]] == [300, 212]
    assert [len(k) for _l, k in s["F_513_keys_grow_to_2048"][:2]] == [300, 213]
    known = s["F_rehash_that_adds_no_key"]
    assert set(known[1][1]) <= set(known[0][1]) and b"" in known[1][1]
    wrap = s["F_chain_across_the_tables_end"][0][1]
    assert sorted(D.ks_hash(k) & 1023 for k in wrap) == [0, 0, 1022, 1022, 1022, 1023, 1023, 1023]
    around = s["F_empty_key_inside_a_chain"][0][1]
    assert sorted((D.ks_hash(k) - e) & 1023 for k in around) == [0, 0, 1023, 1023]
