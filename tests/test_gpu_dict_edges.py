"""The hash dictionary tiers — the lean S-first hash (k_tile_lean kLeanClaim / kLeanEdges), the classic tiers of
build_dictionary (k_insert_round, k_lookup_fast, k_assign_first / k_assign_ids, k_names) and the chunked
build's key set (k_ks_lookup / k_ks_insert, keyset_rehash) — against a Python dict at the sizes, key lengths and
hash values they branch on.  tests/dict_util.py builds the cases and restates the hashes and the host's
geometry; tests/test_dict_cases.py shows on the CPU that each case sits where it claims and that the oracle
equals the dict model there.

Every GFA case runs on three routes: TEST_DICT_HASH (the lean hash first), TEST_DICT_HASH | TEST_NO_HASH_LEAN
(the classic tiers) and TEST_DICT_GENERAL.  On each the node list and the stream-order COO of the plain and the
bidirected build must be first_touch()'s, every mode of test_gpu_diff.MODES must give the oracle's outcome in
float64 and int8, the build must end in the tier the restated premises give (and report the table_init phases
they give: one more when the general rounds overflow their first table), and the routes must agree."""
import ctypes

import numpy as np
import pytest

import dict_util as D
from test_gpu_diff import MODES, gpu_run, oracle_run, outcome

pytestmark = pytest.mark.gpu

PLAIN = {"asymmetric": True}
BIDIR = {"bidirected": True, "keep_directed_bidir": True, "asymmetric": True}
FULL = [c.name for c in D.cases() if c.family != "E"]


def _flags(nat, route):
    return {"lean": nat.TEST_DICT_HASH, "classic": nat.TEST_DICT_HASH | nat.TEST_NO_HASH_LEAN,
            "general": nat.TEST_DICT_GENERAL}[route]


def _build(nat, data, flags, **mode):
    """One build and its phases in order (RawResult.phase_ms sums repeated phases)."""
    lib = nat.load()
    arr = np.frombuffer(data, dtype=np.uint8)
    opts = nat.make_options(test_flags=flags, **mode)
    res = ctypes.POINTER(nat.Result)()
    rc = lib.g2n_build_from_buffer(arr.ctypes.data, arr.size, ctypes.byref(opts), ctypes.byref(res))
    phases = [res.contents.phase_names[k].decode() for k in range(res.contents.n_phases)] if res else []
    return nat._from_result(res, rc), phases


def _tier(phases):
    if "insert_lookup" in phases and "parse" not in phases:
        return "lean"
    if "ids_general" in phases:
        return "general"
    return "fast" if "ids_fast" in phases else "none"


def _names(raw):
    blob, offs = raw.names_blob.tobytes(), raw.names_offsets
    return [blob[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


def _check_direct(nat, c, data, route):
    """Names and stream-order COO against the dict model; the tier and the tables against the restated host."""
    for mode, bidir in ((PLAIN, False), (BIDIR, True)):
        raw, phases = _build(nat, data, _flags(nat, route), **mode)
        nodes, edges = D.first_touch(c.lines, bidir)
        what = (c.name, route, "bidirected" if bidir else "plain")
        assert raw.status == 0 and raw.n_nodes == len(nodes), what
        assert _names(raw) == nodes, what
        assert raw.format == "coo" and raw.rows.tolist() == [u for u, _v in edges], what
        assert raw.cols.tolist() == [v for _u, v in edges], what
        tier = D.expected_tier(c.lines, route, bidir)
        assert tier == "either" or _tier(phases) == tier, (what, phases)
        inits = D.expected_table_inits(c.lines, route, bidir)
        assert inits is None or phases.count("table_init") == inits, (what, phases)


def _check_case(gpu, oracle_lib, monkeypatch, c):
    """One case on the three routes: the direct checks, then every mode x dtype against one oracle outcome."""
    data = b"".join(c.lines)
    grid = [(m, dt) for m in range(len(MODES)) for dt in ("float64", "int8")]
    want = {(m, dt): outcome(oracle_run(oracle_lib, data, MODES[m], dt, None)) for m, dt in grid}
    for route in D.ROUTES:
        _check_direct(gpu, c, data, route)
        monkeypatch.setattr(gpu, "TEST_FLAGS", _flags(gpu, route))
        got = {(m, dt): outcome(gpu_run(data, MODES[m], dt, None)) for m, dt in grid}
        monkeypatch.setattr(gpu, "TEST_FLAGS", 0)
        bad = [(MODES[m], dt) for m, dt in grid if got[m, dt] != want[m, dt]]
        assert not bad, (c.name, route, bad[:3])  # (equal to one oracle outcome: the three routes equal each other)
    return data


@pytest.mark.parametrize("name", FULL)
def test_dictionary_case(gpu, oracle_lib, monkeypatch, name):
    c = D.case(name)
    data = _check_case(gpu, oracle_lib, monkeypatch, c)
    if c.family == "D" and c.expect_retry is not None:  # the retry the case is named for, in the plain build's phases
        _raw, phases = _build(gpu, data, gpu.TEST_DICT_GENERAL, **PLAIN)
        assert phases.count("table_init") == 1 + int(c.expect_retry), (name, phases)


@pytest.mark.parametrize("form", ["S_only", "L_before_S"])
@pytest.mark.parametrize("group", ["H_pad", "last_S_name_of_5", "last_S_name_of_16", "last_S_name_of_17"])
def test_names_blob_cases(gpu, oracle_lib, monkeypatch, group, form):
    """Family E, batched (7 or 8 small files a test), each file checked like every other case: names of 0 .. 17
    bytes at every alignment phase, and a last S name 0 .. 25 bytes before the input's end (k_names' three-word
    path against its byte loop; k_names_lean_bidir on the lean tier); S lines only, and a link before them."""
    some = [c for c in D.cases() if c.family == "E" and group in c.name and c.name.endswith(form)]
    assert len(some) >= 7
    for c in some:
        _check_case(gpu, oracle_lib, monkeypatch, c)


@pytest.mark.parametrize("script", sorted(D.keyset_scripts()))
def test_keyset_script(gpu, script):
    """Family F through HipEngine.keyset(): ids in insertion order across calls, growth at 2 (n_set + n_call) >
    cap (also when the call adds no key), keys of equal tag, length and slot, chains across the table's end and
    around the empty key, and the set's names in id order after every growth."""
    import torch

    from gfa2network_amd.shard import HipEngine
    from shard_prim_util import pack, unpack

    eng = HipEngine(0)
    ks = eng.keyset()
    ref, cap = {}, 0
    try:
        for label, keys in D.keyset_scripts()[script]:
            blob, offs = pack(keys)
            ids, n_tot = ks.add(torch.from_numpy(blob).to(eng.device), torch.from_numpy(offs).to(eng.device))
            grew = D.ks_cap(len(ref), len(keys), cap) != cap
            cap = D.ks_cap(len(ref), len(keys), cap)
            want = [ref.setdefault(k, len(ref)) for k in keys]
            assert ids.cpu().numpy().tolist() == want, (script, label)
            assert n_tot == len(ref), (script, label)
            if grew:
                nb, no = ks.names()
                assert unpack(nb.cpu().numpy(), no.cpu().numpy()) == list(ref), (script, label, "names after growth")
        nb, no = ks.names()
        assert unpack(nb.cpu().numpy(), no.cpu().numpy()) == list(ref), script
        # every key again, in one call: found with its id, nothing new
        blob, offs = pack(list(ref))
        ids, n_tot = ks.add(torch.from_numpy(blob).to(eng.device), torch.from_numpy(offs).to(eng.device))
        assert ids.cpu().numpy().tolist() == list(range(len(ref))) and n_tot == len(ref), script
    finally:
        ks.close()
        eng.close()
