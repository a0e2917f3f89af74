"""The tile parse — k_tile_count_r, k_tile_parse, k_parse_deferred, lean_tile / k_tile_lean in its five modes,
k_tile_lean_check, k_tile_compact — against a plain line model at the positions it branches on: a line's byte in
the 32 KiB tile, its chunk and 64-byte region, its rank in the tile's line list and window, its length against the
48-byte view and the staged windows, the end of input.  tests/tile_util.py builds the cases, restates the geometry
and the tier predicate; tests/test_tile_cases.py shows on the CPU that each case sits where it claims and that the
oracle equals the model there.

Every case runs on eight routes (default, TEST_NO_GROUP, TEST_NO_TILE_LOCAL, TEST_NO_LEAN, TEST_DICT_DIRECT,
TEST_DICT_HASH, TEST_DICT_HASH | TEST_NO_HASH_LEAN, TEST_DICT_GENERAL).  On each, in the plain asymmetric build and
the bidirected keep-directed build, the node names, the stream-order COO, the warning's line and byte (or the
failing line) are the model's and the tier read from the phases ("parse" without "tiles": tile-local) is the
restated one.  On the default route every mode of test_gpu_diff.MODES gives the oracle's outcome in float64 and
int8, and so does the weighted undirected CSR (RC), with and without TEST_NO_EXT_LEAN; the other routes equal the
default on the plain, directed=False and bidirected modes.  Several small files per test."""
import ctypes

import numpy as np
import pytest

import tile_util as T
from test_gpu_diff import MODES, gpu_run, oracle_run, outcome

pytestmark = pytest.mark.gpu

PLAIN = {"asymmetric": True}
BIDIR = {"bidirected": True, "keep_directed_bidir": True, "asymmetric": True}
AGREE = (0, 1, 3)  # MODES the other routes are compared with the default on: {}, directed=False, bidirected


def _flags(nat, route):
    return {"default": 0, "no_group": nat.TEST_NO_GROUP, "no_tile_local": nat.TEST_NO_TILE_LOCAL,
            "no_lean": nat.TEST_NO_LEAN, "direct": nat.TEST_DICT_DIRECT, "hash": nat.TEST_DICT_HASH,
            "hash_classic": nat.TEST_DICT_HASH | nat.TEST_NO_HASH_LEAN, "general": nat.TEST_DICT_GENERAL}[route]


def _build(nat, data, flags, **opts):
    """One build and its phases in order (the test_gpu_dict_edges._build pattern)."""
    lib = nat.load()
    arr = np.frombuffer(data, dtype=np.uint8)
    o = nat.make_options(test_flags=flags, **opts)
    res = ctypes.POINTER(nat.Result)()
    rc = lib.g2n_build_from_buffer(arr.ctypes.data if arr.size else None, arr.size, ctypes.byref(o), ctypes.byref(res))
    phases = [res.contents.phase_names[k].decode() for k in range(res.contents.n_phases)] if res else []
    return nat._from_result(res, rc), phases


def _tier(phases):
    return "local" if "parse" in phases and "tiles" not in phases else "k1"


def _names(raw):
    blob, offs = raw.names_blob.tobytes(), raw.names_offsets
    return [blob[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


def _check_direct(nat, c, data, route, models):
    for mode, bidir in ((PLAIN, False), (BIDIR, True)):
        raw, phases = _build(nat, data, _flags(nat, route), **mode)
        m = models[bidir]
        what = (c.name, route, "bidirected" if bidir else "plain")
        assert _tier(phases) == T.expect_tier(data, route), (what, phases)
        assert (raw.has_warning, raw.warn_line if raw.has_warning else -1) == (m.warn_line >= 0, m.warn_line), what
        assert not raw.has_warning or raw.warn_byte == m.warn_byte, what
        if m.error:
            assert raw.status != 0 and raw.err_line == m.error[0], what
            continue
        assert raw.status == 0 and raw.n_nodes == len(m.nodes), what
        assert _names(raw) == m.nodes, what
        assert raw.format == "coo" and raw.rows.tolist() == [u for u, _v in m.edges], what
        assert raw.cols.tolist() == [v for _u, v in m.edges], what


def _check_weighted(nat, oracle_lib, c, data):
    """The undirected weighted CSR: the extended lean tile into group slots, then K1 + the lean parse."""
    o = oracle_lib.run(data, directed=False, weight_tag="RC")
    want = oracle_lib.to_raw(o, "csr") if o.status == 0 else None
    for flags, tier in ((0, T.expect_tier(data, "default", weighted=True)), (nat.TEST_NO_EXT_LEAN, "k1")):
        raw, phases = _build(nat, data, flags, directed=False, weight_tag="RC", output=nat.OUT_CSR)
        what = (c.name, "weighted", flags)
        assert (raw.status != 0) == (o.status != 0), what
        assert _tier(phases) == tier, (what, phases)
        if want is not None:
            assert raw.format == "csr" and raw.indptr.tolist() == want.indptr.tolist(), what
            assert raw.indices.tolist() == want.indices.tolist() and raw.data.tobytes() == want.data.tobytes(), what


def _check_case(gpu, oracle_lib, monkeypatch, c):
    data = T.data_of(c)
    models = {b: T.model(c.lines, b) for b in (False, True)}
    grid = [(m, dt) for m in range(len(MODES)) for dt in ("float64", "int8")]
    want = {(m, dt): outcome(oracle_run(oracle_lib, data, MODES[m], dt, None)) for m, dt in grid}
    for route in T.ROUTES:
        _check_direct(gpu, c, data, route, models)
        some = grid if route == "default" else [(m, "float64") for m in AGREE]
        monkeypatch.setattr(gpu, "TEST_FLAGS", _flags(gpu, route))
        got = {k: outcome(gpu_run(data, MODES[k[0]], k[1], None)) for k in some}
        monkeypatch.setattr(gpu, "TEST_FLAGS", 0)
        bad = [(MODES[m], dt) for m, dt in some if got[m, dt] != want[m, dt]]
        assert not bad, (c.name, route, bad[:3])  # (the default equals the oracle: the other routes equal the default)
    _check_weighted(gpu, oracle_lib, c, data)


GROUPS = {
    "A_kinds_S_L_LRC": ("A_S_line_at", "A_L_line_at", "A_LRC_line_at"),
    "A_kinds_P_H_W": ("A_P_line_at", "A_H_line_at", "A_W_line_at"),
    "A_offset_15_and_sparse_tiles": ("A_S_L_LRC_lines", "A_P_H_W_lines", "A_tile_"),
    "B_lean_view": ("B_lean_edge_line", "B_P_line"),
    "B_S_second_tab": ("B_S_line_second_tab",),
    "B_lean_window": ("B_lean_window",),
    "B_full_window": ("B_full_window_last",),
    "B_deferred_and_mask_span": ("B_full_window_deferred", "B_full_window_ends", "B_lines_of", "B_S_and_P_line_of"),
    "C_starts_2047_to_2050": ("C_tile_of_2047", "C_tile_of_2048", "C_tile_of_2049", "C_tile_of_2050"),
    "C_starts_4096_4097_regions_caps": ("C_tile_of_4096", "C_tile_of_4097", "C_4_starts", "C_5_starts", "C_6_starts",
                                        "C_32_starts", "C_edge_only", "C_tile_of_2800"),
    "C_S_after_edge": ("C_S_after_edge",),
    "C_S_named_too_high_and_edge_key": ("C_S_line_named", "C_edge_key"),
    "C_W_line": ("C_W_line",),
    "D_lengths": ("D_length", "D_final_tile"),
    "D_last_lines_and_tiny_inputs": ("D_last", "D_input"),
}


def _group(name):
    return [c for c in T.cases() if c.name.startswith(GROUPS[name])]


def test_every_case_is_in_one_group():
    names = [c.name for g in GROUPS for c in _group(g)]
    assert sorted(names) == sorted(c.name for c in T.cases())


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_tile_cases(gpu, oracle_lib, monkeypatch, group):
    some = _group(group)
    assert some
    for c in some:
        _check_case(gpu, oracle_lib, monkeypatch, c)


def test_s_after_edge_file_keeps_the_references_node_order(gpu):
    """The finding this suite started from: an S line ranked past the first window of its tile, after an edge line
    of the same tile, breaks the S-first premise — the tile-local parse must decline, and the node order is the
    first-touch order 1 2 3 5 4, not the decimal 1 2 3 4 5."""
    data = b"".join(T.issue_file())
    raw, phases = _build(gpu, data, 0, **PLAIN)
    assert _names(raw) == [b"1", b"2", b"3", b"5", b"4"] and _tier(phases) == "k1", phases
    assert (raw.rows[0], raw.cols[0]) == (3, 4)
