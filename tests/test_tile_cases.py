"""CPU: the inputs of tests/test_gpu_tile_edges.py sit on the tile thresholds their names say (tests/tile_util.py:
every claim is recomputed from the bytes), the restated geometry is the sources', every route's tier follows from
the restated predicate (never "either"), and on every input the oracle equals the plain line model."""
import re
from pathlib import Path

import pytest

import tile_util as T

CSRC = Path(__file__).resolve().parent.parent / "gfa2network_amd" / "csrc"
CASES = T.cases()
BY_FAMILY = {f: [c for c in CASES if c.family == f] for f in "ABCD"}


def _const(text: str, name: str) -> str:
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", text)
    assert m, name
    return m.group(1).strip()


def test_geometry_is_the_sources():
    h = (CSRC / "g2n_kernels.h").read_text()
    k = (CSRC / "g2n_kernels.hip").read_text()
    p = (CSRC / "g2n_pipeline.hip").read_text()
    assert int(_const(h, "kTile")) == T.K_TILE and int(_const(h, "kTileHalo")) == T.K_TILE_HALO
    assert int(_const(k, "kLeanHalo")) == T.K_LEAN_HALO and int(_const(k, "kLeanLines")) == T.K_LEAN_LINES
    assert int(_const(k, "kLeanBatch")) == T.K_LEAN_BATCH and int(_const(k, "kMaskSpan")) == T.K_MASK_SPAN
    assert int(_const(k, "kK1TPB")) == T.K1_TPB and int(_const(k, "kLeanTPB")) == 512
    assert _const(k, "kTileLines") == "kTileChunks" and _const(k, "kTileChunks") == "(uint32_t)(kTile / 16)"
    assert _const(k, "kLeanRegion") == "(uint32_t)(kTile / 16) / kLeanTPB" and T.K_TILE // 16 // 512 == T.K_LEAN_REGION
    assert _const(p, "kTileEdgeCap") == "(uint32_t)(kTile / 12) + 6" and T.K_TILE_EDGE_CAP == 2736
    assert "if (n > 48 && k != kS) return false;" in k and "n > 48 ? 48 : n" in k  # the 48-byte view
    assert T.K1_WAVE_BYTES == 1024 and T.K1_ROW_BYTES == 8192 and T.REGION == 64


def _offsets(c):
    out, at = [], 0
    for x in c.lines:
        out.append(at)
        at += len(x)
    return out


@pytest.mark.parametrize("family", list("ABCD"))
def test_every_case_sits_on_the_threshold_it_names(family):
    for c in BY_FAMILY[family]:
        data = T.data_of(c)
        table, offs = T.line_table(data), _offsets(c)
        assert [r[0] for r in table] == offs and T.n_tiles(data) <= 5, c.name  # the lines are the bytes' lines
        assert all(x.endswith(b"\n") for x in c.lines[:-1]), c.name
        assert c.claims, c.name
        counts = T.tile_starts(data)
        for what, i, v in c.claims:
            who = (c.name, what, i, v)
            if i is not None and what not in ("starts", "tile_edges", "region_starts"):
                s, n, t, o, r = table[i]
            if what == "tile_off":
                assert (t, o) == v, who
            elif what == "rank":
                assert (t, r) == v, who
            elif what == "len":
                assert n == v and data[s + n:s + n + 1] == b"\n", who
            elif what == "tab2":
                tabs = [j for j in range(n) if data[s + j] == 9]
                assert tabs[1] == v and n > T.VIEW, who
            elif what == "tab2_at":
                assert [j for j in range(n) if data[s + j] == 9][1] == v, who
            elif what == "two_byte_lines":
                inside = [q for q in table if q[2] == 0]
                assert sum(1 for q in inside if q[1] == 1) == v >= 1000, who
                assert max(q[4] for q in inside if q[1] == 1) == len(inside) - 3, who  # up to the last ranks but two
            elif what == "chunk_phase":
                assert o % T.CHUNK == v, who
            elif what == "nl_at":
                assert s + n == v and data[v:v + 1] == b"\n", who
            elif what == "nl_staged":
                assert s + n - t * T.K_TILE == v and data[s + n:s + n + 1] == b"\n", who
                assert all(q[2] != t or q[0] <= s for q in table), (who, "the tile's last line")
            elif what == "end_past":
                assert s + n - t * T.K_TILE >= v, who
            elif what == "spans_tiles":
                assert (s + n) // T.K_TILE - t + 1 == v, who
            elif what == "starts":
                assert counts.get(i, 0) == v and i < T.n_tiles(data), who
            elif what == "tile_edges":
                assert sum(1 for q in table if q[2] == i and data[q[0]:q[0] + 1] == b"L") == v, who
            elif what == "region_starts":
                tile, region, k = v
                lo = tile * T.K_TILE + region * T.REGION
                inside = [q for q in table if lo <= q[0] < lo + T.REGION]
                assert len(inside) == k and inside[0][0] == offs[i] and offs[i + k] >= lo + T.REGION, who
                kinds = [data[q[0]:q[0] + 1] for q in inside]
                assert kinds[-1] == b"L" and (k <= T.K_LEAN_BATCH or b"L" in kinds[T.K_LEAN_BATCH:]), who
            elif what == "total":
                assert len(data) == v, who
            elif what == "no_final_newline":
                assert not data.endswith(b"\n"), who
            elif what == "warns":
                m = T.model(c.lines)
                assert (m.warn_line, m.warn_byte) == (i, v) and any(x[:1] == b"X" for x in c.lines[i + 1:]), who
            else:
                raise AssertionError(who)


def test_family_a_covers_every_kind_at_every_offset():
    seen = set()
    for c in BY_FAMILY["A"]:
        data = T.data_of(c)
        table = T.line_table(data)
        for what, i, v in c.claims:
            if what == "tile_off":
                s, n = table[i][0], table[i][1]
                f = data[s:s + n].split(b"\t")
                kind = "LRC" if f[0] == b"L" and len(f) == 7 else f[0].decode()
                seen.add((kind, v[1]))
                if v[1] == 0:
                    assert v[0] > 0 and data[s - 1:s] == b"\n"
                if v[1] == T.K_TILE - 1 and n > 1:  # the letter on the tile's last byte, its tab the halo's first
                    assert data[s + 1:s + 2] == b"\t" and (s + 1) % T.K_TILE == 0
    assert seen >= {(k, o) for k in T.KINDS for o in T.A_OFFSETS}
    a = {c.name: c for c in BY_FAMILY["A"]}
    assert any(w == "nl_at" and v % T.K_TILE == 0 for w, _i, v in a["A_L_line_at_11_tile_offsets"].claims)
    assert ("starts", 1, 0) in a["A_tile_without_a_start_inside_an_S_line_of_three_tiles"].claims
    assert ("starts", 1, 1) in a["A_tile_holding_exactly_one_start"].claims


def test_families_b_c_d_cover_their_thresholds():
    names = {c.name for c in CASES}
    for n in (47, 48, 49):
        assert {f"B_lean_edge_line_of_{n}_bytes_mid_tile", f"B_lean_edge_line_of_{n}_bytes_at_32767",
                f"B_S_line_second_tab_at_byte_{n}_mid_tile",
                f"B_S_line_second_tab_at_byte_{n}_sequence_past_the_staged_window"} <= names
        for where in ("mid_tile", "at_32767"):  # 47 and 48 stay in the tile-local tier, 49 must leave it
            assert T.expect_local(T.data_of(T.case(f"B_lean_edge_line_of_{n}_bytes_{where}"))) == (n <= 48)
    assert T.expect_local(T.data_of(T.case("B_P_line_second_tab_at_byte_47")))
    assert not T.expect_local(T.data_of(T.case("B_P_line_second_tab_at_byte_48")))
    for halo, tag in ((T.K_LEAN_HALO, "lean"), (T.K_TILE_HALO, "full")):
        for kind in "SLP":
            got = sorted(v for c in CASES if c.name.startswith(f"B_{tag}_window_last_{kind}_")
                         for w, _i, v in c.claims if w == "nl_staged")
            assert got == [T.K_TILE + halo - 1, T.K_TILE + halo, T.K_TILE + halo + 1], (tag, kind)
    for n in (2047, 2048, 2049, 2050, 4096, 4097):
        for form in ("edges_last", "S_lines_last"):
            c = T.case(f"C_tile_of_{n}_starts_{form}")
            data = T.data_of(c)
            last = [q for q in T.line_table(data) if q[2] == 0][-1]
            assert last[4] == n - 1 and data[last[0]:last[0] + 1] == (b"L" if form == "edges_last" else b"S")
            assert last[0] + last[1] == T.K_TILE - 1 and T.expect_local(data), c.name
    ranks = {}
    for c in BY_FAMILY["C"]:
        for w, _i, v in c.claims:
            if w == "rank":
                ranks.setdefault(c.name.rsplit("_at_rank_", 1)[0], set()).add(v[1])
    short = {f"C_tile_of_{n}_starts_2_byte_H_lines": {n - 1} for n in (2049, 4097)}  # their last start's rank
    assert {k: ranks[k] for k in short} == short, ranks
    assert all(ranks[k] == set(T.RANKS) for k in ranks if "2060" not in k and k not in short) and len(ranks) == 8, ranks
    assert min(T.RANKS) == T.K_LEAN_LINES - 1 and max(T.RANKS) > 2 * T.K_LEAN_LINES  # the third window
    e = T.data_of(T.case("C_edge_only_tile_of_2730_edge_lines_of_12_bytes"))
    assert all(e[q[0]:q[0] + 1] == b"L" for q in T.line_table(e) if q[2] == 1) and 2731 <= T.K_TILE_EDGE_CAP < 2800
    assert {len(T.data_of(c)) for c in BY_FAMILY["D"]} >= {0, 1, 5, 15, T.K_TILE - 1, T.K_TILE, T.K_TILE + 1,
                                                          2 * T.K_TILE - 1, 2 * T.K_TILE, 2 * T.K_TILE + 1}


def test_tiers_follow_the_restated_predicate():
    """No case declares its tier "either": expect_tier is a function of the bytes and the route."""
    for c in CASES:
        data = T.data_of(c)
        tiers = {r: T.expect_tier(data, r) for r in T.ROUTES}
        assert set(tiers.values()) <= {"local", "k1"}, c.name
        assert all(tiers[r] == "k1" for r in T.ROUTES if r not in T.LOCAL_ROUTES), c.name
        assert tiers["default"] == tiers["no_group"], c.name
    local = {c.name for c in CASES if T.expect_local(T.data_of(c))}
    assert {c.name for c in CASES if c.name.startswith(("C_S_after_edge", "C_S_line_named", "C_edge_key"))}.isdisjoint(local)
    assert {c.name for c in CASES if c.name.startswith(("A_", "C_W_line", "C_tile_of_20", "C_tile_of_40", "D_length"))} <= local
    assert "C_tile_of_2800_malformed_2_byte_L_lines" not in local and "D_input_of_0_bytes" not in local
    # the predicate's own edges: the view, the window, S first, the weighted tag
    ok = T.S(1) + T.S(2) + T.L(1, "+", 2, "-")
    assert T.expect_local(ok) and not T.expect_local(T.S(2) + ok) and not T.expect_local(ok + T.S(3))
    assert not T.expect_local(ok + T.L(1, "+", 3, "-")) and not T.expect_local(ok + b"L\t1+\t2-\t*\t*\n")
    assert T.expect_local(ok + T.LRC(1, "+", 2, "-", 7), True) and not T.expect_local(ok + T.L(1, "+", 2, "-", b"*", b"RC:i:07"), True)
    assert T.expect_local(ok + T.L(1, "+", 2, "-", b"*", b"RC:i:07"), False)


def _names_of(o):
    blob, offs = o.names_blob.tobytes(), o.names_offsets
    return [blob[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


@pytest.mark.parametrize("family", list("ABCD"))
def test_oracle_equals_the_line_model(oracle_lib, family):
    """Names in id order, the stream-order COO (plain, bidirected keep-directed, bidirected undirected), the
    warning's line and byte, the failing line, and the RC weights of the undirected weighted build."""
    for c in BY_FAMILY[family]:
        data = T.data_of(c)
        assert T.split_lines(data) == list(c.lines), c.name
        for mode, bidir, keep in (({"asymmetric": True}, False, True),
                                  ({"bidirected": True, "keep_directed_bidir": True, "asymmetric": True}, True, True),
                                  ({"bidirected": True}, True, False)):
            o = oracle_lib.run(data, **mode)
            m = T.model(c.lines, bidir, keep)
            assert (o.has_warning, o.warn_line if o.has_warning else -1) == (m.warn_line >= 0, m.warn_line), (c.name, mode)
            assert not o.has_warning or o.warn_byte == m.warn_byte, (c.name, mode)
            if m.error:
                assert c.note == "error" and o.status != 0 and o.err_line == m.error[0], (c.name, mode)
                continue
            assert c.note != "error" and o.status == 0 and _names_of(o) == m.nodes, (c.name, mode)
            rows = [u for u, _v in m.edges] if keep else [x for u, v in m.edges for x in (u, v)]
            cols = [v for _u, v in m.edges] if keep else [x for u, v in m.edges for x in (v, u)]
            assert o.rows.tolist() == rows and o.cols.tolist() == cols, (c.name, mode)
        m = T.model(c.lines)
        if m.error:
            continue
        o = oracle_lib.run(data, directed=False, weight_tag="RC")
        assert o.status == 0 and o.rows.tolist() == [x for u, v in m.edges for x in (u, v)], c.name
        assert o.cols.tolist() == [x for u, v in m.edges for x in (v, u)], c.name
        assert o.weights.tolist() == [w for w in m.weights for _ in (0, 1)], c.name
