"""CPU: the cases of tests/edge_text_util.py sit where they claim, and the model equals the oracle there.

Every claim of every case — a block's text length, its phase in the 16-byte word, p1 - base against the LDS stage,
which blocks are staged, the long keys' lengths, the first undecodable edge, the good edges before a short L line,
the digit counts and thread slots of the decimal keys, the scan's item count — is recomputed from the case's bytes
with block_plan() and the line model.  For every case up to ORACLE_MAX_BYTES the model's text and failure equal
oracle_lib.export_edge_list (the project's CPU restatement of the reference's loop), plain and bidirected, and
tile_util.expect_local says which render the build must take.  No GPU."""
import pytest

import edge_text_util as E
import tile_util as T


def _keys(lines, col):
    return [x.split(b"\t")[col] for x in lines if x[:1] == b"L" and x.count(b"\t") >= 4]


def check_claim(c, claim):
    what, bidir, blk, value = claim
    modes = E.MODES if bidir is None else (bidir,)
    if what == "n_edges":
        assert len(E.render(c.lines)[0]) == value and E.render(c.lines)[2] == -1
    elif what == "blocks":
        assert all(len(E.plan_of(c.lines, m)) == value for m in modes)
    elif what in ("staged", "text_len", "span", "p0_mod16", "p1_mod16"):
        for m in modes:
            p0, p1, base, staged = E.plan_of(c.lines, m)[blk]
            assert base % 16 == 0 and 0 <= p0 - base < 16
            got = {"staged": staged, "text_len": p1 - p0, "span": p1 - base, "p0_mod16": p0 % 16, "p1_mod16": p1 % 16}
            assert got[what] == value, (c.name, claim, got)
            assert staged == (p1 - base <= E.K_TEXT_LDS)
    elif what == "longest_line":
        out = E.render(c.lines, bidir)[0][blk * E.K_TEXT_EDGES:(blk + 1) * E.K_TEXT_EDGES]
        assert max(map(len, out)) == value > E.K_TEXT_LDS
    elif what == "line_len":
        out = E.render(c.lines, bidir)[0][blk * E.K_TEXT_EDGES:(blk + 1) * E.K_TEXT_EDGES]
        assert len(out) == E.K_TEXT_EDGES and {len(x) for x in out} == {value}
    elif what == "self_loops":
        assert any(f[1] == f[3] and f[2] == f[4] for f in (x.split(b"\t") for x in c.lines) if len(f) > 4)
    elif what == "long_keys":
        for col in (1, 3):  # each once as u and once as v
            assert sorted(len(k) for k in _keys(c.lines, col) if len(k) > 1 << 20) == sorted(value)
        assert (E.K_META_LEN - 1, E.K_META_LEN, E.K_EM_LEN - 1, E.K_EM_LEN) == tuple(value[j] for j in (0, 1, 3, 4))
    elif what == "first_bad":
        for m in modes:
            bad = E.render(c.lines, m)[1]
            assert bad[0][0] == value[0] and all(e > value[0] for e, _k in bad[1:])
            with pytest.raises(UnicodeDecodeError):
                bad[0][1].decode()
            if value[1] is not None:  # (bidirected: the key carries its orientation)
                assert bad[0][1] in ((value[1] + b":+", value[1] + b":-") if m else (value[1],))
    elif what == "bad_edges":
        assert tuple(e for e, _k in E.render(c.lines)[1]) == value
    elif what == "malformed_after":
        out, _bad, mal = E.render(c.lines)
        assert len(out) == value and mal >= 0 and c.lines[mal][:1] == b"L" and c.lines[mal].count(b"\t") < 4
        assert sum(1 for x in c.lines[mal + 1:] if x[:1] == b"L") >= 50  # good edges follow it
    elif what == "tail":
        assert len(E.render(c.lines)[0]) % E.K_DEC_PER == value
    elif what == "scan_items":
        nb = len(E.plan_of(c.lines, False))
        assert nb + 1 == value > E.K_SCAN_TILE
    elif what == "digits":
        assert tuple(sorted(E.digits_of(c.lines))) == value
    elif what == "every_value_as_u_and_v":
        for col in (1, 3):
            assert sorted(int(k) for k in _keys(c.lines, col)) == list(range(1, value + 1))
    elif what == "slots":
        every = tuple(range(E.K_DEC_PER))
        for v in value:
            assert E.slots_of(c.lines, v) == (every, every), v
    elif what == "high_halves":
        halves = {int(k) // 10 ** 4 % 10 ** 4 for col in (1, 3) for k in _keys(c.lines, col) if len(k) <= 8}
        assert set(range(value)) <= halves
    else:
        raise AssertionError(f"unknown claim {what}")


def _check_decimal_keys(c):
    """A decimal case names only segments that exist, and 2 N fits the bidirected ids."""
    n = c.head[1]
    vals = {int(k) for col in (1, 3) for k in _keys(set(c.lines), col)}
    lo, hi = min(vals), max(vals)
    assert 1 <= lo and hi <= n and 2 * n < 2 ** 31 - 1, (c.name, lo, hi, n)


NAMES = [c.name for c in E.cases()] + sorted(E.BIG)


def test_the_case_list():
    assert len(NAMES) == len(set(NAMES)) == 73
    assert {c.family for c in E.cases()} == {"A1", "A2", "A3", "A5", "A6", "B1", "B2", "B3", "B4", "B5"}
    for fam, counts in (("A1", E.A1_COUNTS), ("B1", E.B1_COUNTS)):
        got = {v for c in E.cases() if c.family == fam for w, _m, _b, v in c.claims if w == "n_edges"}
        assert set(counts) <= got, fam


@pytest.mark.parametrize("name", NAMES)
def test_case_sits_where_it_claims(name):
    c = E.case(name)
    assert c.claims
    for claim in c.claims:
        check_claim(c, claim)
    if c.dec and any(x[:1] == b"L" for x in c.lines):
        _check_decimal_keys(c)
    if c.dec and c.head[1] >= E.HEAD_DEVICE:  # a decimal line never outgrows the stage
        assert all(st for m in E.MODES for _p0, _p1, _b, st in E.plan_of(c.lines, m))


SMALL = [c.name for c in E.cases() if E.input_bytes(c) <= E.ORACLE_MAX_BYTES]


def test_the_size_cut_off_leaves_out_only_the_multi_megabyte_cases():
    left_out = sorted(set(NAMES) - set(SMALL))
    assert left_out == sorted([E.A4_NAME, E.B1_BIG_NAME, "B3_boundaries_to_8_digits", "B4_9_digits", "B5_10_digits"])


@pytest.mark.parametrize("name", SMALL)
def test_model_equals_oracle(oracle_lib, name):
    c = E.case(name)
    data = E.data_of(c)
    line0 = E.n_head_lines(c)
    for bidir in E.MODES:
        want = E.model(c.lines, bidir, line0)
        text, err, _first = oracle_lib.export_edge_list(data, bidirected=bidir)
        assert text == want.text, (name, bidir)
        if want.status == 0:
            assert err is None
        elif want.status == E.E_UNICODE:
            assert err == ("decode", want.err_detail)
            assert text.count(b"\n") == want.err_index
        else:
            assert err[0] == "status" and (err[1].status, err[1].err_line) == (want.status, want.err_line)
    # which render the build must take: the arithmetic one exactly where the tile-local decimal parse accepts
    if want.status != E.E_MALFORMED_L:
        assert T.expect_local(data) == c.dec, name
    else:  # (the failing build is re-run on the prefix before the line: that prefix decides)
        cut = sum(len(x) for x in E.head_lines(c)) + sum(len(x) for x in c.lines[:want.err_line - line0])
        assert T.expect_local(data[:cut]) == c.dec, name
