"""The edge-list export renders — the blob render (k_name_meta, k_edge_text_len, k_edge_text) and the arithmetic
render of a decimal-id build (k_edge_dec_sum, k_edge_dec_text, decfmt.h), and k_names_dec beside them — against a
plain line model at the sizes they branch on: edge counts around a block and a thread's four edges, a block's text
on and one past the LDS stage at three phases of the 16-byte word, staged blocks beside unstaged ones with every
join inside a word, key lengths around the 23- and 24-bit saturations, undecodable keys racing for the first edge,
a malformed line cut on a block boundary, every decimal key width to 10 digits in every thread slot, a block-sum
scan of two tiles.  tests/edge_text_util.py builds the cases and restates the geometry; tests/test_edge_text_cases.py
shows on the CPU that each case sits where it claims and that the oracle equals the model on the small ones.

Every case runs plain and bidirected: the text byte for byte, the status, err_line, err_index and err_detail are
the model's, and the render read from the phases (a "names" phase: the blob render) is the one the case must take.
A decimal case of up to 10^7 segments gives the same bytes through the blob render (TEST_NO_DEC_TEXT).  The 9- and
10-digit cases live in HBM only: their S section is generated there and the test's L lines copied behind it."""
import ctypes
import gc
import io
import time

import numpy as np
import pytest

import edge_text_util as E

pytestmark = pytest.mark.gpu


def _same(got: bytes, want: bytes, what):
    """got == want, reporting the first byte that differs (the texts reach 150 MB)."""
    if got == want:
        return
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    n = min(len(a), len(b))
    d = np.flatnonzero(a[:n] != b[:n])
    at = int(d[0]) if len(d) else n
    lo = max(0, at - 40)
    raise AssertionError(f"{what}: {len(got)} bytes against the model's {len(want)}; first difference at byte {at} "
                         f"(block {at // 16 * 16}+{at % 16}): {got[lo:at + 24]!r} against {want[lo:at + 24]!r}")


def _check_result(c, bidir, want, status, err_line, err_index, err_detail, text, phases, blob):
    what = (c.name, E.TAG[bidir], "blob render" if blob else "default")
    _same(text, want.text, what)
    assert status == want.status, what
    if want.status == E.E_UNICODE:
        assert (err_line, err_index, err_detail) == (-1, want.err_index, want.err_detail), what
    elif want.status == E.E_MALFORMED_L:
        assert err_line == want.err_line, what
    if status == 0:  # the render the case must take: a "names" phase is the blob render's
        assert ("names" in phases) == blob, (what, sorted(phases))


def _check_host(nat, c, data, line0, no_dec_text=False):
    """Both modes of one case from a host buffer; returns the two builds' phase times."""
    phases = []
    for bidir in E.MODES:
        want = E.model(c.lines, bidir, line0)
        flags = nat.TEST_NO_DEC_TEXT if no_dec_text else 0
        raw = nat.build_from_buffer(data, nat.make_options(bidirected=bidir, output=nat.OUT_EDGE_LIST,
                                                           test_flags=flags))
        text = raw.data.tobytes() if raw.format == "text" else b""
        _check_result(c, bidir, want, raw.status, raw.err_line, raw.err_index, raw.err_detail, text, raw.phase_ms,
                      blob=no_dec_text or not c.dec)
        phases.append(raw.phase_ms)
    return phases


def _check_small(nat, c):
    data = E.data_of(c)
    _check_host(nat, c, data, E.n_head_lines(c))
    if c.dec:
        _check_host(nat, c, data, E.n_head_lines(c), no_dec_text=True)


SMALL_FAMILIES = ("A1", "A2", "A3", "A5", "A6", "B1", "B2")


def test_every_case_has_a_test():
    rest = {c.name for c in E.cases() if c.family not in SMALL_FAMILIES} | set(E.BIG)
    assert rest == {E.A4_NAME, E.B1_BIG_NAME, "B3_boundaries_to_8_digits", "B4_9_digits", "B5_10_digits"}


@pytest.mark.parametrize("family", SMALL_FAMILIES)
def test_edge_text_cases(gpu, family):
    some = [c for c in E.cases() if c.family == family and c.note == ""]
    assert some
    for c in some:
        _check_small(gpu, c)


def test_a4_keys_around_the_length_saturations(gpu):
    """Keys of 0x7FFFFE .. 0x1000000 bytes, each once as u and once as v ("a key longer than 16 MiB
    takes a slower length lookup"): the saturated lengths in `meta` (23 bits) and `em` (24 bits) fall back to the
    offsets.  150 MB of input and of text; every pass that walks a key walks it in one thread: 33 s on the MI355X
    for the two builds (per build insert_lookup 11 s, edge_text 3.2 s, parse 1.9 s) — the one slow test here, at
    the sizes the saturations sit at."""
    c = E.case(E.A4_NAME)
    data = E.data_of(c)
    t0 = time.perf_counter()
    phases = _check_host(gpu, c, data, E.n_head_lines(c))
    print(f"A4: {time.perf_counter() - t0:.2f} s for the plain and the bidirected build of {len(data)} bytes")
    for ms in phases:  # where the time goes: every phase of a second or more
        print("A4 phases (s):", {k: round(v / 1e3, 2) for k, v in ms.items() if v >= 1e3})


def test_b1_block_sums_span_two_scan_tiles(gpu):
    """4096 x 1024 + 5 edges: 4098 block sums against kScanTile = 4096."""
    c = E.case(E.B1_BIG_NAME)
    data = E.data_of(c)
    _check_host(gpu, c, data, E.n_head_lines(c))
    _check_host(gpu, c, data, E.n_head_lines(c), no_dec_text=True)


def test_b3_boundaries_to_8_digits(gpu):
    """N = 10^7 + 2: 10^k - 1, 10^k, 10^k + 1 for k = 1 .. 7, every high half 0 .. 1000 and 2^j - 1, 2^j up to
    j = 23, each as u and as v in each of a thread's four slots."""
    from gfa2network_amd import synth

    c = E.case("B3_boundaries_to_8_digits")
    t0 = time.perf_counter()
    head = synth.host_bytes(c.head[1], 0)
    assert head.count(b"\nS\t") == c.head[1] and head.endswith(b"\n")
    data = head + b"".join(c.lines)
    del head
    _check_host(gpu, c, data, 0)
    _check_host(gpu, c, data, 0, no_dec_text=True)
    print(f"B3: {time.perf_counter() - t0:.2f} s for {len(data)} bytes, four builds")


def _device_case(nat, c, modes):
    """The case's S section generated in HBM, its L lines copied behind it, built with g2n_build_device; the text
    downloaded and compared.  Returns the wall time."""
    from gfa2network_amd import synth

    gc.collect()
    nat.release_shared(0)
    lib, hip = nat.load(), nat.hip_runtime()
    t0 = time.perf_counter()
    tail = b"".join(c.lines) + bytes(64)  # (64 bytes of slack behind the input, as the generator leaves)
    dev = synth.DeviceInput(c.head[1], 0, seed=0)
    buf = ctypes.c_void_p()
    try:
        total = dev.len + len(tail) - 64
        rc = hip.hipMalloc(ctypes.byref(buf), dev.len + len(tail))
        assert rc == 0, f"hipMalloc of {dev.len + len(tail)} bytes: {rc}"
        assert hip.hipMemcpy(buf, dev.ptr, dev.len, 3) == 0
        assert hip.hipMemcpy(buf.value + dev.len, tail, len(tail), 1) == 0
    finally:
        dev.free()
    ctx = lib.g2n_context_create(0)
    try:
        for bidir in modes:
            want = E.model(c.lines, bidir)
            o = nat.make_options(bidirected=bidir, output=nat.OUT_EDGE_LIST)
            res = nat.Result()
            rc = lib.g2n_build_device(ctx, buf, total, ctypes.byref(o), ctypes.byref(res))
            assert rc == 0, (c.name, nat.status_name(rc), nat.last_error())
            assert res.format == nat.FMT_TEXT
            text = np.empty(int(res.nnz), dtype=np.uint8)
            if text.size:
                assert hip.hipMemcpy(text.ctypes.data, res.data, text.nbytes, 2) == 0
            phases = [res.phase_names[k].decode() for k in range(res.n_phases)]
            _check_result(c, bidir, want, res.status, -1, -1, b"", text.tobytes(), phases, blob=False)
    finally:
        lib.g2n_context_destroy(ctx)
        hip.hipFree(buf)
    return time.perf_counter() - t0, total


def test_b4_nine_digits_in_hbm(gpu):
    """N = 10^8 + 64 (2.0 GB of input: the generator's S lines carry sequences): 10^8 - 1, 10^8, 10^8 + 1 in every slot and position, every high half
    0 .. 9999, a full block of maximal 24-byte lines starting at phase 15 of its word."""
    dt, total = _device_case(gpu, E.case("B4_9_digits"), E.MODES)
    print(f"B4: {dt:.2f} s for {total} bytes in HBM, plain and bidirected")


def test_b5_ten_digits_in_hbm(gpu):
    """N = 10^9 + 64 (20.9 GB of input), bidirected: 10^9 - 1, 10^9, 10^9 + 1, the leading digits 1 .. 9 of a
    9-digit key and 10 of a 10-digit one, a full block of 26-byte lines (the static_assert's bound) at phase 15."""
    dt, total = _device_case(gpu, E.case("B5_10_digits"), (True,))
    print(f"B5: {dt:.2f} s for {total} bytes in HBM, bidirected")


@pytest.mark.parametrize("bidir", E.MODES)
def test_b6_arithmetic_node_names(gpu, bidir):
    """k_names_dec / dec_name_off across 10^1 .. 10^6: the node list of parse_gfa is str(k + 1) (+ ":+" / ":-"), and
    the native result's offsets are the cumulative sum of those lengths."""
    from gfa2network_amd import parse_gfa

    n = E.B6_N
    data = b"".join(E.S(k) for k in range(1, n + 1)) + b"".join(E.dec_edges(9, n))
    want = [f"{k}{o}" for k in range(1, n + 1) for o in ((":+", ":-") if bidir else ("",))]
    _A, nodes = parse_gfa(io.BytesIO(data), build_graph=False, build_matrix=True, return_node_list=True,
                          bidirected=bidir)
    assert nodes == want
    raw = gpu.build_from_buffer(data, gpu.make_options(bidirected=bidir))
    assert raw.status == 0 and "parse" in raw.phase_ms and "tiles" not in raw.phase_ms, sorted(raw.phase_ms)
    assert raw.names_offsets.tolist() == E.name_offsets(n, bidir)
    assert raw.names_blob.tobytes() == "".join(want).encode()
