"""BASELINE.json's configs at full size on one MI355X.

* C3 (1M S / 4M L, ``bidirected=True, weight_tag="RC"``) and C4 (50M S / 200M L, default flags:
  the MAX-SYM CSR): bit for bit against the oracle's answers on the same generator bytes, through
  digests the oracle computed in the build container (tests/golden/make_synth_digests.py ->
  tests/golden/expected/synth_digests.json; oracle/g2n_oracle.cpp is pinned against the real
  reference's goldens).  The reference's own C3 timing run on these bytes
  reported the same nnz (profiles/r01/reference_cpu_times.json: 12 698 170).
* C5 (125M S / 500M L, ``directed=False``, 16 GB) on ONE GPU — its single-device size fits
  288 GB of HBM: the SUM CSR through the size-independent properties the reference's semantics
  fix (builders.py:222-228, utils.py:40-63: every L line adds (u, v) and (v, u) with value 1,
  coo.tocsr sums duplicates), no oracle digest (the oracle needs more host memory than the build
  container has at this size: parity unpinned beyond these properties).
"""
import ctypes
import hashlib
import io
import json
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _hbm_to_spare():
    """Each full-size build starts with the device as free as the process can make it: the round-end
    suite runs every test in one process, and earlier tests' garbage, the host entry points' cached
    buffers and torch's cached blocks would otherwise stand in the way of a 1.1G-edge build."""
    import gc

    from gfa2network_amd import _native as nat

    gc.collect()
    nat.release_shared(0)
    yield


DIGESTS = json.loads((Path(__file__).parent / "golden" / "expected" / "synth_digests.json").read_text())


def _digest(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _hip():
    hip = ctypes.CDLL("libamdhip64.so.7")  # the runtime libg2n.so loaded (its SONAME)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return hip


def _down(hip, ptr, n, dtype):
    out = np.empty(n, dtype=dtype)
    if n:
        assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
    return out


def _device_build(n_s, n_l, names="decimal", **opts):
    """g2n_build_device on generator bytes in HBM; the result's arrays downloaded."""
    from gfa2network_amd import _native as nat
    from gfa2network_amd import synth

    lib = nat.load()
    hip = _hip()
    dev = synth.DeviceInput(n_s, n_l, seed=0, names=names)
    ctx = lib.g2n_context_create(0)
    try:
        o = nat.make_options(**opts)
        res = nat.Result()
        rc = lib.g2n_build_device(ctx, dev.ptr, dev.len, ctypes.byref(o), ctypes.byref(res))
        assert rc == 0, (nat.status_name(rc), nat.last_error())
        n, nnz = int(res.n_nodes), int(res.nnz)
        out = {"n": n, "nnz": nnz, "format": res.format, "n_edges": int(res.n_edges)}
        out["phases"] = [res.phase_names[k].decode() for k in range(res.n_phases)]
        if res.format == nat.FMT_CSR:
            out["indptr"] = _down(hip, res.indptr, n + 1, np.int32)
            out["indices"] = _down(hip, res.indices, nnz, np.int32)
        else:
            out["rows"] = _down(hip, res.rows, nnz, np.int32)
            out["cols"] = _down(hip, res.cols, nnz, np.int32)
        out["data"] = _down(hip, res.data, nnz, np.float64)
        offs = _down(hip, res.names_offsets, n + 1, np.int64)
        out["offsets"] = offs
        out["blob"] = _down(hip, res.names_blob, int(offs[-1]), np.uint8)
    finally:
        lib.g2n_context_destroy(ctx)
        dev.free()
    return out


def test_c3_full_size_equals_oracle(gpu):
    """C3 through the reference's call surface (parse_gfa + convert_format) and the CSR output."""
    from gfa2network_amd import _native as nat
    from gfa2network_amd import convert_format, parse_gfa, synth

    d = DIGESTS["C3"]
    data = synth.host_bytes(d["n_segments"], d["n_links"], seed=d["seed"], rc_tag=d["rc_tag"])
    assert len(data) == d["input_bytes"]
    A, nodes = parse_gfa(io.BytesIO(data), build_graph=False, build_matrix=True, return_node_list=True,
                         **d["mode"])
    assert A.format == d["parse"]["format"] == "coo" and A.shape == (d["n_nodes"], d["n_nodes"])
    assert A.nnz == d["parse"]["nnz"]
    assert _digest(A.row.astype(np.int32), A.col.astype(np.int32), A.data) == d["parse"]["digest"]
    assert hashlib.sha256("".join(nodes).encode()).hexdigest() == d["names"]
    C = convert_format(A, "csr")
    assert C.nnz == d["csr"]["nnz"]
    assert _digest(C.indptr, C.indices, C.data) == d["csr"]["digest"]
    # the same CSR straight from the build (G2N_OUT_CSR)
    raw = nat.build_from_buffer(data, nat.make_options(output=nat.OUT_CSR, bidirected=True, weight_tag="RC"))
    assert raw.status == 0 and _digest(raw.indptr, raw.indices, raw.data) == d["csr"]["digest"]


def test_c2_full_size_equals_oracle(gpu):
    """C2 (1M S / 4M L, ``directed=False``) as configured: the stream-order COO parse_gfa returns and
    its ``convert_format(A, "csr")`` (utils.py:55 ``coo.tocsr``: the SUM CSR whose partition pairs
    adjacent mutually transposed entries, g2n_sym.hip pass 4), through parse_gfa + convert_format,
    through G2N_OUT_CSR from a host buffer, and device-resident (g2n_build_device, the bench's
    C2 leg) on the decimal and the hash dictionary tiers."""
    from gfa2network_amd import _native as nat
    from gfa2network_amd import convert_format, parse_gfa, synth

    d = DIGESTS["C2"]
    data = synth.host_bytes(d["n_segments"], d["n_links"], seed=d["seed"], rc_tag=d["rc_tag"])
    assert len(data) == d["input_bytes"]
    A, nodes = parse_gfa(io.BytesIO(data), build_graph=False, build_matrix=True, return_node_list=True,
                         **d["mode"])
    assert A.format == d["parse"]["format"] == "coo" and A.shape == (d["n_nodes"], d["n_nodes"])
    assert _digest(A.row.astype(np.int32), A.col.astype(np.int32), A.data) == d["parse"]["digest"]
    assert hashlib.sha256("".join(nodes).encode()).hexdigest() == d["names"]
    C = convert_format(A, "csr")
    assert C.nnz == d["csr"]["nnz"]
    assert _digest(C.indptr, C.indices, C.data) == d["csr"]["digest"]
    raw = nat.build_from_buffer(data, nat.make_options(output=nat.OUT_CSR, directed=False))
    assert raw.status == 0 and _digest(raw.indptr, raw.indices, raw.data) == d["csr"]["digest"]
    for flags in (0, nat.TEST_DICT_HASH):
        out = _device_build(d["n_segments"], d["n_links"], output=nat.OUT_CSR, directed=False, test_flags=flags)
        assert out["format"] == nat.FMT_CSR and out["n"] == d["n_nodes"] and out["nnz"] == d["csr"]["nnz"]
        assert _digest(out["indptr"], out["indices"], out["data"]) == d["csr"]["digest"], flags
        assert hashlib.sha256(out["blob"].tobytes()).hexdigest() == d["names"], flags


@pytest.mark.parametrize("flags", ["decimal", "hash"])
def test_c4_full_size_equals_oracle(gpu, flags):
    """C4 (200M edges, the bench's workload) bit for bit: decimal-id dictionary + bucket MAX-SYM, and
    the hash dictionary tier on the same bytes."""
    from gfa2network_amd import _native as nat

    d = DIGESTS["C4"]
    out = _device_build(d["n_segments"], d["n_links"], output=nat.OUT_PARSE,
                        test_flags=0 if flags == "decimal" else nat.TEST_DICT_HASH)
    assert out["format"] == nat.FMT_CSR and out["n"] == d["n_nodes"] and out["nnz"] == d["parse"]["nnz"]
    assert _digest(out["indptr"], out["indices"], out["data"]) == d["parse"]["digest"]
    assert hashlib.sha256(out["blob"].tobytes()).hexdigest() == d["names"]


def test_c4_permuted_names_full_size_equals_oracle(gpu):
    """C4's dimensions with the segment names a permutation of 1..N (synth names="permuted"): the
    direct-address dictionary tier (S lines claim direct[v], one 4-byte read per edge name) bit for
    bit against the oracle's digest of the same bytes (tests/golden/make_synth_digests.py C4P)."""
    from gfa2network_amd import _native as nat

    d = DIGESTS["C4P"]
    out = _device_build(d["n_segments"], d["n_links"], names="permuted", output=nat.OUT_PARSE)
    assert out["format"] == nat.FMT_CSR and out["n"] == d["n_nodes"] and out["nnz"] == d["parse"]["nnz"]
    assert _digest(out["indptr"], out["indices"], out["data"]) == d["parse"]["digest"]
    assert hashlib.sha256(out["blob"].tobytes()).hexdigest() == d["names"]


def test_c4_prefixed_names_full_size_equals_oracle(gpu):
    """C4's dimensions with minigraph's names "s1".."sN" in S order (synth names="prefixed"): the
    direct-address tier with a one-byte prefix, bit for bit against the oracle's digest of the same
    bytes (tests/golden/make_synth_digests.py C4X)."""
    from gfa2network_amd import _native as nat

    d = DIGESTS["C4X"]
    out = _device_build(d["n_segments"], d["n_links"], names="prefixed", output=nat.OUT_PARSE)
    assert out["format"] == nat.FMT_CSR and out["n"] == d["n_nodes"] and out["nnz"] == d["parse"]["nnz"]
    assert _digest(out["indptr"], out["indices"], out["data"]) == d["parse"]["digest"]
    assert hashlib.sha256(out["blob"].tobytes()).hexdigest() == d["names"]


def test_maxsym_finish_by_bucket_ranges_equals_row_sum_path(gpu):
    """The bucket finish overlapped by ranges (F1 of range k + 1 beside the scan and F2 of range k) needs
    32 768 buckets; 2^23 rows at 0.25 elements per row (buckets of 256 rows) is the smallest shape with
    that many, so the finish runs in 4 bucket ranges.  Equal to the general row-sum path
    (TEST_NO_BUCKETS), which the goldens pin to the oracle."""
    from gfa2network_amd import _native as nat

    got = _device_build(1 << 23, 1 << 20, output=nat.OUT_PARSE)
    want = _device_build(1 << 23, 1 << 20, output=nat.OUT_PARSE, test_flags=nat.TEST_NO_BUCKETS)
    assert "maxsym" in got["phases"], got["phases"]
    assert got["format"] == want["format"] == nat.FMT_CSR
    assert got["n"] == want["n"] == 1 << 23 and got["nnz"] == want["nnz"]
    for k in ("indptr", "indices", "data"):
        assert np.array_equal(got[k], want[k]), k


def test_c5_single_gpu_properties(gpu):
    """C5 at full size on one GPU (16 GB in HBM): the undirected SUM CSR's size-independent
    properties, and the stream-order COO (parse_gfa's return value for directed=False)."""
    from gfa2network_amd import _native as nat

    n_s, n_l = 125_000_000, 500_000_000
    out = _device_build(n_s, n_l, output=nat.OUT_CSR, directed=False)
    n, nnz = out["n"], out["nnz"]
    indptr, indices, data = out["indptr"], out["indices"], out["data"]
    assert n == n_s and out["n_edges"] == n_l
    assert indptr[0] == 0 and indptr[-1] == nnz and np.all(np.diff(indptr) >= 0)
    # every L line contributes (u, v) and (v, u) with value 1.0; duplicates summed (exact in f64)
    assert data.sum() == 2.0 * n_l and np.all(data >= 1.0) and np.all(data == np.floor(data))
    # canonical: strictly increasing columns inside every row
    inc = np.diff(indices.astype(np.int64))
    row_starts = np.zeros(nnz, dtype=bool)
    row_starts[indptr[1:-1][indptr[1:-1] < nnz]] = True
    assert np.all((inc > 0) | row_starts[1:])
    assert indices.min() >= 0 and indices.max() < n
    # symmetric: (r, c, v) present iff (c, r, v) present — on a sample of 2^17 entries
    rng = np.random.default_rng(5)
    pick = rng.integers(0, nnz, 1 << 17)
    rows_of = np.searchsorted(indptr, pick, side="right") - 1
    cols = indices[pick]
    lo, hi = indptr[cols], indptr[cols + 1]
    found = np.empty(len(pick), dtype=bool)
    vals = np.empty(len(pick))
    for k in range(len(pick)):  # per-row binary searches (rows are short)
        seg = indices[lo[k]:hi[k]]
        j = np.searchsorted(seg, rows_of[k])
        found[k] = j < len(seg) and seg[j] == rows_of[k]
        vals[k] = data[lo[k] + j] if found[k] else -1
    assert found.all() and np.array_equal(vals, data[pick])
    # names: S lines name "1".."N" in order, so node k is str(k + 1)
    lens = np.diff(out["offsets"])
    k = np.arange(1, n + 1, dtype=np.int64)
    assert np.array_equal(lens, np.searchsorted(10 ** np.arange(1, 19, dtype=np.int64), k, side="right") + 1)
    blob = out["blob"]
    for i in rng.integers(0, n, 4096):
        assert blob[out["offsets"][i]:out["offsets"][i + 1]].tobytes() == str(i + 1).encode()
    del out, indices, data, indptr
    # the stream-order COO: entry 2e = (u_e, v_e), 2e + 1 = (v_e, u_e)
    coo = _device_build(n_s, n_l, output=nat.OUT_PARSE, directed=False)
    assert coo["format"] == nat.FMT_COO and coo["nnz"] == 2 * n_l
    r, c = coo["rows"], coo["cols"]
    assert np.array_equal(r[0::2], c[1::2]) and np.array_equal(c[0::2], r[1::2])
    assert np.all(coo["data"] == 1.0)


def test_int64_indices_past_2_31_entries(gpu):
    """One GPU, more than 2^31 - 1 entries: 275M S / 1.1G L undirected (40 GB in HBM, 2.2G COO triplets),
    the CSR convert_format returns (utils.py:55 coo.tocsr, whose index dtype follows the COO's entries
    with duplicates) in scipy's int64 index dtype —
    checked on the device with torch: indptr int64, starts at 0, ends at nnz, non-decreasing; every
    row's columns strictly increasing and < n; the values sum to 2 x edges (each L line adds (u, v)
    and (v, u) with value 1; exact in float64).  Parity beyond these properties is the forced int64
    path's (test_gpu_diff.py::test_int64_index_path_equals_oracle) and the int32 builds'."""
    import torch

    from gfa2network_amd import _native as nat
    from gfa2network_amd import synth

    n_s, n_l = 275_000_000, 1_100_000_000
    lib = nat.load()
    hip = nat.hip_runtime()
    dev = synth.DeviceInput(n_s, n_l, seed=0)
    ctx = lib.g2n_context_create(0)
    try:
        o = nat.make_options(output=nat.OUT_CSR, directed=False, want_node_names=False)
        res = nat.Result()
        rc = lib.g2n_build_device(ctx, dev.ptr, dev.len, ctypes.byref(o), ctypes.byref(res))
        assert rc == 0, (nat.status_name(rc), nat.last_error())
        n, nnz = int(res.n_nodes), int(res.nnz)
        # coo.tocsr() sizes the index dtype by the COO's 2.2G triplets (duplicates included)
        assert n == n_s and int(res.n_edges) == n_l and 2 * n_l > 2**31 - 1 and res.index_width == 8

        def copy(ptr, count, dtype):
            t = torch.empty(count, dtype=dtype, device="cuda")
            assert hip.hipMemcpy(t.data_ptr(), ptr, t.numel() * t.element_size(), 3) == 0
            return t

        indptr = copy(res.indptr, n + 1, torch.int64)
        assert int(indptr[0]) == 0 and int(indptr[-1]) == nnz
        assert bool((indptr[1:] >= indptr[:-1]).all())
        data = copy(res.data, nnz, torch.float64)
        assert float(data.sum()) == 2.0 * n_l and bool((data >= 1).all())
        del data
        torch.cuda.empty_cache()
        indices = copy(res.indices, nnz, torch.int64)
        assert int(indices.min()) >= 0 and int(indices.max()) < n
        starts = torch.zeros(nnz, dtype=torch.bool, device="cuda")
        rs = indptr[1:-1]
        starts[rs[rs < nnz]] = True
        inc = indices[1:] > indices[:-1]
        assert bool((inc | starts[1:]).all())
        del indptr, indices, starts, rs, inc
    finally:
        lib.g2n_context_destroy(ctx)
        dev.free()
        # torch's caching allocator would keep the ~25 GB of checks above reserved for the rest of the
        # process: the next tests' 1.1G-edge builds need that HBM
        torch.cuda.empty_cache()


class _Reader:
    """A file object over bytes already in host memory (parse_gfa reads file objects whole,
    parser.py:90-92): no second copy of a 36 GB input."""

    def __init__(self, arr):
        self.arr = arr

    def read(self):
        return self.arr


def test_convert_format_int64_past_2_31_entries(gpu):
    """`convert --undirected` at more than 2^31 - 1 COO entries (utils.py:55, cli.py:239): 275M S /
    1.1G L through the product's parse_gfa(directed=False) — the stream-order COO of 2.2G triplets in
    host memory — then convert_format(A, "csr") (g2n_coo_to_csr), whose result scipy gives int64
    indptr / indices (_coo_to_compressed sizes by coo.nnz).  Checked: the COO's size and twin pairing,
    int64 indptr from 0 to nnz, non-decreasing; every row's columns strictly increasing and < n; the
    values sum to 2 x edges (exact in float64).  Parity beyond these properties: the forced int64 path
    (test_gpu_diff.py::test_convert_format_int64_path_equals_oracle) and the int32 conversions."""
    from gfa2network_amd import convert_format, parse_gfa
    from gfa2network_amd import synth

    n_s, n_l = 275_000_000, 1_100_000_000
    dev = synth.DeviceInput(n_s, n_l, seed=0)
    try:
        text = np.empty(dev.len, dtype=np.uint8)
        assert synth._lib().g2n_synth_download(text.ctypes.data, dev.ptr, dev.len) == 0
    finally:
        dev.free()
    A = parse_gfa(_Reader(text), build_graph=False, build_matrix=True, directed=False)
    del text
    assert A.format == "coo" and A.shape == (n_s, n_s) and A.nnz == 2 * n_l > 2**31 - 1
    step = 1 << 28
    for k in range(0, A.nnz, step):  # every L line adds (u, v) then (v, u)
        r, c = A.row[k:k + step], A.col[k:k + step]
        assert np.array_equal(r[0::2], c[1::2]) and np.array_equal(c[0::2], r[1::2])
    C = convert_format(A, "csr")
    del A
    assert C.format == "csr" and C.indptr.dtype == np.int64 and C.indices.dtype == np.int64
    ip, ix = C.indptr, C.indices
    nnz = int(ip[-1])
    assert int(ip[0]) == 0 and nnz == len(ix) == len(C.data) and bool(np.all(ip[1:] >= ip[:-1]))
    total = 0.0
    starts = np.zeros(step + 1, dtype=bool)
    for k in range(0, nnz, step):
        seg = ix[k:k + step + 1]
        assert int(seg.min()) >= 0 and int(seg.max()) < n_s
        starts[:] = False  # row starts inside [k, k + len(seg)) may break the increase
        lo, hi = np.searchsorted(ip, [k, k + len(seg)])
        rs = ip[lo:hi] - k
        starts[rs[(rs > 0) & (rs < len(seg))]] = True
        inc = seg[1:] > seg[:-1]
        assert bool(np.all(inc | starts[1:len(seg)]))
        total += float(C.data[k:k + step].sum())
    assert total == 2.0 * n_l


def test_convert_format_weighted_past_2_31_entries(gpu):
    """`convert --undirected --weight-tag RC` at more than 2^31 - 1 COO entries (VERDICT r05 item 5;
    utils.py:55, cli.py:239): 275M S / 1.1G L with RC:i tags through parse_gfa(directed=False,
    weight_tag="RC") — a 2.2G-triplet weighted COO in host memory — then convert_format(A, "csr"),
    which converts a weighted COO past one call's limit in row bands (_coo_to_csr_bands).  Checked:
    int64 indptr / indices (scipy's _coo_to_compressed sizes by coo.nnz), indptr from 0 to nnz and
    non-decreasing, every row's columns strictly increasing and < n, and the values' exact sum equal
    to the COO's (integer weights: exact in float64).  Parity beyond these properties: the banded
    route bit for bit against scipy (test_gpu_diff.py::test_coo_to_csr_row_bands_equal_scipy) and the
    forced int64 route (::test_convert_format_int64_path_equals_oracle)."""
    from gfa2network_amd import convert_format, parse_gfa
    from gfa2network_amd import synth

    n_s, n_l = 275_000_000, 1_100_000_000
    dev = synth.DeviceInput(n_s, n_l, seed=0, rc_tag=True)
    try:
        text = np.empty(dev.len, dtype=np.uint8)
        assert synth._lib().g2n_synth_download(text.ctypes.data, dev.ptr, dev.len) == 0
    finally:
        dev.free()
    A = parse_gfa(_Reader(text), build_graph=False, build_matrix=True, directed=False, weight_tag="RC")
    del text
    assert A.format == "coo" and A.shape == (n_s, n_s) and A.nnz == 2 * n_l > 2**31 - 1
    step = 1 << 28
    want = 0.0
    for k in range(0, A.nnz, step):
        want += float(A.data[k:k + step].sum())
    assert not np.all(A.data[:1000] == 1.0)
    C = convert_format(A, "csr")
    del A
    assert C.format == "csr" and C.indptr.dtype == np.int64 and C.indices.dtype == np.int64
    ip, ix = C.indptr, C.indices
    nnz = int(ip[-1])
    assert int(ip[0]) == 0 and nnz == len(ix) == len(C.data) and bool(np.all(ip[1:] >= ip[:-1]))
    total = 0.0
    starts = np.zeros(step + 1, dtype=bool)
    for k in range(0, nnz, step):
        seg = ix[k:k + step + 1]
        assert int(seg.min()) >= 0 and int(seg.max()) < n_s
        starts[:] = False
        lo, hi = np.searchsorted(ip, [k, k + len(seg)])
        rs = ip[lo:hi] - k
        starts[rs[(rs > 0) & (rs < len(seg))]] = True
        inc = seg[1:] > seg[:-1]
        assert bool(np.all(inc | starts[1:len(seg)]))
        total += float(C.data[k:k + step].sum())
    assert total == want
