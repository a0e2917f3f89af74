"""CPU: the components call surface without a GPU — the completeness of
tests/golden/expected/components.json and its agreement with scipy on the CPU oracle's asymmetric
matrix, the result object's slicing and rebasing (over arrays the checker makes), the CLI schema,
the exports, the C struct's layout, the label writer under the sanitizers, and the loud failure
without a device."""
import ctypes
import gzip
import json
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import components_util as cu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
CSRC = ROOT / "gfa2network_amd" / "csrc"
sys.path.insert(0, str(GOLDEN))
from make_components_golden import rle, unrle  # noqa: E402
from make_stats_golden import cases  # noqa: E402  (the generator's own list of cases)


@pytest.fixture(scope="module")
def expected():
    return json.loads((GOLDEN / "expected" / "components.json").read_text())


def test_fixture_holds_every_case(expected):
    want = [c[0] for c in cases()]
    assert len(want) == len(set(want)) and sorted(expected) == sorted(want)
    stats = json.loads((GOLDEN / "expected" / "stats.json").read_text())
    for key, rec in expected.items():
        assert (rec["labels"] is None) != (rec["exc"] is None), key
        assert rec["exc"] == stats[key]["exc"], key  # the exceptions are compute_stats's
        if rec["labels"] is not None:
            lab = unrle(rec["labels"])
            s = dict(stats[key]["stats"])
            assert len(lab) == s["nodes"] and (max(lab) + 1 if lab else 0) == s["components"], key
            assert rle(lab) == rec["labels"], key


def test_fixture_is_scipys_numbering_of_the_oracles_matrix(oracle_lib, expected):
    """The contract: the reference's numbering (nx.connected_components over first-touch node order) is
    scipy's connected_components(directed=False) of the asymmetric summed CSR the build leaves in HBM."""
    seen = 0
    for key, inp, directed, strip, _raw in cases():
        rec = expected[key]
        if rec["labels"] is None:
            continue
        data = inp.read_bytes()
        if inp.name.endswith(".gz"):
            data = gzip.decompress(data)
        o = oracle_lib.run(data, directed=directed, asymmetric=True, strip_orientation=strip, dtype="float64")
        assert o.status == 0, key
        k, lab = cu.want_labels(o.sum_indptr, o.sum_indices, o.n_nodes)
        assert lab.tolist() == unrle(rec["labels"]), key
        seen += 1
    assert seen >= 200


def numpy_split(A):
    """The result object over arrays made by the checker alone (what the GPU must produce)."""
    from gfa2network_amd.api import ComponentSplit

    n = A.shape[0]
    ip, ix, data = A.indptr, A.indices, A.data
    k, lab = cu.want_labels(ip, ix, n)
    perm, off, _sizes = cu.want_grouping(lab, k)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    lens = (ip[perm + 1] - ip[perm]).astype(np.int64)
    oip = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=oip[1:])
    src = np.repeat(ip[perm].astype(np.int64) - oip[:-1], lens) + np.arange(oip[-1])
    cols = ix[src].astype(np.int64)
    return ComponentSplit(A.dtype, lab, perm, off, oip.astype(ip.dtype), (inv[cols] - off[lab[cols]]).astype(ix.dtype),
                          data[src])


@pytest.mark.parametrize("dtype", cu.DTYPES)
def test_result_object_slices_and_rebases(dtype):
    rng = np.random.default_rng(3)
    n = 301
    r = rng.integers(0, n, 220)
    c = (r + n // 2) % n  # interleaved components: perm is not the identity
    r = np.concatenate([r, [5, 5, 5, 7]])
    c = np.concatenate([c, [9, 3, 9, 7]])  # an unsorted row with a duplicate, a self-loop
    ip, ix = cu.csr_of(r, c, n)
    for idt in (np.int32, np.int64):
        A = cu.matrix(ip, ix, n, idt, cu.telling_values(len(ix), dtype))
        assert not cu.is_canonical(A.indptr, A.indices)
        S = numpy_split(A)
        assert cu.check_split(S, A) == S.n_components > 1 and not np.array_equal(S.perm, np.arange(n))
        B = A.copy()
        B.sum_duplicates()
        B.sort_indices()
        assert cu.is_canonical(B.indptr, B.indices)
        cu.check_split(numpy_split(B), B)
        with pytest.raises(IndexError):
            S.component(S.n_components)
        with pytest.raises(IndexError):
            S.component(-1)


def test_largest_takes_the_lowest_label_on_ties():
    ip, ix = cu.csr_of([0, 2, 4], [1, 3, 5], 7)  # three pairs and a single node
    S = numpy_split(cu.matrix(ip, ix, 7, np.int32))
    assert S.sizes.tolist() == [2, 2, 2, 1]
    L, nodes = S.largest()
    assert nodes.tolist() == [0, 1] and L.toarray().tolist() == [[0.0, 1.0], [0.0, 0.0]]


def test_components_parser():
    from gfa2network_amd.cli import _parser

    p = _parser(extensions=True)
    a = p.parse_args(["components", "x.gfa"])
    assert (a.cmd, a.gfa, a.output, a.directed, a.strip_orientation, a.sizes, a.raw_bytes_id, a.device) == \
        ("components", "x.gfa", "-", True, False, False, False, 0)
    a = p.parse_args(["--raw-bytes-id", "--device", "1", "components", "x.gfa", "-o", "out.tsv", "--undirected",
                      "--strip-orientation", "--sizes"])
    assert (a.output, a.directed, a.strip_orientation, a.sizes, a.raw_bytes_id, a.device) == \
        ("out.tsv", False, True, True, True, 1)
    for bad in (["components"], ["components", "x.gfa", "--directed", "--undirected"], ["components", "a", "b"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit):  # the reference's schema has no such subcommand
        _parser().parse_args(["components", "x.gfa"])


def test_component_functions_are_exported():
    import gfa2network_amd
    from gfa2network_amd import _native, api

    for name in ("graph_components", "split_components", "node_components"):
        assert name in gfa2network_amd.__all__ and callable(getattr(gfa2network_amd, name))
        assert name in api.__all__
    lib = _native.load()
    for sym in ("g2n_csr_components", "g2n_csr_components_host", "g2n_csr_split_components_host",
                "g2n_components_from_path", "g2n_write_node_labels"):
        assert sym in _native.EXPORTED and hasattr(lib, sym)
    assert lib.g2n_abi_version() == 2
    src = (CSRC / "g2n_components.hip").read_text()
    assert f"kSplitShortRow = {_native.SPLIT_SHORT_ROW};" in src
    assert f"kSplitHugeRow = {_native.SPLIT_HUGE_ROW};" in src


def test_components_info_struct_matches_header(tmp_path):
    from gfa2network_amd import _native

    py = _native.ComponentsInfo
    lines = ['printf("sizeof %zu\\n", sizeof(g2n_components_info));']
    lines += [f'printf("{f[0]} %zu\\n", offsetof(g2n_components_info, {f[0]}));' for f in py._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "g2n.h"\nint main(void) {\n'
                   + "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                   text=True).stdout.splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(py)
    for f in py._fields_:
        assert int(got[f[0]]) == getattr(py, f[0]).offset, f[0]


def test_argument_checks_and_empty_matrix():
    from gfa2network_amd import graph_components, node_components, split_components

    for f in (graph_components, split_components):
        with pytest.raises(TypeError):
            f(np.zeros((2, 2)))
        with pytest.raises(ValueError):
            f(sp.csr_matrix((2, 3)))
    with pytest.raises(NotImplementedError):
        split_components(sp.csr_matrix(np.eye(2, dtype=np.int64)))
    with pytest.raises(NotImplementedError):
        split_components(sp.csr_matrix(np.eye(2, dtype=np.complex128)))
    k, lab = graph_components(sp.csr_matrix((0, 0)))  # no GPU call
    assert k == 0 and lab.dtype == np.int32 and lab.shape == (0,)
    S = split_components(sp.csr_matrix((0, 0), dtype=np.float32))
    assert S.n_components == 0 and S.sizes.tolist() == [] and S.labels.dtype == np.int32
    with pytest.raises(NotImplementedError):
        node_components("-")
    import io

    with pytest.raises(NotImplementedError):
        node_components(io.BytesIO(b"S\ta\n"))


@pytest.mark.skipif(shutil.which("g++") is None or not Path("/opt/rocm/include/hip/hip_runtime.h").exists(),
                    reason="needs g++ and the ROCm headers (the HIP upload path is linked, never called)")
def test_label_writer_under_asan_ubsan(tmp_path):
    """g2n_write_node_labels (g2n_writers.cpp) built with g++ under AddressSanitizer +
    UndefinedBehaviorSanitizer and driven by the stand-alone tests/native/labels_check.cpp."""
    exe = tmp_path / "labels_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           str(ROOT / "tests" / "native" / "labels_check.cpp"), str(CSRC / "g2n_ingest.cpp"),
           str(CSRC / "g2n_pinflate.cpp"), str(CSRC / "g2n_split.cpp"), str(CSRC / "g2n_writers.cpp"),
           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-lz", "-lpthread", "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", G2N_HOST_THREADS="4")
    r = subprocess.run([str(exe), str(tmp_path)], env=env, capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == b"OK", r.stderr.decode(errors="replace")[-4000:]


def test_label_writer_matches_python(tmp_path):
    from gfa2network_amd import _native

    names = [b"a", b"", b"s12:+", "été".encode(), b"x" * 300]
    blob = np.frombuffer(b"".join(names), dtype=np.uint8)
    offs = np.cumsum([0] + [len(x) for x in names]).astype(np.int64)
    labels = np.array([0, 1, 0, 2147483647, 12], dtype=np.int32)
    dest = tmp_path / "l.tsv"
    assert _native.write_node_labels(str(dest), blob, offs, labels, True) == -1
    assert dest.read_bytes() == b"".join(n + b"\t%d\n" % v for n, v in zip(names, labels))
    bad = [b"ok", b"\xff\xfe", b"later"]
    blob = np.frombuffer(b"".join(bad), dtype=np.uint8)
    offs = np.cumsum([0] + [len(x) for x in bad]).astype(np.int64)
    assert _native.write_node_labels(str(dest), blob, offs, labels[:3], True) == 1
    assert dest.read_bytes() == b"ok\t0\n"
    assert _native.write_node_labels(str(dest), blob, offs, labels[:3], False) == -1
    assert dest.read_bytes() == b"ok\t0\n\xff\xfe\t1\nlater\t0\n"
    assert _native.write_node_labels(str(dest), np.zeros(0, np.uint8), np.zeros(1, np.int64), labels[:0], True) == -1
    assert dest.read_bytes() == b""
    with pytest.raises(OSError):
        _native.write_node_labels(str(tmp_path / "no" / "such.tsv"), blob, offs, labels[:3], False)


@pytest.mark.skipif(__import__("gfa2network_amd._native", fromlist=["x"]).device_count() > 0,
                    reason="a GPU is visible")
def test_components_without_gpu_fail_loudly(tmp_path):
    from gfa2network_amd import graph_components, node_components, split_components

    p = tmp_path / "a.gfa"
    p.write_bytes(b"S\ta\nL\ta\t+\tb\t+\t*\n")
    A = sp.csr_matrix(np.array([[0.0, 1.0], [0.0, 0.0]]))
    with pytest.raises(RuntimeError, match="G2N_E_DEVICE"):
        node_components(p)
    with pytest.raises(RuntimeError, match="G2N_E_DEVICE"):
        graph_components(A)
    with pytest.raises(RuntimeError, match="G2N_E_DEVICE"):
        split_components(A)
