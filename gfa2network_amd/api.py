"""parse_gfa / convert_format with the reference's call surface, backed by libg2n.so.

Mirrors the matrix subset of sclipman/gfa2network:
  * ``parse_gfa(path, *, build_graph, build_matrix, ...)``   gfa2network/builders.py:30-299
  * ``convert_format(A, fmt, *, verbose=False)``             gfa2network/utils.py:40-63

Same keyword names, defaults, returned objects (scipy ``coo_matrix`` in stream order, or
the MAX-SYM ``csr_matrix``; node list of ``str`` or raw ``bytes``), exception types and
messages, the one-shot ``RuntimeWarning`` and the ``verbose`` progress strings.  Every
numeric step runs on the GPU; only the Python objects are assembled here.  Graph-object
outputs (NetworkX / igraph, and ``split_on_alignment`` with ``build_graph=True``) are outside
this path's scope and raise ``NotImplementedError``; ``split_on_alignment`` matrix outputs are
served (``_parse_gfa_split``).
"""
from __future__ import annotations

import gzip
import io
import os
import sys
import tempfile
import time
import warnings
import zlib
from pathlib import Path
from typing import Any

import numpy as np
import scipy.sparse as sp

from . import _native as nat
from ._native import RawResult

try:  # the reference's verbose progress draws a tqdm bar when tqdm is importable (utils.py:8-14)
    from tqdm.auto import tqdm

    _HAS_TQDM = True
except Exception:  # noqa: BLE001 - the same broad guard as the reference
    tqdm = None  # type: ignore
    _HAS_TQDM = False

__all__ = ["parse_gfa", "parse_gfa_names", "parse_gfa_sharded", "convert_format", "finalize", "raise_for_status",
           "save_npz", "write_dense", "dense_range", "export_edge_list", "export_graph_json", "export_graph_gexf", "compute_stats", "graph_stats", "graph_components", "split_components", "node_components", "write_node_components", "ComponentSplit", "density", "path_distances", "min_table", "mean_table", "weighted_min_table", "weighted_mean_table", "weighted_fold_table", "graph_matrix", "load_paths", "genome_distance", "genome_distance_matrix",
           "sequence_distance", "sequence_nodes", "NodeNotFound", "NetworkXNoPath"]

# Auto-sharding (BASELINE north_star: byte-range-shard "only when it exceeds one GPU's HBM"): a
# build's device working set is at most about this many bytes per input byte (the lean decimal-id
# MAX-SYM build of C4 peaks near 3x; hash-dictionary, bidirected and weighted builds need more).
WORKING_SET_PER_INPUT_BYTE = 8

_MALFORMED = {
    nat.E_MALFORMED_L: "L", nat.E_MALFORMED_E: "E", nat.E_MALFORMED_C: "C",
    nat.E_MALFORMED_P: "P", nat.E_MALFORMED_O: "O",
}


def raise_for_status(raw: RawResult, dtype: np.dtype, path: Any = None) -> None:
    """Raise exactly what the reference raises for this failure (type and message)."""
    s = raw.status
    if s == nat.OK:
        return
    if s in _MALFORMED:  # parser.py:209, 252, 300, 232, 346
        raise ValueError(f"Malformed {_MALFORMED[s]} record")
    if s == nat.E_INDEX_LIST:  # parser.py:163 fields[1]
        raise IndexError("list index out of range")
    if s == nat.E_INDEX_BYTES:  # parser.py:220-221 u_field[-1] on b""
        raise IndexError("index out of range")
    if s == nat.E_UNICODE:  # the same bytes.decode() the reference calls
        bytes(raw.err_detail).decode()
        raise AssertionError("decode of the reported bytes unexpectedly succeeded")
    if s == nat.E_INT_TOO_LARGE:  # builders.py:209 float(int)
        raise OverflowError("int too large to convert to float")
    if s == nat.E_CAST_OVERFLOW:  # numpy cast in coo_matrix(..., dtype) (builders.py:281)
        raise OverflowError(f"Python integer {int(raw.err_value)} out of bounds for {dtype}")
    if s == nat.E_CAST_INF:
        raise OverflowError("cannot convert float infinity to integer")
    if s == nat.E_CAST_NAN:
        raise ValueError("cannot convert float NaN to integer")
    if s == nat.E_IO:
        err = int(raw.err_index)
        raise OSError(err, os.strerror(err), str(path))
    if s == nat.E_GZIP:  # gzip.open(...) failures (parser.py:108-109)
        sub = int(raw.err_index)
        if sub == 2:
            raise EOFError(raw.message)
        if sub == 3:
            raise zlib.error(raw.message)
        raise gzip.BadGzipFile(raw.message)
    raise RuntimeError(f"{nat.status_name(s)}: {raw.message}")


def _node_list(raw: RawResult, raw_bytes_id: bool) -> list:
    """node_list[idx] = node (raw_bytes_id) or node.decode()  (builders.py:284-288)."""
    offs = raw.names_offsets
    n = 0 if offs is None else len(offs) - 1
    if n == 0:
        return []
    blob = raw.names_blob
    # names never contain b"\n" (lines are split on it): join with "\n" and split once
    jb = nat.join_names(blob, offs)
    if raw_bytes_id:
        return bytes(jb).split(b"\n")
    try:
        return jb.decode().split("\n")
    except UnicodeDecodeError:
        pass
    for i in range(n):  # the first undecodable name in id order raises, as in the reference
        bytes(blob[offs[i]:offs[i + 1]]).decode()
    raise AssertionError("unreachable")


def _progress(n_records: int) -> None:
    # builders.py:257-258: every 500 000 records yielded
    for k in range(1, n_records // 500_000 + 1):
        print(f"\r[{k * 500_000:,} lines]", end="", file=sys.stderr)


def finalize(raw: RawResult, *, dtype: np.dtype, return_node_list: bool, raw_bytes_id: bool,
             verbose: bool, build_matrix: bool = True, path: Any = None):
    """Turn one native result into the reference's return value / warning / exception."""
    if raw.status in (nat.E_IO, nat.E_ARG, nat.E_DEVICE, nat.E_NOMEM, nat.E_UNSUPPORTED):
        raise_for_status(raw, dtype, path)
    if raw.status == nat.E_GZIP:  # the lines gzip returned before failing were parsed first
        if raw.has_warning:
            warnings.warn(f"Skipping unsupported record: {chr(raw.warn_byte)}", RuntimeWarning, stacklevel=3)
        if verbose:
            _progress(raw.n_records)
        raise_for_status(raw, dtype, path)
    if raw.has_warning:  # parser.py:124-130
        warnings.warn(f"Skipping unsupported record: {chr(raw.warn_byte)}", RuntimeWarning, stacklevel=3)
    parse_failed = nat.OK < raw.status < nat.E_CAST_OVERFLOW
    if verbose:
        _progress(raw.n_records_before_error if parse_failed else raw.n_records)
    if parse_failed:
        raise_for_status(raw, dtype, path)
    if verbose:
        print("\r[parse_gfa] done")
    if not build_matrix:
        return None
    raise_for_status(raw, dtype, path)  # dtype cast errors (after the parse loop)
    for _ in range(int(raw.n_cast_overflow)):  # numpy's per-element float32 cast warning
        warnings.warn("overflow encountered in cast", RuntimeWarning, stacklevel=3)
    n = int(raw.n_nodes)
    if raw.format == "coo":
        A = sp.coo_matrix((raw.data, (raw.rows, raw.cols)), shape=(n, n), dtype=dtype)
    else:
        A = sp.csr_matrix((raw.data, raw.indices, raw.indptr), shape=(n, n), dtype=dtype)
        if raw.indptr.dtype == np.int64 and A.indptr.dtype != np.int64:
            # scipy's own result keeps int64 here (coo.tocsr of more than 2^31 - 1 triplets sizes its
            # arrays by the triplets; the constructor's content check would narrow them)
            A.indices, A.indptr = raw.indices, raw.indptr
    if return_node_list:
        return A, _node_list(raw, raw_bytes_id)
    return A


def _dtype_of(dtype) -> np.dtype:
    dt = np.dtype(dtype)
    if dt.name not in nat.DTYPE_CODES:
        raise NotImplementedError(
            f"dtype {dt} is not supported by the GPU path (supported: {', '.join(nat.DTYPE_CODES)})")
    return dt


def _unit_dtype(dtype) -> np.dtype | None:
    """A dtype outside the five the kernels compute in, for a build whose every value is dtype(1.0) (no
    weight tag: builders.py:224-228 appends 1.0): the build then runs in int32 and its values — copy counts
    k of each entry (the SUM CSR's k, MAX-SYM's max(k_A, k_AT): builders.py:282-283) — become the sum of
    k ones in that dtype (_unit_values).  None for the five native dtypes."""
    dt = np.dtype(dtype)
    return None if dt.name in nat.DTYPE_CODES else dt


def _unit_values(counts: np.ndarray, dt: np.dtype) -> np.ndarray:
    """The sum of k ones in dtype dt for each copy count k (scipy sums duplicates in the matrix dtype):
    k itself while it is exact; an integer dtype whose sums would wrap raises NotImplementedError (a
    documented limit); scipy.sparse's own dtype check raises first for what it does not support."""
    sp.coo_matrix((np.zeros(0, dtype=dt), (np.zeros(0, np.int32), np.zeros(0, np.int32))), shape=(1, 1))
    k = np.asarray(counts)
    if k.size and dt.kind in "iu" and int(k.max()) > np.iinfo(dt).max:
        raise NotImplementedError(f"copy counts up to {int(k.max())} wrap in {dt}: not supported by the GPU path")
    return k.astype(dt)


def _with_unit_dtype(out, dt: np.dtype, return_node_list: bool):
    """An int32 unit-valued build's result in dtype dt (values: _unit_values of its copy counts)."""
    A = out[0] if return_node_list else out
    if A.format == "coo":  # every value is dtype(1.0)
        A = sp.coo_matrix((_unit_values(np.ones(A.nnz, dtype=np.int32), dt), (A.row, A.col)), shape=A.shape)
    else:
        B = sp.csr_matrix((_unit_values(A.data, dt), A.indices, A.indptr), shape=A.shape)
        if A.indptr.dtype == np.int64 and B.indptr.dtype != np.int64:  # (finalize's index-dtype rule)
            B.indices, B.indptr = A.indices, A.indptr
        A = B
    return (A, out[1]) if return_node_list else A


def parse_gfa(
    path,
    *,
    build_graph: bool,
    build_matrix: bool,
    directed: bool = True,
    weight_tag: str | None = None,
    store_seq: bool = False,
    store_tags: bool = False,
    strip_orientation: bool = False,
    verbose: bool = False,
    bidirected: bool = False,
    keep_directed_bidir: bool = False,
    backend: str = "networkx",
    dtype: str | object = "float64",
    asymmetric: bool = False,
    raw_bytes_id: bool = False,
    return_node_list: bool = False,
    max_tag_mb: float = 100.0,
    split_on_alignment: bool = False,
    device: int = 0,
    shard: str = "never",
    chunk_bytes: int | None = None,
):
    """GPU ``parse_gfa`` (gfa2network/builders.py:30-299), matrix outputs only.

    Returns ``A`` or ``(A, node_list)`` exactly as the reference does for
    ``build_graph=False, build_matrix=True``.

    ``shard`` (extension; the reference has no such argument) decides only whether the ranks of a
    torch.distributed group split the file: ``"never"`` (default) builds on this process's GPU;
    with more than one rank, ``"auto"`` splits the file over the ranks (``parse_gfa_sharded``) when
    its working set would not fit a GPU's free HBM on some rank, ``"always"`` splits it regardless;
    both are collectives — every rank must make the same call on the same file (checked: a different
    path raises ValueError).  On this process's GPU, an input whose working set would not fit its
    free HBM — a plain file, a ``.gz`` (inflated on the host), stdin or a file object — is built in
    line-aligned chunks on that one GPU (``shard.build_chunked``: errors, cast errors and the
    one-shot warning come out as one piece would raise / emit them; the whole-matrix CSR is
    assembled in row bands when it does not fit either).  ``chunk_bytes`` (extension) forces that
    chunked build with chunks of about that many bytes.
    """
    if backend == "igraph":
        raise NotImplementedError("backend='igraph' is outside the GPU GFA->CSR path")
    if split_on_alignment:  # builders.py:110-128 (before the return_node_list check)
        if build_graph:
            raise NotImplementedError("graph objects (build_graph=True) are outside the GPU GFA->CSR path")
        return _parse_gfa_split(path, build_matrix=build_matrix, directed=directed, weight_tag=weight_tag,
                                strip_orientation=strip_orientation, bidirected=bidirected,
                                keep_directed_bidir=keep_directed_bidir, dtype=dtype, asymmetric=asymmetric,
                                raw_bytes_id=raw_bytes_id, return_node_list=return_node_list, device=device)
    if return_node_list and not build_matrix:  # builders.py:129-130
        raise ValueError("return_node_list requires build_matrix=True")
    if build_graph:
        raise NotImplementedError("graph objects (build_graph=True) are outside the GPU GFA->CSR path")
    ext = _unit_dtype(dtype) if build_matrix else None
    if ext is not None:  # another numpy dtype: unit values only, built in int32
        if weight_tag:
            raise NotImplementedError(f"dtype {ext} with a weight tag is not supported by the GPU path "
                                      f"(supported: {', '.join(nat.DTYPE_CODES)})")
        out = parse_gfa(path, build_graph=False, build_matrix=True, directed=directed, weight_tag=None,
                        strip_orientation=strip_orientation, verbose=verbose, bidirected=bidirected,
                        keep_directed_bidir=keep_directed_bidir, dtype="int32", asymmetric=asymmetric,
                        raw_bytes_id=raw_bytes_id, return_node_list=return_node_list, device=device, shard=shard,
                        chunk_bytes=chunk_bytes)
        return _with_unit_dtype(out, ext, return_node_list)
    dt = _dtype_of(dtype) if build_matrix else np.dtype("float64")
    if shard not in ("auto", "always", "never"):
        raise ValueError("shard must be 'auto', 'always' or 'never'")
    if build_matrix and _want_shard(path, shard, device):
        return parse_gfa_sharded(path, directed=directed, weight_tag=weight_tag, strip_orientation=strip_orientation,
                                 verbose=verbose, bidirected=bidirected, keep_directed_bidir=keep_directed_bidir,
                                 dtype=dt.name, asymmetric=asymmetric, raw_bytes_id=raw_bytes_id,
                                 return_node_list=return_node_list, device=device)
    src = path
    if build_matrix:  # one GPU, an input past its working set: chunks of it (any input kind)
        done, src = _one_gpu_chunked(path, chunk_bytes, device, directed=directed, weight_tag=weight_tag,
                                     verbose=verbose, bidirected=bidirected, keep_directed_bidir=keep_directed_bidir,
                                     strip_orientation=strip_orientation, dt=dt, asymmetric=asymmetric,
                                     raw_bytes_id=raw_bytes_id, return_node_list=return_node_list)
        if done is not None:
            return done
    opts = nat.make_options(
        directed=directed, bidirected=bidirected, keep_directed_bidir=keep_directed_bidir,
        asymmetric=asymmetric, strip_orientation=strip_orientation, dtype=dt.name,
        weight_tag=weight_tag or None, output=nat.OUT_PARSE,
        want_node_names=bool(return_node_list), device=device)
    raw = _run(src, opts)
    return finalize(raw, dtype=dt, return_node_list=return_node_list, raw_bytes_id=raw_bytes_id,
                    verbose=verbose, build_matrix=build_matrix, path=path)


def _parse_gfa_split(path, *, build_matrix: bool, directed: bool, weight_tag, strip_orientation: bool,
                     bidirected: bool, keep_directed_bidir: bool, dtype, asymmetric: bool, raw_bytes_id: bool,
                     return_node_list: bool, device: int, build=None):
    """``parse_gfa(..., split_on_alignment=True)`` matrix outputs (builders.py:302-568).

    1. The input is parsed on the GPU as the plain path parses it: every parser error, the
       one-shot unsupported-record warning and gzip failures are the reference's (its split
       path runs the same GFAParser loop over the whole input first, builders.py:330-346).
    2. ``g2n_split_render`` (csrc/g2n_split.cpp) cuts the segments at the E/C coordinates,
       re-targets the records (builders.py:348-430) and renders that record stream as GFA text;
       the ">10x" and "skipping ..." warnings are emitted here in the reference's order.
    3. The GPU builds the rendered stream with the caller's options (builders.py:460-557: the
       same matrix loop, COO, ``A.maximum(A.T)`` and node list).  Bidirected: the interval
       segments mint their plain keys first (builders.py:474-476), ahead of the GPU's nodes.
    verbose prints nothing on this path for matrix outputs (builders.py:536-537 is graph-only).
    ``build(src, mode, want_names) -> RawResult`` runs one build (default: the GPU through the
    C-ABI; src is a path or bytes) — the CPU tests pass the oracle as the checker.
    """
    dt = _dtype_of(dtype) if build_matrix else np.dtype("float64")
    if build is None:
        def build(src, mode: dict, want_names: bool):
            o = nat.make_options(output=nat.OUT_PARSE, want_node_names=want_names, device=device,
                                 **{k: v for k, v in mode.items() if k != "dtype"}, dtype=mode.get("dtype", "float64"))
            return nat.build_from_path(src, o) if isinstance(src, str) else nat.build_from_buffer(src, o)
    data = None
    if hasattr(path, "read"):
        data = path.read()
    elif str(path) == "-":
        data = sys.stdin.buffer.read()
    else:
        p = str(path)
        try:
            with open(p, "rb") as fh:
                blob = fh.read()
        except OSError:
            blob = None  # the build raises the reference's OSError
        if blob is not None and p.endswith(".gz"):
            try:
                data, _ = nat.gunzip(blob)
            except nat.GzipFailure:
                data = None  # corrupt gzip: the plain path's prefix semantics decide
        else:
            data = blob
    raw0 = build(str(path) if data is None else data, {"asymmetric": True}, False)
    finalize(raw0, dtype=np.dtype("float64"), return_node_list=False, raw_bytes_id=raw_bytes_id, verbose=False,
             build_matrix=False, path=path)
    if raw0.status != nat.OK:
        raise_for_status(raw0, np.dtype("float64"), path)
    del raw0
    text, blob, offs, warns, many, per_seg = nat.split_render(data, bidirected)
    if many:
        warnings.warn("split-on-alignment created >10x more nodes", RuntimeWarning, stacklevel=3)
    for kind, seg in warns:
        if kind == 0:
            warnings.warn(f"skipping edge with undefined coordinates on segment {seg.decode()}", RuntimeWarning,
                          stacklevel=3)
        else:
            warnings.warn(f"skipping link with undefined segment {seg.decode()}", RuntimeWarning, stacklevel=3)
    if not build_matrix:
        return None
    raw = build(text, dict(directed=directed, bidirected=bidirected, keep_directed_bidir=keep_directed_bidir,
                           asymmetric=asymmetric, strip_orientation=strip_orientation, dtype=dt.name,
                           weight_tag=weight_tag or None), bool(return_node_list))
    m = len(offs) - 1
    if bidirected and raw.status == nat.OK and m:
        # builders.py:348-377 + 460-476: segment s's records are its k intervals (plain keys), then
        # its k - 1 chain links, which mint its 2k oriented keys (k with keep_directed_bidir) in
        # the GPU's order; the edges' keys follow.  So GPU node g of block s moves to
        # (nodes before s) + k + (g - its block start): a monotonic map.
        n_gpu = int(raw.n_nodes)
        k = per_seg.astype(np.int64)
        c = np.where(k >= 2, k if keep_directed_bidir else 2 * k, 0)
        if m + n_gpu >= 2 ** 31:
            raise NotImplementedError("more than 2**31-1 nodes")
        gmap = np.arange(n_gpu, dtype=np.int64) + m
        blk_start = np.concatenate([[0], np.cumsum(c)])[:-1]
        before = np.concatenate([[0], np.cumsum(k + c)])[:-1]
        n_blk = int(c.sum())
        seg_of_g = np.repeat(np.arange(len(k)), c)
        gmap[:n_blk] = before[seg_of_g] + k[seg_of_g] + (np.arange(n_blk) - blk_start[seg_of_g])
        gmap = gmap.astype(np.int32)
        n_fin = m + n_gpu
        if raw.format == "coo":
            raw.rows = gmap[raw.rows]
            raw.cols = gmap[raw.cols]
        else:
            cnt = np.zeros(n_fin, dtype=np.int64)
            cnt[gmap] = np.diff(raw.indptr.astype(np.int64))
            raw.indptr = np.concatenate([[0], np.cumsum(cnt)]).astype(raw.indptr.dtype)
            raw.indices = gmap[raw.indices]
        if return_node_list:
            gb = raw.names_blob if raw.names_blob is not None else np.zeros(0, dtype=np.uint8)
            go = raw.names_offsets if raw.names_offsets is not None else np.zeros(1, dtype=np.int64)
            # final node p: the next interval segment name (host blob, in order) where no GPU node
            # lands, else GPU node g with gmap[g] = p — one gather over the two blobs (no per-name
            # Python objects)
            is_gpu = np.zeros(n_fin, dtype=bool)
            is_gpu[gmap] = True
            order = np.empty(n_fin, dtype=np.int64)
            order[~is_gpu] = np.arange(m, dtype=np.int64)
            order[gmap] = m + np.arange(n_gpu, dtype=np.int64)
            hb = np.asarray(blob, dtype=np.uint8)[:int(offs[m])] if m else np.zeros(0, dtype=np.uint8)
            src = np.concatenate([hb, np.asarray(gb, dtype=np.uint8)])
            src_offs = np.concatenate([np.asarray(offs[:m + 1], dtype=np.int64),
                                       np.asarray(go[1:], dtype=np.int64) + int(offs[m])])
            raw.names_blob, raw.names_offsets = nat.gather_names(src, src_offs, order)
        raw.n_nodes = n_fin
    elif not bidirected and return_node_list and raw.status == nat.OK and raw.names_offsets is None:
        raw.names_blob, raw.names_offsets = np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64)
    return finalize(raw, dtype=dt, return_node_list=return_node_list, raw_bytes_id=raw_bytes_id, verbose=False,
                    path=path)


def _dist_world() -> int:
    try:
        import torch.distributed as dist
    except ImportError:  # pragma: no cover - torch is in the image
        return 1
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _gz_inflated_estimate(p: str, size: int) -> int:
    """Bytes a .gz inflates to, for the shard decision: the last member's ISIZE (RFC 1952: the
    length mod 2^32) or 4x the compressed size (GFA text compresses 3-4x), whichever is larger."""
    try:
        with open(p, "rb") as fh:
            fh.seek(max(size - 4, 0))
            isize = int.from_bytes(fh.read(4), "little")
    except OSError:
        isize = 0
    return max(isize, 4 * size)


def _free_hbm(device: int, need: int = 0) -> int | None:
    """Free HBM of `device` (hipMemGetInfo through the C-ABI: no torch on the one-GPU path); None
    without such a device (the build itself then raises G2N_E_DEVICE).  When that is less than `need`,
    the host entry points' cached buffers (an earlier build's arena, g2n_release_shared) are released
    first and the free HBM read again: a cache must not send a build that fits to the chunked route."""
    try:
        free = nat.device_memory(device)[0]
        if free < need and nat.release_shared(device):
            free = nat.device_memory(device)[0]
        return free
    except RuntimeError:
        return None


def _chunk_plan(size: int, device: int) -> int:
    """The chunk size that lets an input of `size` bytes whose working set (WORKING_SET_PER_INPUT_BYTE
    x its size) exceeds the GPU's free HBM be built on this GPU alone (shard.build_chunked), or 0 (the
    one-piece build): each chunk's working set is then about half the free HBM."""
    free = _free_hbm(device, need=size * WORKING_SET_PER_INPUT_BYTE)
    if free is None or size * WORKING_SET_PER_INPUT_BYTE <= free:
        return 0
    return max(1 << 26, int(free // (2 * WORKING_SET_PER_INPUT_BYTE)))


class _Bytes:
    """Input already read into host memory, handed to the one-piece build as a file object."""

    def __init__(self, arr):
        self.arr = arr

    def read(self):
        return self.arr


def _one_gpu_chunked(path, chunk_bytes, device: int, **kw):
    """parse_gfa's one-GPU route for an input past the GPU's working set (any input kind the
    reference reads, parser.py:95-112): (the result, None) when it was built in chunks, else (None,
    the input for the one-piece build).  A plain file is measured on disk and its chunks pread;
    stdin and file objects are read into host memory first (the one-piece build would read them
    whole too); a ``.gz`` whose inflated size (last ISIZE, or 4x the compressed bytes) may not fit is
    inflated on the host (member-parallel / chunk-parallel, g2n_gunzip) and chunked from there — one
    that does not inflate cleanly goes to the one-piece build, whose exact reader raises gzip.py's
    error after the lines before it.  `chunk_bytes` (extension) forces chunks of about that size."""
    from .shard import FileSource, HostSource

    if hasattr(path, "read") or str(path) == "-":
        data = path.read() if hasattr(path, "read") else sys.stdin.buffer.read()
        arr = data if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
        cb = chunk_bytes or _chunk_plan(len(arr), device)
        if cb:
            return _parse_gfa_chunked(HostSource(arr), cb, device=device, path=path, **kw), None
        return None, _Bytes(arr)
    p = str(path)
    if not os.path.isfile(p):
        return None, path  # the one-piece build raises the reference's OSError
    size = os.path.getsize(p)
    if p.endswith(".gz"):
        free = None if chunk_bytes else _free_hbm(device, need=_gz_inflated_estimate(p, size) * WORKING_SET_PER_INPUT_BYTE)
        if not chunk_bytes and (free is None or _gz_inflated_estimate(p, size) * WORKING_SET_PER_INPUT_BYTE <= free):
            return None, path
        with open(p, "rb") as fh:
            blob = fh.read()
        try:
            data, _ = nat.gunzip(blob)
        except nat.GzipFailure:
            return None, path
        del blob
        arr = np.frombuffer(data, dtype=np.uint8)
        cb = chunk_bytes or _chunk_plan(len(arr), device)
        if cb:
            return _parse_gfa_chunked(HostSource(arr), cb, device=device, path=path, **kw), None
        return None, _Bytes(arr)
    cb = chunk_bytes or _chunk_plan(size, device)
    if cb:
        return _parse_gfa_chunked(FileSource(p), cb, device=device, path=path, **kw), None
    return None, path


def _parse_gfa_chunked(source, chunk_bytes: int, *, directed: bool, weight_tag, verbose: bool, bidirected: bool,
                       keep_directed_bidir: bool, strip_orientation: bool, dt, asymmetric: bool, raw_bytes_id: bool,
                       return_node_list: bool, device: int, engine=None, path=None, free_hbm=None, bands=None):
    """parse_gfa on one GPU in chunks of the input (shard.build_chunked; source: a path, FileSource or
    HostSource), or None past 2^31 - 1 nodes (the one-piece build reports that limit).  Errors and the
    warning come out as the one-piece build's (finalize).  The engine — two build contexts and their
    grow-only arenas — lives for this call only unless the caller passes one."""
    from .shard import HipEngine, _np, build_chunked, scipy_index_dtype

    gd = keep_directed_bidir or (not bidirected and directed)  # builders.py:143
    maxsym = gd and not asymmetric                               # builders.py:282
    eng = engine or HipEngine(device, torch_buffers=False)  # one GPU, no collective: no torch on this path
    try:
        res = build_chunked(source, engine=eng, chunk_bytes=chunk_bytes, directed=directed, bidirected=bidirected,
                            keep_directed_bidir=keep_directed_bidir, asymmetric=asymmetric,
                            strip_orientation=strip_orientation, dtype=dt.name, weight_tag=weight_tag or None,
                            gather_names=return_node_list, keep_coo=not maxsym, free_hbm=free_hbm, bands=bands)
        if res is None:
            return None
        raw = RawResult(status=res.status, err_line=res.err_line, err_index=res.err_index, err_value=res.err_value,
                        err_detail=res.err_detail, has_warning=res.has_warning, warn_byte=res.warn_byte,
                        warn_line=res.warn_line, n_lines=res.n_lines, n_records=res.n_records,
                        n_records_before_error=res.n_records_before_error, n_nodes=res.n_nodes, dtype=dt,
                        n_cast_overflow=res.n_cast_overflow)
        if res.status == 0:
            if not maxsym:  # parse_gfa's stream-order COO (builders.py:281)
                raw.format = "coo"
                idt = scipy_index_dtype(0, res.n_nodes)
                raw.rows = _np(res.coo[0]).astype(idt, copy=False)
                raw.cols = _np(res.coo[1]).astype(idt, copy=False)
                raw.data = _np(res.coo[2])
            else:
                raw.format = "csr"
                idt = scipy_index_dtype(res.index_maxval, res.n_nodes)
                raw.indptr = _np(res.indptr).astype(idt, copy=False)
                raw.indices = _np(res.indices).astype(idt, copy=False)
                raw.data = _np(res.data)
            if return_node_list:
                raw.names_blob, raw.names_offsets = res.names_blob, res.names_offsets
    finally:
        if engine is None:
            eng.close()
    return finalize(raw, dtype=dt, return_node_list=return_node_list, raw_bytes_id=raw_bytes_id, verbose=verbose,
                    path=path if path is not None else getattr(source, "path", None))


def _want_shard(path, shard: str, device: int) -> bool:
    """Split the file over the process group?  Only for a file on disk, more than one rank, and
    ("auto") a working set beyond a GPU's free HBM.  "auto" and "always" are collectives: the
    ranks agree on the path (every rank must pass the same file) and, for "auto", on the verdict
    (all-reduce MAX of the per-rank "does not fit" flags), so no rank enters the sharded build
    alone."""
    if shard == "never" or _dist_world() < 2:
        return False
    import torch
    import torch.distributed as dist

    here = not hasattr(path, "read") and str(path) != "-" and os.path.isfile(str(path))
    need = 0
    if here and shard == "always":
        need = 1
    elif here:
        p = str(path)
        size = os.path.getsize(p)
        work = (_gz_inflated_estimate(p, size) if p.endswith(".gz") else size) * WORKING_SET_PER_INPUT_BYTE
        free = _free_hbm(device, need=work)
        need = int(free is not None and work > free)
    ident = zlib.crc32(os.fsencode(os.path.abspath(str(path)))) if here else 0
    size = os.path.getsize(str(path)) if here else -1
    nccl = dist.get_backend() == "nccl"
    t = torch.tensor([need, ident, size, -ident, -size, int(here), -int(here)], dtype=torch.int64,
                     device=torch.device("cuda", torch.cuda.current_device()) if nccl else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    v = t.tolist()
    same = v[1] == -v[3] and v[2] == -v[4] and v[5] == -v[6]
    if v[5] and not same:
        raise ValueError(f"parse_gfa(shard={shard!r}) is a collective: every rank must pass the same file")
    return bool(v[5]) and bool(v[0])


def parse_gfa_sharded(path, *, directed: bool = True, weight_tag: str | None = None,
                      strip_orientation: bool = False, verbose: bool = False, bidirected: bool = False,
                      keep_directed_bidir: bool = False, dtype="float64", asymmetric: bool = False,
                      raw_bytes_id: bool = False, return_node_list: bool = False, output: str = "parse",
                      group=None, engine=None, root=None, device=None):
    """``parse_gfa(path, build_graph=False, build_matrix=True, ...)`` with the file split over the
    ranks of a torch.distributed group — a collective: every rank calls it with
    the same path.  Each rank preads only its line-aligned byte range (``file_line_ranges``) into
    its GPU's HBM, the ranks reconcile node ids (the decimal-id fast path or the general owner
    protocol, gfa2network_amd/shard.py) and route triplets to row owners.  The result — what
    parse_gfa returns (the MAX-SYM CSR, or the stream-order COO), or with ``output="csr"`` what
    ``convert_format(parse_gfa(...), "csr")`` returns — is assembled on every rank (``root=None``)
    or on rank ``root`` only (the other ranks return None; a failed build raises on every rank).
    ``device``: this rank's GPU (default: torch's current device) — the one ``shard="auto"`` measured.  Index dtypes follow scipy (int64 once
    the entries pass 2^31 - 1).  Exceptions, the one-shot warning and the verbose strings are the
    reference's (builders.py:95-299).  A multi-member / BGZF ``.gz`` is inflated member-wise: each
    rank inflates the members that start in its share of the compressed bytes and one all-to-all
    moves the text to the line-aligned ranges (``shard.gz_rank_text``); a file that does not split
    into clean member chains (one member, damage) is inflated by every rank, and one that does not
    inflate cleanly is built by every rank on its own GPU through the single-GPU path, whose gzip
    errors and prefix semantics are the reference's."""
    import torch

    from .shard import HipEngine, build_sharded, file_line_ranges, gather_coo, gather_csr, scipy_index_dtype

    dt = _dtype_of(dtype)
    if output not in ("parse", "csr"):
        raise ValueError("output must be 'parse' or 'csr'")
    import torch.distributed as dist

    def dev() -> int:  # this rank's GPU, resolved only where a GPU is used (CPU engines have none)
        if device is not None:
            return device
        d = getattr(engine, "device_index", None)
        return torch.cuda.current_device() if d is None else d

    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    p = str(path)
    gd = keep_directed_bidir or (not bidirected and directed)  # builders.py:143
    maxsym = gd and not asymmetric                               # builders.py:282
    if p.endswith(".gz"):
        from .shard import gz_rank_text, line_ranges

        eng = engine or HipEngine(dev())
        got = gz_rank_text(p, eng, group)  # each rank inflates the members in its share of the bytes
        if got is not None:
            buf = got[0]
        else:  # not a clean member chain in slices (one member, damage): the whole file on every rank
            with open(p, "rb") as fh:
                blob = fh.read()
            try:
                data, _ = nat.gunzip(blob)
            except nat.GzipFailure:
                del blob
                opts = nat.make_options(directed=directed, bidirected=bidirected,
                                        keep_directed_bidir=keep_directed_bidir, asymmetric=asymmetric,
                                        strip_orientation=strip_orientation, dtype=dt.name,
                                        weight_tag=weight_tag or None,
                                        output=nat.OUT_CSR if output == "csr" else nat.OUT_PARSE,
                                        want_node_names=bool(return_node_list), device=dev())
                raw = _run(p, opts)  # the exact reader raises gzip.py's error after the prefix's lines
                out = finalize(raw, dtype=dt, return_node_list=return_node_list, raw_bytes_id=raw_bytes_id,
                               verbose=verbose, path=path)
                return out if root is None or rank == root else None
            del blob
            lo, hi = line_ranges(data, world)[rank]
            buf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8)[lo:hi].copy()).to(eng.device)
            del data
    else:
        eng = engine or HipEngine(dev())
        lo, hi = file_line_ranges(p, world)[rank]
        buf = eng.read_range(p, lo, hi - lo)
    res = build_sharded(buf, engine=eng, group=group, directed=directed, bidirected=bidirected,
                        keep_directed_bidir=keep_directed_bidir, asymmetric=asymmetric,
                        strip_orientation=strip_orientation, dtype=dt.name, weight_tag=weight_tag or None,
                        gather_names=return_node_list, keep_coo=not maxsym and output == "parse", names_root=root,
                        trim=True)  # (a sharded file is one too large for a GPU: free each stage's dead buffers)
    del buf
    raw = RawResult(status=res.status, err_line=res.err_line, err_index=res.err_index, err_value=res.err_value,
                    err_detail=res.err_detail, has_warning=res.has_warning, warn_byte=res.warn_byte,
                    warn_line=res.warn_line, n_lines=res.n_lines, n_records=res.n_records,
                    n_records_before_error=res.n_records_before_error, n_nodes=res.n_nodes, dtype=dt,
                    n_cast_overflow=res.n_cast_overflow)
    if res.status == 0:
        if not maxsym and output == "parse":
            raw.format = "coo"
            got = gather_coo(res, group, root)
            if got is not None:
                raw.rows, raw.cols, raw.data = got
                idt = scipy_index_dtype(0, res.n_nodes)
                raw.rows, raw.cols = raw.rows.astype(idt, copy=False), raw.cols.astype(idt, copy=False)
        else:
            raw.format = "csr"
            got = gather_csr(res, group, root)
            if got is not None:
                raw.indptr, raw.indices, raw.data = got
        if root is not None and rank != root:
            return None
        if return_node_list:
            raw.names_blob, raw.names_offsets = res.names_blob, res.names_offsets
    elif root is not None and rank != root:
        # a failed build (every rank agrees on its status) raises on every rank, not only on the
        # root: None means success.  The warnings and verbose strings stay the root's.
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            finalize(raw, dtype=dt, return_node_list=False, raw_bytes_id=raw_bytes_id, verbose=False, path=path)
        raise AssertionError(f"sharded build status {res.status} did not raise")  # finalize raises on any error
    return finalize(raw, dtype=dt, return_node_list=return_node_list, raw_bytes_id=raw_bytes_id, verbose=verbose,
                    path=path)


def parse_gfa_names(path, *, raw_bytes_id: bool = False, **kw):
    """``parse_gfa(path, build_graph=False, build_matrix=True, return_node_list=True, ...)`` for
    writers that never need the Python list (the convert CLI): returns ``(A, blob, offsets)``, the
    node names as the library's blob + offsets in id order.  A name that is not UTF-8 raises
    here unless raw_bytes_id, exactly where building the list would (builders.py:284-288)."""
    if kw.get("backend", "networkx") == "igraph":
        raise NotImplementedError("backend='igraph' is outside the GPU GFA->CSR path")
    if kw.pop("build_graph", False):
        raise NotImplementedError("graph objects (build_graph=True) are outside the GPU GFA->CSR path")
    if kw.pop("split_on_alignment", False):  # cli.py:111-115 --split-on-alignment: through the list
        A, nodes = parse_gfa(path, build_graph=False, build_matrix=True, return_node_list=True,
                             split_on_alignment=True, raw_bytes_id=raw_bytes_id, **kw)
        enc = [x if raw_bytes_id else x.encode() for x in nodes]
        offs = np.zeros(len(enc) + 1, dtype=np.int64)
        offs[1:] = np.cumsum([len(x) for x in enc], dtype=np.int64)
        return A, np.frombuffer(b"".join(enc), dtype=np.uint8), offs
    for k in ("store_seq", "store_tags", "max_tag_mb", "backend"):
        kw.pop(k, None)
    verbose = kw.pop("verbose", False)
    device = kw.pop("device", 0)
    dt = _dtype_of(kw.pop("dtype", "float64"))
    wt = kw.pop("weight_tag", None)
    opts = nat.make_options(dtype=dt.name, weight_tag=wt or None, output=nat.OUT_PARSE, want_node_names=True,
                            device=device, **kw)
    raw = _run(path, opts)
    A = finalize(raw, dtype=dt, return_node_list=False, raw_bytes_id=raw_bytes_id, verbose=verbose, path=path)
    blob, offs = raw.names_blob, raw.names_offsets
    if offs is None:
        offs = np.zeros(1, dtype=np.int64)
        blob = np.zeros(0, dtype=np.uint8)
    if not raw_bytes_id:
        bad = nat.first_bad_utf8(blob, offs)
        if bad >= 0:
            bytes(blob[offs[bad]:offs[bad + 1]]).decode()
            raise AssertionError("decode of the reported name unexpectedly succeeded")
    return A, blob, offs


def density(n_nodes: int, n_edges: int, directed: bool):
    """``nx.density`` of a graph with these counts (what compute_stats reports, analysis.py:57): the
    int 0 without edges or with at most one node, else m / (n (n - 1)), doubled when undirected —
    from Python ints, whose true division is correctly rounded however large n (n - 1) is."""
    n, m = int(n_nodes), int(n_edges)
    if m == 0 or n <= 1:
        return 0
    d = m / (n * (n - 1))
    if not directed:
        d *= 2
    return d


def _stats_edges(st: dict, directed: bool) -> int:
    """Edges of the nx.DiGraph / nx.Graph whose adjacency structure has these counts: every stored
    entry, or (undirected: each edge is stored from both ends, a self-loop once) half of the entries
    plus the diagonal."""
    return st["n_entries"] if directed else (st["n_entries"] + st["n_diag"]) // 2


def graph_stats(A, *, directed: bool = True, device: int = 0) -> dict:
    """Statistics of the graph whose adjacency structure is the square scipy sparse matrix ``A``
    (extension; the reference has no such function): ``nodes``, ``edges``, ``components``,
    ``max_degree`` and ``density`` as ``compute_stats`` reports them for the graph ``parse_gfa(...,
    asymmetric=True)`` describes — every stored (u, v) is an edge u -> v (``directed``) or u - v; the
    values are never read.  Runs on the GPU over the CSR structure (g2n_csr_stats_host); a matrix in
    another format is converted first, duplicates summed."""
    if not sp.issparse(A):
        raise TypeError("graph_stats takes a scipy sparse matrix")
    if A.shape[0] != A.shape[1]:
        raise ValueError("graph_stats takes a square matrix")
    if A.format != "csr":
        # structure only: unit values in a dtype whose sums cannot overflow
        C = A.tocoo()
        A = sp.coo_matrix((np.ones(C.nnz, dtype=np.float64), (C.row, C.col)), shape=C.shape).tocsr()
        A.sum_duplicates()
    n = int(A.shape[0])
    if n >= 2**31 - 1:
        raise NotImplementedError("GPU graph statistics need node ids below 2^31 - 1")
    idt = np.int64 if np.dtype(A.indptr.dtype) == np.int64 or np.dtype(A.indices.dtype) == np.int64 else np.int32
    st = nat.csr_stats_host(np.asarray(A.indptr, dtype=idt), np.asarray(A.indices, dtype=idt), n, directed, device)
    edges = _stats_edges(st, directed)
    return {"nodes": st["n_nodes"], "edges": edges, "components": st["n_components"],
            "max_degree": st["max_degree"], "density": density(st["n_nodes"], edges, directed)}


_NATIVE_DTYPES = tuple(np.dtype(k) for k in nat.DTYPE_CODES)


def _components_csr(A, who: str, structure_only: bool):
    """The square scipy sparse matrix ``A`` as the component calls take it: (n, indptr, indices — both
    int32 or both int64, the stored entries only —, the CSR itself)."""
    if not sp.issparse(A):
        raise TypeError(f"{who} takes a scipy sparse matrix")
    if A.shape[0] != A.shape[1]:
        raise ValueError(f"{who} takes a square matrix")
    if A.format != "csr":
        if structure_only:  # unit values in a dtype whose sums cannot overflow, as graph_stats
            C = A.tocoo()
            A = sp.coo_matrix((np.ones(C.nnz, dtype=np.float64), (C.row, C.col)), shape=C.shape).tocsr()
        else:
            A = A.tocsr()
    n = int(A.shape[0])
    if n >= 2**31 - 1:
        raise NotImplementedError("GPU components need node ids below 2^31 - 1")
    idt = np.int64 if np.dtype(A.indptr.dtype) == np.int64 or np.dtype(A.indices.dtype) == np.int64 else np.int32
    nnz = int(A.indptr[-1]) if n else 0
    return n, np.asarray(A.indptr, dtype=idt), np.asarray(A.indices[:nnz], dtype=idt), A


def graph_components(A, *, device: int = 0):
    """``(n_components, labels)`` of the graph whose adjacency structure is the square scipy sparse
    matrix ``A`` (extension; the counterpart of ``graph_stats``): every stored (u, v) joins u and v, the
    values are never read.  ``labels`` is an int32 array, equal to
    ``scipy.sparse.csgraph.connected_components(A, directed=False)``'s: components are numbered by
    their smallest node.  Runs on the GPU (g2n_csr_components_host); there is no CPU route."""
    n, ip, ix, _ = _components_csr(A, "graph_components", True)
    if n == 0:
        return 0, np.zeros(0, dtype=np.int32)
    labels, info = nat.csr_components_host(ip, ix, n, device)
    return info["n_components"], labels


class ComponentSplit:
    """What ``split_components`` returns: ``n_components``, ``labels`` (int32, one per node), ``sizes``
    (``np.bincount(labels)``), ``perm`` (the nodes ordered by label: ``np.argsort(labels,
    kind="stable")``) and ``offsets`` (component j's nodes are ``perm[offsets[j]:offsets[j + 1]]``), over
    the whole matrix regrouped by component on the GPU (``indptr`` / ``indices`` / ``data``: row p is
    row ``perm[p]`` of the input, its columns local to its component)."""

    def __init__(self, shape_dtype, labels, perm, offsets, indptr, indices, data, info=None):
        self.dtype = np.dtype(shape_dtype)
        self.labels, self.perm, self.offsets = labels, perm, offsets
        self.indptr, self.indices, self.data = indptr, indices, data
        self.n_components = len(offsets) - 1
        self.sizes = np.diff(offsets)
        self.info = info or {}

    def component(self, j: int):
        """``(A_j, nodes_j)``: component j as a CSR matrix of the input's dtype and the nodes it holds
        (ascending; ``np.flatnonzero(labels == j)``).  Each row keeps its entries in stored order: for a
        canonical input ``A_j`` has the arrays of ``A[nodes_j][:, nodes_j]``."""
        j = int(j)
        if not 0 <= j < self.n_components:
            raise IndexError(f"component {j} of {self.n_components}")
        lo, hi = int(self.offsets[j]), int(self.offsets[j + 1])
        ip = self.indptr[lo:hi + 1]
        b, e = int(ip[0]), int(ip[-1])
        A = sp.csr_matrix((self.data[b:e], self.indices[b:e], ip - ip[0]), shape=(hi - lo, hi - lo), dtype=self.dtype,
                          copy=False)
        return A, self.perm[lo:hi]

    def largest(self):
        """``component(j)`` of the largest component, the lowest label on ties."""
        return self.component(int(np.argmax(self.sizes)))


def split_components(A, *, device: int = 0) -> ComponentSplit:
    """The connected components of the square scipy sparse matrix ``A`` as matrices of their own
    (extension): labels as ``graph_components``, and the matrix regrouped by component on the GPU
    (g2n_csr_split_components_host) so that ``component(j)`` is a slice.  ``A``'s dtype is one of the
    five native ones; a matrix in another format goes through ``A.tocsr()`` first."""
    if sp.issparse(A) and np.dtype(A.dtype) not in _NATIVE_DTYPES:
        raise NotImplementedError(f"split_components: dtype {A.dtype} is not one of bool, int8, int32, float32, float64")
    n, ip, ix, A = _components_csr(A, "split_components", False)
    dt = np.dtype(A.dtype)
    if n == 0:
        z = np.zeros(0, dtype=np.int64)
        return ComponentSplit(dt, np.zeros(0, dtype=np.int32), z, np.zeros(1, dtype=np.int64),
                              np.zeros(1, dtype=ip.dtype), np.zeros(0, dtype=ip.dtype), np.zeros(0, dtype=dt))
    data = np.ascontiguousarray(A.data[:len(ix)])
    bits = data.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[dt.itemsize])
    labels, perm, off, oip, oix, oval, info = nat.csr_split_components_host(ip, ix, bits, n, device)
    return ComponentSplit(dt, labels, perm, off, oip, oix, oval.view(dt), info)


def min_table(D: np.ndarray) -> np.ndarray:
    """The directed float64 table of g2n_csr_path_distances' uint32 ``D``: ``M[i][j]`` = the fewest
    hops from a step of path i to a step of path j, ``inf`` where none is reached (0xFFFFFFFF), 0.0
    on the diagonal (genome_distance_matrix sets it without a search)."""
    M = D.astype(np.float64)
    M[D == np.uint32(0xFFFFFFFF)] = np.inf
    np.fill_diagonal(M, 0.0)
    return M


def mean_table(S: np.ndarray, C: np.ndarray) -> np.ndarray:
    """genome_distance_matrix's symmetric mean from g2n_csr_path_distances' directed uint64 sums
    ``S`` and counts ``C``: ``(S[i][j] + S[j][i]) / (C[i][j] + C[j][i])`` — one correctly rounded
    division of two integers below 2^53 — ``inf`` where nothing is reached, 0.0 on the diagonal."""
    num, den = S + S.T, C + C.T
    if num.size and int(num.max()) >= 2**53:
        raise NotImplementedError("a distance sum of 2^53 or more is not exact in float64")
    M = np.full(S.shape, np.inf, dtype=np.float64)
    np.divide(num.astype(np.float64), den.astype(np.float64), out=M, where=den > 0)
    np.fill_diagonal(M, 0.0)
    return M


def weighted_min_table(D: np.ndarray) -> np.ndarray:
    """The directed float64 table of g2n_csr_path_distances_weighted's ``D`` (already float64, ``inf``
    where no step is reached) with 0.0 on the diagonal."""
    M = np.array(D, dtype=np.float64)
    np.fill_diagonal(M, 0.0)
    return M


def weighted_mean_table(S: np.ndarray, C: np.ndarray) -> np.ndarray:
    """The symmetric mean from g2n_csr_path_distances_weighted's directed float64 sums ``S`` and uint64
    counts ``C``: ``(S[i][j] + S[j][i]) / float(C[i][j] + C[j][i])`` — one addition and one division
    in float64 —, ``inf`` where nothing is reached, 0.0 on the diagonal."""
    S, C = np.asarray(S, dtype=np.float64), np.asarray(C, dtype=np.uint64)
    den = C + C.T
    M = np.full(S.shape, np.inf, dtype=np.float64)
    np.divide(S + S.T, den.astype(np.float64), out=M, where=den > 0)
    np.fill_diagonal(M, 0.0)
    return M


def weighted_fold_table(S: np.ndarray, C: np.ndarray) -> np.ndarray:
    """genome_distance_matrix's symmetric mean over a weighted graph from G2N_DIST_MEAN_FOLD's tables:
    for i < j, ``S[i][j]`` is already the reference's running total of the cell (analysis.py:254-264:
    path i's steps against path j's distances, then path j's steps against path i's), divided here by
    ``float(C[i][j] + C[j][i])`` and written to both triangles; ``inf`` where nothing is reached, 0.0
    on the diagonal."""
    S, C = np.asarray(S, dtype=np.float64), np.asarray(C, dtype=np.uint64)
    den = (C + C.T).astype(np.float64)
    M = np.full(S.shape, np.inf, dtype=np.float64)
    iu = np.triu_indices(len(M), 1)
    vals = np.full(len(iu[0]), np.inf, dtype=np.float64)
    np.divide(S[iu], den[iu], out=vals, where=den[iu] > 0)
    M[iu] = vals
    M.T[iu] = vals
    np.fill_diagonal(M, 0.0)
    return M


def _weighted_csr(A):
    """``A`` as a CSR whose data is float64, every value finite and >= 0 (checked here, on the host):
    a CSR keeps its entries as they are stored (repeated ones are parallel edges), another format goes
    through scipy's own ``tocsr()``."""
    if np.issubdtype(A.dtype, np.complexfloating):
        raise TypeError("path_distances(weighted=True) takes real edge lengths, not a complex matrix")
    if A.format != "csr":
        A = A.tocsr()
    data = np.ascontiguousarray(A.data, dtype=np.float64)
    if data.size and not (np.isfinite(data).all() and (data >= 0).all()):
        raise ValueError("path_distances(weighted=True) takes finite edge lengths >= 0")
    return A, data


def _path_arrays(paths):
    lists = [np.asarray(p, dtype=np.int64).reshape(-1) for p in paths]
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in lists], out=ptr[1:])
    return ptr, np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64)


def _distance_csr(A, who: str, weighted: bool, what: str = "path"):
    """``A`` as the distance functions take it: (indptr, indices, float64 data or None, n).  ``who`` is
    the function the messages name, ``what`` the distances the size limit's message names."""
    if not sp.issparse(A):
        raise TypeError(f"{who} takes a scipy sparse matrix")
    if A.shape[0] != A.shape[1]:
        raise ValueError(f"{who} takes a square matrix")
    data = None
    if weighted:
        A, data = _weighted_csr(A)
    elif A.format != "csr":
        # structure only: unit values in a dtype whose sums cannot overflow
        C = A.tocoo()
        A = sp.coo_matrix((np.ones(C.nnz, dtype=np.float64), (C.row, C.col)), shape=C.shape).tocsr()
        A.sum_duplicates()
    n = int(A.shape[0])
    if n >= 2**31 - 1:
        raise NotImplementedError(f"GPU {what} distances need node ids below 2^31 - 1")
    idt = np.int64 if np.dtype(A.indptr.dtype) == np.int64 or np.dtype(A.indices.dtype) == np.int64 else np.int32
    return np.asarray(A.indptr, dtype=idt), np.asarray(A.indices, dtype=idt), data, n


def path_distances(A, paths, *, method: str = "min", weighted: bool = False, device: int = 0,
                   return_info: bool = False):
    """``weighted=False`` (the default) — hop distances, as described below.  ``weighted=True`` — the
    stored values are edge lengths: ``A.data`` is taken as float64 (bool, integer and float32 values
    convert exactly; a complex matrix raises TypeError), every value must be finite and >= 0
    (ValueError otherwise, before the GPU is touched), an explicit zero is an edge of length 0 and
    the repeated entries of a non-canonical CSR are parallel edges; a matrix that is not CSR goes
    through ``A.tocsr()``.  The distances are those of NetworkX's ``multi_source_dijkstra_path_length
    (G, nodes, weight="weight")`` / scipy's ``dijkstra``, bit for bit (g2n_wdist.hip): ``min`` is the
    directed float64 table, any other method ``(S[i][j] + S[j][i]) / float(C[i][j] + C[j][i])`` with
    ``S`` summed in step order; ``return_info=True`` then returns the g2n_wdist_info fields (rounds,
    launches, batches, batch_paths, ms_*).

    Hop distances between node lists over the graph whose adjacency structure is the square scipy
    sparse matrix ``A`` (extension; the counterpart of ``graph_stats``): every stored (u, v) is an
    edge u -> v of weight 1, the values are never read.  ``paths`` is a list of lists of node
    indices, duplicates kept.  ``method="min"`` returns the directed K x K float64 table
    (``M[i][j]`` = the fewest hops from path i to path j, ``inf`` when unreachable; the reference's
    ``genome_distance_matrix`` holds ``M[i][j]`` for i < j in both triangles); any other value
    returns its symmetric mean.  Runs on the GPU as a bit-parallel breadth-first search, 64 paths at
    a time (g2n_csr_path_distances_host); a matrix in another format is converted first.
    ``return_info=True`` also returns the g2n_dist_info fields (levels, launches, batches, ms_*)."""
    ip, ix, data, n = _distance_csr(A, "path_distances", weighted)
    ptr, nodes = _path_arrays(paths)
    mean = method != "min"
    if weighted:
        tabs, info = nat.csr_path_distances_weighted_host(ip, ix, data, n, ptr, nodes, mean, device)
        M = weighted_mean_table(*tabs) if mean else weighted_min_table(tabs[0])
    else:
        tabs, info = nat.csr_path_distances_host(ip, ix, n, ptr, nodes, mean, device)
        M = mean_table(*tabs) if mean else min_table(tabs[0])
    return (M, info) if return_info else M


def node_distances(A, sources, targets, *, weighted: bool = False, device: int = 0, return_info: bool = False):
    """The node-to-node distance table over the graph of the square scipy sparse matrix ``A`` (taken as
    ``path_distances`` takes it; extension): a ``(len(sources), len(targets))`` float64 array,
    ``M[i][t]`` = the hops — with ``weighted=True`` the length of the shortest path over the stored
    values, bit for bit Dijkstra's — from node ``sources[i]`` to node ``targets[t]``, 0.0 where they are
    the same node, ``inf`` where there is no path.  Both lists keep their order and their duplicates;
    ``-1`` is no node (a row or column of ``inf``), any other id outside ``[0, n)`` raises ValueError.
    One bit-parallel search carries 64 sources (g2n_csr_pair_distances_host, g2n_pairs.hip).
    ``return_info=True`` also returns the g2n_dist_info (weighted: g2n_wdist_info) fields."""
    ip, ix, data, n = _distance_csr(A, "node_distances", weighted, "pair")
    (D,), info = nat.csr_pair_distances_host(ip, ix, data, n, sources, targets, True, device)
    if not weighted:
        M = D.astype(np.float64)
        M[D == np.uint32(0xFFFFFFFF)] = np.inf
        D = M
    return (D, info) if return_info else D


def pair_sums(A, sources, targets, *, device: int = 0, return_info: bool = False):
    """``(S, C)``, uint64 arrays of ``len(sources)``: ``C[i]`` = how many entries of ``targets`` node
    ``sources[i]`` reaches (itself included, each occurrence counted), ``S[i]`` = the sum of their hop
    distances — the row sums of ``node_distances`` over its finite cells, without the table: the
    accumulators are O(len(sources)) whatever ``len(targets)`` (extension; G2N_PAIR_SUMS).  Lists as
    ``node_distances`` takes them."""
    ip, ix, _data, n = _distance_csr(A, "pair_sums", False, "pair")
    (S, C), info = nat.csr_pair_distances_host(ip, ix, None, n, sources, targets, False, device)
    return (S, C, info) if return_info else (S, C)


def mean_of_sums(S, C) -> float:
    """genome_distance(method="mean") from G2N_PAIR_SUMS' sums and counts: ``float(total) / count`` with
    ``total`` and ``count`` as Python ints — the reference's float total is exact below 2^53 —;
    NetworkXNoPath when nothing is reached."""
    total, count = int(np.sum(S, dtype=object)) if len(S) else 0, int(np.sum(C, dtype=object)) if len(C) else 0
    if count == 0:
        raise NetworkXNoPath("no path between node sets")
    if total >= 2**53:
        raise NotImplementedError("a distance sum of 2^53 or more is not exact in float64")
    return float(total) / count


def mean_of_table(D) -> float:
    """genome_distance(method="mean") over a weighted graph from the float64 table: the reference's
    running total in its order of additions (analysis.py:148-156: u outer, v inner, from 0.0, the
    unreachable pairs skipped), divided by the count; NetworkXNoPath when nothing is reached."""
    total, count = 0.0, 0
    for d in np.asarray(D, dtype=np.float64).reshape(-1).tolist():
        if d != np.inf:
            total += d
            count += 1
    if count == 0:
        raise NetworkXNoPath("no path between node sets")
    return total / count


def _stats_one_piece(path, device: int, who: str = "compute_stats", then: str = "graph_stats") -> None:
    """compute_stats (and the path distances) build the file in one piece on one GPU: an input
    parse_gfa would build in chunks (its working set past the GPU's free HBM) is outside them."""
    p = str(path)
    if not os.path.isfile(p):
        return  # the build raises the reference's OSError
    size = os.path.getsize(p)
    if _chunk_plan(_gz_inflated_estimate(p, size) if p.endswith(".gz") else size, device):
        raise NotImplementedError(
            f"{who} builds the graph in one piece on one GPU and this input's working set exceeds its free "
            "HBM: build the matrix with parse_gfa(..., asymmetric=True) (chunked or sharded) and pass it to "
            f"{then}")


def compute_stats(path, *, directed: bool = True, strip_orientation: bool = False, raw_bytes_id: bool = False,
                  device: int = 0) -> dict:
    """GPU ``compute_stats`` (gfa2network/analysis.py:33-65): ``nodes``, ``edges``, ``paths``,
    ``components``, ``max_degree`` and ``density`` of the graph ``parse_gfa(path, build_graph=True,
    directed=..., strip_orientation=..., raw_bytes_id=...)`` builds, in that key order, with the
    reference's exceptions and its one-shot warning.  The file is parsed once: the asymmetric summed
    CSR is built in HBM, the statistics are taken from it there (g2n_stats.hip) and only scalars come
    back.  Stdin and file objects raise NotImplementedError (the reference reads its input twice, so a
    pipe gives it no paths).  ``device`` is an extension."""
    raw, st, n_paths = _plain_graph_pass(path, "compute_stats", directed, strip_orientation, raw_bytes_id, device,
                                         nat.stats_from_path)
    dt = np.dtype("float64")
    finalize(raw, dtype=dt, return_node_list=False, raw_bytes_id=raw_bytes_id, verbose=False, build_matrix=False,
             path=path)
    raise_for_status(raw, dt, path)
    edges = _stats_edges(st, directed)
    return {"nodes": st["n_nodes"], "edges": edges, "paths": n_paths, "components": st["n_components"],
            "max_degree": st["max_degree"], "density": density(st["n_nodes"], edges, directed)}


def _plain_graph_pass(path, who: str, directed: bool, strip_orientation: bool, raw_bytes_id: bool, device: int, call):
    """``call(path, opts)`` (stats_from_path / components_from_path) on the graph compute_stats
    measures, with its named-file and one-piece rules and the graph path's ASCII decode of node keys;
    returns what the call returned (the caller finalizes its result: the warning names its caller)."""
    if hasattr(path, "read") or str(path) == "-":
        raise NotImplementedError(f"{who} reads a named file (the reference parses its input twice)")
    _stats_one_piece(path, device, who, "graph_stats" if call is nat.stats_from_path else "graph_components")
    opts = nat.make_options(directed=directed, strip_orientation=strip_orientation, asymmetric=True,
                            output=nat.OUT_CSR, want_node_names=not raw_bytes_id, device=device)
    out = call(str(path), opts)
    raw = out[0]
    if raw.status == nat.E_UNICODE and raw.err_line < 0:
        # builders.py:155-162: the graph path decodes every node key as ASCII (the parse itself was clean)
        if raw.has_warning:
            warnings.warn(f"Skipping unsupported record: {chr(raw.warn_byte)}", RuntimeWarning, stacklevel=3)
        bytes(raw.err_detail).decode("ascii")
        raise AssertionError("decode of the reported key unexpectedly succeeded")
    return out


def node_components(path, *, directed: bool = True, strip_orientation: bool = False, raw_bytes_id: bool = False,
                    device: int = 0):
    """``(nodes, labels)`` of the graph ``compute_stats`` measures (extension): the nodes in first-touch
    order (``str``, or ``bytes`` with ``raw_bytes_id``) and each one's component as an int32 array,
    numbered as ``enumerate(nx.connected_components(G.to_undirected()))`` numbers them on the
    reference's graph.  The file is parsed once, the CSR stays in HBM and is labelled there
    (g2n_components_from_path).  Exceptions, the warning and the named-file and one-piece rules are
    ``compute_stats``'s."""
    raw, labels, _info = _plain_graph_pass(path, "node_components", directed, strip_orientation, raw_bytes_id, device,
                                           nat.components_from_path)
    dt = np.dtype("float64")
    finalize(raw, dtype=dt, return_node_list=False, raw_bytes_id=raw_bytes_id, verbose=False, build_matrix=False,
             path=path)
    raise_for_status(raw, dt, path)
    return _node_list(raw, raw_bytes_id), labels


def write_node_components(path, output="-", *, directed: bool = True, strip_orientation: bool = False,
                          raw_bytes_id: bool = False, sizes: bool = False, device: int = 0) -> None:
    """The ``components`` subcommand: ``node\\tcomponent\\n`` per node of ``node_components(path, ...)`` in
    node order, or (``sizes``) ``component\\tsize\\n`` per component, to the file ``output`` or to
    standard output (``"-"``).  The listing is written natively from the names blob, no Python list;
    with ``raw_bytes_id`` names are decoded while writing, as ``save_node_map_native`` does."""
    raw, labels, info = _plain_graph_pass(path, "components", directed, strip_orientation, raw_bytes_id, device,
                                          nat.components_from_path)
    dt = np.dtype("float64")
    finalize(raw, dtype=dt, return_node_list=False, raw_bytes_id=raw_bytes_id, verbose=False, build_matrix=False,
             path=path)
    raise_for_status(raw, dt, path)
    to_stdout = str(output) == "-"
    if sizes:
        text = "".join(f"{j}\t{c}\n" for j, c in enumerate(np.bincount(labels, minlength=info["n_components"])))
        if to_stdout:
            sys.stdout.write(text)
        else:
            Path(output).write_text(text)
        return
    blob = raw.names_blob if raw.names_blob is not None else np.zeros(0, dtype=np.uint8)
    offs = raw.names_offsets if raw.names_offsets is not None else np.zeros(1, dtype=np.int64)
    tmp = None
    dest = str(output)
    if to_stdout:
        try:
            direct = sys.stdout.fileno() == 1
        except (AttributeError, OSError, ValueError):
            direct = False
        if direct:
            sys.stdout.flush()
        else:  # a replaced sys.stdout: through a file of the listing
            fd, tmp = tempfile.mkstemp(suffix=".tsv")
            os.close(fd)
            dest = tmp
    else:
        with open(dest, "w"):  # the same OSError cases as Python's open(dest, "w")
            pass
    try:
        bad = nat.write_node_labels(dest, blob, offs, labels, check_utf8=raw_bytes_id)
        if tmp is not None:
            with open(tmp, "rb") as fh:
                sys.stdout.write(fh.read().decode())
    finally:
        if tmp is not None:
            os.unlink(tmp)
    if bad >= 0:
        bytes(blob[offs[bad]:offs[bad + 1]]).decode()
        raise AssertionError("decode of the reported name unexpectedly succeeded")


try:  # networkx is imported only for the exception types the reference's callers catch
    from networkx import NetworkXNoPath, NodeNotFound
except Exception:  # noqa: BLE001 - any import failure: the same names, the same messages
    class NodeNotFound(KeyError):  # type: ignore[no-redef]
        """A source step is not a node of the graph (networkx.NodeNotFound where networkx imports)."""

        def __str__(self) -> str:
            return str(self.args[0]) if self.args else ""

    class NetworkXNoPath(Exception):  # type: ignore[no-redef]
        """No step of the target is reached (networkx.NetworkXNoPath where networkx imports)."""

_ORIENTED_WARNING = "distance functions ignore orientation; use G.to_undirected()"


def _warn_unsupported(raw: RawResult, stacklevel: int) -> None:
    warnings.warn(f"Skipping unsupported record: {chr(raw.warn_byte)}", RuntimeWarning, stacklevel=stacklevel)


def _named_file(path, who: str) -> str:
    if hasattr(path, "read") or str(path) == "-":
        raise NotImplementedError(f"{who} reads a named file (the reference parses its input twice)")
    return str(path)


def _load_paths_pass(raw: RawResult, ps: "nat.Paths", raw_bytes: bool, path) -> None:
    """What the reference's load_paths raises and warns on its own pass over the file, from the one
    build's result: the parser's errors in file order, with the ASCII decode of the first non-ASCII
    P / O name or step at its record's line (a parse error on the same line comes first: the
    parser raises inside the record), the gzip error after the lines read before it, and the
    unsupported-record warning when its line precedes the error."""
    dt = np.dtype("float64")
    parse_failed = nat.OK < raw.status < nat.E_CAST_OVERFLOW and raw.err_line >= 0
    if not raw_bytes and ps.bad_line >= 0 and not (parse_failed and raw.err_line <= ps.bad_line) and \
            raw.status not in (nat.E_IO, nat.E_ARG, nat.E_DEVICE, nat.E_NOMEM, nat.E_UNSUPPORTED):
        if 0 <= raw.warn_line < ps.bad_line:
            _warn_unsupported(raw, 4)
        ps.bad_bytes.decode("ascii")
        raise AssertionError("decode of the reported bytes unexpectedly succeeded")
    if parse_failed or raw.status >= nat.E_ARG:
        finalize(raw, dtype=dt, return_node_list=False, raw_bytes_id=raw_bytes, verbose=False, build_matrix=False,
                 path=path)
        raise_for_status(raw, dt, path)
    if raw.has_warning:
        _warn_unsupported(raw, 4)


def _graph_pass(raw: RawResult, raw_bytes_id: bool, verbose: bool, path) -> None:
    """The graph build's own pass after a clean load_paths: its warning, progress strings and the
    ASCII decode of node keys (builders.py:155-162)."""
    dt = np.dtype("float64")
    if raw.status == nat.E_UNICODE and raw.err_line < 0:
        if raw.has_warning:
            _warn_unsupported(raw, 4)
        bytes(raw.err_detail).decode("ascii")
        raise AssertionError("decode of the reported key unexpectedly succeeded")
    finalize(raw, dtype=dt, return_node_list=False, raw_bytes_id=raw_bytes_id, verbose=verbose, build_matrix=False,
             path=path)
    raise_for_status(raw, dt, path)


def _warn_oriented(raw: RawResult, oriented: bool) -> None:
    """_warn_directed_bidirected on a directed graph (analysis.py:19-30).  Raw byte keys are decoded
    as UTF-8 one by one until an oriented one is found: when a key has a byte >= 0x80 the build
    returned the names, and the same loop runs here (its decode raises the reference's error)."""
    if raw.names_offsets is not None:
        blob, offs = bytes(raw.names_blob), raw.names_offsets.tolist()
        oriented = False
        for i in range(len(offs) - 1):
            key = blob[offs[i]:offs[i + 1]].decode()
            if key.endswith(":+") or key.endswith(":-"):
                oriented = True
                break
    if oriented:
        warnings.warn(_ORIENTED_WARNING, RuntimeWarning, stacklevel=3)


def _unreadable(path: str, device: int) -> None:
    """load_paths could not read the file: the build's own read raises the reference's OSError."""
    raw = nat.build_from_path(path, nat.make_options(device=device))
    dt = np.dtype("float64")
    finalize(raw, dtype=dt, return_node_list=False, raw_bytes_id=False, verbose=False, build_matrix=False, path=path)
    raise_for_status(raw, dt, path)
    raise RuntimeError(f"load_paths: cannot read {path}")


def load_paths(path, *, raw_bytes: bool = False, device: int = 0) -> dict:
    """``load_paths`` (gfa2network/analysis.py:164-177): the P / O records as ``{name: [step, ...]}``
    in first-occurrence order, a repeated name taking its last record's steps; ``str`` decoded as
    ASCII unless ``raw_bytes``.  The records are read natively on host threads (g2n_load_paths); the
    parser's own errors and its warning come from one GPU parse of the file.  ``device`` is an
    extension."""
    p = _named_file(path, "load_paths")
    ps = nat.Paths(p)
    if ps.status != nat.OK:
        _unreadable(p, device)
    raw, _st, _n = nat.stats_from_path(p, nat.make_options(asymmetric=True, output=nat.OUT_CSR, want_node_names=False,
                                                           device=device))
    _load_paths_pass(raw, ps, raw_bytes, path)
    d = ps.as_dict()
    if raw_bytes:
        return d
    return {k.decode("ascii"): [s.decode("ascii") for s in v] for k, v in d.items()}


def _dist_opts(directed: bool, raw_bytes_id: bool, device: int, weight_tag=None):
    return nat.make_options(directed=directed, asymmetric=True, output=nat.OUT_CSR, want_node_names=not raw_bytes_id,
                            device=device, weight_tag=weight_tag or None)


_BAD_WEIGHT = ("edge weights must be finite and >= 0 for the GPU distance search (NetworkX's result on such a graph "
               "depends on its heap's order and is not reproduced)")


def _paths_raw(raw: RawResult, p: str, directed: bool, raw_bytes_id: bool, device: int) -> RawResult:
    """The build result load_paths' own pass is judged by.  load_paths parses without a weight tag, so
    an integer tag too large for float() (builders.py:209) is the graph build's error alone: what
    load_paths raises before it comes from a build of the same file without the tag."""
    if raw.status != nat.E_INT_TOO_LARGE:
        return raw
    return nat.stats_from_path(p, _dist_opts(directed, raw_bytes_id, device))[0]


def _missing_step(step: bytes, raw_bytes_id: bool):
    node = step if raw_bytes_id else step.decode("ascii")
    return NodeNotFound(f"Node {node} not found in graph")


def genome_distance_matrix(gfa_path, method: str = "min", *, raw_bytes_id: bool = False, backend: str = "networkx",
                           verbose: bool = False, device: int = 0, return_info: bool = False, weight_tag=None):
    """GPU ``genome_distance_matrix`` (gfa2network/analysis.py:180-272): the pairwise hop distances
    between the file's P / O paths over the directed graph ``parse_gfa(gfa_path, build_graph=True)``
    builds — ``min``: the fewest hops from a step of path i to a step of path j (i < j, in both
    triangles); any other ``method``: the mean over both paths' steps of the distance from the other
    path — as a ``pandas.DataFrame`` labelled with the path names when pandas imports, else an
    ``ndarray``; with the reference's exceptions and warnings in its order.  The file is parsed once:
    the CSR and the node names stay in HBM, the step names are looked up there and one bit-parallel
    breadth-first search serves 64 paths (g2n_dist.hip); only the K x K tables come back.
    ``backend="igraph"``, stdin and file objects raise NotImplementedError.  ``device`` and
    ``return_info`` (also return the g2n_dist_info fields) are extensions.

    ``weight_tag`` (extension; ``None`` or ``""``: the hop distances above, unchanged): the distances the
    reference computes over ``parse_gfa(gfa_path, build_graph=True, weight_tag=...)`` — Dijkstra with
    ``weight="weight"`` over the graph whose edge lengths are ``graph_matrix``'s —, bit for bit; the
    mean is the reference's running total per cell in its order of additions.  An integer tag too
    large for a float raises the reference's OverflowError; a stored length that is negative, NaN or
    infinite raises NotImplementedError.  ``return_info`` then returns the g2n_wdist_info fields."""
    if backend == "igraph":
        raise NotImplementedError("backend='igraph' is outside the GPU path")
    p = _named_file(gfa_path, "genome_distance_matrix")
    _stats_one_piece(p, device, "genome_distance_matrix", "path_distances")
    ps = nat.Paths(p)
    if ps.status != nat.OK:
        _unreadable(p, device)
    mean = method != "min"
    bad = False
    if weight_tag:
        raw, tabs, info, oriented, missing, bad = nat.wdistances_from_path(
            p, _dist_opts(True, raw_bytes_id, device, weight_tag), ps, -1, -1, "fold" if mean else False)
        _load_paths_pass(_paths_raw(raw, p, True, raw_bytes_id, device), ps, raw_bytes_id, gfa_path)
    else:
        raw, tabs, info, oriented, missing = nat.distances_from_path(p, _dist_opts(True, raw_bytes_id, device), ps, -1,
                                                                     -1, mean)
        _load_paths_pass(raw, ps, raw_bytes_id, gfa_path)
    names = [ps.name(k) if raw_bytes_id else ps.name(k).decode("ascii") for k in range(ps.n_paths)]
    _graph_pass(raw, raw_bytes_id, verbose, gfa_path)
    _warn_oriented(raw, oriented)
    if bad:
        raise NotImplementedError(_BAD_WEIGHT)
    if missing >= 0:
        raise _missing_step(ps.step(missing), raw_bytes_id)
    if mean:
        M = weighted_fold_table(*tabs) if weight_tag else mean_table(*tabs)
    else:
        M = weighted_min_table(tabs[0]) if weight_tag else min_table(tabs[0])
        iu = np.triu_indices(len(M), 1)
        M.T[iu] = M[iu]
    try:
        import pandas as pd
    except Exception:  # noqa: BLE001 - the same broad guard as the reference
        pd = None
    if pd is not None:
        labels = [n.decode() if isinstance(n, bytes) else str(n) for n in names]
        M = pd.DataFrame(M, index=labels, columns=labels)
    return (M, info) if return_info else M


_QUADRATIC_WARNING = "Mean distance scales quadratically; this may be very slow on large sets"


def genome_distance(path, name_a, name_b, *, method: str = "min", directed: bool = True, raw_bytes_id: bool = False,
                    verbose: bool = False, device: int = 0, weight_tag=None):
    """``gfa2network distance GFA --path A B`` as a function (cli.py:323-346): the fewest hops from
    a step of path ``name_a`` to a step of path ``name_b`` (an int; the search runs from A only) over
    the graph ``parse_gfa(path, build_graph=True, directed=...)`` builds.  KeyError(name) for an
    unknown path name (raised before the graph is built, after load_paths' own errors),
    NodeNotFound when a step of A is no node, NetworkXNoPath when no step of B is reached.

    ``weight_tag`` (extension; ``None`` or ``""``: the hops above, an int, unchanged): the length of
    the shortest path over the graph ``parse_gfa(path, build_graph=True, directed=...,
    weight_tag=...)`` builds, as ``genome_distance_matrix`` describes — always a ``float`` (the
    reference returns an equal ``int`` when the best path crosses untagged edges only).

    ``method="mean"`` (analysis.py:142-159): the mean of the shortest-path lengths over every pair (u in
    A, v in B) that has a path, each occurrence of a step counted, a ``float``.  One bit-parallel search
    carries 64 steps of A (g2n_pairs.hip), so the |A| x |B| searches of the reference are ceil(|A| / 64)
    passes over the CSR; only |A| sums and counts come back.  Hops: ``float(total) / count`` from
    integer sums (NotImplementedError at a total of 2^53 or more).  With ``weight_tag``: the float64
    table comes back and is folded here in the reference's order of additions.  After the orientation
    warning the reference's RuntimeWarning about quadratic cost is raised past 1000 pairs, unless
    ``GFANET_DISABLE_WARNINGS=1`` — callers filter on it; the cost it speaks of is not this search's.
    NetworkXNoPath when a path is empty or no pair has a path, else NodeNotFound for the first step of A
    that is no node; a step of B that is none is never reached.  Any other ``method`` raises
    ValueError(f"unknown method: {method}") where the reference does: after the build's own errors and
    warnings."""
    p = _named_file(path, "genome_distance")
    _stats_one_piece(p, device, "genome_distance", "path_distances")
    ps = nat.Paths(p)
    if ps.status != nat.OK:
        _unreadable(p, device)
    index = {ps.name(k): k for k in range(ps.n_paths)}

    def find(name):
        key = name if isinstance(name, bytes) else str(name).encode()
        if not raw_bytes_id and max(key, default=0) >= 0x80:
            return None  # (the ASCII-decoded names hold no such key)
        return index.get(key)

    a, b = find(name_a), find(name_b)
    opts = _dist_opts(directed, raw_bytes_id, device)
    if a is None or b is None:
        raw, _st, _n = nat.stats_from_path(p, opts)
        _load_paths_pass(raw, ps, raw_bytes_id, path)
        raise KeyError(name_a if a is None else name_b)
    bad = False
    if method == "mean":
        wopts = _dist_opts(directed, raw_bytes_id, device, weight_tag) if weight_tag else opts
        raw, tabs, _info, oriented, missing, bad = nat.pair_distances_from_path(p, wopts, ps, a, b)
        _load_paths_pass(_paths_raw(raw, p, directed, raw_bytes_id, device) if weight_tag else raw, ps, raw_bytes_id,
                         path)
    elif weight_tag:
        raw, tabs, _info, oriented, missing, bad = nat.wdistances_from_path(
            p, _dist_opts(directed, raw_bytes_id, device, weight_tag), ps, a, b, False)
        _load_paths_pass(_paths_raw(raw, p, directed, raw_bytes_id, device), ps, raw_bytes_id, path)
    else:
        raw, tabs, _info, oriented, missing = nat.distances_from_path(p, opts, ps, a, b, False)
        _load_paths_pass(raw, ps, raw_bytes_id, path)
    _graph_pass(raw, raw_bytes_id, verbose, path)
    if directed:
        _warn_oriented(raw, oriented)
    if method not in ("min", "mean"):
        raise ValueError(f"unknown method: {method}")
    if bad:
        raise NotImplementedError(_BAD_WEIGHT)
    if method == "mean":
        n_a = int(ps.path_ptr[a + 1] - ps.path_ptr[a])
        n_b = int(ps.path_ptr[b + 1] - ps.path_ptr[b])
        if n_a * n_b > 1000 and os.getenv("GFANET_DISABLE_WARNINGS") != "1":
            warnings.warn(_QUADRATIC_WARNING, RuntimeWarning, stacklevel=2)
        if n_a == 0 or n_b == 0:
            raise NetworkXNoPath("no path between node sets")
        if missing >= 0:
            raise _missing_step(ps.step(int(ps.path_ptr[a]) + missing), raw_bytes_id)
        return mean_of_table(tabs[0]) if weight_tag else mean_of_sums(*tabs)
    if missing >= 0:
        raise _missing_step(ps.step(int(ps.path_ptr[a]) + missing), raw_bytes_id)
    if weight_tag:
        w = float(tabs[0][0, 1])
        if w == np.inf:
            raise NetworkXNoPath("no path between node sets")
        return w
    d = int(tabs[0][0, 1])
    if d == 0xFFFFFFFF:
        raise NetworkXNoPath("no path between node sets")
    return d


def _seq_pass(path, seq_a, seq_b, directed: bool, raw_bytes_id: bool, verbose: bool, device: int, who: str,
              weight_tag=None):
    """The one GPU pass of sequence_distance / sequence_nodes: the build's errors and warnings, the
    orientation warning, then KeyError for a sequence no node carries (analysis.py:103-105: repr of
    each missing argument as passed).  Returns (distance or 0xFFFFFFFF, [keys_a, keys_b], info)."""
    p = _named_file(path, who)
    _stats_one_piece(p, device, who, "path_distances")
    a = seq_a if isinstance(seq_a, bytes) else seq_a.encode()
    b = seq_b if isinstance(seq_b, bytes) else seq_b.encode()
    bad = False
    if weight_tag:
        raw, dist, _ids, keys, info, oriented, bad = nat.seq_distance_from_path(
            p, _dist_opts(directed, raw_bytes_id, device, weight_tag), a, b, weighted=True)
    else:
        raw, dist, _ids, keys, info, oriented = nat.seq_distance_from_path(p, _dist_opts(directed, raw_bytes_id, device),
                                                                           a, b)
    _graph_pass(raw, raw_bytes_id, verbose, path)
    if directed:
        _warn_oriented(raw, oriented)
    if bad:
        raise NotImplementedError(_BAD_WEIGHT)
    missing = [repr(x) for x, k in ((seq_a, keys[0]), (seq_b, keys[1])) if not k]
    if missing:
        raise KeyError(f"sequence(s) {', '.join(missing)} not found")
    if not raw_bytes_id:
        keys = [[k.decode("ascii") for k in ks] for ks in keys]
    return dist, keys, info


def sequence_distance(path, seq_a, seq_b, *, directed: bool = True, raw_bytes_id: bool = False,
                      verbose: bool = False, device: int = 0, return_info: bool = False, weight_tag=None):
    """``sequence_distance`` (gfa2network/analysis.py:68-113) / ``gfa2network distance GFA --seq A B``
    (cli.py:308-321) on a file where the reference takes a graph built with ``store_seq=True``: the
    fewest hops (an int) from any node whose sequence is ``seq_a`` to any node whose sequence is
    ``seq_b`` (``str`` encoded as UTF-8), 0 when the two sets meet.  A node's sequence is that of the
    last S record of its name that has one (parser.py:135-163, builders.py:164-189).  The file is
    parsed once: its bytes, the CSR and the node names stay in HBM, the S records are matched there
    (g2n_seq.hip) and the two node sets go to the path-distance search; no sequence comes back.
    After the build's own errors and warnings: the orientation warning on a directed graph,
    KeyError("sequence(s) 'X' not found"), NetworkXNoPath("no path between sequences").  Stdin and
    file objects raise NotImplementedError.  ``device`` and ``return_info`` (also return the
    g2n_seq_info fields) are extensions.  ``weight_tag`` (extension; ``None`` or ``""``: the hops
    above, unchanged): the shortest path's length, a ``float``, over the graph a weight tag builds, as
    ``genome_distance``'s."""
    dist, _keys, info = _seq_pass(path, seq_a, seq_b, directed, raw_bytes_id, verbose, device, "sequence_distance",
                                  weight_tag)
    if dist == (np.inf if weight_tag else 0xFFFFFFFF):
        raise NetworkXNoPath("no path between sequences")
    return (dist, info) if return_info else dist


def sequence_nodes(path, seq_a, seq_b, *, directed: bool = True, raw_bytes_id: bool = False, device: int = 0,
                   weight_tag=None):
    """The reference's ``seq2nodes[seq_a]``, ``seq2nodes[seq_b]`` (analysis.py:96-108) without the
    search (extension): the keys (``str``, or ``bytes`` with ``raw_bytes_id``) of the nodes that carry
    each sequence, in node order.  Errors and warnings as ``sequence_distance``'s, up to the
    KeyError.  ``weight_tag`` is accepted and ignored: the node sets do not depend on it."""
    _dist, keys, _info = _seq_pass(path, seq_a, seq_b, directed, raw_bytes_id, False, device, "sequence_nodes")
    return keys[0], keys[1]


def graph_matrix(path, *, directed: bool = True, weight_tag=None, raw_bytes_id: bool = False,
                 return_node_list: bool = False, device: int = 0):
    """The weighted adjacency matrix of the GRAPH ``parse_gfa(path, build_graph=True, directed=...,
    weight_tag=...)`` builds (extension), as a float64 ``scipy.sparse.csr_matrix`` with the nodes in
    first-touch order: what ``nx.to_scipy_sparse_array(G, weight="weight", format="csr")`` gives for
    it, and the matrix to hand to ``path_distances(A, paths, weighted=True)``.  It is not the matrix
    ``parse_gfa(build_matrix=True, weight_tag=...)`` returns, which sums repeated records: a graph
    edge's length is the weight of the last record of that edge carrying a numeric tag
    (builders.py:246-256: ``add_edge`` overwrites, and sets ``weight`` only for such a record), 1.0
    when none does; an undirected build stores both cells of an edge, an explicit 0.0 stays stored.
    Built on the GPU in one pass over the file (g2n_graph_weights_from_path); without a tag every
    stored value is 1.0.  Errors and the unsupported-record warning as ``parse_gfa``'s; the node
    list as its ``return_node_list``."""
    p = _named_file(path, "graph_matrix")
    _stats_one_piece(p, device, "graph_matrix", "path_distances")
    dt = np.dtype("float64")
    if weight_tag:
        raw = nat.graph_weights_from_path(p, nat.make_options(directed=directed, weight_tag=weight_tag,
                                                              want_node_names=return_node_list, device=device))
        return finalize(raw, dtype=dt, return_node_list=return_node_list, raw_bytes_id=raw_bytes_id, verbose=False,
                        path=path)
    raw = nat.build_from_path(p, nat.make_options(directed=directed, asymmetric=True, dtype="bool", output=nat.OUT_CSR,
                                                  want_node_names=return_node_list, device=device))
    out = finalize(raw, dtype=np.dtype("bool"), return_node_list=return_node_list, raw_bytes_id=raw_bytes_id,
                   verbose=False, path=path)
    A = out[0] if return_node_list else out
    A = sp.csr_matrix((np.ones(A.nnz, dtype=dt), A.indices, A.indptr), shape=A.shape)
    return (A, out[1]) if return_node_list else A


def _run(path, opts) -> RawResult:
    """GFAParser's source rules (parser.py:95-112): file object, '-' = stdin, else a path."""
    if hasattr(path, "read"):
        return nat.build_from_buffer(path.read(), opts)
    p = str(path)
    if p == "-":
        return nat.build_from_buffer(sys.stdin.buffer.read(), opts)
    return nat.build_from_path(p, opts)


def export_edge_list(gfa, output="-", *, bidirected: bool = False, device: int = 0) -> None:
    """``gfa2network export GFA --format edge-list [--bidirected] --output PATH`` (cli.py:264-281).

    One ``u\tv`` line per L/E/C record in stream order (bidirected: ``u:ori\tv:ori``), the
    record keys the reference's parser yields (parser.py:206-341), rendered on the GPU from the
    same parse as the matrix path (``G2N_OUT_EDGE_LIST``).  Failure behaviour follows the
    reference's streaming loop: the output file is opened first, the lines of the records
    before a failing one are written, then the failure is raised (a malformed record, the
    ``u.decode()`` / ``v.decode()`` of a key that is not UTF-8, or a gzip error after the lines
    gzip returned); the unsupported-record warning is emitted as by ``GFAParser``.
    """
    opts = nat.make_options(bidirected=bidirected, output=nat.OUT_EDGE_LIST, device=device)
    fh = open(output, "wb") if output != "-" else None  # cli.py:266-267: opened before parsing
    try:
        src = gfa
        if not hasattr(gfa, "read") and str(gfa) == "-":
            src = io.BytesIO(sys.stdin.buffer.read())  # parser.py:104: sys.stdin.buffer, not gunzipped
        if hasattr(src, "read"):
            raw = nat.build_from_buffer(src.read(), opts)
        else:
            raw = nat.build_from_path(str(src), opts)
        if raw.has_warning:  # parser.py:124-130
            warnings.warn(f"Skipping unsupported record: {chr(raw.warn_byte)}", RuntimeWarning, stacklevel=2)
        # on a failure the text holds the lines the reference wrote before it: the records before
        # a malformed line, before an undecodable key, or before the gzip error (the lines gzip
        # returned) — rendered by the native build from the input it already holds
        text = raw.data if raw.format == "text" and raw.data is not None else np.zeros(0, np.uint8)
        if fh is not None:
            fh.write(memoryview(text))
        else:
            sys.stdout.flush()
            sys.stdout.buffer.write(memoryview(text))
            sys.stdout.buffer.flush()
        raise_for_status(raw, np.dtype("bool"), gfa)
    finally:
        if fh is not None:
            fh.close()


_JSON_NODES_PREFIX = '{"directed": true, "multigraph": false, "graph": {}, "nodes": [{"id": '


def export_graph_json(gfa, output="-", *, bidirected: bool = False, keep_directed_bidir: bool = False,
                      raw_bytes_id: bool = False, device: int = 0) -> None:
    """``gfa2network [--raw-bytes-id] export GFA --format json [--bidirected [--keep-directed-bidir]]
    --output PATH`` (cli.py:282-306): ``json.dump(nx.node_link_data(G))`` of the graph
    ``parse_gfa(GFA, build_graph=True, directed=True, ...)`` builds — a ``DiGraph``, with ``--bidirected``
    a ``MultiGraph``, with ``--keep-directed-bidir`` too a ``MultiDiGraph`` — byte for byte, without a
    graph object: the nodes in first-touch order, the links in NetworkX's adjacency order (a repeated
    directed pair keeps its last record's orientations, a repeated multigraph pair counts its ``key``),
    grouped, ordered and rendered on the GPU from the same parse as the matrix path
    (``G2N_OUT_GRAPH_JSON``).  Sources as ``export_edge_list``: a named file, ``"-"`` (stdin) or a file
    object; ``output`` a path or ``"-"`` (stdout).

    As in the reference the graph is built before the output is opened: the one-shot warning comes first,
    then any error of the build (the parser's, or the ASCII decode of a node key, whichever the stream
    meets first) leaves no file.  With ``raw_bytes_id`` the keys stay ``bytes``, which ``json.dump``
    cannot serialise: a graph with a node writes the document up to the first node's id and raises its
    ``TypeError``.  NetworkX's own ``FutureWarning`` about ``node_link_data``'s ``edges=`` default is
    not reproduced.  A file whose working set exceeds one GPU's free HBM raises ``NotImplementedError``.
    """
    src = gfa
    if not hasattr(gfa, "read") and str(gfa) == "-":
        src = io.BytesIO(sys.stdin.buffer.read())  # parser.py:104: sys.stdin.buffer, not gunzipped
    if not hasattr(src, "read"):
        _stats_one_piece(src, device, "export_graph_json", "convert_format")
    opts = nat.make_options(bidirected=bidirected, keep_directed_bidir=keep_directed_bidir,
                            want_node_names=not raw_bytes_id, output=nat.OUT_GRAPH_JSON, device=device)
    raw = nat.build_from_buffer(src.read(), opts) if hasattr(src, "read") else nat.build_from_path(str(src), opts)
    _graph_pass(raw, raw_bytes_id, False, gfa)
    if raw_bytes_id and raw.n_nodes:
        text = _JSON_NODES_PREFIX.encode()  # json.dump streams: what it wrote before it met the bytes key
    else:
        text = raw.data if raw.format == "text" and raw.data is not None else np.zeros(0, np.uint8)
    if output != "-":
        with open(output, "wb") as fh:  # cli.py:302-306: opened only once the graph exists
            fh.write(memoryview(text))
    else:
        sys.stdout.flush()
        sys.stdout.buffer.write(memoryview(text))
        sys.stdout.buffer.flush()
    if raw_bytes_id and raw.n_nodes:
        raise TypeError("Object of type bytes is not JSON serializable")


def _gexf_head(creator: str, lastmodified: str) -> bytes:
    """What ``nx.write_gexf`` writes before the ``<graph>`` element (networkx/readwrite/gexf.py
    GEXFWriter.__init__, version 1.2draft, prettyprint), with ElementTree's escapes: the date is an
    attribute (``_escape_attrib``), the creator a text (``_escape_cdata``)."""
    date = lastmodified.replace("&", "&amp;").replace("<", "&lt;").replace(">", "&gt;").replace('"', "&quot;")
    date = date.replace("\r", "&#13;").replace("\n", "&#10;").replace("\t", "&#09;")
    text = creator.replace("&", "&amp;").replace("<", "&lt;").replace(">", "&gt;")
    head = ("<?xml version='1.0' encoding='utf-8'?>\n"
            '<gexf xmlns="http://www.gexf.net/1.2draft" xmlns:xsi="http://www.w3.org/2001/XMLSchema-instance" '
            'xsi:schemaLocation="http://www.gexf.net/1.2draft http://www.gexf.net/1.2draft/gexf.xsd" version="1.2">\n'
            f'  <meta lastmodifieddate="{date}">\n'
            f"    <creator>{text}</creator>\n"
            "  </meta>\n")
    return head.encode("utf-8", "xmlcharrefreplace")


def export_graph_gexf(gfa, output, *, bidirected: bool = False, keep_directed_bidir: bool = False,
                      raw_bytes_id: bool = False, device: int = 0, creator: str | None = None,
                      lastmodified: str | None = None) -> None:
    """``gfa2network [--raw-bytes-id] export GFA --format gexf [--bidirected [--keep-directed-bidir]]
    --output PATH`` (cli.py:296-297): ``nx.write_gexf(G, PATH)`` of the graph ``parse_gfa(GFA,
    build_graph=True, directed=True, ...)`` builds — the GEXF 1.2draft document Gephi reads, byte for
    byte, without a graph object.  The graph, its node order and its edge order are ``export_graph_json``'s
    (a ``DiGraph`` edge carries its last record's ``orientation_from`` / ``orientation_to``, a multigraph
    edge its ``networkx_key``); the XML is rendered on the GPU from the same parse
    (``G2N_OUT_GRAPH_GEXF``).  NetworkX's GEXF writer uses ``xml.etree.ElementTree`` only, so the bytes
    depend on nothing but the graph and two strings, both arguments here (extensions):

    * ``creator``: the ``<creator>`` text; ``None`` = ``f"NetworkX {networkx.__version__}"`` (when
      networkx does not import, its ``ImportError`` is raised: the reference could not run either);
    * ``lastmodified``: the ``lastmodifieddate``; ``None`` = ``time.strftime("%Y-%m-%d")``, taken when
      the document is written.

    Sources as ``export_graph_json``: a named file, ``"-"`` (stdin) or a file object.  ``output`` is a
    path or a binary file object, as ``nx.write_gexf`` takes both.  The path ``"-"`` is a FILE named
    ``-``: the reference passes ``args.output`` straight to ``nx.write_gexf``, so its default
    ``--output -`` creates ``./-``; pass a file object such as ``sys.stdout.buffer`` to write to stdout.

    As in the reference the graph is built first: the one-shot warning, then any error of the build (the
    parser's, or the ASCII decode of a node key, whichever the stream meets first), which leaves no file;
    the output is opened only after the build succeeded.  With ``raw_bytes_id`` the keys stay ``bytes`` and
    the document holds ``str(key)``, the bytes repr (unlike JSON, a complete document).  A file whose
    working set exceeds one GPU's free HBM raises ``NotImplementedError``.
    """
    if creator is None:
        import networkx

        creator = f"NetworkX {networkx.__version__}"
    src = gfa
    if not hasattr(gfa, "read") and str(gfa) == "-":
        src = io.BytesIO(sys.stdin.buffer.read())  # parser.py:104: sys.stdin.buffer, not gunzipped
    if not hasattr(src, "read"):
        _stats_one_piece(src, device, "export_graph_gexf", "convert_format")
    opts = nat.make_options(bidirected=bidirected, keep_directed_bidir=keep_directed_bidir,
                            want_node_names=not raw_bytes_id, output=nat.OUT_GRAPH_GEXF, device=device)
    # the head the device renders behind has the final length only when the date is given: the build gets a
    # head of its own and the document's first bytes are composed again when it is written
    built = _gexf_head(creator, lastmodified if lastmodified is not None else time.strftime("%Y-%m-%d"))
    if hasattr(src, "read"):
        raw = nat.graph_gexf_from_buffer(src.read(), opts, built)
    else:
        raw = nat.graph_gexf_from_path(str(src), opts, built)
    _graph_pass(raw, raw_bytes_id, False, gfa)
    if raw.format != "text" or raw.data is None or raw.data[:len(built)].tobytes() != built:
        raise RuntimeError("export_graph_gexf: the build returned no document")
    head = built if lastmodified is not None else _gexf_head(creator, time.strftime("%Y-%m-%d"))
    body = memoryview(raw.data)[len(built):]
    if hasattr(output, "write"):
        output.write(head)
        output.write(body)
        return
    with open(output, "wb") as fh:  # nx.write_gexf's open_file: any path, "-" included, names a file
        fh.write(head)
        fh.write(body)


def _keep_index_dtype(M, raw):
    """scipy's coo.tocsr() / tocsc() past 2^31 - 1 COO entries keeps int64 indptr / indices even when
    summing duplicates leaves fewer entries (_coo_to_compressed sizes by coo.nnz); the compressed
    constructor's content check alone would narrow them."""
    if raw.indptr.dtype == np.int64 and M.indptr.dtype != np.int64:
        M.indices, M.indptr = raw.indices, raw.indptr
    return M


def _coo_data(A):
    """The COO's values as the kernels take them: a dtype outside the native five only when every value
    is 1 (then int32 ones, the sums mapped back by _unit_values), else NotImplementedError."""
    ext = _unit_dtype(A.dtype)
    if ext is None:
        return A.data, None
    if not bool(np.all(A.data == 1)):
        raise NotImplementedError(f"GPU COO->CSR of dtype {ext} takes unit values only "
                                  f"(any values: {', '.join(nat.DTYPE_CODES)})")
    return np.ones(len(A.data), dtype=np.int32), ext


def _native_tocsr(A, device: int = 0):
    """scipy coo.tocsr() on the GPU: duplicates summed in dtype in scipy's order."""
    n_rows, n_cols = A.shape
    data, ext = _coo_data(A)
    raw = nat.coo_to_csr(A.row, A.col, data, n_rows, n_cols, device)
    vals = raw.data if ext is None else _unit_values(raw.data, ext)
    return _keep_index_dtype(sp.csr_matrix((vals, raw.indices, raw.indptr), shape=A.shape, dtype=A.dtype), raw)


def _native_tocsc(A, device: int = 0):
    """scipy coo.tocsc(): the CSR of the transposed coordinates, read as CSC."""
    n_rows, n_cols = A.shape
    data, ext = _coo_data(A)
    raw = nat.coo_to_csr(A.col, A.row, data, n_cols, n_rows, device)
    vals = raw.data if ext is None else _unit_values(raw.data, ext)
    return _keep_index_dtype(sp.csc_matrix((vals, raw.indices, raw.indptr), shape=A.shape, dtype=A.dtype), raw)


def convert_format(A, fmt: str, *, verbose: bool = False):
    """GPU ``convert_format`` (gfa2network/utils.py:40-63)."""
    fmt = fmt.lower()
    if fmt not in {"csr", "csc", "coo", "dok"}:
        raise ValueError("matrix-format must be csr|csc|coo|dok")
    if fmt == "coo":
        return A
    if verbose:  # utils.py:49-53
        if _HAS_TQDM:
            bar = tqdm(total=1, bar_format="{desc} …{elapsed}", desc=f"[convert→{fmt}")
        else:
            start = time.perf_counter()
            print(f"[convert] -> {fmt} …", end="", file=sys.stderr, flush=True)
    if fmt == A.format:
        out = A
    elif fmt == "dok":
        # a Python dict of (row, col) -> value: scipy's own asformat("dok") on the GPU-built
        # matrix (for a COO it sums duplicates in place, in stream order, as the reference's
        # A.asformat(fmt) does, utils.py:55)
        out = A.asformat("dok")
    else:
        coo = A if A.format == "coo" else A.tocoo()
        out = _native_tocsr(coo) if fmt == "csr" else _native_tocsc(coo)
    if verbose:  # utils.py:56-62
        if _HAS_TQDM:
            bar.update(1)
            bar.close()
        else:
            print(f" done in {time.perf_counter() - start:,.1f}s", file=sys.stderr)
    return out


def save_matrix(A, dest: Path, *, verbose: bool = False, max_dense_gb: float = 5.0):
    """Writer of ``convert --matrix`` (gfa2network/utils.py:66-105): same guard and formats."""
    MAX_DENSE_BYTES = max_dense_gb * 1_000_000_000
    dest = Path(dest)
    if dest.suffix in {".csv", ".npy"}:
        nnz = A.nnz if sp.issparse(A) else A.size
        itemsize = A.dtype.itemsize if hasattr(A, "dtype") else 8
        if nnz * itemsize > MAX_DENSE_BYTES:
            raise MemoryError(
                f"dense export would allocate {nnz*itemsize/1e9:.1f} GB; choose a sparse .npz or write an edge list instead"
            )
    if verbose:  # utils.py:77-83
        msg = f"[save] {dest.suffix[1:]} → {dest}"
        if _HAS_TQDM:
            bar = tqdm(total=1, bar_format="{desc} …{elapsed}", desc=msg)
        else:
            start = time.perf_counter()
            print(msg, "...", end="", file=sys.stderr, flush=True)
    if dest.suffix == ".npz":
        save_npz(dest, A)
    elif dest.suffix in {".npy", ".csv"} and _dense_native(A) and not write_dense(A, dest, return_info=True)["declined"]:
        pass  # rendered from the CSR on the GPU: the same bytes, no dense array
    elif dest.suffix == ".npy":
        np.save(dest, A.toarray() if sp.issparse(A) else A)
    elif dest.suffix == ".csv":
        np.savetxt(dest, A.toarray() if sp.issparse(A) else A, delimiter=",", fmt="%.6g")
    else:
        raise ValueError("matrix path must end with .npz, .npy, or .csv")
    if verbose:  # utils.py:99-105
        if _HAS_TQDM:
            bar.update(1)
            bar.close()
        else:
            print(f" done in {time.perf_counter() - start:,.1f}s", file=sys.stderr)


def _dense_native(A) -> bool:
    """Whether save_matrix renders A's dense .csv / .npy on the GPU: a scipy CSR or CSC of one of the five native
    dtypes with no empty dimension, and a device to run on.  Everything else — COO and DOK (whose toarray() sums
    duplicates in an order that is scipy's), ndarray and DataFrame, other dtypes, empty shapes, no GPU — is
    numpy's, as in the reference."""
    return (sp.issparse(A) and A.format in ("csr", "csc") and len(A.shape) == 2 and min(A.shape) >= 1
            and np.dtype(A.dtype).name in nat.DTYPE_CODES and nat.device_count() > 0)


_DENSE_KINDS = {".csv": nat.DENSE_CSV, "csv": nat.DENSE_CSV, nat.DENSE_CSV: nat.DENSE_CSV,
                ".npy": nat.DENSE_NPY, "npy": nat.DENSE_NPY, nat.DENSE_NPY: nat.DENSE_NPY}


def _dense_csr(A, device: int, kind: int):
    """A's CSR arrays for the dense writers, as (indptr, indices, data, rows, columns of the array they describe).
    A CSC's csv goes through the native COO -> CSR (a canonical CSC holds no duplicates, so nothing is added); its
    .npy needs no conversion: csc.toarray() is Fortran-ordered, so the body is the C-order array of the transpose,
    whose CSR the CSC's own arrays are.  Index arrays of other or mixed dtypes are widened to int64."""
    if not sp.issparse(A) or A.format not in ("csr", "csc") or len(A.shape) != 2:
        raise TypeError("the GPU dense writers take a scipy sparse CSR or CSC matrix")
    if np.dtype(A.dtype).name not in nat.DTYPE_CODES:
        raise NotImplementedError(f"GPU dense writers support {sorted(nat.DTYPE_CODES)}, not {A.dtype}")
    if min(A.shape) < 1:
        raise ValueError("the GPU dense writers take a matrix without an empty dimension")
    n_rows, n_cols = int(A.shape[0]), int(A.shape[1])
    if A.format == "csc":
        if kind == nat.DENSE_NPY:
            n_rows, n_cols = n_cols, n_rows
        else:
            A = _native_tocsr(A.tocoo(), device)
    indptr, indices = A.indptr, A.indices
    if indptr.dtype != indices.dtype or indptr.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
        indptr, indices = indptr.astype(np.int64), indices.astype(np.int64)
    return indptr, indices, A.data, n_rows, n_cols


def write_dense(A, dest, *, device: int = 0, band_bytes: int | None = None, return_info: bool = False):
    """``np.savetxt(dest, A.toarray(), delimiter=",", fmt="%.6g")`` (dest ending in .csv) or ``np.save(dest,
    A.toarray())`` (.npy) of a scipy CSR / CSC matrix, byte for byte, without the dense array: the document is
    rendered on the GPU in bands of ``band_bytes`` and streamed to the file (g2n_write_dense).  The info dict
    (``return_info``) holds doc_bytes, bands, tile_bytes, band_bytes and declined; declined = 1 means nothing was
    written — a row that is not sorted or holds a duplicate, which numpy's route adds up in scipy's order.
    There is no CPU route here: without a GPU the call raises."""
    dest = Path(dest)
    if dest.suffix not in (".csv", ".npy"):
        raise ValueError("a dense matrix path must end with .npy or .csv")
    kind = _DENSE_KINDS[dest.suffix]
    indptr, indices, data, n_rows, n_cols = _dense_csr(A, device, kind)
    # (an array with one row or one column is C-contiguous whatever its order: numpy's header says so)
    fortran = A.format == "csc" and min(A.shape) > 1
    head = _npy_header_of(A.shape, data.dtype, fortran) if kind == nat.DENSE_NPY else b""
    with open(dest, "wb" if kind == nat.DENSE_NPY else "w"):  # numpy's own open: the same OSError cases
        pass
    info = nat.write_dense(os.fspath(dest), kind, head, indptr, indices, data, n_rows, n_cols,
                           band_bytes=band_bytes or 0, device=device)
    return info if return_info else None


def dense_range(A, kind, b0: int, b1: int, *, device: int = 0) -> bytes:
    """Bytes [b0, b1) of the body of the document write_dense writes for A (``kind``: "csv" or "npy"; the .npy
    body follows its header; a CSC's is Fortran-ordered, as csc.toarray() is): any place of a document too large to
    write (g2n_dense_range)."""
    if kind not in _DENSE_KINDS:
        raise ValueError('kind must be "csv" or "npy"')
    indptr, indices, data, n_rows, n_cols = _dense_csr(A, device, _DENSE_KINDS[kind])
    out, _info = nat.dense_range(_DENSE_KINDS[kind], indptr, indices, data, n_rows, n_cols, int(b0), int(b1),
                                 device=device)
    if out is None:
        raise ValueError("GPU dense range: a row of the matrix is not sorted or holds a duplicate")
    return out


def _npy_header_of(shape: tuple, dtype, fortran_order: bool = False) -> bytes:
    """The .npy header of an array of this shape, dtype and order (numpy's own format code)."""
    import io

    from numpy.lib import format as npf

    bio = io.BytesIO()
    npf._write_array_header(bio, {"shape": tuple(int(x) for x in shape), "fortran_order": bool(fortran_order),
                                  "descr": npf.dtype_to_descr(np.dtype(dtype))}, None)
    return bio.getvalue()


def _npy_header(val: np.ndarray) -> bytes:
    """The .npy header numpy.lib.format.write_array puts before val's bytes."""
    import io

    from numpy.lib import format as npf

    bio = io.BytesIO()
    npf._write_array_header(bio, npf.header_data_from_array_1_0(val), None)
    return bio.getvalue()


def save_npz(file, matrix, compressed: bool = True) -> None:
    """scipy.sparse.save_npz (scipy 1.15 _matrix_io.py, members in its order) with the zip written
    natively: members deflated on host threads (g2n_write_npz), numpy's zip64 layout; loads with
    scipy.sparse.load_npz / numpy.load.  Uncompressed or unsupported formats fall back to scipy."""
    fmt = matrix.format
    if not compressed or fmt not in ("csr", "csc", "bsr", "coo") or fmt == "bsr":
        sp.save_npz(file, matrix, compressed=compressed)
        return
    path = os.fspath(file)
    if not path.endswith(".npz"):  # numpy _savez
        path = path + ".npz"
    members = {}
    if fmt in ("csr", "csc"):
        members.update(indices=matrix.indices, indptr=matrix.indptr)
    else:
        members.update(row=matrix.row, col=matrix.col)
    members.update(format=fmt.encode("ascii"), shape=matrix.shape, data=matrix.data)
    if isinstance(matrix, sp.sparray):
        members.update(_is_array=True)
    out = []
    for key, val in members.items():
        val = np.asanyarray(val)
        if val.dtype.hasobject:
            sp.save_npz(file, matrix, compressed=compressed)
            return
        arr = val if val.flags.c_contiguous else np.ascontiguousarray(val)
        out.append((key + ".npy", _npy_header(val), arr.reshape(-1).view(np.uint8) if arr.size else arr))
    with open(path, "wb"):  # the reference's zipfile.ZipFile(path, "w") open: same OSError cases
        pass
    nat.write_npz(path, out, int(os.environ.get("G2N_NPZ_LEVEL", "-1")))


def save_node_map_native(blob: np.ndarray, offsets: np.ndarray, dest: Path, raw_bytes_id: bool) -> None:
    """save_node_map (utils.py:108-114) from the names blob, written on host threads.  raw_bytes_id:
    names are decoded while writing, so the first non-UTF-8 name raises after the lines before it
    were written, as in the reference."""
    with open(dest, "w"):  # the reference's open(dest, "w"): same OSError cases
        pass
    bad = nat.write_node_map(str(dest), blob, offsets, check_utf8=raw_bytes_id)
    if bad >= 0:
        bytes(blob[offsets[bad]:offsets[bad + 1]]).decode()
        raise AssertionError("decode of the reported name unexpectedly succeeded")


def save_node_map(nodes, dest: Path) -> None:
    """``<matrix>.nodes.tsv`` sidecar (gfa2network/utils.py:108-114): ``i\\tname\\n``."""
    with open(dest, "w") as fh:
        for i, node in enumerate(nodes):
            if isinstance(node, (bytes, bytearray)):
                node = node.decode()
            fh.write(f"{i}\t{node}\n")
