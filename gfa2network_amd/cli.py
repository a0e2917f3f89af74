"""``python -m gfa2network_amd convert ...`` — the reference's ``convert --matrix`` front-end.

Same global flags (they precede the subcommand) and ``convert`` flags as
gfa2network/cli.py:22-135, same handler order (cli.py:193-250): print the backend, parse,
``convert_format``, ``save_matrix`` (dense guard -> SystemExit), then the
``<matrix>.nodes.tsv`` sidecar.  ``--matrix x.csv`` and ``x.npy`` of the CSR or CSC a build returns are rendered
on the GPU from the sparse matrix (``write_dense``: numpy's bytes, no dense array; the five ``--dtype`` choices,
rows without duplicates); ``--matrix-format coo|dok`` keeps numpy's ``toarray()`` route.  ``export --format edge-list`` (cli.py:264-281) renders its
lines on the GPU from the same parse, ``export --format json`` (cli.py:282-306) the graph's node-link
document (``export_graph_json``), ``export --format gexf`` (cli.py:296-297) its GEXF document
(``export_graph_gexf``); ``stats`` (cli.py:152-159, 364-376) prints
``compute_stats``'s six numbers, taken on the GPU from the CSR; ``distance --path``, ``distance
--seq`` and ``distance-matrix`` (cli.py:161-189, 307-363) run their searches on the GPU over the same
CSR (``--seq`` finds the nodes that carry the two sequences there too: ``sequence_distance``; an input
that is no named file is a usage error, exit status 2, where the function raises the reference's
FileNotFoundError).  ``distance --path
A B --method mean`` (extension; the default ``min`` prints what it printed) is ``genome_distance(...,
method="mean")``.  As in
the reference, ``distance`` and ``distance-matrix`` have no ``--weight-tag``: the functions take
``weight_tag=``.  Of the two XML exports gexf is served: NetworkX writes it with
``xml.etree.ElementTree`` alone, so its bytes depend on the graph, the NetworkX version (the creator
string) and the date only, and ``export_graph_gexf`` takes both as arguments.  graphml stays out:
``nx.write_graphml`` picks lxml or ElementTree, whichever it finds, and its bytes differ.  ``--graph``
(a NetworkX object) is outside the GPU GFA->CSR path.
"""
from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

from . import __version__
from .api import (compute_stats, convert_format, export_edge_list, export_graph_gexf, export_graph_json, genome_distance, genome_distance_matrix, parse_gfa,
                  parse_gfa_names, save_matrix, save_node_map_native, sequence_distance, write_node_components)


def _parser(extensions: bool = False) -> argparse.ArgumentParser:
    """The reference's parser (its flags, nothing else below the global ``--device``); ``extensions``:
    plus this build's own subcommand flags and subcommands — ``distance --method``, ``components`` — as
    ``main`` parses."""
    parser = argparse.ArgumentParser(prog="gfa2network")
    parser.add_argument("--version", action="version", version=f"gfa2network-amd {__version__}")
    parser.add_argument("--raw-bytes-id", action="store_true", help="Use raw bytes for node identifiers (legacy)")
    parser.add_argument("--max-dense-gb", type=float, default=5.0, help="Abort dense matrix saves over N GB (default 5)")
    parser.add_argument("--max-tag-mb", type=float, default=100.0, help="Warn when stored tags exceed N MB (default 100)")
    parser.add_argument("--device", type=int, default=0, help="HIP device ordinal (GPU build option)")
    sub = parser.add_subparsers(dest="cmd", required=True)

    p = sub.add_parser("convert", help="Convert GFA to a sparse adjacency matrix")
    p.add_argument("gfa", help="Input *.gfa* file or - for stdin")
    p.add_argument("--backend", choices=["networkx", "igraph"], default="networkx", help="Graph backend to use")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--directed", dest="directed", action="store_true", default=True, help="Treat graph as directed")
    g.add_argument("--undirected", dest="directed", action="store_false", help="Treat graph as undirected")
    p.add_argument("--graph", action="store_true", help="Build a NetworkX object (not supported on the GPU path)")
    p.add_argument("--matrix", metavar="PATH", help="Write adjacency matrix to PATH (.npz|.npy|.csv)")
    p.add_argument("--save-matrix", dest="matrix", metavar="PATH", help=argparse.SUPPRESS)
    p.add_argument("--matrix-format", default="csr", help="Sparse format for .npz (csr|csc|coo|dok)")
    p.add_argument("--dtype", choices=["bool", "int8", "int32", "float32", "float64"], default="float64",
                   help="Data type for adjacency matrix")
    p.add_argument("--asymmetric", action="store_true", help="Do not mirror upper triangle")
    p.add_argument("--no-node-map", action="store_true", help="Do not write <matrix>.nodes.tsv sidecar")
    p.add_argument("--weight-tag")
    p.add_argument("--store-seq", action="store_true")
    p.add_argument("--store-tags", action="store_true")
    p.add_argument("--split-on-alignment", action="store_true", help="Split segments at alignment boundaries")
    p.add_argument("--strip-orientation", action="store_true", help="Strip +/- from IDs (v0.1 behaviour)")
    p.add_argument("--bidirected", action="store_true", help="Use bidirected representation")
    p.add_argument("--keep-directed-bidir", action="store_true", help="Keep original directed bidirected behaviour")
    p.add_argument("--verbose", action="store_true")
    p.add_argument("-o", "--output", metavar="PATH", help="Write graph pickle to PATH (not supported)")
    p_exp = sub.add_parser("export", help="Stream edges in simple formats")  # cli.py:137-149
    p_exp.add_argument("gfa")
    p_exp.add_argument("--format", default="edge-list", choices=["edge-list", "graphml", "gexf", "json"])
    p_exp.add_argument("--bidirected", action="store_true")
    p_exp.add_argument("--keep-directed-bidir", action="store_true",
                       help="Keep original directed bidirected behaviour")
    p_exp.add_argument("--output", help="Output path", default="-")
    p_stats = sub.add_parser("stats", help="Print basic graph statistics", aliases=["stat"])  # cli.py:152-159
    p_stats.add_argument("gfa", help="Input *.gfa* file")
    g2 = p_stats.add_mutually_exclusive_group()
    g2.add_argument("--directed", dest="directed", action="store_true", default=True)
    g2.add_argument("--undirected", dest="directed", action="store_false")
    p_stats.add_argument("--strip-orientation", action="store_true")
    p_dist = sub.add_parser("distance", help="Compute distances")  # cli.py:161-175
    p_dist.add_argument("gfa", help="Input *.gfa* file")
    g3 = p_dist.add_mutually_exclusive_group(required=True)
    g3.add_argument("--seq", nargs=2, metavar=("SEQ_A", "SEQ_B"))
    g3.add_argument("--path", nargs=2, metavar=("PATH_A", "PATH_B"))
    g4 = p_dist.add_mutually_exclusive_group()
    g4.add_argument("--directed", dest="directed", action="store_true", default=True)
    g4.add_argument("--undirected", dest="directed", action="store_false")
    p_dist.add_argument("--backend", choices=["networkx", "igraph"], default="networkx", help="Graph backend to use")
    if extensions:
        p_dist.add_argument("--method", choices=["min", "mean"], default="min",
                            help="--path: the minimal distance, or the mean over all node pairs (GPU build option)")
    p_dist.add_argument("--verbose", action="store_true")
    p_dm = sub.add_parser("distance-matrix", help="Pairwise distances between paths")  # cli.py:177-189
    p_dm.add_argument("gfa", help="Input *.gfa* file")
    p_dm.add_argument("-o", "--output", required=True, help="Write matrix to PATH (.csv|.npy|.npz)")
    p_dm.add_argument("--method", choices=["min", "mean"], default="min")
    p_dm.add_argument("--backend", choices=["networkx", "igraph"], default="networkx", help="Graph backend to use")
    p_dm.add_argument("--verbose", action="store_true")
    if extensions:
        p_cc = sub.add_parser("components", help="List each node's connected component (GPU build option)")
        p_cc.add_argument("gfa", help="Input *.gfa* file")
        p_cc.add_argument("-o", "--output", metavar="PATH", default="-", help="Write the listing to PATH (default: stdout)")
        g5 = p_cc.add_mutually_exclusive_group()
        g5.add_argument("--directed", dest="directed", action="store_true", default=True)
        g5.add_argument("--undirected", dest="directed", action="store_false")
        p_cc.add_argument("--strip-orientation", action="store_true")
        p_cc.add_argument("--sizes", action="store_true", help="Print component<TAB>size per component instead")
    return parser


def main(argv: list[str] | None = None) -> None:
    parser = _parser(extensions=True)
    args = parser.parse_args(argv)
    if args.cmd == "export":
        if args.format == "json":  # cli.py:282-306
            export_graph_json(args.gfa, args.output, bidirected=args.bidirected,
                              keep_directed_bidir=args.keep_directed_bidir, raw_bytes_id=args.raw_bytes_id,
                              device=args.device)
            return
        if args.format == "gexf":  # cli.py:296-297: args.output goes to nx.write_gexf as it is ("-" names a file)
            export_graph_gexf(args.gfa, args.output, bidirected=args.bidirected,
                              keep_directed_bidir=args.keep_directed_bidir, raw_bytes_id=args.raw_bytes_id,
                              device=args.device)
            return
        if args.format != "edge-list":
            parser.error(f"export --format {args.format}: nx.write_graphml's bytes depend on the XML library NetworkX "
                         "finds (lxml or ElementTree); it stays with the reference")
        export_edge_list(args.gfa, args.output, bidirected=args.bidirected, device=args.device)
        return
    if args.cmd == "stats":  # cli.py:364-376 (the alias reaches no branch there either)
        stats = compute_stats(args.gfa, directed=args.directed, strip_orientation=args.strip_orientation,
                              raw_bytes_id=args.raw_bytes_id, device=args.device)
        print("nodes\t", stats["nodes"])
        print("edges\t", stats["edges"])
        print("paths\t", stats["paths"])
        print("components\t", stats["components"])
        print("max_degree\t", stats["max_degree"])
        print("density\t", f"{stats['density']:.6g}")
        return
    if args.cmd == "stat":
        return
    if args.cmd == "components":  # (extension) node<TAB>component per node of the graph stats measures
        write_node_components(args.gfa, args.output, directed=args.directed, strip_orientation=args.strip_orientation,
                              raw_bytes_id=args.raw_bytes_id, sizes=args.sizes, device=args.device)
        return
    if args.cmd == "distance":  # cli.py:307-346
        if args.backend == "igraph":
            parser.error("--backend igraph is outside the GPU GFA->CSR path")
        if args.seq:  # cli.py:308-321
            if args.method != "min":
                parser.error("distance --method mean takes --path (sequence_distance has no method)")
            seq_a, seq_b = args.seq
            # sequence_distance matches the sequences in the file's staged bytes: it takes a named file,
            # not stdin.  An input that is none is a usage error here, before a GPU is touched (the
            # function itself raises the reference's FileNotFoundError)
            if args.gfa == "-" or not os.path.isfile(args.gfa):
                parser.error(f"distance --seq reads a named file (sequence_distance(GFA, A, B)): {args.gfa!r} is none")
            print(sequence_distance(args.gfa, seq_a, seq_b, directed=args.directed, raw_bytes_id=args.raw_bytes_id,
                                    verbose=args.verbose, device=args.device))
            return
        name_a, name_b = args.path
        try:
            dist = genome_distance(args.gfa, name_a.encode() if args.raw_bytes_id else name_a,
                                   name_b.encode() if args.raw_bytes_id else name_b, method=args.method,
                                   directed=args.directed, raw_bytes_id=args.raw_bytes_id, verbose=args.verbose, device=args.device)
        except KeyError as exc:
            if type(exc) is not KeyError:  # (a NodeNotFound defined without networkx)
                raise
            msg = exc.args[0]
            if isinstance(msg, bytes):
                msg = msg.decode()
            raise SystemExit(f"unknown path: {msg}") from exc
        print(dist)
        return
    if args.cmd == "distance-matrix":  # cli.py:347-363
        M = genome_distance_matrix(args.gfa, method=args.method, raw_bytes_id=args.raw_bytes_id, backend=args.backend,
                                   verbose=args.verbose, device=args.device)
        try:
            save_matrix(M, Path(args.output), verbose=args.verbose, max_dense_gb=args.max_dense_gb)
        except MemoryError as exc:
            raise SystemExit(str(exc)) from exc
        return
    if args.cmd != "convert":
        parser.error(f"'{args.cmd}' is outside the GPU GFA->CSR path; use the reference gfa2network for it")
    if not args.graph and not args.matrix:
        parser.error("convert requires --graph or --matrix")
    if args.graph:
        parser.error("--graph (NetworkX / igraph objects) is outside the GPU GFA->CSR path")
    print(f"Using backend: {args.backend}")
    want_nodes = not args.no_node_map
    kw = dict(
        directed=args.directed,
        weight_tag=args.weight_tag,
        store_seq=args.store_seq,
        store_tags=args.store_tags,
        strip_orientation=args.strip_orientation,
        verbose=args.verbose,
        bidirected=args.bidirected,
        keep_directed_bidir=args.keep_directed_bidir,
        backend=args.backend,
        dtype=args.dtype,
        asymmetric=args.asymmetric,
        raw_bytes_id=args.raw_bytes_id,
        max_tag_mb=args.max_tag_mb,
        split_on_alignment=args.split_on_alignment,
        device=args.device,
    )
    if want_nodes:  # names stay a blob: the sidecar is written natively (no Python list)
        A, blob, offs = parse_gfa_names(args.gfa, **kw)
    else:
        A = parse_gfa(args.gfa, build_graph=False, build_matrix=True, return_node_list=False, **kw)
    A = convert_format(A, args.matrix_format, verbose=args.verbose)
    try:
        save_matrix(A, Path(args.matrix), verbose=args.verbose, max_dense_gb=args.max_dense_gb)
    except MemoryError as exc:
        raise SystemExit(str(exc)) from exc
    if want_nodes:
        save_node_map_native(blob, offs, Path(str(args.matrix) + ".nodes.tsv"), args.raw_bytes_id)


if __name__ == "__main__":  # pragma: no cover
    main(sys.argv[1:])
