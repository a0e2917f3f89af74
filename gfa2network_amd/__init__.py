"""gfa2network_amd — MI355X-native GFA -> CSR ingest for the gfa2network call surface.

Drop-in for the reference's matrix path: ``parse_gfa(..., build_matrix=True)``,
``convert_format``, ``compute_stats``, ``load_paths``, ``genome_distance_matrix``, ``sequence_distance`` and the
``convert --matrix`` / ``export --format edge-list|json|gexf`` / ``stats`` / ``components`` / ``distance --path`` / ``distance --seq`` / ``distance-matrix`` CLI (sclipman/gfa2network
gfa2network/__init__.py:3-14).  The work runs in hand-written gfx950 kernels behind the
C-ABI in include/g2n.h (libg2n.so, loaded with ctypes).
"""
from .api import (compute_stats, convert_format, dense_range, export_edge_list, export_graph_gexf, export_graph_json, genome_distance, genome_distance_matrix,
                  graph_matrix, graph_stats, load_paths, node_distances, pair_sums, parse_gfa, parse_gfa_sharded, path_distances,
                  sequence_distance, sequence_nodes, write_dense, graph_components, split_components, node_components)

__version__ = "0.3.0"

__all__ = ["parse_gfa", "parse_gfa_sharded", "convert_format", "export_edge_list", "export_graph_json", "export_graph_gexf", "compute_stats", "graph_stats",
           "graph_matrix",
           "path_distances", "node_distances", "pair_sums", "load_paths", "genome_distance", "genome_distance_matrix", "sequence_distance",
           "sequence_nodes", "write_dense", "dense_range", "graph_components", "split_components", "node_components",
           "__version__"]
