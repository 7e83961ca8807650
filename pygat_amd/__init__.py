"""pygat_amd -- MI355X-native GAT attention layer (hand-written HIP for gfx950).

Drop-in for the hot path of ArielleRosinski/pyGAT: `GraphAttentionLayer`,
`SpGraphAttentionLayer` (reference layers.py) and `GAT` (reference models.py).
Importing this package loads libpygat_amd.so and fails loudly when it is absent:
there is no CPU / eager fallback.
"""
from ._lib import lib, LIB_PATH, padded_width          # noqa: F401  (raises if the .so is missing)
from .graph import CSRGraph, as_graph                   # noqa: F401
from .ops import gat_level, GATLevelFn, gemm, set_gemm_mode, get_gemm_mode, gemm_mode            # noqa: F401
from .layers import GraphAttentionLayer, SpGraphAttentionLayer  # noqa: F401
from .models import GAT                                 # noqa: F401
from .graphed import GraphedLevel, FusedEpoch           # noqa: F401
from .losses import EluLogSoftmaxNLL, BCEWithLogits                    # noqa: F401
from .optim import Adam                                 # noqa: F401
from .gatv2 import GraphAttentionLayerV2, SpGraphAttentionLayerV2, gatv2_level, GATv2LevelFn  # noqa: F401
from .spmm import EdgePattern, spmm, SpecialSpmmFunction, SpecialSpmm, clear_pattern_cache    # noqa: F401
from .edge_softmax import edge_softmax                  # noqa: F401
from .dot_attention import edge_dot, dot_attention, dot_attention_dropout, attention_dropout_mask, dot_attention_edge      # noqa: F401
from .additive_attention import additive_attention, additive_attention_bf16, additive_attention_dropout    # noqa: F401
from .gatv2_attention import (gatv2_attention, gatv2_attention_bf16, gatv2_attention_dropout, gatv2_attention_edge,    # noqa: F401
                              gatv2_attention_edge_bf16)
from .sampling import sample_neighbors, sample_blocks, SampledBlock    # noqa: F401
from .sampling import sample_neighbors_weighted, sample_blocks_weighted    # noqa: F401
from .subgraph import induced_subgraph, random_walk, InducedSubgraph       # noqa: F401
from .linkpred import find_edges, negative_edges, link_batch, LinkBatch    # noqa: F401

__all__ = ["Adam", "BCEWithLogits", "CSRGraph", "as_graph", "gat_level", "GATLevelFn", "gemm", "set_gemm_mode", "get_gemm_mode", "gemm_mode", "GraphAttentionLayer",
           "SpGraphAttentionLayer", "GAT", "padded_width", "LIB_PATH", "GraphAttentionLayerV2",
           "SpGraphAttentionLayerV2", "gatv2_level", "GATv2LevelFn", "GraphedLevel", "FusedEpoch", "EluLogSoftmaxNLL",
           "EdgePattern", "spmm", "SpecialSpmmFunction", "SpecialSpmm", "clear_pattern_cache", "edge_softmax", "edge_dot", "dot_attention",
           "dot_attention_dropout", "attention_dropout_mask", "dot_attention_edge", "additive_attention"]
__all__ += ["gatv2_attention", "additive_attention_dropout", "gatv2_attention_dropout", "gatv2_attention_edge"]
__all__ += ["additive_attention_bf16", "gatv2_attention_bf16", "gatv2_attention_edge_bf16"]
__all__ += ["sample_neighbors", "sample_blocks", "SampledBlock", "sample_neighbors_weighted", "sample_blocks_weighted"]
__all__ += ["induced_subgraph", "random_walk", "InducedSubgraph"]
__all__ += ["find_edges", "negative_edges", "link_batch", "LinkBatch"]
