"""dgn_amd: MI355X-native implementation of the DGN directional-aggregation layer.

Host side in Python on PyTorch-ROCm (device memory, streams, torch.distributed);
the aggregation itself is hand-written HIP for gfx950 behind the C ABI of
``include/dgn_hip.h`` (``libdgn_hip.so``, loaded with ctypes).  GPU only: there is no
CPU fallback anywhere in this package.
"""
from .graph import DGNGraph, as_dgn_graph, compute_edge_weights
from .spec import AGGREGATOR_NAMES, SCALER_NAMES, make_plan
from .ops import directional_aggregate
from .layers import FCLayer, MLP, get_activation
from .dgn_layer import (AGGREGATORS, SCALERS, DGNLayer, DGNLayerComplex, DGNLayerSimple, DGNLayerTower, DGNTower, EdgeTypeFeatures, get_dropout_state, reset_dropout_state, set_dropout_state)
from .readout import VirtualNode, max_nodes, mean_nodes, readout, sum_nodes
from .eig import laplacian_eigvecs, laplacian_eig_small, laplacian_eig_mid, batch_eig, positional_encoding, eig_multiplicity, EigAugment
from .ops import balanced_cross_entropy, masked_bce_with_logits, mlp_head, multi_embedding
from .superpixels import coord_encoding, knn_edge_counts, knn_graph, sort_eig, superpixel_eig
from .nets import AtomEncoder, BondEncoder, DGNHIVNet, DGNNet, DGNNodeNet, DGNPCBANet, accuracy_sbm, ap_ogb, rocauc_ogb
from .ops import class_cross_entropy, feature_embedding
from .nets import DGNSuperpixelNet, accuracy_mnist_cifar
from .ops import masked_l1_loss, node_input
from .data import Batch, PackedGraphs

__all__ = ["DGNGraph", "as_dgn_graph", "compute_edge_weights", "make_plan", "directional_aggregate", "FCLayer", "MLP",
           "get_activation", "AGGREGATORS", "SCALERS", "DGNLayer", "DGNLayerSimple", "DGNLayerComplex", "DGNLayerTower",
           "DGNTower", "EdgeTypeFeatures", "AGGREGATOR_NAMES", "SCALER_NAMES", "VirtualNode", "sum_nodes", "mean_nodes", "max_nodes", "readout",
           "laplacian_eigvecs", "laplacian_eig_small", "laplacian_eig_mid", "batch_eig", "positional_encoding", "eig_multiplicity", "balanced_cross_entropy", "DGNNet", "DGNNodeNet", "accuracy_sbm",
           "multi_embedding", "masked_bce_with_logits", "mlp_head", "AtomEncoder", "BondEncoder", "DGNHIVNet", "DGNPCBANet", "rocauc_ogb", "ap_ogb",
           "knn_edge_counts", "knn_graph", "coord_encoding", "sort_eig", "superpixel_eig",
           "feature_embedding", "class_cross_entropy", "DGNSuperpixelNet", "accuracy_mnist_cifar",
           "node_input", "masked_l1_loss", "PackedGraphs", "Batch", "EigAugment"]
