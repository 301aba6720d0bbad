"""Host-side mirrors of the reference's nets (the direct callers of the layer): graph regression,
``realworld_benchmark/nets/molecules_graph_regression/dgn_net.py:8-95`` (DGNNet) and ``nets/mlp_readout_layer.py:13-32`` (MLPReadout); node
classification on SBM graphs, ``nets/SBMs_node_classification/dgn_net.py:8-81`` (DGNNodeNet, with ``accuracy_sbm``); graph classification on
the OGB molecule sets, ``nets/HIV_graph_classification/dgn_net.py`` and ``nets/PCBA_graph_classification/dgn_net.py`` (DGNHIVNet, DGNPCBANet
with ogb's AtomEncoder / BondEncoder and the evaluator's two metrics, at the end of this file); graph classification on the MNIST / CIFAR10
superpixel graphs, ``nets/superpixels_graph_classification/dgn_net.py:7-78`` (DGNSuperpixelNet, with ``accuracy_mnist_cifar``).

Same constructor dictionary, ``forward(g, h, e, snorm_n, snorm_e)``, ``loss`` and ``state_dict`` keys (a reference checkpoint loads
as is); no DGL call: the layers are ``dgn_amd.DGNLayer``, the readouts ``dgn_amd.readout``, and with ``edge_feat`` the bond-type
embedding is handed to the layers as ``EdgeTypeFeatures(embedding_e.weight, bond_type)`` -- the K x F table inside the sweep instead
of the gathered ``[E, edge_dim]`` rows (dgn_net.py:75).  ``g`` is a ``DGNGraph`` (or anything ``as_dgn_graph`` accepts) that carries
``batch_num_nodes`` for the readout and ``ndata['eig']``.  Parity: fixture G10 (tests/golden/make_golden.py::g10_net), produced by
the unmodified reference net."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .dgn_layer import DGNLayer, EdgeTypeFeatures
from .readout import VirtualNode, readout


class MLPReadout(nn.Module):
    """``L`` hidden Linear + ReLU layers (widths halving when ``decreasing_dim``) and an output Linear; keys ``FC_layers.{i}.*``.  On the
    device the whole head is ``ops.mlp_head``: one launch forward, two backward (widths up to 128, up to four Linears); other shapes, CPU
    tensors and ``ops.FUSED_MLP_HEAD = False`` run the ``nn.Linear`` loop."""

    def __init__(self, input_dim: int, output_dim: int, L: int = 2, decreasing_dim: bool = True):
        super().__init__()
        widths = [input_dim // 2 ** i if decreasing_dim else input_dim for i in range(L + 1)]
        self.FC_layers = nn.ModuleList([nn.Linear(widths[i], widths[i + 1], bias=True) for i in range(L)] +
                                       [nn.Linear(widths[L], output_dim, bias=True)])
        self.L = L

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from . import ops
        weights = [fc.weight for fc in self.FC_layers]
        if ops.FUSED_MLP_HEAD and ops.mlp_head_supported(x, weights):
            return ops.mlp_head(x, weights, [fc.bias for fc in self.FC_layers])
        for fc in self.FC_layers[:-1]:
            x = F.relu(fc(x))
        return self.FC_layers[-1](x)


class _SmallTableEmbedding(torch.autograd.Function):
    """``nn.Embedding`` lookup (nets/molecules_graph_regression/dgn_net.py:44, :66: 28 atom types) whose weight gradient is the product
    one_hot(idx)^T g instead of torch's sort-based ``embedding_dense_backward``: on a 3 000-node batch that backward is ~100 us of sort /
    scatter kernels (149 us eager) next to 0.1 ms layers; the product is two small kernels, and deterministic."""

    @staticmethod
    def forward(ctx, weight, idx):
        ctx.save_for_backward(idx)
        ctx.rows = weight.shape[0]
        return weight.index_select(0, idx)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        onehot = torch.zeros(idx.numel(), ctx.rows, dtype=g.dtype, device=g.device)
        onehot.scatter_(1, idx.reshape(-1, 1), 1.0)
        return onehot.t().mm(g.reshape(idx.numel(), -1)), None


def small_table_embedding(emb: nn.Embedding, idx: torch.Tensor) -> torch.Tensor:
    """``emb(idx)`` for small tables of plain embeddings (no padding_idx / max_norm / sparse), else the module itself."""
    if (emb.num_embeddings <= 256 and idx.dim() == 1 and idx.is_cuda and emb.padding_idx is None and emb.max_norm is None and not emb.sparse
            and not emb.scale_grad_by_freq):
        return _SmallTableEmbedding.apply(emb.weight, idx)
    return emb(idx)


def _input_with_pos_enc(net: nn.Module, tables, idx: torch.Tensor, embed, g) -> torch.Tensor:
    """``h = in_feat_dropout(embedding_h(h)) + embedding_pos_enc(g.ndata['pos_enc'])`` (nets/molecules_graph_regression/dgn_net.py:59-62,
    nets/SBMs_node_classification/dgn_net.py:56-59, nets/HIV_graph_classification/dgn_net.py:62-66).  The dropout acts on the embedding
    before the add, so the two terms are fused -- ``ops.node_input``: one launch forward, two backward -- only while it is inactive
    (``p == 0`` or ``eval()``) and the op supports the shapes; otherwise the composition: ``embed(idx)``, ``nn.Linear``, add.  ``tables``:
    the plain embedding weights behind ``embed``, or None where the module is no plain lookup."""
    from . import ops
    pe = g.ndata["pos_enc"].to(idx.device)
    fc, drop = net.embedding_pos_enc, net.in_feat_dropout
    if (tables is not None and idx.is_cuda and not (drop.training and drop.p > 0) and idx.dtype == torch.int64
            and ops.node_input_supported(tables, pe, fc.weight)):
        return ops.node_input(idx, tables, pe, fc.weight, fc.bias)
    return drop(embed(idx)) + fc(pe)


def _plain_table(emb: nn.Embedding):
    """``[emb.weight]`` for an embedding that is nothing but a lookup (what ``ops.node_input`` fuses), else None."""
    plain = emb.padding_idx is None and emb.max_norm is None and not emb.sparse and not emb.scale_grad_by_freq
    return [emb.weight] if plain else None


def _dgn_layers(p: dict, towers=None) -> nn.ModuleList:
    """The nets' layer stack from the constructor dictionary: ``L - 1`` layers ``hidden_dim -> hidden_dim`` and one to ``out_dim``, created
    in that order (the order of the initialisation's RNG draws); ``towers=None`` leaves the layer factory's default."""
    hidden = p["hidden_dim"]
    extra = {} if towers is None else {"towers": towers}
    make = lambda o: DGNLayer(in_dim=hidden, out_dim=o, dropout=p["dropout"], graph_norm=p["graph_norm"], batch_norm=p["batch_norm"],
                              residual=p["residual"], aggregators=p["aggregators"], scalers=p["scalers"], avg_d=p["avg_d"],
                              type_net=p["type_net"], edge_features=p["edge_feat"], edge_dim=p["edge_dim"],
                              pretrans_layers=p["pretrans_layers"], posttrans_layers=p["posttrans_layers"], **extra).model
    return nn.ModuleList([make(hidden) for _ in range(p["L"] - 1)] + [make(p["out_dim"])])


class DGNNet(nn.Module):
    def __init__(self, net_params: dict):
        super().__init__()
        p = net_params
        hidden, out_dim = p["hidden_dim"], p["out_dim"]
        self.type_net, self.pos_enc_dim, self.readout = p["type_net"], p["pos_enc_dim"], p["readout"]
        self.edge_feat, self.device = p["edge_feat"], p["device"]
        self.in_feat_dropout = nn.Dropout(p["in_feat_dropout"])
        self.embedding_h = nn.Embedding(p["num_atom_type"], hidden)
        if self.pos_enc_dim > 0:
            self.embedding_pos_enc = nn.Linear(self.pos_enc_dim, hidden)
        if self.edge_feat:
            self.embedding_e = nn.Embedding(p["num_bond_type"], p["edge_dim"])
        self.layers = _dgn_layers(p)
        directional = self.readout in ("directional", "directional_abs")
        self.MLP_layer = MLPReadout(2 * out_dim if directional else out_dim, 1)

    def forward(self, g, h, e, snorm_n, snorm_e=None):
        if self.pos_enc_dim > 0:
            h = _input_with_pos_enc(self, _plain_table(self.embedding_h) if h.dim() == 1 else None, h,
                                    lambda idx: small_table_embedding(self.embedding_h, idx), g)
        else:
            h = self.in_feat_dropout(small_table_embedding(self.embedding_h, h))
        if self.edge_feat:
            e = EdgeTypeFeatures(self.embedding_e.weight, e)
        for conv in self.layers:
            h = conv(g, h, e, snorm_n)
        g.ndata["h"] = h
        mode = self.readout if self.readout in ("sum", "max", "mean", "directional", "directional_abs") else "mean"
        return self.MLP_layer(readout(g, h, mode))

    def loss(self, scores, targets):
        """``nn.L1Loss()`` (dgn_net.py:90-92).  On the device it is ``ops.masked_l1_loss``: two launches forward and one backward, and a
        NaN target marks an entry that does not count (the graph rows behind the batch of a captured step)."""
        if scores.is_cuda and targets.is_cuda and scores.dtype == torch.float32 and scores.shape == targets.shape and scores.dim() in (1, 2):
            from .ops import masked_l1_loss
            return masked_l1_loss(scores, targets)
        return F.l1_loss(scores, targets)


class DGNNodeNet(nn.Module):
    """Mirror of the reference's node-classification net (``nets/SBMs_node_classification/dgn_net.py:8-65``: PATTERN / CLUSTER): node-type
    embedding, ``L`` DGN layers, a per-node ``MLPReadout`` to ``n_classes`` scores.  Same constructor dictionary, ``forward`` signature and
    ``state_dict`` keys (``embedding_h``, optional ``embedding_pos_enc``, ``layers.{i}.*``, ``MLP_layer.FC_layers.{i}.*``).  ``loss`` is the
    reference's batch-balanced cross-entropy (:67-81) as ``ops.balanced_cross_entropy``: three launches, no host read-back.  The MLP head
    (widths such as 47 -> 23 -> 11 -> 2, outside the tall-skinny Linear's shapes) is ``ops.mlp_head``: one launch on every node forward,
    two backward.  Parity: fixture G11
    (tests/golden/make_golden_node.py), produced by the unmodified reference net."""

    def __init__(self, net_params: dict):
        super().__init__()
        p = net_params
        hidden, out_dim = p["hidden_dim"], p["out_dim"]
        self.type_net, self.pos_enc_dim, self.readout = p["type_net"], p["pos_enc_dim"], p["readout"]
        self.edge_feat, self.device, self.n_classes = p["edge_feat"], p["device"], p["n_classes"]
        if self.pos_enc_dim > 0:
            self.embedding_pos_enc = nn.Linear(self.pos_enc_dim, hidden)
        self.embedding_h = nn.Embedding(p["in_dim"], hidden)
        self.in_feat_dropout = nn.Dropout(p["in_feat_dropout"])
        self.layers = _dgn_layers(p)
        self.MLP_layer = MLPReadout(out_dim, self.n_classes)

    def forward(self, g, h, e, snorm_n, snorm_e=None):
        if self.pos_enc_dim > 0:
            h = _input_with_pos_enc(self, _plain_table(self.embedding_h) if h.dim() == 1 else None, h,
                                    lambda idx: small_table_embedding(self.embedding_h, idx), g)
        else:
            h = self.in_feat_dropout(small_table_embedding(self.embedding_h, h))
        for conv in self.layers:
            h = conv(g, h, e, snorm_n)
        return self.MLP_layer(h)

    def loss(self, pred, label, confusion: bool = False):
        """``label < 0`` marks a padding row.  ``confusion=True``: ``(loss, [C, C] int64 device matrix)`` for ``accuracy_sbm``."""
        from .ops import balanced_cross_entropy
        return balanced_cross_entropy(pred, label, self.n_classes, confusion=confusion)


def accuracy_sbm(confusion: torch.Tensor) -> torch.Tensor:
    """The reference's ``accuracy_SBM`` (train/metrics.py:41-53) from the confusion matrix of ``ops.balanced_cross_entropy`` (which holds the
    reference's prediction rule), device ops only, a 0-dim float64 tensor: ``100 * sum_r recall_r / #{r: CM[r, r] > 0}`` over the classes
    present among the labels.  No class with a hit: 0 (the reference divides by zero).  Matrices of several batches may be added up first;
    the reference averages per-batch accuracies instead, so add up accuracies to reproduce its epoch figure."""
    cm = confusion.to(torch.float64)
    count, hit = cm.sum(1), cm.diagonal()
    recall = hit / count.clamp_min(1.0)                   # (an absent class has no hit either: 0 / 1)
    scored = (hit > 0).sum()
    return 100.0 * recall.sum() / scored.clamp_min(1)     # (no class with a hit: 0 / 1)


# ---- superpixel graph classification (MNIST, CIFAR10) -------------------------------------------------------------------------------

def _feature_linear(fc: nn.Linear, x: torch.Tensor) -> torch.Tensor:
    """``fc(x)`` for an input embedding: ``ops.feature_embedding`` where it is supported, ``F.linear`` otherwise (CPU tensors, wider
    inputs, an ``x`` that asks for a gradient)."""
    from . import ops
    if ops.feature_embedding_supported(x, fc.weight):
        return ops.feature_embedding(x, fc.weight, fc.bias)
    return F.linear(x, fc.weight, fc.bias)


class DGNSuperpixelNet(nn.Module):
    """Mirror of the reference's superpixel graph-classification net (``nets/superpixels_graph_classification/dgn_net.py:7-78``: MNIST /
    CIFAR10): ``nn.Linear`` embedding of the node features (mean pixel value(s) + two coordinates), ``L`` DGN layers, sum / max / mean
    readout (anything else: mean), ``MLPReadout`` to ``n_classes`` scores.  Same constructor dictionary (no ``pos_enc_dim``, no
    ``device``), ``forward`` signature and ``state_dict`` keys (``embedding_h``, optional ``embedding_e``, ``layers.{i}.*``,
    ``MLP_layer.FC_layers.{i}.*``); the layers' ``towers`` stays at the factory's default as there.  The embeddings run as
    ``ops.feature_embedding`` (one launch forward, two backward); with ``edge_feat`` the embedded ``[E, edge_dim]`` rows go to the layers
    as a dense ``e``.  ``loss`` is ``ops.class_cross_entropy``: two launches, no host read-back, with the hit count of
    ``accuracy_MNIST_CIFAR`` on request.  Parity: fixture G16 (tests/golden/make_golden_superpixel_net.py), produced by the unmodified net."""

    def __init__(self, net_params: dict):
        super().__init__()
        p = net_params
        hidden, out_dim = p["hidden_dim"], p["out_dim"]
        self.type_net, self.readout, self.edge_feat, self.n_classes = p["type_net"], p["readout"], p["edge_feat"], p["n_classes"]
        self.embedding_h = nn.Linear(p["in_dim"], hidden)
        self.in_feat_dropout = nn.Dropout(p["in_feat_dropout"])
        if self.edge_feat:
            self.embedding_e = nn.Linear(p["in_dim_edge"], p["edge_dim"])
        self.layers = _dgn_layers(p)
        self.MLP_layer = MLPReadout(out_dim, self.n_classes)

    def forward(self, g, h, e, snorm_n, snorm_e=None):
        h = self.in_feat_dropout(_feature_linear(self.embedding_h, h))
        if self.edge_feat:
            e = _feature_linear(self.embedding_e, e)
        for conv in self.layers:
            h = conv(g, h, e, snorm_n)
        g.ndata["h"] = h
        return self.MLP_layer(readout(g, h, self.readout if self.readout in ("sum", "max", "mean") else "mean"))

    def loss(self, pred, label, hits: bool = False):
        """On the device ``label < 0`` marks a padding row.  ``hits=True``: ``(loss, 0-dim int64 count of the correct arg-max predictions)``.
        CPU tensors: ``F.cross_entropy``, the reference's own call."""
        if not pred.is_cuda:
            loss = F.cross_entropy(pred, label)
            return (loss, accuracy_mnist_cifar(pred, label)) if hits else loss
        from .ops import class_cross_entropy
        return class_cross_entropy(pred, label, hits=hits)


def accuracy_mnist_cifar(scores: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """The reference's ``accuracy_MNIST_CIFAR`` (train/metrics.py:25-28) without its ``.item()``: the number of rows whose arg-max score
    sits at the label, a 0-dim int64 tensor on the scores' device (a label < 0 never matches: padding rows count nowhere)."""
    return (scores.detach().argmax(dim=1) == labels).sum()



OGB_ATOM_DIMS = [119, 4, 12, 12, 10, 6, 6, 2, 2]      # atomic number, chirality, degree, formal charge, H count, radical e-, hybridisation, aromatic, in ring
OGB_BOND_DIMS = [5, 6, 2]                             # bond type, stereo, conjugated


class _MultiEncoder(nn.Module):
    """Sum of one ``nn.Embedding`` per integer feature column (xavier-uniform weights), as ``ops.multi_embedding``: one launch forward,
    two backward, the parameters the separate embedding weights of the ``state_dict``."""

    _LIST = "embedding_list"

    def __init__(self, emb_dim: int, dims):
        super().__init__()
        self.dims = [int(d) for d in dims]
        embs = nn.ModuleList()
        for d in self.dims:
            emb = nn.Embedding(d, emb_dim)
            nn.init.xavier_uniform_(emb.weight.data)
            embs.append(emb)
        setattr(self, self._LIST, embs)

    @property
    def weights(self):
        return [emb.weight for emb in getattr(self, self._LIST)]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from .ops import multi_embedding
        return multi_embedding(self.weights, x)

    def validate(self, x: torch.Tensor) -> None:
        """Raise what ``nn.Embedding`` raises for a value outside its column's table (one host sync; the kernels clamp instead)."""
        from .ops import multi_embedding_validate
        multi_embedding_validate(self.weights, x)


class AtomEncoder(_MultiEncoder):
    """``ogb.graphproppred.mol_encoder.AtomEncoder``: nine embeddings of the atom feature columns, summed; keys
    ``atom_embedding_list.{i}.weight``.  The default ``dims`` are ogb's ``get_atom_feature_dims()`` of the releases before 1.3.0 (four
    chirality values); from 1.3.0 on the chirality list has a fifth, 'misc' entry: a checkpoint of such a release loads with
    ``dims=[119, 5, 12, 12, 10, 6, 6, 2, 2]``."""

    _LIST = "atom_embedding_list"

    def __init__(self, emb_dim: int, dims=OGB_ATOM_DIMS):
        super().__init__(emb_dim, dims)


class BondEncoder(_MultiEncoder):
    """``ogb.graphproppred.mol_encoder.BondEncoder``: three embeddings of the bond feature columns, summed; keys
    ``bond_embedding_list.{i}.weight``; the default ``dims`` are ogb's ``get_bond_feature_dims()`` (the same in the releases before and
    after 1.3.0).  ``forward`` gives the ``[E, emb_dim]`` rows; ``edge_type_features`` hands the layers the same numbers as an
    ``EdgeTypeFeatures``: the combined table ``[prod(dims) = 60, emb_dim]`` -- the differentiable sum of the three tables in the forward's
    own order of adds -- and one mixed-radix type per edge, so that a layer that can keeps the table inside its sweep."""

    _LIST = "bond_embedding_list"

    def __init__(self, emb_dim: int, dims=OGB_BOND_DIMS):
        super().__init__(emb_dim, dims)

    def combined_table(self) -> torch.Tensor:
        """``table[(i_0 d_1 + i_1) d_2 + i_2] = ((0 + T_0[i_0]) + T_1[i_1]) + T_2[i_2]`` (any number of columns)."""
        table = None
        for w in self.weights:
            table = (0 + w) if table is None else (table.unsqueeze(1) + w.unsqueeze(0)).reshape(-1, w.shape[1])
        return table

    def combined_types(self, e: torch.Tensor, graph=None) -> torch.Tensor:
        """The mixed-radix type of every edge (columns clamped into their tables first), cached on ``graph`` for the batch's tensor."""
        ent = graph.__dict__.get("_bond_types") if graph is not None else None
        if ent is not None and ent[0] is e and ent[1] == e._version and ent[3] == self.dims:
            return ent[2]
        hi = torch.tensor(self.dims, dtype=e.dtype, device=e.device) - 1
        cols = torch.minimum(e.clamp_min(0), hi)
        radix = [1] * len(self.dims)
        for c in range(len(self.dims) - 2, -1, -1):
            radix[c] = radix[c + 1] * self.dims[c + 1]
        t = (cols * torch.tensor(radix, dtype=e.dtype, device=e.device)).sum(1)
        if graph is not None:
            graph.__dict__["_bond_types"] = (e, e._version, t, list(self.dims))
        return t

    def edge_type_features(self, e: torch.Tensor, graph=None):
        """What the layers take as ``e``: ``EdgeTypeFeatures(combined table, combined types)``, or the gathered rows where the combined
        table would exceed ``ops.MAX_EDGE_TABLE`` floats."""
        from .ops import MAX_EDGE_TABLE
        n_types = 1
        for d in self.dims:
            n_types *= d
        if n_types * self.weights[0].shape[1] > MAX_EDGE_TABLE:
            return self(e)
        return EdgeTypeFeatures(self.combined_table(), self.combined_types(e, graph))


class _DGNMolNet(nn.Module):
    """What the reference's two OGB graph-classification nets share: AtomEncoder (+ BondEncoder with ``edge_feat``), ``L`` DGN layers
    (with ``VirtualNode`` layers after all but the last one where the net has them), sum / max / mean readout, ``MLPReadout``, and the
    binary cross-entropy with logits over the labelled entries as ``ops.masked_bce_with_logits``."""

    def __init__(self, net_params: dict, n_tasks: int, towers, decreasing_dim: bool, virtual_node, pos_enc_dim: int):
        super().__init__()
        p = net_params
        hidden, out_dim, n_layers = p["hidden_dim"], p["out_dim"], p["L"]
        self.type_net, self.readout, self.edge_feat, self.device = p["type_net"], p["readout"], p["edge_feat"], p["device"]
        self.pos_enc_dim, self.n_tasks, self.virtual_node = pos_enc_dim, n_tasks, virtual_node
        if self.pos_enc_dim > 0:
            self.embedding_pos_enc = nn.Linear(self.pos_enc_dim, hidden)
        self.in_feat_dropout = nn.Dropout(p["in_feat_dropout"])
        self.embedding_h = AtomEncoder(emb_dim=hidden)
        if self.edge_feat:
            self.embedding_e = BondEncoder(emb_dim=p["edge_dim"])
        self.layers = _dgn_layers(p, towers)
        self.MLP_layer = MLPReadout(out_dim, n_tasks, decreasing_dim=decreasing_dim)
        self.virtual_node_layers = None
        if virtual_node is not None and virtual_node.lower() != "none":
            self.virtual_node_layers = nn.ModuleList([VirtualNode(dim=hidden, dropout=p["dropout"], batch_norm=p["batch_norm"], bias=True,
                                                                  vn_type=virtual_node, residual=p["residual"]) for _ in range(n_layers - 1)])

    def forward(self, g, h, e, snorm_n, snorm_e=None):
        if self.pos_enc_dim > 0:
            h = _input_with_pos_enc(self, self.embedding_h.weights if h.dim() == 2 else None, h, self.embedding_h, g)
        else:
            h = self.in_feat_dropout(self.embedding_h(h))
        if self.edge_feat:
            e = self.embedding_e.edge_type_features(e, g if hasattr(g, "__dict__") else None)
        vn_h = 0
        for i, conv in enumerate(self.layers):
            h = conv(g, h, e, snorm_n)
            if self.virtual_node_layers is not None and i < len(self.virtual_node_layers):
                vn_h, h = self.virtual_node_layers[i](g, h, vn_h)
        g.ndata["h"] = h
        return self.MLP_layer(readout(g, h, self.readout if self.readout in ("sum", "max", "mean") else "mean"))

    def loss(self, scores, labels):
        """The reference's signature.  ``labels`` with one dimension less than ``scores`` (ogbg-molhiv: ``[G]`` of any dtype) get the task
        dimension; 1-D scores and labels (ogbg-molpcba, selected by the loop's boolean index) are taken as they are; un-masked ``[G, T]``
        labels with NaN for "not measured" are masked by the kernel -- no read-back, capturable."""
        from .ops import masked_bce_with_logits
        if labels.dim() == scores.dim() - 1:
            labels = labels.unsqueeze(-1)
        return masked_bce_with_logits(scores, labels)


class DGNHIVNet(_DGNMolNet):
    """Mirror of ``nets/HIV_graph_classification/dgn_net.py:13-89`` (ogbg-molhiv): same constructor dictionary, ``forward`` signature and
    ``state_dict`` keys (optional ``embedding_pos_enc``, ``embedding_h.atom_embedding_list.{i}``, optional
    ``embedding_e.bond_embedding_list.{i}``, ``layers.{i}.*``, ``MLP_layer.FC_layers.{i}.*``); one score per graph; the layers' ``towers``
    stays at the factory's default as there.  Parity: fixture G13 (tests/golden/make_golden_mol.py), produced by the unmodified net."""

    def __init__(self, net_params: dict):
        super().__init__(net_params, 1, None, True, None, net_params["pos_enc_dim"])


class DGNPCBANet(_DGNMolNet):
    """Mirror of ``nets/PCBA_graph_classification/dgn_net.py:9-102`` (ogbg-molpcba): 128 scores per graph, ``towers``,
    ``decreasing_dim`` of the head, ``virtual_node`` (``VirtualNode`` layers, keys ``virtual_node_layers.{i}.*``); no positional
    encoding.  Parity: fixture G13."""

    def __init__(self, net_params: dict):
        p = net_params
        super().__init__(p, 128, p["towers"], p["decreasing_dim"], p["virtual_node"], 0)


def _ranked_tasks(scores: torch.Tensor, labels: torch.Tensor):
    """Per task column, in DESCENDING score order with the unlabelled rows behind: positives / negatives as float64 0/1, their inclusive
    running counts, and for every slot the first and last slot of its group of equal scores."""
    if scores.dim() == 1:
        scores, labels = scores.unsqueeze(-1), labels.unsqueeze(-1)
    labels = labels.to(torch.float64)
    labelled = labels == labels
    s = torch.where(labelled, scores.to(torch.float64), torch.full_like(labels, float("-inf")))
    s, order = torch.sort(s, dim=0, descending=True, stable=True)
    y = torch.gather(labels, 0, order)
    pos, neg = (y == 1).to(torch.float64), (y == 0).to(torch.float64)
    G = s.shape[0]
    slot = torch.arange(G, device=s.device).unsqueeze(1).expand_as(s)
    change = s[1:] != s[:-1]
    edge = torch.ones(1, s.shape[1], dtype=torch.bool, device=s.device)
    first = torch.cummax(torch.where(torch.cat([edge, change]), slot, torch.zeros_like(slot)), dim=0).values
    last = torch.cummin(torch.where(torch.cat([change, edge]), slot, torch.full_like(slot, G - 1)).flip(0), dim=0).values.flip(0)
    return pos, neg, pos.cumsum(0), neg.cumsum(0), first, last


def _mean_over_scorable(per_task, n_pos, n_neg):
    ok = (n_pos > 0) & (n_neg > 0)
    return torch.where(ok, per_task, torch.zeros_like(per_task)).sum() / ok.sum()         # (no scorable task: 0 / 0 = nan)


def rocauc_ogb(scores: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """The ``rocauc`` of ogb's ``Evaluator('ogbg-molhiv')`` (train/train_HIV_graph_classification.py:43-45): per task column over its
    labelled rows (label == label), only for tasks with at least one positive (== 1) and one negative (== 0), the area under the ROC
    curve with tied scores sharing their average rank (scikit-learn's ``roc_auc_score``); the mean over those tasks.  Device ops only
    (sort, cumsum), a 0-dim float64 tensor, once per epoch.  No scorable task: ``nan`` -- ogb raises a RuntimeError there."""
    if scores.shape[0] == 0:
        return torch.full((), float("nan"), dtype=torch.float64, device=scores.device)
    pos, neg, cpos, cneg, first, last = _ranked_tasks(scores, labels)
    n_pos, n_neg = cpos[-1], cneg[-1]
    # a positive beats the negatives behind its group of equal scores and half of those inside it
    before = torch.gather(cneg - neg, 0, first)
    through = torch.gather(cneg, 0, last)
    wins = (pos * (n_neg.unsqueeze(0) - 0.5 * (before + through))).sum(0)
    return _mean_over_scorable(wins / (n_pos * n_neg), n_pos, n_neg)


def ap_ogb(scores: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """The ``ap`` of ogb's ``Evaluator('ogbg-molpcba')`` (train/train_PCBA_graph_classification.py:40-41): per task column over its
    labelled rows, only for tasks with at least one positive and one negative, scikit-learn's ``average_precision_score`` -- the step-wise
    sum over the distinct thresholds of (recall step) x precision; the mean over those tasks.  Device ops only, a 0-dim float64 tensor,
    once per epoch.  No scorable task: ``nan`` -- ogb raises a RuntimeError there."""
    if scores.shape[0] == 0:
        return torch.full((), float("nan"), dtype=torch.float64, device=scores.device)
    pos, neg, cpos, cneg, first, last = _ranked_tasks(scores, labels)
    n_pos, n_neg = cpos[-1], cneg[-1]
    tp, fp = torch.gather(cpos, 0, last), torch.gather(cneg, 0, last)               # at the threshold of the slot's group
    precision = tp / (tp + fp).clamp_min(1.0)
    return _mean_over_scorable((pos * precision).sum(0) / n_pos, n_pos, n_neg)
