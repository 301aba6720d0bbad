"""DGNLayer operator API of the reference on the MI355X kernels.

Same factory, constructor arguments, ``.model`` attribute, ``forward(g, h, e, snorm_n)`` and ``state_dict``
keys/shapes as realworld_benchmark/nets/dgn_layer.py:52-352, so the benchmark nets (nets/*/dgn_net.py) can
construct and call these layers unchanged.

What differs is everything between ``g.apply_edges`` and the layer's output:
* one fused CSR sweep (``ops.directional_aggregate``) instead of DGL's degree bucketing;
* a 1-layer ``pretrans`` (every shipped config) is affine in ``[h_src || h_dst || ef]`` and is decomposed as
  ``P[src] + Q[dst] + R[edge]`` with node-level GEMMs, so no ``[E, 2F]`` concat is ever built;
* all towers run in ONE sweep (they are column blocks of the message), written tower-major so that the per-tower
  posttrans is one batched GEMM on contiguous matrices;
* the degree scalers are per-row factors and are folded behind the post-aggregation Linear; ``[h || agg]`` is
  produced by the sweep itself (h_in pass-through block); scalers, bias and graph norm are applied by one
  streaming kernel (``ops.scale_combine``), BatchNorm + ReLU + residual by another (``ops.bn_tail``).
Configurations outside these fast paths (multi-layer pretrans/posttrans, a scaler list without ``identity``,
BatchNorm variants the fused tail does not cover) run the same kernels through the generic, unfused route.
"""
from __future__ import annotations

import math

from typing import List, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from .graph import DGNGraph, as_dgn_graph
from .layers import MLP, FCLayer
from . import ops as _ops
from .ops import (bn_tail, bn_tail_fused, bn_tail_supported, combine_bn_tail, directional_aggregate, linear_combine_bn_tail,
                  linear_combine_supported, node_linear, scale_combine, towers_layer, towers_layer_supported)
from .spec import (AGGREGATOR_NAMES, SCALE_AMPLIFICATION, SCALE_IDENTITY, SCALER_NAMES, X_IN_NAME, make_plan,
                   parse_aggregator, parse_scaler)


class _Named:
    """Registry entry: what ``AGGREGATORS[name]`` / ``SCALERS[name]`` return."""

    def __init__(self, name: str):
        self.name = name

    def __repr__(self):
        return f"<{self.__class__.__name__} {self.name}>"


class _Aggregator(_Named):
    """``AGGREGATORS[name](h, eig_s, eig_d, h_in)`` with the reference's mailbox-level signature
    (nets/aggregators.py:8-71): ``h [n, D, F]`` messages, ``eig_s/eig_d [n, D, K]``, ``h_in [n, F]`` -> ``[n, F]``.
    Runs on the HIP kernels: the mailbox is a CSR with constant degree D and slot-level eig inputs."""

    def __call__(self, h, eig_s, eig_d, h_in):
        import numpy as np  # noqa: F401  (kept local: only this convenience path needs nothing else)
        from .graph import compute_edge_weights
        n, D, F_ = h.shape
        dev = h.device
        indptr = torch.arange(0, (n + 1) * D, D, dtype=torch.int64, device=dev)
        g = DGNGraph.from_csr(indptr, torch.zeros(n * D, dtype=torch.int64, device=dev))
        plan = make_plan([self.name], ["identity"])
        w = None
        if plan.n_channels:
            w = compute_edge_weights(g, plan.channels, eig_s_edge=eig_s.reshape(n * D, -1).float().contiguous(),
                                     eig_d_edge=eig_d.reshape(n * D, -1).float().contiguous())
        return directional_aggregate(g, plan, 1.0, m_edge=h.reshape(n * D, F_), x_in=h_in, weights=w)


class _Scaler(_Named):
    """``SCALERS[name](h, D, avg_d)`` (nets/scalers.py:7-18): D is the python-int degree of the bucket."""

    def __call__(self, h, D=None, avg_d=None):
        import numpy as np
        kind = parse_scaler(self.name)
        if kind == SCALE_IDENTITY:
            return h
        if kind == SCALE_AMPLIFICATION:
            return h * (np.log(D + 1) / avg_d["log"])
        return h * (avg_d["log"] / np.log(D + 1))


class _Registry(dict):
    def __init__(self, names, parser, cls):
        super().__init__()
        self._parser, self._cls = parser, cls
        for n in names:
            self[n] = cls(n)

    def __missing__(self, key):
        self._parser(key)          # raises KeyError for unknown names
        self[key] = self._cls(key)  # accepted alias (dirK-smooth)
        return self[key]


AGGREGATORS = _Registry(AGGREGATOR_NAMES, parse_aggregator, _Aggregator)   # nets/aggregators.py:74-93
SCALERS = _Registry(SCALER_NAMES, parse_scaler, _Scaler)              # nets/scalers.py:21


def _names(items: Sequence) -> List[str]:
    return [x if isinstance(x, str) else x.name for x in items]


def _avg_log(avg_d) -> float:
    v = avg_d["log"]
    return float(v.item()) if torch.is_tensor(v) else float(v)


def _slot_dst(graph: DGNGraph) -> torch.Tensor:
    if not hasattr(graph, "_dst_slots"):
        graph._dst_slots = torch.repeat_interleave(torch.arange(graph.num_nodes, device=graph.device), graph.in_degree)
    return graph._dst_slots


_DROP_STATE = {}     # device -> [seed tensor (device int64 scalar, drawn ONCE from torch's generator of that device), calls so far]


def _dropout(x, p, training):
    """F.dropout of the reference's tails; CUDA fp32 tensors through the bit-mask kernels (ops.dropout), anything else through torch.
    One Philox key per device for the life of the process (so ``torch.manual_seed`` BEFORE the first training step fixes every mask of
    the run) and a call counter as the stream offset: no per-call seed kernel -- at the reference's batch sizes the layer is
    launch-bound and a ``torch.randint`` per layer call costs as much as the dropout itself."""
    if training and p > 0 and x.is_cuda and x.dtype == torch.float32:
        seed, offset = _next_dropout_key(x.device)
        y = _ops.dropout(x, p, True, seed=seed, offset=offset)
        _dropout_key_used(seed)
        return y
    return F.dropout(x, p, training=training)


def _block_dropout(layer, h):
    """``(p, key tensor, offset)`` for ops.block_layer / ops.towers_layer when the layer's F.dropout is active (training, 0 < p < 1), else
    None: these routes draw the keep bits inside their tail kernels -- the bits ops.dropout would draw for the same key and offset."""
    if layer.training and 0 < layer.dropout < 1:
        seed, offset = _next_dropout_key(h.device)
        return (float(layer.dropout), seed, offset)
    return None


def _next_dropout_key(device):
    """(key tensor, stream offset) of the next dropout call on ``device``; ``_dropout_key_used(key)`` after the kernels are enqueued."""
    st = _DROP_STATE.get(device)
    if st is None:
        if torch.cuda.is_current_stream_capturing():
            # (the key would be allocated from the capture's private pool and drawn by a captured randint: every replay the same key)
            raise RuntimeError("dgn_amd dropout: the first dropout call of a device must run outside a stream capture "
                               "(run one warm-up step, or call dgn_amd.dgn_layer.set_dropout_state(device, key, 0) first)")
        st = _DROP_STATE[device] = [torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=device), 0]
    st[1] += 1
    return st[0], st[1]


def _dropout_key_used(seed):
    if torch.cuda.is_current_stream_capturing():
        # inside a capture the call counter is frozen into the graph: the KEY moves instead, on the device, as part of the captured
        # work -- every replay draws new masks (tests/test_dropout_gpu.py::test_captured_dropout_draws_new_masks_per_replay)
        seed.add_(1)


def reset_dropout_state():
    """Forget the per-device Philox keys (the next dropout draws new ones from torch's generators: call after ``torch.manual_seed``
    to replay a run's masks).  The dropout masks are NOT part of torch's RNG state: ``torch.get_rng_state / set_rng_state`` do not
    cover them -- a checkpoint that must resume with the same masks saves ``get_dropout_state`` next to them."""
    _DROP_STATE.clear()


def get_dropout_state(device=None):
    """(key, calls so far) of ``device``'s dropout stream as Python ints, or None before its first dropout (one read-back).  With
    ``set_dropout_state`` this is what a checkpoint stores to resume with the masks the uninterrupted run would have drawn, and what
    ``torch.utils.checkpoint``-style recomputation restores before re-running a forward (F.dropout replays its mask there by itself)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    st = _DROP_STATE.get(dev)
    return None if st is None else (int(st[0].item()), int(st[1]))


def set_dropout_state(device, key: int, calls: int = 0):
    """Install a dropout stream: Philox key ``key`` and ``calls`` calls already made (the next mask is number ``calls + 1``)."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    _DROP_STATE[dev] = [torch.tensor([int(key)], dtype=torch.int64, device=dev), int(calls)]


class EdgeTypeFeatures:
    """Edge features that are an embedding lookup -- ``e = embedding_e(bond_type)`` in the reference's nets
    (nets/molecules_graph_regression/dgn_net.py:53,75) -- handed to the layers as (table, types) instead of the gathered [E, edge_dim]
    tensor: ``table`` [K, edge_dim] (e.g. ``embedding_e.weight``), ``types`` [E] integer edge types in the graph's edge order.  A layer
    whose pretrans is one affine map then adds row ``types[j]`` of the K x F table ``table W_e^T`` inside the sweep (the table lives in
    LDS): no [E, F] edge term is written or read, and the table's gradient is a reduction of the per-edge gradient rows the backward
    stages anyway.  Layers that cannot use the table (other pretrans depths, tables over ops.MAX_EDGE_TABLE floats) gather it."""

    def __init__(self, table: torch.Tensor, types: torch.Tensor, validate: bool = False):
        """``validate=True``: one host sync (two read-backs) checking every type against the table, the host-side twin of the device
        assert ``nn.Embedding`` raises in the reference -- for loaders / tests, ONCE per dataset.  Off by default: the nets build this
        object on every forward, the steps are launch-bound, and out-of-range types are CLAMPED by ``slot_types`` (memory-safe)."""
        if table.dim() != 2 or types.dim() != 1:
            raise ValueError("EdgeTypeFeatures: table [K, edge_dim], types [E]")
        self.table, self.types = table, types
        if validate and not (types.is_cuda and torch.cuda.is_current_stream_capturing()):
            self.validate()

    def dense(self) -> torch.Tensor:
        return self.table.index_select(0, self.types.long())

    def slot_types(self, graph: DGNGraph) -> torch.Tensor:
        """The types in CSR slot order, int32, CLAMPED to the table's rows (a type outside [0, K) would index outside the sweep's LDS
        table; ``nn.Embedding`` raises a device assert there, ``validate()`` is the host-side equivalent); cached per graph."""
        ent = graph.__dict__.get("_slot_types")
        K = int(self.table.shape[0])
        if ent is not None and ent[0] is self.types and ent[1] == self.types._version and ent[3] == K:
            return ent[2]
        t = graph.to_slot_order(self.types).clamp(0, K - 1).to(torch.int32).contiguous()
        graph.__dict__["_slot_types"] = (self.types, self.types._version, t, K)
        return t

    def validate(self) -> None:
        """Raise if a type lies outside the table (one host sync; what ``nn.Embedding`` would assert on the device)."""
        if self.types.numel() and (int(self.types.min()) < 0 or int(self.types.max()) >= self.table.shape[0]):
            raise IndexError(f"EdgeTypeFeatures: edge types must lie in [0, {self.table.shape[0]})")


def _edge_term(graph: DGNGraph, e, w_edge):
    """(m_edge, edge_type) of the pretrans Linear's edge-feature block: the [E, F] rows ef W_e^T in CSR slot order, or -- for
    EdgeTypeFeatures -- the [K, F] table and the slots' types."""
    if isinstance(e, EdgeTypeFeatures):
        Fm = w_edge.shape[0]
        if e.table.shape[0] * Fm <= _ops.MAX_EDGE_TABLE and _ops._two_phase_scatter(Fm) and not hasattr(graph, "_pad"):
            return F.linear(e.table, w_edge), e.slot_types(graph)
        e = e.dense()
    # the permuted copy is edge_dim floats per edge (40 B), the product runs on the streaming Linear kernels (k = edge_dim)
    return node_linear(graph.to_slot_order(e), w_edge), None


def _messages(pretrans: MLP, graph: DGNGraph, h, e, in_dim, edge_features, pad_to=None):
    """(x_pair, m_edge, edge_type) such that m_j = P[src_j] + Q[i] + m_edge[j] (or + m_edge[edge_type[j]]) with
    x_pair = P | Q [N, 2*in] equals pretrans([h_src || h_dst (|| ef)]) of dgn_layer.py:75-80.
    ``pad_to`` = Fp > in: ``h`` is [N, Fp] (zero columns appended) and the messages come out Fp wide with zero columns
    (zero weight rows / bias entries): an odd hidden size (ZINC json: 45, PATTERN json: 47) then runs the 8-byte-lane
    sweep and the two-phase scatter like an even one."""
    if pretrans.is_single_affine():
        lin = pretrans.fully_connected[0].linear
        W = lin.weight                                     # [in, 2*in (+edge_dim)]
        bias = lin.bias
        Fp = in_dim if pad_to is None else pad_to
        if Fp != in_dim:
            # rows in -> Fp (the padded message columns), columns in -> Fp (the padded input columns)
            w_sd = F.pad(torch.stack([W[:, :in_dim], W[:, in_dim:2 * in_dim]]), (0, Fp - in_dim, 0, Fp - in_dim)).reshape(2 * Fp, Fp)
            b_sd = None if bias is None else F.pad(bias, (Fp, Fp - in_dim))
            w_e = F.pad(W[:, 2 * in_dim:], (0, 0, 0, Fp - in_dim)) if edge_features else None
        else:
            w_sd = torch.cat([W[:, :in_dim], W[:, in_dim:2 * in_dim]], dim=0)   # [2*in, in]
            b_sd = None if bias is None else torch.cat([torch.zeros_like(bias), bias])
            w_e = W[:, 2 * in_dim:]
        pq = node_linear(h, w_sd, b_sd)                    # [N, 2*Fp]: P | Q
        m_edge, edge_type = _edge_term(graph, e, w_e) if edge_features else (None, None)
        return pq, m_edge, edge_type
    # general pretrans (ReLU between layers): materialise the messages, directly in slot order
    z = [h.index_select(0, graph.src.long()), h.index_select(0, _slot_dst(graph))]
    if edge_features:
        z.append(graph.to_slot_order(e.dense() if isinstance(e, EdgeTypeFeatures) else e))
    return None, pretrans(torch.cat(z, dim=1)), None


def _scale_table(graph: DGNGraph, kinds, avg_log: float) -> torch.Tensor:
    """[N, S] degree-scaler factors of scalers.py:7-18 (log in fp64 -> fp32, fp32 division)."""
    key = (tuple(kinds), float(avg_log))
    cache = graph.__dict__.setdefault("_scale_cache", {})
    if key not in cache:
        logd = graph.log_deg
        cols = []
        for k in kinds:
            if k == SCALE_IDENTITY:
                cols.append(torch.ones_like(logd))
            elif k == SCALE_AMPLIFICATION:
                cols.append(logd / avg_log)
            else:
                # zero in-degree rows aggregate to 0; keep avg/log(1) = inf out of 0 * inf
                cols.append(torch.where(graph.in_degree > 0, avg_log / logd, torch.zeros_like(logd)))
        cache[key] = torch.stack(cols, dim=1).contiguous()
    return cache[key]


def _identity_slot(applied_scalers):
    """Index of the identity scaler among the applied ones (None if absent): the h block of posttrans([h || agg])
    is not scaled, so in the folded form its weights live in the identity scaler's output block."""
    for i, k in enumerate(applied_scalers):
        if k == SCALE_IDENTITY:
            return i
    return None


def _folded_weight(w_agg, w_h, S, id_slot):
    """[fo, S*K] (scaler-major) and [fo, fi] -> [S*fo, K+fi] acting on [agg | h]: row block s holds W_s, and the
    h columns are W_h in the identity block, zero elsewhere."""
    fo = w_agg.shape[0]
    K = w_agg.shape[1] // S
    w = w_agg.reshape(fo, S, K).permute(1, 0, 2)                                     # [S, fo, K]
    hcols = torch.zeros(S, fo, w_h.shape[1], dtype=w_h.dtype, device=w_h.device)
    hcols = torch.cat([hcols[:id_slot], w_h.unsqueeze(0), hcols[id_slot + 1:]], dim=0)
    return torch.cat([w, hcols], dim=2).reshape(S * fo, K + w_h.shape[1])


def _pad_blocks(weight, n_blocks, F0, Fp):
    """[fo, n_blocks*F0] -> [fo, n_blocks*Fp]: a zero column after every F0-wide block (the padded feature)."""
    if Fp == F0:
        return weight
    fo = weight.shape[0]
    return F.pad(weight.reshape(fo, n_blocks, F0), (0, Fp - F0)).reshape(fo, n_blocks * Fp)


def _posttrans_split(posttrans: MLP, h, agg, in_dim):
    """posttrans(cat([h, agg])) without building the concat when posttrans is one Linear."""
    if posttrans.is_single_affine():
        lin = posttrans.fully_connected[0].linear
        return node_linear(agg, lin.weight[:, in_dim:]) + node_linear(h, lin.weight[:, :in_dim], lin.bias)
    return posttrans(torch.cat([h, agg], dim=1))


def _block_route_ok(layer, h) -> bool:
    """Conditions every layer type shares for the graph-block route: a training step with BatchNorm on CUDA fp32 rows (a padded batch
    takes it when its graph carries a static block table: DGNGraph.set_block_capacity)."""
    # (a training step -- or the evaluation loops' regime: eval() under no_grad; the two mixed forms keep the streaming kernels)
    return (_ops.BLOCK_LAYER_MAX_NODES > 0 and layer.training == torch.is_grad_enabled() and (layer.training or not h.requires_grad)
            and layer.batch_norm and h.is_cuda
            and h.dtype == torch.float32 and h.dim() == 2
            and 0 < h.shape[0] <= (_ops.BLOCK_LAYER_MAX_NODES if layer.training else max(_ops.BLOCK_LAYER_MAX_NODES, _ops.BLOCK_LAYER_EVAL_MAX_NODES))
            and all(_ops._bn_fusable(bn, layer.training) for bn in _bns_of(layer)))


def _bns_of(layer):
    return [t.batchnorm_h for t in layer.towers] if hasattr(layer, "towers") else [layer.batchnorm_h]


class _Layer(nn.Module):
    """``forward`` of the three layer types (registers nothing: the subclasses' state_dict is the reference's)."""

    def forward(self, g, h, e, snorm_n):
        # (a batch padded to a fixed row capacity carries its valid-row count as a device scalar: BatchNorm must know, ops.padded_rows)
        with _ops.padded_rows(getattr(g, "n_valid", None)):
            return self._forward(g, h, e, snorm_n)


class _SingleLayer(_Layer):
    """What DGNLayerSimple and DGNLayerComplex share: the order of the routes, the two fused routes (whose entry points take both layers
    as ``type`` 0 / 1) and the tail.  A subclass states ``_TYPE_NET``, ``_WHOLE_PLAN`` (the attribute holding the whole-layer call's sweep
    list), ``_fused_pretrans`` and its own message path, ``_per_op_forward``."""

    def _forward(self, g, h, e, snorm_n):
        y = self._block_layer(g, h, snorm_n)
        if y is not None:
            return y                                              # (dropout included)
        y = self._whole_layer(g, h, snorm_n)
        if y is not None:
            return _dropout(y, self.dropout, self.training)       # (nets/dgn_layer.py:130, :201: the layer's last op)
        return self._per_op_forward(g, h, e, snorm_n)

    def _whole_layer(self, g, h, snorm_n):
        """The layer through dgn_dense_layer_forward / _backward (one C call per direction), or None outside that entry point's domain
        (training-mode BatchNorm, single-affine posttrans, what ``_fused_pretrans`` adds, enough rows for this library's own GEMM
        kernels; the dropout follows the call)."""
        bn = self.batchnorm_h
        if not (_ops.WHOLE_LAYER and self.training and torch.is_grad_enabled() and self.batch_norm and h.is_cuda
                and h.dtype == torch.float32 and h.dim() == 2 and h.shape[0] >= _ops.WHOLE_LAYER_MIN_ROWS and self.posttrans.is_single_affine()
                and bn_tail_supported([bn], h, True, bn.num_features)):
            return None
        ok, pre, id_slot = self._fused_pretrans(False)
        if not ok:
            return None
        lin, plan = self.posttrans.fully_connected[0].linear, getattr(self, self._WHOLE_PLAN)
        S, A = self.plan.n_scalers, len(self.aggregators)
        if len(plan.launches) != 1 or not _ops.dense_layer_supported(self._TYPE_NET, h.shape[1], lin.weight.shape[0], S, A):
            return None
        eig = g.ndata["eig"]
        graph = as_dgn_graph(g, h.device)
        if _ops.split_training_route(graph, S):
            return None      # (hub rows: the per-op route runs posttrans per in-degree class + the folded product on the hubs alone)
        sc = _scale_table(graph, self.plan.applied_scalers, self._avg_log) if S > 1 else None
        return _ops.dense_layer(graph, plan, self._avg_log, graph.edge_weights(plan, eig), h, snorm_n if self.graph_norm else None, sc, bn,
                                None if pre is None else pre.weight, None if pre is None else pre.bias, lin.weight, lin.bias, self._TYPE_NET, A,
                                id_slot, self.residual)

    def _block_layer(self, g, h, snorm_n):
        """The layer on the graph-block route (ops.block_layer: batches at the reference's batch size), or None."""
        bn, lin = self.batchnorm_h, self.posttrans.fully_connected[0].linear
        if not (_block_route_ok(self, h) and self.posttrans.is_single_affine() and lin.bias is not None and 0 <= self.dropout < 1):
            return None
        ok, pre, _ = self._fused_pretrans(True)
        if not ok:
            return None
        graph = as_dgn_graph(g, h.device)
        if not _ops.block_layer_supported(graph, self.plan, self._TYPE_NET, 1, h.shape[1], lin.weight.shape[0], eval_only=not self.training):
            return None
        drop = _block_dropout(self, h)      # the layer's last op (nets/dgn_layer.py:130, :201) inside the route's tail kernels
        params = (lin.weight, lin.bias, bn.weight, bn.bias) if pre is None else (pre.weight, pre.bias, lin.weight, lin.bias, bn.weight, bn.bias)
        y = _ops.block_layer(graph, self.plan, self._avg_log, g.ndata["eig"], h, snorm_n if self.graph_norm else None, bn.running_mean, bn.running_var,
                             bn.num_batches_tracked, params, self._TYPE_NET, 1, h.shape[1], lin.weight.shape[0], self.residual, bn.momentum, bn.eps,
                             training=self.training, dropout=drop)
        if drop is not None:
            _dropout_key_used(drop[1])
        return y

    def _tail(self, h, h_in):
        """BatchNorm -> ReLU -> residual -> dropout (nets/dgn_layer.py:123-130, :194-201)."""
        if self.batch_norm:
            h = bn_tail(h, self.batchnorm_h, self.training, relu=True, residual=h_in if self.residual else None)
        else:
            h = F.relu(h)
            h = h_in + h if self.residual else h
        return _dropout(h, self.dropout, self.training)

    def _combine_and_tail(self, z, sc, bias, snorm_n, h_in):
        """scale_combine -> the tail; combine and BatchNorm -> ReLU -> residual are one autograd node in training."""
        row_scale = snorm_n if self.graph_norm else None
        bn = self.batchnorm_h
        width = z.shape[0] * (z.shape[2] // (sc.shape[1] if sc is not None else 1))
        if self.batch_norm and self.training and bn_tail_supported([bn], z, True, width):
            h = combine_bn_tail(z, sc, bias, row_scale, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                bn.momentum, bn.eps, relu=True, residual=h_in if self.residual else None)
            return _dropout(h, self.dropout, self.training)
        return self._tail(scale_combine(z, sc, bias, row_scale), h_in)


class DGNLayerSimple(_SingleLayer):
    """dgn_layer.py:135-202: message = h[src]; posttrans on the aggregation only."""
    _TYPE_NET, _WHOLE_PLAN = 0, "_kplan"

    def __init__(self, in_dim, out_dim, dropout, graph_norm, batch_norm, aggregators, scalers, residual, avg_d,
                 posttrans_layers=1):
        super().__init__()
        self.dropout, self.graph_norm, self.batch_norm, self.residual = dropout, graph_norm, batch_norm, residual
        self.aggregators, self.scalers = _names(aggregators), _names(scalers)
        self.plan = make_plan(self.aggregators, self.scalers)
        self._kplan = make_plan(self.aggregators, ["identity"])      # sweep without scalers (folded into posttrans)
        self.batchnorm_h = nn.BatchNorm1d(out_dim)
        self.posttrans = MLP(in_size=(len(self.aggregators) * len(self.scalers)) * in_dim, hidden_size=out_dim,
                             out_size=out_dim, layers=posttrans_layers, mid_activation="relu", last_activation="none")
        self.avg_d = avg_d
        self._avg_log = _avg_log(avg_d)
        if in_dim != out_dim:
            self.residual = False

    def aggregate(self, g, h, plan=None, eig=None):
        """``eig``: the caller's CURRENT ``g.ndata['eig']`` (read before any conversion of ``g``: a cached conversion
        must never supply a stale eig when the train loop reassigns it per batch)."""
        eig = g.ndata["eig"] if eig is None else eig
        graph = as_dgn_graph(g, h.device)
        return directional_aggregate(graph, plan or self.plan, self._avg_log, x_src=h, x_in=h, eig=eig)

    def _fused_pretrans(self, block_route):
        """(the fused routes take the layer, its pretrans Linear, id_slot of ops.dense_layer): no pretrans, nothing to ask."""
        return True, None, 0

    def _per_op_forward(self, g, h, e, snorm_n):
        h_in = h
        F0 = h.shape[1]
        # Odd widths (ZINC simple: 75, CIFAR10: 65) would run the sweep with 4-byte lanes, a second, nearly empty
        # feature tile and the atomic scatter.  One zero column keeps the 8-byte-lane kernels: the aggregates of a zero
        # column meet zero weights (the padded columns of W below), so the layer output is unchanged.
        hp = F.pad(h, (0, 1)) if F0 % 2 else h
        Fp = hp.shape[1]
        eig = g.ndata["eig"]
        if self.posttrans.is_single_affine():
            graph = as_dgn_graph(g, h.device)
            lin = self.posttrans.fully_connected[0].linear
            fo = lin.weight.shape[0]
            A = len(self.aggregators)
            if self.plan.n_scalers > 1:
                # scalers folded behind the Linear: sweep without scalers -> one GEMM -> scale-combine (+bias, +snorm)
                S = self.plan.n_scalers
                agg = self.aggregate(graph, hp, self._kplan, eig)                             # [N, A*Fp]
                if _ops.dc_posttrans_split_supported(graph, agg, fo, S):
                    # inference on a graph that may hold hub rows: one product per in-degree class, the hubs on the folded product
                    sc = _scale_table(graph, self.plan.applied_scalers, self._avg_log)
                    h = _ops.dc_posttrans_split(graph, agg, lin.weight, lin.bias, sc, snorm_n if self.graph_norm else None, A, F0)
                    del agg
                    return self._tail(h, h_in)
                w = _pad_blocks(lin.weight, S * A, F0, Fp).reshape(fo, S, A * Fp).permute(1, 0, 2).reshape(S * fo, A * Fp)
                z = node_linear(agg, w)
                sc = _scale_table(graph, self.plan.applied_scalers, self._avg_log)
                return self._combine_and_tail(z.unsqueeze(0), sc, lin.bias, snorm_n, h_in)     # (+snorm, BatchNorm, ReLU, residual, dropout)
            else:
                agg = self.aggregate(graph, hp, None, eig)                                    # [N, A*Fp] (single scaler: not applied)
                h = node_linear(agg, _pad_blocks(lin.weight, A, F0, Fp), lin.bias)
                if self.graph_norm:
                    h = h * snorm_n
        else:
            agg = self.aggregate(g, hp, None, eig)
            if Fp != F0:
                agg = agg.view(agg.shape[0], -1, Fp)[:, :, :F0].reshape(agg.shape[0], -1)
            h = self.posttrans(agg)
            if self.graph_norm:
                h = h * snorm_n
        return self._tail(h, h_in)


class DGNLayerComplex(_SingleLayer):
    """dgn_layer.py:52-132: message = pretrans([h_src || h_dst (|| ef)]); posttrans on [h || agg]."""
    _TYPE_NET, _WHOLE_PLAN = 1, "_kplan_x"

    def __init__(self, in_dim, out_dim, dropout, graph_norm, batch_norm, aggregators, scalers, avg_d, residual,
                 edge_features, edge_dim, pretrans_layers=1, posttrans_layers=1):
        super().__init__()
        self.dropout, self.graph_norm, self.batch_norm = dropout, graph_norm, batch_norm
        self.edge_features, self.residual, self.in_dim = edge_features, residual, in_dim
        self.aggregators, self.scalers = _names(aggregators), _names(scalers)
        self.plan = make_plan(self.aggregators, self.scalers)
        self._kplan = make_plan(self.aggregators, ["identity"])
        self._kplan_x = make_plan(self.aggregators + [X_IN_NAME], ["identity"])     # + h_in pass-through block
        self.batchnorm_h = nn.BatchNorm1d(out_dim)
        self.pretrans = MLP(in_size=2 * in_dim + (edge_dim if edge_features else 0), hidden_size=in_dim,
                            out_size=in_dim, layers=pretrans_layers, mid_activation="relu", last_activation="none")
        self.posttrans = MLP(in_size=(len(self.aggregators) * len(self.scalers) + 1) * in_dim, hidden_size=out_dim,
                             out_size=out_dim, layers=posttrans_layers, mid_activation="relu", last_activation="none")
        self.avg_d = avg_d
        self._avg_log = _avg_log(avg_d)
        if in_dim != out_dim:
            self.residual = False

    def aggregate(self, g, h, e, plan=None, eig=None, pad_to=None):
        eig = g.ndata["eig"] if eig is None else eig           # (the caller's current eig, see DGNLayerSimple.aggregate)
        graph = as_dgn_graph(g, h.device)
        x_pair, m_edge, edge_type = _messages(self.pretrans, graph, h, e, self.in_dim, self.edge_features, pad_to)
        return directional_aggregate(graph, plan or self.plan, self._avg_log, x_pair=x_pair, m_edge=m_edge,
                                     x_in=h, eig=eig, edge_type=edge_type)

    def _fused_pretrans(self, block_route):
        """What the fused routes ask of the message path: a single-affine pretrans without edge features; the graph-block route reads
        its bias, the whole-layer call needs the identity among the applied scalers (the slot the h block of posttrans acts through)."""
        pre = self.pretrans.fully_connected[0].linear
        id_slot = _identity_slot(self.plan.applied_scalers)
        ok = not self.edge_features and self.pretrans.is_single_affine() and (pre.bias is not None if block_route else id_slot is not None)
        return ok, pre, id_slot

    def _per_op_forward(self, g, h, e, snorm_n):
        h_in = h
        eig = g.ndata["eig"]
        id_slot = _identity_slot(self.plan.applied_scalers)
        if self.posttrans.is_single_affine() and self.plan.n_scalers > 1 and id_slot is not None:
            # sweep without scalers and WITH the h_in pass-through block -> posttrans([h || agg]) is one GEMM ->
            # scale-combine (+bias, +snorm)
            graph = as_dgn_graph(g, h.device)
            lin = self.posttrans.fully_connected[0].linear
            S, fo = self.plan.n_scalers, lin.weight.shape[0]
            F0 = self.in_dim
            w_agg, w_h = lin.weight[:, F0:], lin.weight[:, :F0]
            if F0 % 2 and self.pretrans.is_single_affine():
                # odd hidden size (ZINC json 45, PATTERN json 47): one zero feature column through the whole message path, met by
                # zero posttrans columns -- outputs and gradients unchanged, the sweep runs its 8-byte-lane kernels
                Fp = F0 + 1
                aggx = self.aggregate(graph, F.pad(h, (0, 1)), e, self._kplan_x, eig, pad_to=Fp)  # [N, A*Fp | Fp]
                w_agg, w_h = _pad_blocks(w_agg, S * len(self.aggregators), F0, Fp), F.pad(w_h, (0, 1))
            else:
                aggx = self.aggregate(graph, h, e, self._kplan_x, eig)                     # [N, A*F | F]
            if _ops.dc_posttrans_split_supported(graph, aggx, fo, S):
                # inference on a graph that may hold hub rows: one product per in-degree class, the hubs on the folded product
                sc = _scale_table(graph, self.plan.applied_scalers, self._avg_log)
                h = _ops.dc_posttrans_split(graph, aggx, lin.weight, lin.bias, sc, snorm_n if self.graph_norm else None, len(self.aggregators), F0,
                                            id_slot=id_slot)
                del aggx
                return self._tail(h, h_in)
            w = _folded_weight(w_agg, w_h, S, id_slot)
            z = node_linear(aggx, w)
            sc = _scale_table(graph, self.plan.applied_scalers, self._avg_log)
            return self._combine_and_tail(z.unsqueeze(0), sc, lin.bias, snorm_n, h_in)        # (+snorm, BatchNorm, ReLU, residual, dropout)
        h = _posttrans_split(self.posttrans, h, self.aggregate(g, h, e, None, eig), self.in_dim)
        if self.graph_norm:
            h = h * snorm_n
        return self._tail(h, h_in)


class DGNTower(nn.Module):
    """dgn_layer.py:205-276.  Holds one tower's parameters (same state_dict keys) and can run on
    its own; DGNLayerTower normally evaluates all towers in one fused sweep instead."""

    def __init__(self, in_dim, out_dim, dropout, graph_norm, batch_norm, aggregators, scalers, avg_d,
                 pretrans_layers, posttrans_layers, edge_features, edge_dim):
        super().__init__()
        self.dropout, self.graph_norm, self.batch_norm, self.edge_features = dropout, graph_norm, batch_norm, edge_features
        self.in_dim, self.out_dim = in_dim, out_dim
        self.aggregators, self.scalers = _names(aggregators), _names(scalers)
        self.plan = make_plan(self.aggregators, self.scalers)
        self.batchnorm_h = nn.BatchNorm1d(out_dim)
        self.pretrans = MLP(in_size=2 * in_dim + (edge_dim if edge_features else 0), hidden_size=in_dim,
                            out_size=in_dim, layers=pretrans_layers, mid_activation="relu", last_activation="none")
        self.posttrans = MLP(in_size=(len(self.aggregators) * len(self.scalers) + 1) * in_dim, hidden_size=out_dim,
                             out_size=out_dim, layers=posttrans_layers, mid_activation="relu", last_activation="none")
        self.avg_d = avg_d
        self._avg_log = _avg_log(avg_d)

    def forward(self, g, h, e, snorm_n):
        graph = as_dgn_graph(g, h.device)
        h = h.contiguous()
        x_pair, m_edge, edge_type = _messages(self.pretrans, graph, h, e, self.in_dim, self.edge_features)
        agg = directional_aggregate(graph, self.plan, self._avg_log, x_pair=x_pair, m_edge=m_edge, x_in=h,
                                    eig=g.ndata["eig"], edge_type=edge_type)
        h = _posttrans_split(self.posttrans, h, agg, self.in_dim)
        if self.graph_norm:
            h = h * snorm_n
        if self.batch_norm:
            h = self.batchnorm_h(h)
        return _dropout(h, self.dropout, self.training)


class DGNLayerTower(_Layer):
    """dgn_layer.py:279-325."""

    def __init__(self, in_dim, out_dim, aggregators, scalers, avg_d, dropout, graph_norm, batch_norm, towers=5,
                 pretrans_layers=1, posttrans_layers=1, divide_input=True, residual=False, edge_features=False,
                 edge_dim=0):
        super().__init__()
        assert ((not divide_input) or in_dim % towers == 0), "if divide_input is set the number of towers has to divide in_dim"
        assert (out_dim % towers == 0), "the number of towers has to divide the out_dim"
        assert avg_d is not None
        self.divide_input = divide_input
        self.input_tower = in_dim // towers if divide_input else in_dim
        self.output_tower = out_dim // towers
        self.in_dim, self.out_dim = in_dim, out_dim
        self.edge_features, self.residual = edge_features, residual
        self.dropout, self.graph_norm, self.batch_norm = dropout, graph_norm, batch_norm
        if in_dim != out_dim:
            self.residual = False
        self.towers = nn.ModuleList()
        for _ in range(towers):
            self.towers.append(DGNTower(in_dim=self.input_tower, out_dim=self.output_tower, aggregators=aggregators,
                                        scalers=scalers, avg_d=avg_d, pretrans_layers=pretrans_layers,
                                        posttrans_layers=posttrans_layers, batch_norm=batch_norm, dropout=dropout,
                                        graph_norm=graph_norm, edge_features=edge_features, edge_dim=edge_dim))
        self.mixing_network = FCLayer(out_dim, out_dim, activation="LeakyReLU")
        self.plan = self.towers[0].plan
        self._kplan = make_plan(self.plan.aggregators, ["identity"])
        self._kplan_x = make_plan(list(self.plan.aggregators) + [X_IN_NAME], ["identity"])
        self._avg_log = _avg_log(avg_d)

    def _fusable(self) -> bool:
        t0 = self.towers[0]
        return t0.pretrans.is_single_affine() and t0.posttrans.is_single_affine()

    # ---- fused operands -----------------------------------------------------------------------------------------
    # The per-tower parameters keep the reference's state_dict layout.  The operands of the fused layer are
    # re-arrangements of them (block diagonals, scaler-major permutations, zero blocks):
    #   w_sd [2Fm, Fm]   P | Q weights, block diagonal with divide_input       bias_sd [2Fm]   0 | pretrans biases
    #   w_edge [Fm, ed]  edge-feature part of the pretrans weights             b_p [T*fo]      posttrans biases
    #   w [T, S*fo, K+fi] posttrans weights acting on [agg | h_in] (identity slot), or w_a [T, S*fo, K] and w_h [T, fo, fi]
    def _param_list(self):
        """The towers' parameters in assembly order.  Cached (module attribute look-ups are ~1 us each and there are a
        hundred of them per call: at batch 128 the step is host-bound); re-read when a Parameter object was replaced."""
        cached = self.__dict__.get("_plist")
        t0, t1 = self.towers[0], self.towers[-1]
        if (cached is not None and cached[0] is t0.pretrans.fully_connected[0].linear.weight
                and cached[-1] is t1.batchnorm_h.bias and cached[-4] is t1.posttrans.fully_connected[0].linear.weight):
            return cached
        out = []
        for t in self.towers:
            pre, post = t.pretrans.fully_connected[0].linear, t.posttrans.fully_connected[0].linear
            out += [pre.weight, pre.bias, post.weight, post.bias, t.batchnorm_h.weight, t.batchnorm_h.bias]
        self.__dict__["_plist"] = out
        return out

    def _linked_bn_stats(self, dev):
        """(running_mean [T*fo], running_var [T*fo], num_batches_tracked [T]) as single tensors that the per-tower
        BatchNorm modules VIEW: the tail kernels update the statistics of all towers in place, the state_dict keeps
        the reference's per-tower keys, and nothing is concatenated or scattered per step.  Re-linked whenever the
        modules' buffers were replaced (``.to()``, ``deepcopy``, ...)."""
        bns = [t.batchnorm_h for t in self.towers]
        fo = self.output_tower
        link = self.__dict__.get("_bn_link")
        if link is not None and link[0].device == dev and all(
                b.running_mean.data_ptr() == link[0].data_ptr() + 4 * i * fo and b.running_var.data_ptr() == link[1].data_ptr() + 4 * i * fo
                and b.num_batches_tracked.data_ptr() == link[2].data_ptr() + 8 * i for i, b in enumerate(bns)):
            return link
        with torch.no_grad():
            rm = torch.cat([b.running_mean.reshape(-1) for b in bns]).to(dev)
            rv = torch.cat([b.running_var.reshape(-1) for b in bns]).to(dev)
            nbt = torch.stack([b.num_batches_tracked.reshape(()) for b in bns]).to(dev)
            for i, b in enumerate(bns):
                b.running_mean, b.running_var = rm[i * fo:(i + 1) * fo], rv[i * fo:(i + 1) * fo]
                b.num_batches_tracked = nbt[i]
        self.__dict__["_bn_link"] = (rm, rv, nbt)
        return self.__dict__["_bn_link"]

    def _assemble(self, plist):
        """Operands from the parameter list with plain tensor ops (stack / indexed assignment / cat): the definition
        of the layout.  Also run ONCE on tensors of element ids to derive the index map of the fast path."""
        T, fi, fo = len(self.towers), self.input_tower, self.output_tower
        w_pre, b_pre = torch.stack(plist[0::6]), torch.stack(plist[1::6])                      # [T, fi, 2fi(+ed)], [T, fi]
        w_post, b_post = torch.stack(plist[2::6]), torch.stack(plist[3::6])                    # [T, fo, fi + S*K], [T, fo]
        dev, dt = w_pre.device, w_pre.dtype
        Fm = T * fi
        ops = {}
        if self.divide_input:
            idx = torch.arange(T, device=dev)
            bd = torch.zeros(2, T, fi, T, fi, dtype=dt, device=dev)                            # block diagonals of W_s, W_d
            bd[:, idx, :, idx, :] = torch.stack([w_pre[:, :, :fi], w_pre[:, :, fi:2 * fi]], dim=1)
            ops["w_sd"] = bd.view(2 * Fm, Fm)
        else:
            ops["w_sd"] = torch.cat([w_pre[:, :, :fi].reshape(Fm, fi), w_pre[:, :, fi:2 * fi].reshape(Fm, fi)], dim=0)
        ops["bias_sd"] = torch.cat([torch.zeros(Fm, dtype=dt, device=dev), b_pre.reshape(Fm)])
        if self.edge_features:
            ops["w_edge"] = w_pre[:, :, 2 * fi:].reshape(Fm, -1)
        ops["b_p"] = b_post.reshape(T * fo)
        ops["bn_gamma"], ops["bn_beta"] = torch.cat(plist[4::6]), torch.cat(plist[5::6])       # the towers' BatchNorms, channel-concatenated
        S = self.plan.n_scalers
        K = (w_post.shape[2] - fi) // S
        w_h = w_post[:, :, :fi]                                                                # [T, fo, fi]
        w_a = w_post[:, :, fi:].reshape(T, fo, S, K).permute(0, 2, 1, 3)                       # [T, S, fo, K]
        id_slot = _identity_slot(self.plan.applied_scalers)
        if id_slot is not None:
            hcols = torch.zeros(T, S, fo, fi, dtype=dt, device=dev)
            hcols[:, id_slot] = w_h                                                            # h block: identity scaler only
            ops["w"] = torch.cat([w_a, hcols], dim=3).reshape(T, S * fo, K + fi)
        else:
            ops["w_a"] = w_a.reshape(T, S * fo, K)
            ops["w_h"] = w_h.contiguous()
        return ops

    def _operands(self, dev):
        """The operands through ONE gather/scatter pair instead of ~15 small kernels (and as many backward nodes): all
        parameters are concatenated into a flat vector and scattered into one zero-initialised buffer by a precomputed
        index map; the operands are views of that buffer.  At batch 128 the layer is launch-bound: the assembly cost
        as much as the sweep itself.  The map is derived by running _assemble on element ids, so the layout has a
        single definition."""
        plist = self._param_list()
        key = (dev, id(plist), plist[0].shape, plist[2].shape)
        cache = self.__dict__.setdefault("_opmap", {})
        if key not in cache:
            with torch.no_grad():
                sizes = [p.numel() for p in plist]
                ids = torch.arange(1, sum(sizes) + 1, dtype=torch.float64, device=dev).split(sizes)
                id_ops = self._assemble([i.view(p.shape) for i, p in zip(ids, plist)])
                names = list(id_ops)
                flat_ids = torch.cat([id_ops[k].reshape(-1) for k in names])
                pos = torch.nonzero(flat_ids).flatten()
                sel = (flat_ids[pos] - 1).long()
                shapes = [tuple(id_ops[k].shape) for k in names]
                native = None
                n_flat = sum(sizes)
                if dev.type == "cuda" and sel.numel() == n_flat and all(p.dtype == torch.float32 and p.is_contiguous() for p in plist):
                    # every parameter element lands exactly once: the assembly is ONE gather kernel over a table of the
                    # parameters' addresses (ops.assemble_operands), its backward one index_select
                    starts = torch.zeros(len(sizes) + 1, dtype=torch.long, device=dev)
                    starts[1:] = torch.cumsum(torch.tensor(sizes, device=dev), 0)
                    gid = (flat_ids - 1).long()                                            # -1 where the operand is a structural zero
                    which = torch.bucketize(gid.clamp(min=0), starts[1:], right=True)
                    map_param = torch.where(gid >= 0, which, torch.full_like(which, -1)).int()
                    map_off = torch.where(gid >= 0, gid - starts[which], torch.zeros_like(gid)).int()
                    inv = torch.empty(n_flat, dtype=torch.long, device=dev)
                    inv[sel] = pos
                    native = dict(ptr_table=torch.zeros(len(plist), dtype=torch.int64, device=dev), ptr_host=None, map_param=map_param,
                                  map_off=map_off, inv=inv, total=flat_ids.numel(), sizes=sizes, shapes=[tuple(p.shape) for p in plist])
                cache[key] = (names, shapes, pos, sel, flat_ids.numel(), [math.prod(shp) for shp in shapes], native)
        names, shapes, pos, sel, total, sizes, native = cache[key]
        if native is not None and all(p.is_cuda and p.is_contiguous() for p in plist):
            native.setdefault("op_sizes", sizes)
            native.setdefault("op_shapes", shapes)
            return dict(zip(names, _ops.assemble_operands(native, plist)))
        else:
            flat = torch.cat([p.reshape(-1) for p in plist])
            fused = flat.new_zeros(total).index_put((pos,), flat.index_select(0, sel))
        # (split, not slicing: its backward is ONE concatenation instead of a zero-fill + copy + add per operand)
        return {k: part.view(shp) for k, part, shp in zip(names, fused.split(sizes), shapes)}

    def _fused_towers(self, g, h, e, snorm_n):
        """All towers in one sweep: towers are column blocks of the message."""
        graph = as_dgn_graph(g, h.device)
        T, fi, fo = len(self.towers), self.input_tower, self.output_tower
        ops = self._operands(h.device)
        x_in = h if self.divide_input else h.repeat(1, T)                                          # (else every tower reads all of h)
        if self.divide_input and _ops.pair_linear_supported(h, T, fi):
            pq = _ops.pair_linear(h, ops["w_sd"], ops["bias_sd"], T, fi)                           # (the towers' diagonal blocks only)
        else:
            pq = node_linear(h, ops["w_sd"], ops["bias_sd"])                                        # [N, 2*Fm]: P | Q
        m_edge, edge_type = _edge_term(graph, e, ops["w_edge"]) if self.edge_features else (None, None)      # R = ef W_e^T, slot order
        b_p = ops["b_p"]
        S = self.plan.n_scalers
        N = h.shape[0]
        row_scale = snorm_n if self.graph_norm else None
        if "w" in ops:
            # The sweep runs WITHOUT scalers (per-row factors, folded behind the GEMM) and WITH the h_in
            # pass-through block, tower-major: posttrans([h_t || agg_t]) of all towers is ONE batched GEMM on
            # contiguous matrices, then one scale-combine kernel (+bias, +snorm) writes [N, T*fo].
            sc = _scale_table(graph, self.plan.applied_scalers, self._avg_log) if S > 1 else None
            needs_grad = torch.is_grad_enabled() and (h.requires_grad or any(q.requires_grad for q in self.parameters()))
            if (_ops.FUSED_FORWARD and not needs_grad and m_edge is None and h.is_cuda and self.divide_input
                    and _ops.fused_sweep_posttrans_supported(graph, self._kplan_x, T, x_in.shape[1], S, fo)):
                # inference: sweep + posttrans + scale-combine in ONE kernel, the aggregate rows stay in LDS
                w_edge = graph.edge_weights(self._kplan_x, g.ndata["eig"])
                y = _ops.fused_sweep_posttrans_forward(graph, self._kplan_x, T, self._avg_log, w_edge, pq, x_in.contiguous(), ops["w"], sc, b_p,
                                                       row_scale)
                return self._towers_tail(y, ops)
            aggx = directional_aggregate(graph, self._kplan_x, self._avg_log, x_pair=pq, m_edge=m_edge, x_in=x_in,
                                         eig=g.ndata["eig"], n_towers=T, tower_major=True, edge_type=edge_type)
            bns = [t.batchnorm_h for t in self.towers]
            fused_tail = self.batch_norm and self.training and bn_tail_supported(bns, aggx, True, T * fo)
            if fused_tail and linear_combine_supported(aggx, ops["w"], S):
                rm, rv, nbt = self._linked_bn_stats(aggx.device)                                   # posttrans + combine + BatchNorm: one autograd node
                y = linear_combine_bn_tail(aggx, ops["w"], sc, b_p, row_scale, ops["bn_gamma"], ops["bn_beta"], rm, rv, nbt,
                                           bns[0].momentum, bns[0].eps)
                return _dropout(y, self.dropout, self.training)
            z = node_linear(aggx, ops["w"])                                                        # [T, N, S*fo]
            if fused_tail:
                rm, rv, nbt = self._linked_bn_stats(z.device)                                      # combine + BatchNorm: one autograd node
                y = combine_bn_tail(z, sc, b_p, row_scale, ops["bn_gamma"], ops["bn_beta"], rm, rv, nbt, bns[0].momentum, bns[0].eps)
                return _dropout(y, self.dropout, self.training)
            y = scale_combine(z, sc, b_p, row_scale)                                               # [N, T*fo]
        else:
            agg = directional_aggregate(graph, self._kplan, self._avg_log, x_pair=pq, m_edge=m_edge,
                                        x_in=x_in, eig=g.ndata["eig"], n_towers=T, tower_major=True, edge_type=edge_type)   # [T, N, A*fi]
            z = node_linear(agg, ops["w_a"])                                                       # [T, N, S*fo]
            sc = _scale_table(graph, self.plan.applied_scalers, self._avg_log)
            y = scale_combine(z, sc, b_p, None)
            y = y + torch.bmm(x_in.view(N, T, fi).transpose(0, 1), ops["w_h"].transpose(1, 2)).transpose(0, 1).reshape(N, T * fo)
            if row_scale is not None:
                y = y * row_scale
        return self._towers_tail(y, ops)

    def _towers_tail(self, y, ops):
        """The towers' BatchNorms (channel-concatenated: one BatchNorm of width T * fo) and dropout on y [N, T * fo] (:272-275)."""
        if self.batch_norm:
            bns = [t.batchnorm_h for t in self.towers]
            if bn_tail_supported(bns, y, self.training):
                rm, rv, nbt = self._linked_bn_stats(y.device)
                y = bn_tail_fused(y, ops["bn_gamma"], ops["bn_beta"], rm, rv, nbt, bns[0].momentum, bns[0].eps, self.training)
            else:
                y = bn_tail(y, bns, self.training)
        return _dropout(y, self.dropout, self.training)

    def _whole_layer(self, g, h, snorm_n):
        """The layer through dgn_towers_layer_forward / _backward (one C call per direction), or None when the configuration
        is outside that entry point's domain: training-mode BatchNorm, mixing network Linear -> LeakyReLU, no edge features,
        identity among the scalers, widths the streaming Linear kernels take.  The towers' dropout (:275) rides in the call (the
        normalised rows are then materialised and masked in place)."""
        T, fi, fo = len(self.towers), self.input_tower, self.output_tower
        if not (_ops.WHOLE_LAYER and self.training and torch.is_grad_enabled() and self.batch_norm and T > 1 and self.divide_input
                and not self.edge_features and 0 <= self.dropout < 1 and h.is_cuda and h.dtype == torch.float32 and h.dim() == 2
                and _identity_slot(self.plan.applied_scalers) is not None and self._fusable()
                and towers_layer_supported(T, fi, fo, self.plan.n_scalers, self._kplan_x.n_agg)):
            return None
        act = self.mixing_network._fused_act()
        bns = [t.batchnorm_h for t in self.towers]
        if act is None or act[0] != "leaky_relu" or self.mixing_network.linear.bias is None or not bn_tail_supported(bns, h, True, T * fo):
            return None
        eig = g.ndata["eig"]
        graph = as_dgn_graph(g, h.device)
        ops = self._operands(h.device)
        S = self.plan.n_scalers
        sc = _scale_table(graph, self.plan.applied_scalers, self._avg_log) if S > 1 else None
        rm, rv, nbt = self._linked_bn_stats(h.device)
        w_edge = graph.edge_weights(self._kplan_x, eig)
        mix = self.mixing_network.linear
        drop = _block_dropout(self, h)
        y = towers_layer(graph, self._kplan_x, self._avg_log, w_edge, h, snorm_n if self.graph_norm else None, sc, rm, rv, nbt,
                         ops["w_sd"], ops["bias_sd"], ops["w"], ops["b_p"], ops["bn_gamma"], ops["bn_beta"], mix.weight, mix.bias,
                         T, fi, fo, self.residual, bns[0].momentum, bns[0].eps, act[1], dropout=drop,
                         id_slot=_identity_slot(self.plan.applied_scalers))
        if drop is not None:
            _dropout_key_used(drop[1])
        return y

    def _block_layer(self, g, h, snorm_n):
        """The layer on the graph-block route (ops.block_layer), or None: as _whole_layer's domain, per-tower parameters as they are."""
        T, fi, fo = len(self.towers), self.input_tower, self.output_tower
        if not (_block_route_ok(self, h) and T > 1 and T <= 8 and self.divide_input and not self.edge_features and 0 <= self.dropout < 1
                and self._fusable()):
            return None
        act = self.mixing_network._fused_act()
        mix = self.mixing_network.linear
        if act is None or act[0] != "leaky_relu" or mix.bias is None:
            return None
        plist = self._param_list()
        if any(p is None for p in plist):
            return None
        graph = as_dgn_graph(g, h.device)
        if not _ops.block_layer_supported(graph, self.plan, 2, T, fi, fo, eval_only=not self.training):
            return None
        bns = [t.batchnorm_h for t in self.towers]
        rm, rv, nbt = self._linked_bn_stats(h.device)
        drop = _block_dropout(self, h)      # the towers' F.dropout (:275) inside the route's tail kernels (round 6)
        y = _ops.block_layer(graph, self.plan, self._avg_log, g.ndata["eig"], h, snorm_n if self.graph_norm else None, rm, rv, nbt,
                             (*plist, mix.weight, mix.bias), 2, T, fi, fo, self.residual, bns[0].momentum, bns[0].eps, act[1], training=self.training,
                             dropout=drop)
        if drop is not None:
            _dropout_key_used(drop[1])
        return y

    def _forward(self, g, h, e, snorm_n):
        h_in = h
        y = self._block_layer(g, h, snorm_n)
        if y is None:
            y = self._whole_layer(g, h, snorm_n)
        if y is not None:
            return y
        if self._fusable():
            h_cat = self._fused_towers(g, h, e, snorm_n)
        elif self.divide_input:
            h_cat = torch.cat([tower(g, h[:, n * self.input_tower:(n + 1) * self.input_tower], e, snorm_n)
                               for n, tower in enumerate(self.towers)], dim=1)
        else:
            h_cat = torch.cat([tower(g, h, e, snorm_n) for tower in self.towers], dim=1)
        if len(self.towers) > 1:
            return self.mixing_network(h_cat, residual=h_in if self.residual else None)       # Linear -> LeakyReLU (+ h_in): one tail kernel
        return h_in + h_cat if self.residual else h_cat


class DGNLayer(nn.Module):
    """Factory with the reference's signature (dgn_layer.py:328-352); use ``.model``."""

    def __init__(self, in_dim, out_dim, dropout, graph_norm, batch_norm, aggregators, scalers, avg_d, type_net,
                 residual, towers=5, divide_input=True, edge_features=None, edge_dim=None, pretrans_layers=1,
                 posttrans_layers=1):
        super().__init__()
        aggregators = [AGGREGATORS[aggr] for aggr in aggregators.split()]
        scalers = [SCALERS[scale] for scale in scalers.split()]
        if type_net == "simple":
            self.model = DGNLayerSimple(in_dim=in_dim, out_dim=out_dim, dropout=dropout, graph_norm=graph_norm,
                                        batch_norm=batch_norm, residual=residual, aggregators=aggregators,
                                        scalers=scalers, avg_d=avg_d, posttrans_layers=posttrans_layers)
        elif type_net == "complex":
            self.model = DGNLayerComplex(in_dim=in_dim, out_dim=out_dim, dropout=dropout, graph_norm=graph_norm,
                                         batch_norm=batch_norm, aggregators=aggregators, residual=residual,
                                         scalers=scalers, avg_d=avg_d, edge_features=edge_features, edge_dim=edge_dim,
                                         pretrans_layers=pretrans_layers, posttrans_layers=posttrans_layers)
        elif type_net == "towers":
            self.model = DGNLayerTower(in_dim=in_dim, out_dim=out_dim, aggregators=aggregators, scalers=scalers,
                                       avg_d=avg_d, dropout=dropout, graph_norm=graph_norm, batch_norm=batch_norm,
                                       towers=towers, pretrans_layers=pretrans_layers,
                                       posttrans_layers=posttrans_layers, divide_input=divide_input, residual=residual,
                                       edge_features=edge_features, edge_dim=edge_dim)
