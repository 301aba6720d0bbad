"""HIP-graph capture of a launch-bound training step.

At the reference's batch size (128 molecules, ~3 000 nodes) a DGN layer step is ~80 kernel launches around 0.3-0.4 ms
of GPU work: the host, not the GPU, sets the pace.  Every launch of this package goes to the caller's stream with no
host synchronisation (the C ABI's contract), so a whole step -- edge weights, forward, backward -- can be captured
once into a HIP graph (``torch.cuda.CUDAGraph`` is hipGraph on ROCm) and replayed with one launch.  Valid only while
the batch SHAPE is fixed: the graph freezes every kernel argument (pointers, sizes, the CSR of the batch).

Training batches differ in node and edge count from step to step.  ``PaddedBatch`` holds a batch at a fixed CAPACITY in static
device buffers (``DGNGraph.padded`` + ``rebuild``: the CSR, its transposed view, eig, a device scalar with the number of real
rows), so ONE captured graph per capacity bucket serves every batch that fits: rows beyond the batch are isolated zero rows that
the sweep, the Linears and the elementwise kernels process like any other, and BatchNorm -- the only place where they would
matter -- reads the valid-row count from the device (``ops.padded_rows``).  Per step the host then does: ``load`` (two C calls
that rebuild the graph in place + small copies) and one graph launch.  Contract for the captured step function: it reads its
inputs from the batch's buffers, starts with ``batch.graph.invalidate_caches()`` (so that edge weights and scaler tables are
recomputed inside the captured region) and the cotangent rows of the padding must be zero.
"""
from __future__ import annotations

from typing import TYPE_CHECKING, Callable, Dict, Optional, Tuple

import torch

if TYPE_CHECKING:
    from .eig import EigAugment


def capture(step: Callable[[], None], warmup: int = 3) -> torch.cuda.CUDAGraph:
    """Run ``step`` ``warmup`` times on a side stream (allocator pools, per-graph caches such as the csc view and the
    scaler tables), then capture one more call.  ``step`` must not synchronise and must leave ``.grad`` fields to the
    backward (set them to None before calling this: the captured backward then writes fresh gradient tensors from
    the graph's private pool on every replay instead of accumulating).  Do not keep autograd-attached outputs of
    EARLIER steps alive across the capture (keep ``y.detach()``): releasing such a graph inside the capture region
    crashes ``capture_end`` on this ROCm / PyTorch."""
    import gc
    gc.collect()                      # autograd graphs of earlier eager steps that only a reference cycle keeps alive (e.g. a graph
    torch.cuda.synchronize()          # object whose ndata holds the features computed ON it) must not be released inside the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            step()
    torch.cuda.current_stream().wait_stream(side)
    gc.collect()
    graph = torch.cuda.CUDAGraph()
    was_enabled = gc.isenabled()
    gc.disable()                      # (no collection in the middle of the capture region either)
    try:
        with torch.cuda.graph(graph):
            step()
    finally:
        if was_enabled:
            gc.enable()
    return graph


class PaddedBatch:
    """Static buffers for one capacity bucket: the padded graph plus named per-node / per-edge tensors (features, graph norm,
    cotangent ...) whose rows beyond the loaded batch are kept at zero."""

    def __init__(self, n_cap: int, e_cap: int, device, eig_dim: int):
        from .graph import DGNGraph
        self.n_cap, self.e_cap, self.device = int(n_cap), int(e_cap), torch.device(device)
        self.graph = DGNGraph.padded(n_cap, e_cap, device, eig_dim=eig_dim)
        self.node: Dict[str, torch.Tensor] = {}
        self.edge: Dict[str, torch.Tensor] = {}

    def add_node_tensor(self, name: str, width: int, requires_grad: bool = False) -> torch.Tensor:
        t = torch.zeros(self.n_cap, width, dtype=torch.float32, device=self.device)
        self.node[name] = t.requires_grad_(requires_grad)
        return self.node[name]

    def add_edge_tensor(self, name: str, width: int, requires_grad: bool = False) -> torch.Tensor:
        t = torch.zeros(self.e_cap, width, dtype=torch.float32, device=self.device)
        self.edge[name] = t.requires_grad_(requires_grad)
        return self.edge[name]

    def fits(self, num_nodes: int, num_edges: int) -> bool:
        return num_nodes <= self.n_cap and num_edges <= self.e_cap

    @torch.no_grad()
    def load(self, src: torch.Tensor, dst: torch.Tensor, num_nodes: int, eig: Optional[torch.Tensor] = None, node: Optional[dict] = None,
             edge: Optional[dict] = None, graph_sizes=None) -> None:
        """Rebuild the graph in place and copy the batch's tensors into the static buffers (rows beyond the batch zeroed)."""
        self.graph.rebuild(src, dst, num_nodes, eig, graph_sizes=graph_sizes)      # (graph_sizes: required once set_block_capacity was called)
        for name, val in (node or {}).items():
            buf = self.node[name]
            buf[:num_nodes].copy_(val, non_blocking=True)
            buf[num_nodes:].zero_()
        E = src.numel()
        for name, val in (edge or {}).items():
            buf = self.edge[name]
            buf[:E].copy_(val, non_blocking=True)
            buf[E:].zero_()


def bucket_capacity(num_nodes: int, num_edges: int, granularity: int = 256, headroom: float = 1.1) -> Tuple[int, int]:
    """Capacity bucket of a batch: sizes with ``headroom`` rounded up to multiples of ``granularity`` (one captured graph per
    distinct pair; batches of a data loader with a fixed number of graphs fall into very few buckets)."""
    up = lambda v: int(-(-int(v * headroom) // granularity) * granularity)
    return up(num_nodes), up(num_edges)


def rewrap_parameters(module: torch.nn.Module) -> None:
    """Replace every Parameter of ``module`` by a NEW Parameter object on the same storage.  A parameter that took part in an eager
    autograd pass on the DEFAULT stream keeps a gradient-accumulation node bound to that stream for the life of the Parameter object,
    and a later capture of a backward pass through it crashes in ``capture_end`` (ROCm 7 / PyTorch 2.10: measured, tools-free repro
    in tests/test_net_gpu.py).  New Parameter objects start clean; values, ``state_dict`` and storage are untouched, but optimizers and
    other holders of the OLD Parameter objects must be re-created.  The layers' parameter-list caches are dropped too."""
    for m in module.modules():
        for k, q in list(m._parameters.items()):
            if q is not None:
                m._parameters[k] = torch.nn.Parameter(q.detach(), requires_grad=q.requires_grad)
        m.__dict__.pop("_plist", None)
        m.__dict__.pop("_opmap", None)


class _CapturedStep:
    """What the captured steps share: the device, the refusal of nets the static buffers cannot hold, the ``PaddedBatch`` with the graph
    norm buffer, the loss scalar, the optimizer and the capture / replay of ``_step`` (the subclass's: one whole training step that reads
    the static buffers and leaves the loss in ``self.loss``)."""

    _REFUSED = ()      # (test of the net, the ValueError's text) pairs, in the order they are checked

    def __init__(self, net, n_cap: int, e_cap: int, eig_dim: int, device=None, augment: Optional["EigAugment"] = None):
        dev = torch.device(device if device is not None else next(net.parameters()).device)
        for refused, why in self._REFUSED:
            if refused(net):
                raise ValueError(why)
        self.net, self.device = net, dev
        self.pb = PaddedBatch(n_cap, e_cap, dev, eig_dim)
        self.snorm = self.pb.add_node_tensor("snorm", 1)
        # eigenvector augmentation (``dgn_amd.EigAugment``): the loads write the batch's eig into ``eig_src`` and the step's first launch
        # draws the augmented ``ndata['eig']`` from it -- new values on every replay; ``pos_enc`` stays as loaded, as in the reference's loops
        self.augment, self.eig_src = augment, None
        if augment is not None:
            from .eig import EigAugment
            if not isinstance(augment, EigAugment):
                raise TypeError(f"{type(self).__name__}: augment must be a dgn_amd.EigAugment, got {type(augment).__name__}")
            if not 1 <= eig_dim <= 32 or (augment.rotate_deg != 0 and eig_dim < 3):
                raise ValueError(f"{type(self).__name__}: augment takes 1 <= eig_dim <= 32, and >= 3 with a rotation (it turns columns 1 and 2); "
                                 f"eig_dim = {eig_dim}")
            if augment.device != self.pb.graph.ndata["eig"].device:
                raise ValueError(f"{type(self).__name__}: the EigAugment lives on {augment.device}, the step on {self.pb.graph.ndata['eig'].device}")
            self.eig_src = torch.zeros(n_cap, eig_dim, dtype=torch.float32, device=dev)
        # positional encodings: a static [n_cap, K] buffer the net reads from the graph's ndata (rows behind the batch stay zero)
        self.pos_enc_dim = int(getattr(net, "pos_enc_dim", 0) or 0)
        if self.pos_enc_dim > 0:
            self.pb.graph.ndata["pos_enc"] = self.pb.add_node_tensor("pos_enc", self.pos_enc_dim)
        self.loss = torch.zeros((), device=dev)
        self.graph: Optional[torch.cuda.CUDAGraph] = None

    def _node_tensors(self, snorm, pos_enc, who: str) -> dict:
        """What ``PaddedBatch.load`` copies per node; a net with positional encodings needs ``pos_enc [num_nodes, K]`` and no other takes one."""
        if (pos_enc is not None) != (self.pos_enc_dim > 0):
            raise ValueError(f"{who}.load: the net has pos_enc_dim = {self.pos_enc_dim}: " +
                             ("pass pos_enc [num_nodes, pos_enc_dim]" if pos_enc is None else "it takes no pos_enc"))
        if pos_enc is None:
            return {"snorm": snorm}
        if pos_enc.dim() != 2 or pos_enc.shape[1] != self.pos_enc_dim:
            raise ValueError(f"{who}.load: pos_enc must be [num_nodes, {self.pos_enc_dim}], got {tuple(pos_enc.shape)}")
        return {"snorm": snorm, "pos_enc": pos_enc}

    def _load_eig(self, eig, num_nodes: int):
        """The ``eig`` argument of ``PaddedBatch.load``: the batch's own without an ``augment``; with one the batch's eig goes to ``eig_src``
        (zero behind the batch) and the graph's buffer is left to the step's first launch."""
        if self.augment is None:
            return eig
        num_nodes = int(num_nodes)
        self.eig_src[:num_nodes].copy_(eig, non_blocking=True)
        self.eig_src[num_nodes:].zero_()
        return None

    def _augment(self) -> None:
        """The first launch of a step with an ``augment``: ``ndata['eig']`` drawn from ``eig_src`` (the reference's loops replace
        ``batch_graphs.ndata['eig']`` ahead of ``model.forward``; the layers and the directional readouts read it from there)."""
        if self.augment is not None:
            self.augment(self.eig_src, out=self.pb.graph.ndata["eig"])

    def _set_optimizer(self, optimizer, lr: float) -> None:
        """The last act of a constructor (a refused construction leaves the net's Parameter objects alone)."""
        if optimizer is None:
            rewrap_parameters(self.net)
            try:                   # one multi-tensor kernel for all ~120 parameter tensors (the per-tensor form is ~1 ms of tiny kernels per step)
                optimizer = torch.optim.Adam(self.net.parameters(), lr=lr, capturable=True, fused=True)
            except Exception:
                optimizer = torch.optim.Adam(self.net.parameters(), lr=lr, capturable=True)
        self.opt = optimizer

    def capture(self, warmup: int = 3) -> None:
        """Capture the step on the batch currently loaded (the warm-up steps DO update the parameters)."""
        self.graph = capture(self._step, warmup=warmup)

    def step(self) -> torch.Tensor:
        """One training step on the loaded batch; returns the (device) loss of that step."""
        if self.graph is None:
            self._step()
        else:
            self.graph.replay()
        return self.loss


_HAS_EDGE_FEAT = lambda net: getattr(net, "edge_feat", False)
_HAS_POS_ENC = lambda net: getattr(net, "pos_enc_dim", 0) > 0


class CapturedNetStep(_CapturedStep):
    """One captured HIP graph for the whole training step of a net around the layers (``dgn_amd.nets.DGNNet``: embedding, L layers,
    readout, MLP, L1 loss, backward, Adam) at a fixed capacity: ``load(batch)`` writes the batch into static buffers (graph rebuilt in
    place, atoms / graph norm / targets / the readout's graph -> nodes CSR copied), ``step()`` is one graph launch.

    At the reference's batch size (128 molecules) the eager step is host-bound (~5 ms for ~1 ms of GPU work: per-parameter autograd and
    optimizer bookkeeping for the ~120 per-tower tensors of the reference's ``state_dict`` layout); the replay is GPU-bound.

    Padding: node rows beyond the batch are isolated (``PaddedBatch``); graph rows beyond the batch are empty, and the padding nodes
    are shared out among the last PAD_ROWS graph rows, whose loss terms are masked -- every slot of the readout CSR stays referenced, so its backward defines
    (zero) gradients for the padding rows.  The loss is the mean absolute error over the real graphs (``nets.DGNNet.loss`` =
    ``ops.masked_l1_loss``: the target buffer holds NaN behind the batch and the loss kernel itself masks those rows).

    A net with ``pos_enc_dim > 0`` reads its positional encodings from a static ``[n_cap, pos_enc_dim]`` buffer placed once in the padded
    graph's ``ndata['pos_enc']`` (zero behind the batch); ``load(..., pos_enc=eig[:, 1:K+1])`` fills it.

    An ``optimizer`` passed in must be capturable (``capturable=True`` for Adam-type optimizers; plain SGD is) and must have been built
    on parameters that never took part in a default-stream autograd pass (``rewrap_parameters`` first).  Unless an ``optimizer`` is
    passed in, the net's Parameter objects are re-created on construction (``rewrap_parameters``: eager
    training steps on the default stream before a capture are otherwise fatal) and a capturable Adam is built on the new ones."""

    PAD_ROWS = 16      # readout rows behind the real graphs that share the padding nodes
    _REFUSED = ((_HAS_EDGE_FEAT, "CapturedNetStep: nets with edge_feat=True are not supported (the captured step has no static bond-type "
                                 "buffer); run them eagerly or build the net with edge_feat=False"),)

    def __init__(self, net, n_cap: int, e_cap: int, g_cap: int, eig_dim: int, lr: float = 1e-3, optimizer=None, device=None,
                 max_graph_nodes: Optional[int] = None, max_graph_edges: Optional[int] = None, augment: Optional["EigAugment"] = None):
        """``max_graph_nodes`` / ``max_graph_edges``: the largest graph (nodes, directed edges) of the dataset.  Given both, the padded graph
        gets a static block table (``DGNGraph.set_block_capacity``) and the captured step runs its layers on the graph-block route -- five
        launches per layer and step instead of ~28.  ``augment``: a ``dgn_amd.EigAugment`` -- every step (and every replay) then starts by drawing a
        newly augmented ``eig`` from the loaded batch's, as the reference's loops do with ``--flip`` / ``--augmentation``: one more launch."""
        from .graph import DGNGraph
        super().__init__(net, n_cap, e_cap, eig_dim, device, augment=augment)
        dev = self.device
        # graph rows of the readout: g_cap - 1 real graphs at most, then PAD_ROWS rows that share the padding nodes (ONE padding row was a
        # single wave walking ~10 % of the batch's nodes in sequence: 40 us per direction of a 0.77 ms step)
        self.g_cap = int(g_cap)
        g_cap = self.g_rows = self.g_cap - 1 + self.PAD_ROWS
        if max_graph_nodes and max_graph_edges:
            self.pb.graph.set_block_capacity(g_cap, max_graph_nodes, max_graph_edges)
        self.atoms = torch.zeros(n_cap, dtype=torch.int64, device=dev)
        self.targets = torch.full((g_cap, 1), float("nan"), device=dev)      # NaN behind the batch: the loss kernel masks those rows
        self._h_sizes = torch.zeros(g_cap, dtype=torch.int64).pin_memory()
        self._d_sizes = torch.zeros(g_cap, dtype=torch.int64, device=dev)
        # the readout's CSR: rows = graphs (the last one collects the padding nodes), slots = nodes in order
        # (built from an even split: no row may look like a hub row -- more than 2048 slots -- at construction, the hub description of
        #  a DGNGraph is static)
        indptr = (torch.arange(g_cap + 1, dtype=torch.int64, device=dev) * n_cap) // g_cap
        if int((indptr[1:] - indptr[:-1]).max()) > 2048:
            raise ValueError("capacity of more than 2048 nodes per graph row")
        rg = DGNGraph.from_csr(indptr, torch.arange(n_cap, dtype=torch.int32, device=dev), num_src=n_cap)
        assert rg.n_hub == 0
        i32 = lambda n: torch.arange(n, dtype=torch.int32, device=dev)
        rg.csc_ptr, rg.csc_pos = i32(n_cap + 1), i32(n_cap)                 # node j sits in slot j of exactly one row
        rg._c.csc_ptr, rg._c.csc_pos = rg.csc_ptr.data_ptr(), rg.csc_pos.data_ptr()
        rg._csc_ready = True
        rg.sizes = rg.in_degree
        self.rg = rg
        self.pb.graph._dgn_readout = rg
        self._set_optimizer(optimizer, lr)

    @torch.no_grad()
    def load(self, src, dst, num_nodes: int, eig, atoms, snorm, sizes, targets, pos_enc=None) -> None:
        """sizes: nodes per graph (host list or tensor), targets [n_graphs, 1]; pos_enc [num_nodes, pos_enc_dim] (any strides: the
        ``eig[:, 1:K+1]`` slice as it is) for a net with positional encodings, None for every other."""
        self._load_batch(src, dst, num_nodes, eig, atoms, snorm, sizes, targets, pos_enc)
        self.targets[len(sizes):].fill_(float("nan"))             # (the subclasses write their own marker: their load calls _load_batch)

    @torch.no_grad()
    def _load_batch(self, src, dst, num_nodes: int, eig, atoms, snorm, sizes, targets, pos_enc=None) -> None:
        """``load`` without the marker behind the batch's target rows."""
        node = self._node_tensors(snorm, pos_enc, type(self).__name__)
        sizes = torch.as_tensor(sizes, dtype=torch.int64)
        G = sizes.numel()
        self._check_graph_rows(G, num_nodes)
        self.pb.load(src, dst, num_nodes, self._load_eig(eig, num_nodes), node=node, graph_sizes=sizes)
        self.atoms[:num_nodes].copy_(atoms, non_blocking=True)
        self.atoms[num_nodes:].zero_()
        self._load_readout(sizes, num_nodes)
        self.targets[:G].copy_(targets, non_blocking=True)

    def _check_graph_rows(self, G: int, num_nodes: int) -> None:
        if G >= self.g_cap:
            raise ValueError(f"{G} graphs need a capacity of at least {G + 1} graph rows (rows behind the batch collect the padding)")
        if self.pb.n_cap - int(num_nodes) > 2048 * self.PAD_ROWS:
            raise ValueError(f"more than {2048 * self.PAD_ROWS} padding nodes: pick a smaller capacity bucket (a padding row must not be a hub row)")

    def _load_readout(self, sizes: torch.Tensor, num_nodes: int) -> None:
        """The batch's graph sizes (host int64 tensor) -> the readout CSR."""
        n_cap, g_cap, G = self.pb.n_cap, self.g_rows, sizes.numel()
        pad, R = n_cap - int(num_nodes), self.PAD_ROWS
        # graph sizes -> the readout CSR, on the device: ONE copy from a pinned staging buffer (a pageable host tensor copied
        # "non_blocking" right in front of a graph launch stalled the launch by ~20 ms on this runtime), everything else device ops
        h = self._h_sizes
        h.zero_()
        h[:G] = sizes
        h[g_cap - R:] = pad // R                                  # the padding rows
        h[g_cap - R:g_cap - R + pad % R] += 1
        self._d_sizes.copy_(h, non_blocking=True)
        rg = self.rg
        rg.indptr[1:].copy_(torch.cumsum(self._d_sizes, 0))
        rg.in_degree.copy_(self._d_sizes)
        rg.log_deg.copy_(torch.log((self._d_sizes + 1).double()))

    @torch.no_grad()
    def load_packed(self, ds, ids) -> None:
        """``load`` from a device-resident dataset (``dgn_amd.data.PackedGraphs``): ONE gather launch writes the padded graph's arrays,
        ``eig``, ``pos_enc``, the graph norm, the features (node column ``feat``) and the targets (graph column ``label``, whose pad value
        -- NaN, or -1 for classes -- is the marker behind the batch) straight into the static buffers; the readout CSR and the block
        table follow from the host-known sizes as in ``load``.  A batch beyond the capacity raises before anything is written."""
        p = ds.plan(ids)
        self._check_graph_rows(p.G, p.N)
        marker = ds.pads.get(("graph", "label"))
        if self.targets.dtype == torch.int64 and marker != -1 or self.targets.dtype != torch.int64 and marker == marker:
            raise ValueError(f"{type(self).__name__}.load_packed: the dataset's graph column 'label' must pad with "
                             f"{-1 if self.targets.dtype == torch.int64 else 'NaN'} (the rows the loss masks), not {marker}")
        node = {"feat": self.atoms}
        if self.pos_enc_dim > 0:
            node["pos_enc"] = self.pb.node["pos_enc"]
        if self.augment is not None:
            node["eig"] = self.eig_src
        self.pb.graph.load_packed(ds, p, node=node, graph={"label": self.targets}, g_rows_out=self.g_rows, snorm_n=self.snorm)
        self._load_readout(torch.from_numpy(p.sizes), p.N)

    def _step(self) -> None:
        self._augment()
        self.opt.zero_grad(set_to_none=True)
        self.pb.graph.invalidate_caches()
        scores = self.net(self.pb.graph, self.atoms, None, self.snorm, None)
        loss = self._loss(scores)
        loss.backward()
        self.opt.step()
        self.loss.copy_(loss.detach().reshape(()))
        # nothing attached to this step's autograd graph may outlive the step (the net parks the node features on the graph object:
        # released inside the NEXT capture region it would crash capture_end, see capture())
        self.pb.graph.ndata.pop("h", None)
        del scores, loss

    def _loss(self, scores: torch.Tensor) -> torch.Tensor:
        """The net's loss over the real graph rows (mean absolute error; the NaN targets behind the batch mask their rows)."""
        return self.net.loss(scores, self.targets)


class CapturedMolStep(CapturedNetStep):
    """``CapturedNetStep`` for the OGB molecule nets (``dgn_amd.nets.DGNHIVNet`` / ``DGNPCBANet``: AtomEncoder, L layers, readout, MLP,
    binary cross-entropy over the labelled entries, backward, optimizer) -- the same padding scheme and static buffers, with two changes:
    the atom buffer is ``[n_cap, 9]`` (one column per ogb atom feature; the padding rows carry zeros, a valid index of every table), and
    the targets are a ``[g_rows, n_tasks]`` label buffer that holds NaN behind the batch, so that the loss kernel itself masks the padding
    graph rows (``net.loss`` = ``ops.masked_bce_with_logits``: they count nowhere and their gradient rows are exactly zero).

    Refused with a ValueError: ``edge_feat=True`` (as ``CapturedNetStep``), ``pos_enc_dim > 0`` (no static positional-encoding buffer), and
    ``virtual_node`` (the VirtualNode layers' BatchNorm runs over the graph rows and would count the padding rows in its statistics, and
    their broadcast to the nodes has a data-dependent size): run those nets eagerly."""

    _REFUSED = ((_HAS_POS_ENC, "CapturedMolStep: nets with pos_enc_dim > 0 are not supported (no static positional-encoding buffer)"),
                (lambda net: getattr(net, "virtual_node_layers", None) is not None,
                 "CapturedMolStep: nets with virtual_node are not supported (the VirtualNode layers' BatchNorm over the graph rows "
                 "would count the padding rows); run them eagerly or build the net with virtual_node=None")) + CapturedNetStep._REFUSED

    def __init__(self, net, n_cap: int, e_cap: int, g_cap: int, eig_dim: int, **kwargs):
        super().__init__(net, n_cap, e_cap, g_cap, eig_dim, **kwargs)
        n_cols = len(net.embedding_h.dims)
        self.atoms = torch.zeros(self.pb.n_cap, n_cols, dtype=torch.int64, device=self.device)
        self.targets = torch.full((self.g_rows, int(net.n_tasks)), float("nan"), device=self.device)

    @torch.no_grad()
    def load(self, src, dst, num_nodes: int, eig, atoms, snorm, sizes, labels) -> None:
        """atoms [num_nodes, 9] int64; labels [n_graphs] or [n_graphs, n_tasks] of any dtype, NaN = not measured."""
        G = len(sizes)
        labels = torch.as_tensor(labels).to(device=self.device, dtype=torch.float32).reshape(G, -1)
        self._load_batch(src, dst, num_nodes, eig, atoms, snorm, sizes, labels)
        self.targets[G:].fill_(float("nan"))

    def _loss(self, scores: torch.Tensor) -> torch.Tensor:
        return self.net.loss(scores, self.targets)


class CapturedSuperpixelStep(CapturedNetStep):
    """``CapturedNetStep`` for the superpixel graph-classification net (``dgn_amd.nets.DGNSuperpixelNet``: feature embedding, L layers,
    readout, MLP, cross-entropy with the hit count of ``accuracy_mnist_cifar``, backward, optimizer) -- the same padding scheme and readout
    CSR, with two changes: the atom buffer is a float ``[n_cap, in_dim]`` feature buffer (zero behind the batch), and the targets are an
    int64 ``[g_rows]`` label buffer that holds -1 behind the batch, so that the loss kernel itself masks the padding graph rows
    (``net.loss`` = ``ops.class_cross_entropy``: they count nowhere and their gradient rows are exactly zero).  ``step()`` returns
    ``(loss, hits)`` device tensors.

    Refused with a ValueError: ``edge_feat=True`` (no static edge-feature buffer): run such a net eagerly."""

    _REFUSED = ((_HAS_EDGE_FEAT, "CapturedSuperpixelStep: nets with edge_feat=True are not supported (no static edge-feature buffer)"),)

    def __init__(self, net, n_cap: int, e_cap: int, g_cap: int, eig_dim: int, **kwargs):
        super().__init__(net, n_cap, e_cap, g_cap, eig_dim, **kwargs)
        self.atoms = torch.zeros(self.pb.n_cap, int(net.embedding_h.in_features), device=self.device)
        self.targets = torch.full((self.g_rows,), -1, dtype=torch.int64, device=self.device)
        self.hits = torch.zeros((), dtype=torch.int64, device=self.device)

    @torch.no_grad()
    def load(self, src, dst, num_nodes: int, eig, feats, snorm, sizes, labels) -> None:
        """feats [num_nodes, in_dim] float32; labels [n_graphs] int64 classes."""
        G = len(sizes)
        labels = torch.as_tensor(labels).to(device=self.device, dtype=torch.int64).reshape(G)
        self._load_batch(src, dst, num_nodes, eig, feats, snorm, sizes, labels)
        self.targets[G:].fill_(-1)

    def _loss(self, scores: torch.Tensor) -> torch.Tensor:
        loss, hits = self.net.loss(scores, self.targets, hits=True)
        self.hits.copy_(hits)
        return loss

    def step(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """One training step on the loaded batch; returns the (device) loss and hit count of that step."""
        super().step()
        return self.loss, self.hits


class CapturedNodeStep(_CapturedStep):
    """One captured HIP graph for the whole training step of the node-classification net (``dgn_amd.nets.DGNNodeNet``: embedding, L
    layers, per-node MLP, batch-balanced cross-entropy with the confusion matrix of ``accuracy_sbm``, backward, Adam) at a fixed capacity:
    ``load(batch)`` writes the batch into static buffers, ``step()`` is one graph launch and returns ``(loss, confusion)`` device tensors.

    Padding: node rows beyond the batch are isolated (``PaddedBatch``) and carry the label -1 -- the loss kernel counts them nowhere and
    writes zero gradient rows for them, which is the zero cotangent ``PaddedBatch`` asks for; no readout CSR and no graph rows are needed.
    A net with ``pos_enc_dim > 0`` gets a static ``[n_cap, pos_enc_dim]`` buffer in ``ndata['pos_enc']``, filled by ``load(..., pos_enc=...)``.

    ``optimizer``: as for ``CapturedNetStep`` (capturable, built on parameters that never took part in a default-stream autograd pass);
    by default the net's Parameter objects are re-created (``rewrap_parameters``) and a capturable Adam is built on them."""

    _REFUSED = ((_HAS_EDGE_FEAT, "CapturedNodeStep: nets with edge_feat=True are not supported (no static edge-feature buffer)"),)

    def __init__(self, net, n_cap: int, e_cap: int, eig_dim: int, lr: float = 1e-3, optimizer=None, device=None, augment: Optional["EigAugment"] = None):
        """``augment``: as for ``CapturedNetStep``."""
        super().__init__(net, n_cap, e_cap, eig_dim, device, augment=augment)
        dev = self.device
        self.n_classes = int(net.n_classes)
        self.feats = torch.zeros(n_cap, dtype=torch.int64, device=dev)
        self.labels = torch.full((n_cap,), -1, dtype=torch.int64, device=dev)
        self.confusion = torch.zeros(self.n_classes, self.n_classes, dtype=torch.int64, device=dev)
        self._set_optimizer(optimizer, lr)

    @torch.no_grad()
    def load(self, src, dst, num_nodes: int, eig, feats, snorm, labels, sizes=None, pos_enc=None) -> None:
        """feats [num_nodes] int64 node types, labels [num_nodes] int64 classes; sizes: nodes per graph (only for a graph with a block table);
        pos_enc [num_nodes, pos_enc_dim] (any strides) for a net with positional encodings, None for every other."""
        num_nodes = int(num_nodes)
        self.pb.load(src, dst, num_nodes, self._load_eig(eig, num_nodes), node=self._node_tensors(snorm, pos_enc, "CapturedNodeStep"), graph_sizes=sizes)
        self.feats[:num_nodes].copy_(feats, non_blocking=True)
        self.feats[num_nodes:].zero_()
        self.labels[:num_nodes].copy_(labels, non_blocking=True)
        self.labels[num_nodes:].fill_(-1)

    @torch.no_grad()
    def load_packed(self, ds, ids) -> None:
        """``load`` from a device-resident dataset (``dgn_amd.data.PackedGraphs``; node columns ``feat`` and ``label``, the latter padding
        with -1): ONE gather launch into the static buffers.  A batch beyond the capacity raises before anything is written."""
        if ds.pads.get(("node", "label")) != -1:
            raise ValueError("CapturedNodeStep.load_packed: the dataset's node column 'label' must pad with -1 (the rows the loss masks)")
        node = {"feat": self.feats, "label": self.labels}
        if self.pos_enc_dim > 0:
            node["pos_enc"] = self.pb.node["pos_enc"]
        if self.augment is not None:
            node["eig"] = self.eig_src
        self.pb.graph.load_packed(ds, ids, node=node, snorm_n=self.snorm)

    def _step(self) -> None:
        self._augment()
        self.opt.zero_grad(set_to_none=True)
        self.pb.graph.invalidate_caches()
        scores = self.net(self.pb.graph, self.feats, None, self.snorm, None)
        loss, cm = self.net.loss(scores, self.labels, confusion=True)
        loss.backward()
        self.opt.step()
        self.loss.copy_(loss.detach())
        self.confusion.copy_(cm)
        del scores, loss, cm

    def step(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """One training step on the loaded batch; returns the (device) loss and confusion matrix of that step."""
        super().step()
        return self.loss, self.confusion
