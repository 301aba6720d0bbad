"""Device-resident datasets: the reference's ``collate`` as one HIP gather.

The reference forms every batch on the host, at every step: ``collate`` (data/molecules.py:219-230, data/SBMs.py:167-179,
data/HIV.py:113-125, data/PCBA.py:266-278, data/superpixels.py:316-330) calls ``dgl.batch`` on the samples' graph objects and builds the
per-node and per-edge graph-norm vectors.  Every dataset of the reference fits the GPU many times over, so ``PackedGraphs`` keeps the
whole dataset there as concatenated columns and builds its CSR ONCE (one ``DGNGraph`` over all nodes: ``dgn_graph_build`` +
``dgn_graph_build_csc``).  The graphs of a batch are disjoint and each one's nodes, edges, CSR slots and CSC ranks are one contiguous
range of the dataset, so a batch -- its columns, graph norms, edge list and the complete CSR / CSC of ``DGNGraph`` -- is a shifted copy
of rows of the dataset: ``dgn_collate`` of the C ABI, one kernel launch and one small pinned copy per batch, no sort, no scan, nothing
read back.

    ds = PackedGraphs.from_graphs(graphs, device)         # graphs: dicts with src, dst (local ids), num_nodes and named columns
    for ids in ds.batches(128, shuffle=True):
        b = ds.collate(ids)                               # b.graph (a DGNGraph), b.labels, b.snorm_n, b.snorm_e: the reference's tuple
        step.load_packed(ds, ids)                         # ... or straight into a captured step's static buffers

Columns are ``int64`` or ``float32``, 1-D or 2-D, named per domain: node ``feat`` / ``eig`` / ``pos_enc`` / ``label``, edge ``feat``,
graph ``label``.  Each has a PAD VALUE for the rows behind the batch in capacity buffers: 0, except -1 for int64 labels and NaN for float
labels -- what the captured steps' loss kernels mask on.
"""
from __future__ import annotations

import ctypes as C
import struct
from types import SimpleNamespace
from typing import Dict, Iterator, Optional

import numpy as np
import torch

from . import _lib

_DOMAINS = ("node", "edge", "graph")
_MAX_COLS = {"node": _lib.DGN_COLLATE_MAX_NODE_COLS, "edge": _lib.DGN_COLLATE_MAX_EDGE_COLS, "graph": _lib.DGN_COLLATE_MAX_GRAPH_COLS}
MAX_BATCH_GRAPHS = _lib.DGN_COLLATE_MAX_GRAPHS
_INT32_LIMIT = 2 ** 31 - 1
# the batch's DGNGraph arrays dgn_collate can write: name in DgnCollate -> (dtype, "node" rows + extra | "edge" rows | fixed length)
_CSR_OUTPUTS = {"indptr": (torch.int32, "node", 1), "src_csr": (torch.int32, "edge", 0), "dst_csr": (torch.int32, "edge", 0),
                "eid": (torch.int64, "edge", 0), "in_degree": (torch.int64, "node", 0), "log_deg": (torch.float32, "node", 0),
                "csc_ptr": (torch.int32, "node", 1), "csc_pos": (torch.int32, "edge", 0), "csc_order": (torch.int32, "edge", 0),
                "stats": (torch.int32, None, 4), "n_valid": (torch.int64, None, 1)}


def graph_norm(sizes) -> torch.Tensor:
    """The graph-norm value of a graph of ``size`` nodes (edges), by the reference's own expression
    ``torch.FloatTensor(size, 1).fill_(1. / float(size)).sqrt()`` (data/molecules.py:224-228): the double 1 / size rounded to fp32, then
    fp32's square root.  One value per entry of ``sizes`` (0 where the size is 0: a graph without edges has no ``snorm_e`` rows)."""
    s = torch.as_tensor(np.asarray(sizes, dtype=np.int64))
    v = (1.0 / s.clamp(min=1).double()).float().sqrt()
    return torch.where(s > 0, v, torch.zeros_like(v))


def default_pad(name: str, dtype: torch.dtype):
    """0; -1 for int64 labels, NaN for float labels (what the loss kernels mask on)."""
    if name == "label":
        return -1 if dtype == torch.int64 else float("nan")
    return 0


def _pad_pattern(value, dtype: torch.dtype) -> int:
    """The 8-byte pattern dgn_collate writes behind the batch: an int64, or a float's bits in both halves."""
    if dtype == torch.int64:
        return int(value)
    bits = struct.unpack("<I", struct.pack("<f", float(value)))[0]
    return struct.unpack("<q", struct.pack("<II", bits, bits))[0]


def _as_column(x, what: str) -> torch.Tensor:
    t = torch.as_tensor(x)
    if t.dtype in (torch.float64, torch.float16, torch.bfloat16):
        t = t.float()
    elif t.dtype in (torch.int32, torch.int16, torch.int8, torch.uint8, torch.bool):
        t = t.long()
    if t.dtype not in (torch.int64, torch.float32):
        raise ValueError(f"{what}: columns are int64 or float32, got {t.dtype}")
    if t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[1] == 0):
        raise ValueError(f"{what}: columns are 1-D or 2-D with a fixed width, got shape {tuple(t.shape)}")
    return t.contiguous()


def _row_bytes(t: torch.Tensor) -> int:
    return (t.shape[1] if t.dim() == 2 else 1) * t.element_size()


class Batch:
    """What ``PackedGraphs.collate`` returns: the reference's ``(batched_graph, labels, snorm_n, snorm_e)`` and the batch's edge list."""

    def __init__(self, graph, labels, snorm_n, snorm_e, src, dst, node, edge, graph_columns, sizes, edge_sizes):
        self.graph, self.labels, self.snorm_n, self.snorm_e, self.src, self.dst = graph, labels, snorm_n, snorm_e, src, dst
        self.node, self.edge, self.graph_columns = node, edge, graph_columns
        self.batch_num_nodes, self.batch_num_edges = sizes, edge_sizes
        self.num_nodes, self.num_edges, self.num_graphs = graph.num_nodes, graph.num_edges, len(sizes)

    def __iter__(self):                       # batched_graph, labels, snorm_n, snorm_e = ds.collate(ids)
        return iter((self.graph, self.labels, self.snorm_n, self.snorm_e))


class PackedGraphs:
    """A dataset of graphs as concatenated arrays: host pointers and per-graph tables (numpy, built once), and -- with a ``device`` -- the
    columns and ONE ``DGNGraph`` over all nodes on that device."""

    # ---- construction -----------------------------------------------------------------------------------------------------------
    @classmethod
    def from_graphs(cls, graphs, device=None, pads: Optional[dict] = None) -> "PackedGraphs":
        """``graphs``: a list of dicts with ``src``, ``dst`` (LOCAL node ids in edge-id order), ``num_nodes`` and columns under
        ``"node"`` / ``"edge"`` / ``"graph"`` (dicts name -> array; a graph column holds ONE row per graph: a scalar or a 1-D row)."""
        graphs = list(graphs)
        if not graphs:
            raise ValueError("PackedGraphs: no graphs")
        num_nodes = np.asarray([int(g["num_nodes"]) for g in graphs], dtype=np.int64)
        srcs = [np.asarray(torch.as_tensor(g["src"]).cpu(), dtype=np.int64).reshape(-1) for g in graphs]
        dsts = [np.asarray(torch.as_tensor(g["dst"]).cpu(), dtype=np.int64).reshape(-1) for g in graphs]
        for i, (s, d) in enumerate(zip(srcs, dsts)):
            if s.shape != d.shape:
                raise ValueError(f"PackedGraphs: graph {i}: src and dst differ in length")
        num_edges = np.asarray([s.size for s in srcs], dtype=np.int64)
        cols = {}
        for dom in _DOMAINS:
            names = list(graphs[0].get(dom, {}))
            for i, g in enumerate(graphs):
                if list(g.get(dom, {})) != names:
                    raise ValueError(f"PackedGraphs: graph {i} has other {dom} columns than graph 0")
            if dom == "graph":
                cols[dom] = {k: torch.stack([torch.as_tensor(g[dom][k]) for g in graphs]) for k in names}
            else:
                cols[dom] = {k: torch.cat([torch.as_tensor(g[dom][k]) for g in graphs]) for k in names}
        return cls.from_packed(np.concatenate(srcs), np.concatenate(dsts), num_nodes, num_edges, cols["node"], cols["edge"], cols["graph"],
                               device=device, pads=pads, local_ids=True)

    @classmethod
    def from_packed(cls, src, dst, num_nodes, num_edges, node=None, edge=None, graph=None, device=None, pads: Optional[dict] = None,
                    local_ids: bool = False) -> "PackedGraphs":
        """Already-concatenated arrays: ``src`` / ``dst`` [E_total] in edge-id order, graph after graph (ids into the concatenated node
        array as ``dgl.batch`` leaves them, or each graph's own with ``local_ids``), ``num_nodes`` / ``num_edges`` [D] per graph, and the
        concatenated columns.  ``pads``: ``{(domain, name): value}`` where a column's pad value is not the default.  ``device`` None:
        the host side only (pointers, capacities, offset tables); ``to(device)`` completes it."""
        self = cls.__new__(cls)
        nn = np.asarray(torch.as_tensor(num_nodes).cpu(), dtype=np.int64).reshape(-1)
        ne = np.asarray(torch.as_tensor(num_edges).cpu(), dtype=np.int64).reshape(-1)
        if nn.size == 0 or nn.shape != ne.shape:
            raise ValueError("PackedGraphs: num_nodes and num_edges must be [n_graphs] arrays of one length (at least one graph)")
        if int(nn.min()) < 1:
            raise ValueError(f"PackedGraphs: graph {int(np.argmin(nn))} has no nodes (every graph needs at least one)")
        if int(ne.min()) < 0:
            raise ValueError("PackedGraphs: negative edge count")
        D = int(nn.size)
        self.num_graphs = D
        self.node_ptr = np.concatenate([[0], np.cumsum(nn)]).astype(np.int64)
        self.edge_ptr = np.concatenate([[0], np.cumsum(ne)]).astype(np.int64)
        N, E = int(self.node_ptr[-1]), int(self.edge_ptr[-1])
        if N >= _INT32_LIMIT or E >= _INT32_LIMIT:
            raise ValueError(f"PackedGraphs: {N} nodes / {E} edges exceed the int32 CSR range")
        self.num_nodes, self.num_edges = N, E
        s = np.asarray(torch.as_tensor(src).cpu(), dtype=np.int64).reshape(-1)
        d = np.asarray(torch.as_tensor(dst).cpu(), dtype=np.int64).reshape(-1)
        if s.size != E or d.size != E:
            raise ValueError(f"PackedGraphs: {s.size} / {d.size} edge endpoints for {E} edges")
        lo = np.repeat(self.node_ptr[:-1], ne)
        if local_ids:
            s, d = s + lo, d + lo
        hi = np.repeat(self.node_ptr[1:], ne)
        bad = (s < lo) | (s >= hi) | (d < lo) | (d >= hi)
        if bad.any():
            e = int(np.argmax(bad))
            g = int(np.searchsorted(self.edge_ptr, e, side="right") - 1)
            raise ValueError(f"PackedGraphs: edge {e - int(self.edge_ptr[g])} of graph {g} has an endpoint outside the graph")
        from .graph import HUB_THRESHOLD
        deg = np.bincount(d, minlength=N) if E else np.zeros(N, dtype=np.int64)
        self.max_in_degree = np.maximum.reduceat(deg, self.node_ptr[:-1]).astype(np.int64)      # per graph (every graph has a node)
        if int(self.max_in_degree.max()) > HUB_THRESHOLD:
            g = int(np.argmax(self.max_in_degree))
            raise ValueError(f"PackedGraphs: graph {g} has a node of in-degree {int(self.max_in_degree[g])} > {HUB_THRESHOLD} "
                             "(padded batches take no hub rows)")
        self.snorm_n, self.snorm_e = graph_norm(nn), graph_norm(ne)                              # [D] fp32, host
        self._src, self._dst = torch.from_numpy(s), torch.from_numpy(d)                          # dataset node ids, edge-id order
        rows = {"node": N, "edge": E, "graph": D}
        self.columns: Dict[str, Dict[str, torch.Tensor]] = {}
        self.pads: Dict[tuple, object] = {}
        for dom, given in zip(_DOMAINS, (node, edge, graph)):
            given = dict(given or {})
            if len(given) > _MAX_COLS[dom]:
                raise ValueError(f"PackedGraphs: {len(given)} {dom} columns (dgn_collate takes at most {_MAX_COLS[dom]})")
            self.columns[dom] = {}
            for name, x in given.items():
                t = _as_column(x, f"PackedGraphs: {dom} column '{name}'")
                if t.shape[0] != rows[dom]:
                    raise ValueError(f"PackedGraphs: {dom} column '{name}' has {t.shape[0]} rows for {rows[dom]} {dom}s")
                self.columns[dom][name] = t
                self.pads[(dom, name)] = (pads or {}).get((dom, name), default_pad(name, t.dtype))
        for key in (pads or {}):
            if key not in self.pads:
                raise ValueError(f"PackedGraphs: pad value for an unknown column {key}")
        self.device = None
        self.graph = None
        if device is not None:
            self.to(device)
        return self

    def to(self, device) -> "PackedGraphs":
        """Move the columns to ``device`` and build the dataset's CSR / CSC there (once)."""
        from .graph import DGNGraph
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if self.device == dev:
            return self
        if dev.type != "cuda":
            raise _lib.DgnError("dgn_amd runs on the GPU only: a PackedGraphs is collated on a CUDA device")
        for dom in _DOMAINS:
            self.columns[dom] = {k: v.to(dev) for k, v in self.columns[dom].items()}
        self._src, self._dst = self._src.to(dev), self._dst.to(dev)
        self._snorm_n_dev, self._snorm_e_dev = self.snorm_n.to(dev), self.snorm_e.to(dev)
        g = DGNGraph(self._src, self._dst, self.num_nodes)
        g.ensure_csc()
        self.graph, self.device = g, dev
        self._ring, self._turn = [None, None], 0
        return self

    # ---- host-side helpers ------------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return self.num_graphs

    def sizes(self, ids=None):
        """(nodes, edges) per graph, host int64 arrays."""
        nn, ne = np.diff(self.node_ptr), np.diff(self.edge_ptr)
        return (nn, ne) if ids is None else (nn[ids], ne[ids])

    def batches(self, batch_size: int, shuffle: bool = False, generator=None, drop_last: bool = False) -> Iterator[np.ndarray]:
        """Host id arrays of one epoch.  ``generator``: a ``numpy.random.Generator``, a ``torch.Generator`` or a seed."""
        D, bs = self.num_graphs, int(batch_size)
        if bs < 1:
            raise ValueError("batches: batch_size must be at least 1")
        if not shuffle:
            order = np.arange(D, dtype=np.int64)
        elif isinstance(generator, torch.Generator):
            order = torch.randperm(D, generator=generator).numpy().astype(np.int64)
        else:
            rng = generator if isinstance(generator, np.random.Generator) else np.random.default_rng(generator)
            order = rng.permutation(D).astype(np.int64)
        for i in range(0, D, bs):
            ids = order[i:i + bs]
            if drop_last and ids.size < bs:
                return
            yield ids

    def capacity(self, batch_size: int):
        """``(n_cap, e_cap, max_graph_nodes, max_graph_edges)``: nodes / edges of the ``batch_size`` largest graphs together and of the
        largest single graph -- what a captured step's constructor needs so that every batch of an epoch fits one capture."""
        nn, ne = self.sizes()
        k = min(int(batch_size), self.num_graphs)
        return (int(np.sort(nn)[::-1][:k].sum()), int(np.sort(ne)[::-1][:k].sum()), int(nn.max()), int(ne.max()))

    def plan(self, ids):
        """The host side of one batch: its graphs' sizes and the offset table ``dgn_collate`` reads -- int32 [5, G + 1], rows: batch node
        offset, batch edge offset, dataset node base, dataset edge base, dataset graph id (numpy cumsums: N and E are known without a
        read-back).  ``ids``: a host sequence, array or CPU tensor; any order, repeats allowed."""
        if isinstance(ids, SimpleNamespace):
            return ids
        ids = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids, dtype=np.int64).reshape(-1)
        G = int(ids.size)
        if G > MAX_BATCH_GRAPHS:
            raise ValueError(f"a batch of {G} graphs (dgn_collate takes at most {MAX_BATCH_GRAPHS})")
        if G and (int(ids.min()) < 0 or int(ids.max()) >= self.num_graphs):
            raise IndexError(f"graph ids outside [0, {self.num_graphs})")
        nn, ne = self.sizes(ids)
        node_off, edge_off = np.cumsum(nn), np.cumsum(ne)
        N, E = (int(node_off[-1]), int(edge_off[-1])) if G else (0, 0)
        if N >= _INT32_LIMIT or E >= _INT32_LIMIT:
            raise ValueError(f"a batch of {N} nodes / {E} edges exceeds the int32 CSR range")
        table = np.zeros((5, G + 1), dtype=np.int32)
        table[0, 1:], table[1, 1:] = node_off, edge_off
        table[2, :G], table[3, :G], table[4, :G] = self.node_ptr[ids], self.edge_ptr[ids], ids
        return SimpleNamespace(ids=ids, G=G, N=N, E=E, sizes=nn, edge_sizes=ne, table=table,
                               max_in_degree=int(self.max_in_degree[ids].max()) if G else 0)

    # ---- the gather ---------------------------------------------------------------------------------------------------------------
    def _upload(self, table: np.ndarray):
        """The table on the device through one of TWO pinned staging buffers, each guarded by an event recorded after the kernel that
        read its upload: a buffer is rewritten only when the copy out of it (and the kernel behind it) is done."""
        n = table.size
        slot = self._ring[self._turn]
        if slot is not None:
            slot.done.synchronize()
        if slot is None or slot.host.numel() < n:
            cap = max(1024, 2 * n)
            slot = SimpleNamespace(host=torch.empty(cap, dtype=torch.int32).pin_memory(),
                                   dev=torch.empty(cap, dtype=torch.int32, device=self.device), done=torch.cuda.Event())
            self._ring[self._turn] = slot
        self._turn ^= 1
        slot.host[:n].copy_(torch.from_numpy(table.reshape(-1)))
        slot.dev[:n].copy_(slot.host[:n], non_blocking=True)
        return slot

    def gather(self, ids, n_rows_out: Optional[int] = None, e_rows_out: Optional[int] = None, g_rows_out: Optional[int] = None,
               node: Optional[dict] = None, edge: Optional[dict] = None, graph: Optional[dict] = None, snorm_n=None, snorm_e=None,
               graph_id=None, src=None, dst=None, csr: Optional[dict] = None):
        """One ``dgn_collate`` launch into caller-owned tensors: the named columns (``node`` / ``edge`` / ``graph``: name -> output
        tensor of ``*_rows_out`` rows), the graph norms, ``graph_id``, the edge list and the ``DGNGraph`` arrays named in ``csr``
        (indptr, src_csr, dst_csr, eid, in_degree, log_deg, csc_ptr, csc_pos, csc_order, stats, n_valid).  Rows behind the batch get the
        pad values.  Everything is checked before anything is written: a ``ValueError`` leaves the outputs as they were."""
        if self.device is None:
            raise _lib.DgnError("PackedGraphs.gather: the dataset is on the host only (from_packed(..., device=...) or to(device))")
        p = self.plan(ids)
        rows = {"node": p.N if n_rows_out is None else int(n_rows_out), "edge": p.E if e_rows_out is None else int(e_rows_out),
                "graph": p.G if g_rows_out is None else int(g_rows_out)}
        if p.N > rows["node"] or p.E > rows["edge"] or p.G > rows["graph"]:
            raise ValueError(f"batch ({p.N} nodes, {p.E} edges, {p.G} graphs) exceeds the capacity ({rows['node']}, {rows['edge']}, {rows['graph']})")
        c = _lib.DgnCollate()
        c.n_graphs, c.n_nodes, c.n_edges = p.G, p.N, p.E
        c.n_rows_out, c.e_rows_out, c.g_rows_out = rows["node"], rows["edge"], rows["graph"]
        c.max_in_degree = p.max_in_degree

        def check(t, what, dtype, n, row_bytes=None):
            if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != dtype or not t.is_contiguous():
                raise ValueError(f"gather: output {what} must be a contiguous {dtype} tensor on {self.device}")
            if t.shape[0] != n or (row_bytes is not None and (t.numel() // max(n, 1)) * t.element_size() != row_bytes and n > 0):
                raise ValueError(f"gather: output {what} has shape {tuple(t.shape)}; {n} rows" +
                                 (f" of {row_bytes} bytes" if row_bytes is not None else "") + " expected")
            return t.data_ptr() or None

        for dom, outs in zip(_DOMAINS, (node, edge, graph)):
            outs = outs or {}
            for name in outs:
                if name not in self.columns[dom]:
                    raise ValueError(f"gather: the dataset has no {dom} column '{name}' (it has {sorted(self.columns[dom])})")
            setattr(c, f"n_{dom}_cols", len(self.columns[dom]))
            for i, (name, col) in enumerate(self.columns[dom].items()):
                getattr(c, f"{dom}_in")[i] = col.data_ptr() or None
                getattr(c, f"{dom}_row_bytes")[i] = _row_bytes(col)
                getattr(c, f"{dom}_pad")[i] = _pad_pattern(self.pads[(dom, name)], col.dtype)
                out = outs.get(name)
                getattr(c, f"{dom}_out")[i] = None if out is None else check(out, f"{dom} column '{name}'", col.dtype, rows[dom], _row_bytes(col))
        if snorm_n is not None:
            c.snorm_n = check(snorm_n, "snorm_n", torch.float32, rows["node"], 4)
        if snorm_e is not None:
            c.snorm_e = check(snorm_e, "snorm_e", torch.float32, rows["edge"], 4)
        if graph_id is not None:
            c.graph_id = check(graph_id, "graph_id", torch.int32, rows["node"], 4)
        if src is not None:
            c.src = check(src, "src", torch.int64, rows["edge"], 8)
        if dst is not None:
            c.dst = check(dst, "dst", torch.int64, rows["edge"], 8)
        for name, t in (csr or {}).items():
            if name not in _CSR_OUTPUTS:
                raise ValueError(f"gather: unknown graph array '{name}' (known: {sorted(_CSR_OUTPUTS)})")
            dtype, dom, extra = _CSR_OUTPUTS[name]
            setattr(c, name, check(t, name, dtype, extra if dom is None else rows[dom] + extra, t.element_size()))
        D = self.graph
        ptr = lambda t: t.data_ptr() or None
        c.d_indptr, c.d_src, c.d_dst_csr, c.d_eid = ptr(D.indptr), ptr(D.src), ptr(D.dst_csr), ptr(D.eid)
        c.d_in_degree, c.d_log_deg = ptr(D.in_degree), ptr(D.log_deg)
        c.d_csc_ptr, c.d_csc_pos, c.d_csc_order = ptr(D.csc_ptr), ptr(D.csc_pos), ptr(D.csc_order)
        c.d_edge_src, c.d_edge_dst = ptr(self._src), ptr(self._dst)
        c.d_snorm_n, c.d_snorm_e = ptr(self._snorm_n_dev), ptr(self._snorm_e_dev)
        lib = _lib.load()
        slot = self._upload(p.table)
        c.table = slot.dev.data_ptr()
        rc = lib.dgn_collate(C.byref(c), _lib.stream_ptr(self.device))
        slot.done.record(torch.cuda.current_stream(self.device))
        _lib.check(rc, "dgn_collate")
        return p

    def collate(self, ids) -> Batch:
        """The eager counterpart of the reference's ``collate``: ``Batch`` with ``graph`` (a ``DGNGraph`` adopted from the gathered CSR /
        CSC: no sort, nothing read back; ``ndata`` holds the node columns and ``graph_id``, ``edata`` the edge columns,
        ``batch_num_nodes`` / ``batch_num_edges`` the host lists), ``labels`` (the graph column ``label``, else the node column
        ``label``), ``snorm_n [N, 1]``, ``snorm_e [E, 1]``, ``src`` / ``dst``.  One launch and one pinned copy."""
        from .graph import HUB_CHUNK, HUB_THRESHOLD, DGNGraph
        p = self.plan(ids)
        dev, N, E, G = self.device, p.N, p.E, p.G
        if dev is None:
            raise _lib.DgnError("PackedGraphs.collate: the dataset is on the host only (from_packed(..., device=...) or to(device))")
        like = lambda col, n: torch.empty((n,) + tuple(col.shape[1:]), dtype=col.dtype, device=dev)
        outs = {dom: {k: like(v, n) for k, v in self.columns[dom].items()} for dom, n in zip(_DOMAINS, (N, E, G))}
        new = lambda n, dtype: torch.empty(n, dtype=dtype, device=dev)
        csr = {name: new((E if dom == "edge" else N if dom == "node" else 0) + extra, dtype) for name, (dtype, dom, extra) in _CSR_OUTPUTS.items()
               if name != "n_valid"}
        snorm_n, snorm_e, graph_id = new(N, torch.float32), new(E, torch.float32), new(N, torch.int32)
        src, dst = new(E, torch.int64), new(E, torch.int64)
        self.gather(p, node=outs["node"], edge=outs["edge"], graph=outs["graph"], snorm_n=snorm_n, snorm_e=snorm_e, graph_id=graph_id,
                    src=src, dst=dst, csr=csr)
        g = DGNGraph.__new__(DGNGraph)
        g.dst_csr, g._stats = csr["dst_csr"], csr["stats"]
        g._init_csr(csr["indptr"], csr["src_csr"], csr["eid"], N, E, csr["in_degree"], HUB_THRESHOLD, HUB_CHUNK, log_deg=csr["log_deg"],
                    max_in_degree=p.max_in_degree, n_hub_hint=0)
        g.csc_ptr, g.csc_pos, g.csc_order = csr["csc_ptr"], csr["csc_pos"], csr["csc_order"]
        g._c.csc_ptr, g._c.csc_pos = g.csc_ptr.data_ptr(), g.csc_pos.data_ptr()
        g._csc_ready = True
        g.ndata, g.edata = dict(outs["node"]), dict(outs["edge"])
        g.ndata["graph_id"] = graph_id
        g.batch_num_nodes, g.batch_num_edges = [int(x) for x in p.sizes], [int(x) for x in p.edge_sizes]
        labels = outs["graph"].get("label", outs["node"].get("label"))
        return Batch(g, labels, snorm_n.unsqueeze(1), snorm_e.unsqueeze(1), src, dst, outs["node"], outs["edge"], outs["graph"],
                     g.batch_num_nodes, g.batch_num_edges)
