"""Superpixel graphs (MNIST / CIFAR10) from raw data to a layer input on the GPU (csrc/dgn_superpixels.hip).

The reference builds every graph on the CPU (realworld_benchmark/data/superpixels.py): ``sigma``, ``compute_adjacency_matrix_images`` and
``compute_edges_list`` (:17-69) are a ``cdist``, two ``np.partition`` calls and an ``exp`` per graph for 60-70 k graphs, and ``get_eig``
(:154-159, :346-428) runs a sparse eigen-solve per graph plus ``sort_eig`` -- or ``coord_encoding`` -- at every dataset load.  Here
``knn_graph`` builds the edges and their values of a whole batch in one launch, ``batch_eig`` (dgn_amd/eig.py) solves the Laplacians and
``sort_eig`` picks the column order, all on the device.

The reference's edges are NOT each node's 8 most similar nodes: ``np.argpartition(A, n - 10)[:, n - 9:-1]`` keeps eight of the nine largest
entries of a row and drops the one that lands in the last position, the row's maximum.  Node i therefore sends edges to the nodes ranked
2nd to 9th by similarity.  ``knn_graph`` reproduces that by default (``skip_nearest=True``); ``synth.knn_batch`` is a plain k-NN of random
points, a different graph.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

MAX_NODES = 256            # dgn_knn_graph_max_nodes()
_STATUS = {-1: f"has more than {MAX_NODES} nodes", -2: "has a node or edge range outside the arrays, or an edge count that is not the rule's"}


def knn_edge_counts(sizes, k: int = 8) -> torch.Tensor:
    """``[G]`` int64: the edges ``knn_graph`` emits per graph of ``sizes`` nodes -- 1 (a self-loop) for one node, ``n (n - 1)`` (fully
    connected) for ``2 <= n <= k + 1``, ``n k`` from ``k + 2`` nodes on.  Pure torch arithmetic on the tensor's device; a host sequence
    or CPU tensor is also checked: every graph has at least one node."""
    if not 1 <= int(k) <= 32:
        raise ValueError(f"knn_edge_counts: k = {k} outside 1 .. 32")
    n = torch.as_tensor(sizes, dtype=torch.int64).flatten()
    if n.device.type == "cpu" and n.numel() and int(n.min()) < 1:
        raise ValueError("knn_edge_counts: a graph has at least one node")
    per_node = torch.where(n == 1, torch.ones_like(n), torch.where(n <= k + 1, n - 1, torch.full_like(n, int(k))))
    return n * per_node


def _offsets(counts: torch.Tensor) -> torch.Tensor:
    off = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=counts.device)
    off[1:] = torch.cumsum(counts, 0)
    return off


def _capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def knn_graph(coord: torch.Tensor, sizes, feat: Optional[torch.Tensor] = None, k: int = 8, skip_nearest: bool = True, check: bool = True, *,
              out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None, status: Optional[torch.Tensor] = None):
    """``(src, dst, value)`` -- int64, int64, fp32 ``[E]`` -- of the superpixel graphs of a batch: what ``SuperPixDGL._prepare`` stores as
    each graph's edges and ``edata['feat']`` (data/superpixels.py:104-152), in one launch of ``dgn_knn_graph``.

    ``coord``: ``[N, 2]`` CUDA tensor, already divided by the image size; ``feat``: ``[N, C]``, ``1 <= C <= 8`` (the mean pixel values:
    ``use_mean_px``) or None for coordinates only.  fp32 or fp64: the kernel computes in fp64, to which fp32 converts exactly.  ``sizes``:
    the graphs' node counts, at most 256 each.  Graph g owns the next ``sizes[g]`` rows.

    Per graph: ``A`` as ``compute_adjacency_matrix_images`` forms it, then for ``n >= k + 2`` the ``n - 1`` other nodes of row i ranked by A
    descending (equal values: lower index first); ``skip_nearest=True`` emits ranks 1 .. k, which is the reference's neighbour choice at
    ``k = 8`` (see the module docstring), ``False`` ranks 0 .. k - 1.  ``2 <= n <= k + 1``: fully connected, ascending j.  ``n == 1``: one
    self-loop of value 0.  Edge ``edge_off[g] + i * per_node + slot`` runs from ``src = n0 + i`` to ``dst = n0 + j`` with
    ``value = float32(A[i, j])``; within a row the values do not increase.  The caller may round ``value`` to half as the reference's
    files do.

    If ``sizes`` is a Python sequence or a CPU tensor, the offsets and E are computed on the host and nothing is synchronised.  If it is
    a device tensor, E is read back once -- unless ``out`` is passed: E is then its length, which the kernel checks against the offsets
    (status -2), and with ``check=False`` the call is capturable.  ``check=True`` reads the per-graph status back once and raises
    ``DgnError`` on a negative entry, naming the graph and the reason; ``check=False`` -- and any call under stream capture -- reads nothing back: a refused graph's edge
    range keeps what the buffers held.  ``out``: preallocated ``(src, dst, value)`` of E entries; ``status``: an int32 ``[G]`` buffer."""
    from . import _lib
    if not coord.is_cuda:
        raise _lib.DgnError("dgn_amd runs on the GPU only: coord must be a CUDA tensor")
    dev = coord.device
    if coord.dim() != 2 or coord.shape[1] != 2:
        raise ValueError("knn_graph: coord is [N, 2]")
    N = coord.shape[0]
    if feat is not None:
        if feat.dim() == 1:
            feat = feat.unsqueeze(1)
        if feat.device != dev or feat.dim() != 2 or feat.shape[0] != N or not 1 <= feat.shape[1] <= 8:
            raise ValueError("knn_graph: feat is [N, C] on coord's device with 1 <= C <= 8")
    sizes_t = torch.as_tensor(sizes, dtype=torch.int64).flatten()
    counts = knn_edge_counts(sizes_t, k)
    G = sizes_t.numel()
    if sizes_t.is_cuda:
        graph_off, edge_off = _offsets(sizes_t.to(dev)), _offsets(counts.to(dev))
        E = int(out[0].numel()) if out is not None else int(edge_off[-1])        # (the one read-back of a device `sizes`)
    else:
        if int(sizes_t.sum()) != N:
            raise ValueError(f"knn_graph: the sizes add up to {int(sizes_t.sum())} nodes, coord has {N} rows")
        edge_host = _offsets(counts)
        E = int(edge_host[-1])
        graph_off, edge_off = _offsets(sizes_t).to(dev, non_blocking=True), edge_host.to(dev, non_blocking=True)
    if out is None:
        out = (torch.empty(E, dtype=torch.int64, device=dev), torch.empty(E, dtype=torch.int64, device=dev),
               torch.empty(E, dtype=torch.float32, device=dev))
    src, dst, value = out
    for t, dt in ((src, torch.int64), (dst, torch.int64), (value, torch.float32)):
        if tuple(t.shape) != (E,) or t.dtype != dt or t.device != dev or not t.is_contiguous():
            raise ValueError(f"knn_graph: out holds contiguous int64, int64, float32 [{E}] tensors on {dev}")
    if status is None:
        status = torch.zeros(G, dtype=torch.int32, device=dev)
    if tuple(status.shape) != (G,) or status.dtype != torch.int32 or status.device != dev or not status.is_contiguous():
        raise ValueError(f"knn_graph: status is a contiguous int32 [{G}] tensor on {dev}")
    if G == 0:
        return src, dst, value
    c64 = coord.to(torch.float64).contiguous()
    f64 = feat.to(torch.float64).contiguous() if feat is not None else None
    _lib.check(_lib.load().dgn_knn_graph(c64.data_ptr(), f64.data_ptr() if f64 is not None else None, f64.shape[1] if f64 is not None else 0,
                                         N, graph_off.data_ptr(), edge_off.data_ptr(), G, int(k), int(bool(skip_nearest)), E, src.data_ptr(),
                                         dst.data_ptr(), value.data_ptr(), status.data_ptr(), _lib.stream_ptr(dev)), "dgn_knn_graph")
    if check and not _capturing():
        st = status.cpu()
        bad = torch.nonzero(st < 0).flatten().tolist()
        if bad:
            raise _lib.DgnError(f"knn_graph: graph {bad[0]} {_STATUS.get(int(st[bad[0]]), 'was refused')}"
                                + (f" (and {len(bad) - 1} more graphs)" if len(bad) > 1 else ""))
    return src, dst, value


def coord_encoding(coord: torch.Tensor) -> torch.Tensor:
    """``[N, 3]`` fp32 ``[0, x, y]``: the reference's ``coord_encoding`` (data/superpixels.py:423-428), its stand-in for ``eig``."""
    if coord.dim() != 2 or coord.shape[1] != 2:
        raise ValueError("coord_encoding: coord is [N, 2]")
    c = coord.to(torch.float32)
    return torch.cat([torch.zeros_like(c[:, :1]), c], dim=1)


def sort_eig(eig: torch.Tensor, coord: torch.Tensor, sizes) -> torch.Tensor:
    """The reference's ``sort_eig`` (data/superpixels.py:371-420) on every graph of a batch, in place on ``eig [N, K >= 3]`` fp32 (rows may
    be strided); returns ``eig``.  Per graph and column c in {1, 2}: ``hor_c = |sum over eig[i, c] > 0 of (x_i > 0.5 ? 1 : -1)|``, ``ver_c``
    with y.  Where ``hor_1`` or ``ver_2`` is the largest of the four the rows stay.  Otherwise column 1 is overwritten with column 2: the
    reference's ``eigs[:, 1] = eig2; eigs[:, 2] = eig1`` reads as an exchange, but ``eig1`` is a view of column 1, so its datasets hold
    column 2 twice -- and so does this.  One launch of ``dgn_superpixel_sort_eig``, nothing read back.  ``coord``: ``[N, 2]`` (x, y);
    ``sizes``: host sequence, CPU or device tensor."""
    from . import _lib
    if not eig.is_cuda:
        raise _lib.DgnError("dgn_amd runs on the GPU only: eig must be a CUDA tensor")
    dev = eig.device
    if eig.dim() != 2 or eig.shape[1] < 3 or eig.dtype != torch.float32 or eig.stride(1) != 1:
        raise ValueError("sort_eig: eig is fp32 [N, K >= 3] with unit column stride")
    N = eig.shape[0]
    if coord.dim() != 2 or tuple(coord.shape) != (N, 2) or coord.device != dev:
        raise ValueError("sort_eig: coord is [N, 2] on eig's device")
    sizes_t = torch.as_tensor(sizes, dtype=torch.int64).flatten()
    G = sizes_t.numel()
    if G == 0 or N == 0:
        return eig
    graph_off = _offsets(sizes_t).to(dev, non_blocking=True)
    xy = coord.to(torch.float32).t().contiguous()                               # [2, N]: x row, y row
    _lib.check(_lib.load().dgn_superpixel_sort_eig(eig.data_ptr(), eig.stride(0), eig.shape[1], xy[0].data_ptr(), xy[1].data_ptr(), N,
                                                   graph_off.data_ptr(), G, _lib.stream_ptr(dev)), "dgn_superpixel_sort_eig")
    return eig


def superpixel_eig(graph, coord: torch.Tensor, sizes, coord_eig: bool = False, k: int = 7) -> torch.Tensor:
    """``[N, k]`` fp32 (``[N, 3]`` with ``coord_eig``): what the reference's ``get_eig`` leaves in ``g.ndata['eig']``
    (data/superpixels.py:154-159).  ``coord_eig=True``: ``coord_encoding``.  ``False``: ``batch_eig(graph, sizes, k=k, norm='sym')`` -- the
    ``positional_encoding`` of :346-368 -- followed by ``sort_eig``.  ``batch_eig`` solves the Laplacian of the SYMMETRISED adjacency
    ``(A + A^T) / 2`` of the directed k-NN graph (the reference takes the real part of a non-symmetric ARPACK solve there)."""
    if coord_eig:
        return coord_encoding(coord)
    from .eig import batch_eig
    eig, _ = batch_eig(graph, sizes, k=k, norm="sym")
    return sort_eig(eig, coord, sizes)
