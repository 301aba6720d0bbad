"""Laplacian eigenvectors of a batch of graphs on the GPU, and the eigenvector augmentations of the training loops
(SURVEY.md section 8(f) rank 3).

The reference computes ``g.ndata['eig']`` per graph on the CPU at dataset-load time: ``L = D - A`` (or the sym / walk
normalisation) and the k eigenvectors of smallest eigenvalue by ARPACK with ``tol=5e-1`` and a random start vector
(realworld_benchmark/data/molecules.py:100-116, data/PCBA.py:23-78, data/HIV.py likewise) -- minutes for a dataset,
and neither signs nor degenerate subspaces are reproducible.  Here a whole batch is one batched dense symmetric
eigendecomposition on the GPU (``torch.linalg.eigh`` -> rocSOLVER): graphs are bucketed by size, each Laplacian is
padded to the bucket's width with a large diagonal (the padding eigenpairs sort last and, L being block diagonal,
never mix with the graph's), and the k lowest eigenvectors are scattered back to ``[N, k]`` in node order.  Exact
eigenvectors instead of ARPACK's loosely converged ones: same subspaces, signs arbitrary (the training loops flip
them at random anyway, train_molecules_graph_regression.py:29-33).

Scope: graphs given with a symmetric edge list (molecules, SBMs); for a directed graph the symmetrised adjacency
``(A + A^T)/2`` is used (the reference takes the real part of a non-symmetric ARPACK solve there).  Giant single
graphs (config 5: 10 M nodes) cannot be densified: ``lobpcg_eigvecs`` finds the k lowest eigenpairs with a block
LOBPCG iteration whose only large operation is ``L X`` for a thin block ``X [N, m]`` -- evaluated by the aggregation
sweep itself (``A X`` is the ``sum`` aggregator of the block's rows, ``A^T X`` its backward), so the solver runs at the
sweep's HBM rate and needs no sparse-matrix library.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import _lib

_PAD = 1.0e4      # diagonal of the padding rows: far above any Laplacian eigenvalue (<= 2 * max degree)


def laplacian_eigvecs(src: torch.Tensor, dst: torch.Tensor, sizes: Sequence[int], k: int, norm: str = "none",
                      bucket: int = 8) -> torch.Tensor:
    """``[N, k]`` fp32: column j is the eigenvector of the j-th smallest eigenvalue of every graph's Laplacian (what
    ``get_eig(pos_enc_dim=k)`` stores, molecules.py:100-116); graphs with fewer than k nodes get zero columns.
    ``src``/``dst``: edges of the batched graph (global node ids, graphs occupy consecutive ranges ``sizes``)."""
    return _bucketed_eigh(src, dst, sizes, k, norm, bucket)[0]


def _bucketed_eigh(src: torch.Tensor, dst: torch.Tensor, sizes: Sequence[int], k: int, norm: str = "none", bucket: int = 8):
    """``laplacian_eigvecs`` and the eigenvalues of the same ``eigh`` calls: ``(eig [N, k] fp32, values [G, k] fp64, NaN
    beyond a graph's size)``."""
    if norm not in ("none", "sym", "walk"):
        raise ValueError(norm)
    dev = src.device
    sizes_t = torch.as_tensor(list(sizes), dtype=torch.long, device=dev)
    G, N = sizes_t.numel(), int(sizes_t.sum().item())
    vals = torch.full((G, k), float("nan"), dtype=torch.float64, device=dev)
    off = torch.zeros(G + 1, dtype=torch.long, device=dev)
    off[1:] = torch.cumsum(sizes_t, 0)
    gid = torch.repeat_interleave(torch.arange(G, device=dev), sizes_t)            # node -> graph
    loc = torch.arange(N, device=dev) - off[gid]                                    # node -> index inside its graph
    src, dst = src.long(), dst.long()
    deg = torch.bincount(dst, minlength=N).double().clamp_(min=1.0)                 # in-degrees, clipped like :104
    out = torch.zeros(N, k, dtype=torch.float32, device=dev)
    width = ((sizes_t + bucket - 1) // bucket) * bucket                              # bucket width of every graph
    for w in torch.unique(width).tolist():
        if w == 0:
            continue
        sel = torch.nonzero(width == w).flatten()                                    # graphs of this bucket
        slot = torch.full((G,), -1, dtype=torch.long, device=dev)
        slot[sel] = torch.arange(sel.numel(), device=dev)
        L = torch.zeros(sel.numel(), w, w, dtype=torch.float64, device=dev)
        e_ok = slot[gid[dst]] >= 0
        b, i, j = slot[gid[dst[e_ok]]], loc[dst[e_ok]], loc[src[e_ok]]
        a = torch.ones(b.numel(), dtype=torch.float64, device=dev)
        if norm == "sym":                                                           # I - D^-1/2 A D^-1/2   (:106-108)
            a = a / torch.sqrt(deg[dst[e_ok]] * deg[src[e_ok]])
        elif norm == "walk":                                                        # I - D^-1 A has the eigenvalues of the sym form,
            a = a / torch.sqrt(deg[dst[e_ok]] * deg[src[e_ok]])                     # eigenvectors D^-1/2 v (applied below)   (:109-111)
        L.index_put_((b, i, j), -0.5 * a, accumulate=True)                          # symmetrised adjacency
        L.index_put_((b, j, i), -0.5 * a, accumulate=True)
        n_ok = slot[gid] >= 0
        nb, ni = slot[gid[n_ok]], loc[n_ok]
        diag = deg[n_ok] if norm == "none" else torch.ones_like(deg[n_ok])
        L[nb, ni, ni] += diag
        pad = torch.arange(w, device=dev).unsqueeze(0) >= sizes_t[sel].unsqueeze(1)  # [g, w] padding positions
        L[:, torch.arange(w), torch.arange(w)] += pad.double() * _PAD
        lam, vec = torch.linalg.eigh(L)                                              # ascending eigenvalues
        kk = min(k, w)
        v = vec[:, :, :kk]                                                           # [g, w, kk]
        if norm == "walk":
            dpad = torch.ones(sel.numel(), w, dtype=torch.float64, device=dev)
            dpad[nb, ni] = deg[n_ok]
            v = v / torch.sqrt(dpad).unsqueeze(-1)
            v = v / v.norm(dim=1, keepdim=True).clamp_min(1e-30)
        valid = (torch.arange(kk, device=dev).unsqueeze(0) < sizes_t[sel].unsqueeze(1)).unsqueeze(1)   # fewer nodes than k
        v = torch.where(valid, v, torch.zeros_like(v))
        out[n_ok, :kk] = v[nb, ni].float()
        vals[sel, :kk] = torch.where(valid.squeeze(1), lam[:, :kk], torch.full_like(lam[:, :kk], float("nan")))
    return out, vals


# ---- graphs up to 192 nodes: one Jacobi workgroup per graph (csrc/dgn_eig_small.hip, csrc/dgn_eig_mid.hip) -----------------------

_NORMS = {"none": _lib.DGN_EIG_NORM_NONE, "sym": _lib.DGN_EIG_NORM_SYM, "walk": _lib.DGN_EIG_NORM_WALK}
_SMALL_MAX, _MID_MAX = 64, 192                   # dgn_eig_small_max_nodes(), dgn_eig_mid_max_nodes()


def _eig_buffers(who: str, graph, graph_offsets: torch.Tensor, k: int, out, values, status):
    """The checked ``(out [N, k] fp32, values [G, k] fp64, status [G] int32)`` of a thin launch: made here as zeros / NaN / 0 where not passed."""
    dev = graph.device
    if graph_offsets.dtype != torch.int64 or graph_offsets.device != dev or not graph_offsets.is_contiguous() or graph_offsets.dim() != 1:
        raise ValueError("graph_offsets: a contiguous int64 [G + 1] tensor on the graph's device")
    G, N = graph_offsets.numel() - 1, graph.num_nodes
    if out is None:
        out = torch.zeros(N, k, dtype=torch.float32, device=dev)
    if values is None:
        values = torch.full((G, k), float("nan"), dtype=torch.float64, device=dev)
    if status is None:
        status = torch.zeros(G, dtype=torch.int32, device=dev)
    for t, shape, dt in ((out, (N, k), torch.float32), (values, (G, k), torch.float64), (status, (G,), torch.int32)):
        if tuple(t.shape) != shape or t.dtype != dt or t.device != dev or not t.is_contiguous():
            raise ValueError(f"{who}: a buffer is not a contiguous {dt} {shape} tensor on {dev}")
    return out, values, status


def laplacian_eig_small(graph, graph_offsets: torch.Tensor, k: int, norm: str = "none", *, out: Optional[torch.Tensor] = None,
                        values: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None, max_sweeps: int = 30):
    """The thin launch of ``dgn_eig_small``: the ``k`` lowest Laplacian eigenpairs of every graph of at most 64 nodes, one
    workgroup per graph, nothing read back (usable under ``torch.cuda.graph``).  ``graph``: a ``DGNGraph`` of the batch;
    ``graph_offsets``: device int64 ``[G + 1]`` node offsets.  Returns ``(vec [N, k] fp32, values [G, k] fp64, status [G]
    int32)``: ``status`` is the number of Jacobi sweeps, ``-1`` for a graph of more than 64 nodes, ``-2`` for one with an
    edge from outside its node range -- the rows of such graphs keep what ``out`` / ``values`` held (zeros / NaN when the
    buffers are made here)."""
    import ctypes as C
    if norm not in _NORMS:
        raise ValueError(norm)
    out, values, status = _eig_buffers("laplacian_eig_small", graph, graph_offsets, k, out, values, status)
    dev, G = graph.device, graph_offsets.numel() - 1
    _lib.check(_lib.load().dgn_eig_small(C.byref(graph.c_graph), graph_offsets.data_ptr(), G, int(k), _NORMS[norm], int(max_sweeps),
                                         out.data_ptr(), values.data_ptr(), status.data_ptr(), _lib.stream_ptr(dev)), "dgn_eig_small")
    return out, values, status


def laplacian_eig_mid(graph, graph_offsets: torch.Tensor, k: int, norm: str = "none", *, graph_ids: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None, values: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None,
                      workspace: Optional[torch.Tensor] = None, max_sweeps: int = 30):
    """The thin launch of ``dgn_eig_mid`` (csrc/dgn_eig_mid.hip): the ``k`` lowest Laplacian eigenpairs of every graph of 65 to 192 nodes,
    one workgroup per graph, nothing read back (usable under ``torch.cuda.graph`` when ``workspace`` is preallocated).  Arguments and
    returns as ``laplacian_eig_small``; a graph of at most 64 nodes is not touched (``status`` 0 when the buffer is made here), one of more
    than 192 gets ``-1``.  Called after ``laplacian_eig_small`` on the same ``out`` / ``values`` / ``status`` the two cover every graph up to
    192 nodes: the small call's ``-1`` is overwritten.  ``graph_ids``: device int32 indices of the graphs to solve, one workgroup and one
    log slot each (default: every graph).  ``workspace``: a uint8 tensor of ``dgn_eig_mid_workspace_bytes(slots, max_sweeps)`` bytes --
    ``max_sweeps * 146 688`` per slot -- made here when none is passed."""
    import ctypes as C
    if norm not in _NORMS:
        raise ValueError(norm)
    out, values, status = _eig_buffers("laplacian_eig_mid", graph, graph_offsets, k, out, values, status)
    dev, G = graph.device, graph_offsets.numel() - 1
    n_ids = 0
    if graph_ids is not None:
        if graph_ids.dtype != torch.int32 or graph_ids.device != dev or not graph_ids.is_contiguous() or graph_ids.dim() != 1:
            raise ValueError("graph_ids: a contiguous int32 [n_ids] tensor on the graph's device")
        n_ids = graph_ids.numel()
    lib = _lib.load()
    slots = n_ids if graph_ids is not None else G
    if workspace is None:
        workspace = torch.empty(max(int(lib.dgn_eig_mid_workspace_bytes(slots, int(max_sweeps))), 1), dtype=torch.uint8, device=dev)
    if workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError(f"laplacian_eig_mid: workspace is not a contiguous uint8 tensor on {dev}")
    _lib.check(lib.dgn_eig_mid(C.byref(graph.c_graph), graph_offsets.data_ptr(), G, graph_ids.data_ptr() if graph_ids is not None else None,
                               n_ids, int(k), _NORMS[norm], int(max_sweeps), out.data_ptr(), values.data_ptr(), status.data_ptr(),
                               workspace.data_ptr(), workspace.numel(), _lib.stream_ptr(dev)), "dgn_eig_mid")
    return out, values, status


def _eigh_fallback(graph, off: torch.Tensor, big, k: int, norm: str, eig: torch.Tensor, values: torch.Tensor) -> None:
    """Fill the rows and eigenvalues of the graphs ``big`` (those no Jacobi kernel solved) from the bucketed ``eigh`` on their sub-batch."""
    dev = graph.device
    G = off.numel() - 1
    sizes = off[1:] - off[:-1]
    pick = torch.zeros(G, dtype=torch.bool)
    pick[big] = True
    keep = torch.repeat_interleave(pick, sizes).to(dev)                               # node -> belongs to a big graph
    new_id = torch.cumsum(keep, 0) - 1
    dst = torch.repeat_interleave(torch.arange(graph.num_nodes, device=dev), (graph.indptr[1:] - graph.indptr[:-1]).long())
    src = graph.src.long()[:dst.numel()]
    m = keep[dst]
    v, lam = _bucketed_eigh(new_id[src[m]], new_id[dst[m]], sizes[big].tolist(), k, norm)
    eig[keep] = v
    values[torch.as_tensor(big, device=dev)] = lam


def batch_eig(graph, sizes=None, k: int = 6, norm: str = "none", check: bool = True, *, max_sweeps: int = 30, mid: Optional[bool] = None):
    """``(eig [N, k] fp32, values [G, k] fp64)``: the k lowest Laplacian eigenvectors of every graph of a batch -- what
    ``get_eig`` stores in ``g.ndata['eig']`` (data/molecules.py:100-116) -- and their eigenvalues (``get_eig_val``,
    data/multiplicity_eig.py:14-27).  ``graph``: a ``DGNGraph`` or anything ``as_dgn_graph`` accepts; ``sizes``: the graphs'
    node counts (host list or tensor; default: the graph's ``batch_num_nodes``).  Graphs of at most 64 nodes are solved by
    ``dgn_eig_small`` in one launch pair.  ``mid`` (default: as ``check``): the graphs of 65 to 192 nodes, picked from the host
    ``sizes``, are solved by ``dgn_eig_mid`` in a second launch pair over exactly those, with a log workspace of
    ``max_sweeps * 146 688`` bytes per such graph that is freed afterwards.  ``check=True`` reads the statuses back once: an edge
    from outside a graph's node range or a solve that did not converge raises, graphs no kernel solved (more than 192 nodes;
    more than 64 with ``mid=False``) go through ``laplacian_eigvecs``.  ``check=False`` reads nothing back: the rows of unsolved
    graphs stay zero, their eigenvalues NaN."""
    from .graph import DGNGraph, as_dgn_graph
    if norm not in _NORMS:
        raise ValueError(norm)
    if not isinstance(graph, DGNGraph):
        if sizes is None:
            sizes = getattr(graph, "batch_num_nodes", None)
        graph = as_dgn_graph(graph)
    if sizes is None:
        sizes = getattr(graph, "batch_num_nodes", None)
    if callable(sizes):
        sizes = sizes()
    if sizes is None:
        raise ValueError("batch_eig: pass the graphs' sizes (the graph carries no batch_num_nodes)")
    sizes_t = torch.as_tensor(sizes, dtype=torch.int64).flatten()
    off = torch.zeros(sizes_t.numel() + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(sizes_t, 0)
    if int(off[-1]) != graph.num_nodes:
        raise ValueError(f"batch_eig: the sizes add up to {int(off[-1])} nodes, the graph has {graph.num_nodes}")
    off_dev = off.to(graph.device)
    eig, values, status = laplacian_eig_small(graph, off_dev, k, norm, max_sweeps=max_sweeps)
    if check if mid is None else mid:
        ids = torch.nonzero((sizes_t > _SMALL_MAX) & (sizes_t <= _MID_MAX)).flatten().to(torch.int32)      # host sizes: no read-back
        if ids.numel():
            laplacian_eig_mid(graph, off_dev, k, norm, graph_ids=ids.to(graph.device), out=eig, values=values, status=status,
                              max_sweeps=max_sweeps)
    if not check:
        return eig, values
    st = status.cpu()
    bad = torch.nonzero(st == -2).flatten().tolist()
    if bad:
        raise _lib.DgnError(f"batch_eig: graph {bad[0]} has an edge whose source lies outside its node range"
                            + (f" (and {len(bad) - 1} more graphs)" if len(bad) > 1 else ""))
    slow = torch.nonzero(st >= max_sweeps).flatten().tolist()
    if slow:
        raise _lib.DgnError(f"batch_eig: the Jacobi solve of graph {slow[0]} did not converge in {max_sweeps} sweeps (max_sweeps= raises the cap)")
    big = torch.nonzero(st == -1).flatten().tolist()
    if big:
        _eigh_fallback(graph, off, big, k, norm, eig, values)
    return eig, values


def positional_encoding(graph, sizes=None, pos_enc_dim: int = 2) -> torch.Tensor:
    """``[N, pos_enc_dim]`` fp32: eigenvectors 1 .. pos_enc_dim of the symmetric normalised Laplacian, the reference's
    ``positional_encoding`` (data/molecules.py:18-32; its ``pos_enc`` of :118-121 is the same slice of ``eig``)."""
    return batch_eig(graph, sizes, k=pos_enc_dim + 1, norm="sym")[0][:, 1:]


def eig_multiplicity(values: torch.Tensor, first: int = 1, second: int = 2, tol: float = 1e-3):
    """``(fraction, count, n)``: the graphs whose eigenvalues ``first`` and ``second`` differ by more than ``tol`` -- the
    reference's check that a direction is well defined on a dataset (data/multiplicity_eig.py:52-55).  ``values``: ``[G, k]``
    as ``batch_eig`` returns it; a NaN slot (fewer nodes than eigenvalues asked for) counts as not distinct.  Pure torch."""
    n = int(values.shape[0])
    if n == 0:
        return 0.0, 0, 0
    count = int((torch.abs(values[:, first] - values[:, second]) > tol).sum())      # (NaN > tol is False)
    return count / n, count, n


# ---- iterative solver for graphs that cannot be densified ---------------------------------------------------------------

def _gram_basis(S: torch.Tensor, rtol: float = 1e-10) -> torch.Tensor:
    """M [c, r] such that Q = S M has orthonormal columns spanning span(S) (eigen-decomposition of the Gram matrix,
    directions below ``rtol`` of the largest dropped: converged residuals make S rank deficient, which a Cholesky /
    Householder factor would turn into infinities).  The columns of S are scaled to unit length first."""
    d = S.norm(dim=0).clamp_min(1e-300)
    G = (S.T @ S) / (d.unsqueeze(0) * d.unsqueeze(1))
    sig, V = torch.linalg.eigh(0.5 * (G + G.T))
    keep = sig > rtol * sig[-1]
    return (V[:, keep] / torch.sqrt(sig[keep]).unsqueeze(0)) / d.unsqueeze(1)


def lobpcg_lowest(matvec, n: int, k: int, diag: Optional[torch.Tensor] = None, block: Optional[int] = None, iters: int = 80,
                  tol: float = 1e-4, device=None, generator: Optional[torch.Generator] = None, x0: Optional[torch.Tensor] = None):
    """The k lowest eigenpairs of a symmetric positive semi-definite operator given as ``matvec(X [n, m]) -> L X``
    (Knyazev's LOBPCG with a Jacobi preconditioner ``diag``; Rayleigh-Ritz on span[X, W, P] in fp64, the basis
    orthonormalised through its Gram matrix so that converged directions drop out instead of breaking the factorisation).
    One ``matvec`` of an m-column block per iteration.  Returns (eigenvalues [k], eigenvectors [n, k] fp64, iterations,
    residual norms [k])."""
    m = block or (k + 4 + (k % 2))
    dev = device or (x0.device if x0 is not None else "cpu")
    if x0 is not None:
        X = x0.double()
    else:
        X = torch.randn(n, m, dtype=torch.float64, device=dev, generator=generator)
        X[:, 0] = 1.0                           # the constant vector spans the null space of a connected graph's L
    m = X.shape[1]
    M0 = _gram_basis(X)
    X = X @ M0
    m = X.shape[1]
    LX = matvec(X)
    P = LP = None
    lam = res = None
    best = None                                                      # (residual, lam, X, iteration) of the best iterate so far
    it = 0
    for it in range(1, iters + 1):
        if it % 10 == 0:
            # L X and L P are carried along as linear combinations of earlier products: refresh them now and then so that
            # rounding does not accumulate (one extra product every ten iterations)
            X = X @ _gram_basis(X)
            LX = matvec(X)
            P = LP = None
        lam, C = torch.linalg.eigh(X.T @ LX)                        # Rayleigh-Ritz inside span(X): X becomes the Ritz vectors
        X, LX = X @ C, LX @ C
        R = LX - X * lam.unsqueeze(0)
        res = R.norm(dim=0)
        scale = max(float(lam.abs().max()), 1e-12)
        worst = float(res[:k].max())
        if best is None or worst < best[0]:
            best = (worst, lam[:k].clone(), X[:, :k].clone(), it, res[:k].clone())
        if worst <= tol * scale:
            break
        if it - best[3] >= 15:                                       # stagnation at the rounding floor of the products
            break
        W = R / diag.unsqueeze(1) if diag is not None else R
        W = W - X @ (X.T @ W)                                        # keep the search directions out of span(X)
        live = W.norm(dim=0) > 1e-14 * scale                         # (converged columns contribute no direction)
        W = W[:, live]
        if W.shape[1] == 0:
            break
        LW = matvec(W)
        S = torch.cat([X, W] + ([P] if P is not None else []), dim=1)
        LS = torch.cat([LX, LW] + ([LP] if P is not None else []), dim=1)
        M = _gram_basis(S)                                           # [cols(S), r]
        T = M.T @ (S.T @ LS) @ M
        _, Cq = torch.linalg.eigh(0.5 * (T + T.T))
        Y = M @ Cq[:, :m]                                            # new X = S Y
        Xn, LXn = S @ Y, LS @ Y
        # implicit conjugate direction: the part of the new X that does not come from the old X
        P, LP = S[:, m:] @ Y[m:], LS[:, m:] @ Y[m:]
        pn = P.norm(dim=0)
        ok = pn > 1e-14
        P, LP = P[:, ok] / pn[ok], LP[:, ok] / pn[ok]
        if P.shape[1] == 0:
            P = LP = None
        X, LX = Xn, LXn
    return best[1], best[2], it, best[4]


def sweep_laplacian_matvec(graph, norm: str = "none", symmetric: bool = False):
    """``X [N, m] fp64 -> L X`` for the graph's Laplacian, the product evaluated by the aggregation kernels in fp32:
    ``(A X)[i] = sum over in-edges of X[src]`` is the ``sum`` aggregator (dgn_agg_forward), ``A^T X`` its backward
    (dgn_agg_backward with the block as upstream gradient); L = D - (A + A^T)/2 with the in-degrees clipped to 1
    (molecules.py:104-105), or I - D^-1/2 (A + A^T)/2 D^-1/2 for ``norm='sym'`` (:106-108).  ``symmetric=True`` skips
    the transposed product (undirected graphs stored as symmetric edge lists).  Returns (matvec, diag(L))."""
    from .ops import launch_backward, launch_forward
    from .spec import make_plan
    if norm not in ("none", "sym"):
        raise ValueError(norm)
    plan = make_plan(["sum"], ["identity"])
    N, dev = graph.num_nodes, graph.device
    deg = graph.in_degree.to(torch.float64).clamp(min=1.0)
    dinv = deg.rsqrt() if norm == "sym" else None

    def adj(X32):
        out = torch.empty_like(X32)
        launch_forward(graph, plan, 1, 1.0, None, X32, None, None, None, out)
        if symmetric:
            return out
        gt = torch.empty_like(X32)
        launch_backward(graph, plan, 1, 1.0, None, X32, None, None, None, X32, gt, None, None, None, accumulate=False)
        return 0.5 * (out + gt)

    def matvec(X):
        pad = X.shape[1] % 2                                          # (even widths: 8-byte lanes, atomic-free scatter)
        Z = X * dinv.unsqueeze(1) if dinv is not None else X
        Z32 = Z.float()
        if pad:
            Z32 = torch.nn.functional.pad(Z32, (0, 1))
        AZ = adj(Z32.contiguous())[:, :X.shape[1]].double()
        if dinv is not None:
            return X - AZ * dinv.unsqueeze(1)
        return X * deg.unsqueeze(1) - AZ

    diag = torch.ones_like(deg) if norm == "sym" else deg
    return matvec, diag


def lobpcg_eigvecs(graph, k: int, norm: str = "none", symmetric: bool = False, iters: int = 80, tol: float = 1e-3,
                   generator: Optional[torch.Generator] = None):
    """``[N, k]`` fp32 eigenvectors of the k smallest Laplacian eigenvalues of ONE (large) graph given as a ``DGNGraph``
    -- what ``get_eig`` (molecules.py:100-116) would store in ``g.ndata['eig']`` -- plus (eigenvalues, iterations, residuals).
    The reference's ARPACK call stops at ``tol=5e-1``; ``tol`` here is the relative residual ``||L x - lambda x|| / lambda_max``."""
    matvec, diag = sweep_laplacian_matvec(graph, norm, symmetric)
    lam, X, it, res = lobpcg_lowest(matvec, graph.num_nodes, k, diag=diag, iters=iters, tol=tol, device=graph.device,
                                    generator=generator)
    return X.float(), lam, it, res


# ---- augmentations of the training loops (train/train_superpixels_graph_classification.py:29-48) -------------------

def flip_sign(eig: torch.Tensor, col: Optional[int] = None, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """Random +-1 per ENTRY (as the reference draws it: ``torch.rand(eig.size())``), on one column or on all
    (train_superpixels...:39-43, train_molecules_graph_regression.py:29-33)."""
    tgt = eig if col is None else eig[:, col]
    sign = torch.where(torch.rand(tgt.shape, device=eig.device, generator=generator) >= 0.5, 1.0, -1.0).to(eig.dtype)
    out = eig.clone()
    if col is None:
        return out * sign
    out[:, col] = tgt * sign
    return out


def distort(eig: torch.Tensor, distortion: float, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """Per-node random offset of the (eig1, eig2) pair, scaled by the batch mean of |column| (train_superpixels...:43-47):
    ``eig[:, c] += dist * mean(|eig[:, c]|)`` with ONE ``dist ~ U(-distortion, distortion)`` per node for both columns.
    (The reference's line for column 2 adds the whole ``[N, K]`` tensor instead of column 2 -- a shape error unless
    ``N == K``; the evident intent, the same formula as for column 1, is what is implemented.)"""
    dist = (torch.rand(eig.shape[0], device=eig.device, generator=generator) - 0.5) * 2 * distortion
    out = eig.clone()
    out[:, 1] = dist * eig[:, 1].abs().mean() + eig[:, 1]
    out[:, 2] = dist * eig[:, 2].abs().mean() + eig[:, 2]
    return out


def rotate(eig: torch.Tensor, augmentation_deg: float, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """Per-node random rotation of the (eig1, eig2) pair by up to +-augmentation degrees (train_superpixels...:29-37)."""
    angle = (torch.rand(eig.shape[0], device=eig.device, generator=generator) - 0.5) * 2 * augmentation_deg
    sine = torch.sin(angle * math.pi / 180)
    cos = (1 - sine ** 2) ** 0.5
    out = eig.clone()
    out[:, 1] = cos * eig[:, 1] + sine * eig[:, 2]
    out[:, 2] = cos * eig[:, 2] - sine * eig[:, 1]
    return out


# ---- the same augmentations as one kernel with a device-resident random stream (csrc/dgn_eig_augment.hip) -------------------------

def _flip_mask(flip) -> int:
    """``flip`` of ``EigAugment`` -> the kernel's column mask (bit j = column j): None -> 0, "all" -> every column, a column index, or a
    sequence of column indices."""
    if flip is None:
        return 0
    if isinstance(flip, str):
        if flip != "all":
            raise ValueError(f"EigAugment: flip must be None, 'all', a column index or a sequence of column indices, got '{flip}'")
        return 0xFFFFFFFF
    if isinstance(flip, bool):
        raise TypeError("EigAugment: flip takes column indices, not a bool (flip='all' for the molecule loop's --flip, "
                        "EigAugment.superpixels(augmentation, flip) for the superpixel loop's)")
    cols = [flip] if isinstance(flip, int) else list(flip)
    mask = 0
    for c in cols:
        if isinstance(c, bool) or not isinstance(c, int):
            raise TypeError(f"EigAugment: a flip column must be an int, got {c!r}")
        if not 0 <= c < 32:
            raise ValueError(f"EigAugment: flip column {c} outside 0 .. 31")
        mask |= 1 << c
    return mask


class EigAugment:
    """The eigenvector augmentations of the reference's training loops as ONE kernel launch (``ops.eig_augment``) that draws from a random
    stream kept on the device, so it can sit inside a captured step (``hipgraph.Captured*Step(..., augment=...)``) and draw new values on
    every replay:

    * ``EigAugment.molecules()``: a random sign per ENTRY of ``eig`` (train/train_molecules_graph_regression.py:29-33, ``--flip``);
    * ``EigAugment.superpixels(augmentation, flip)``: a random per-node rotation of the (eig1, eig2) pair by up to ``augmentation`` degrees,
      then a random sign per node on column 2 (train/train_superpixels_graph_classification.py:29-42).

    ``rotate_deg``: the largest angle, 0 = no rotation (the reference's ``sqrt(1 - sin^2)`` form: it differs from a rotation beyond 90
    degrees, as there); ``flip``: None, ``"all"``, a column index or a sequence of column indices.  The object owns the stream, a device int64
    ``[4]`` tensor ``state = {key, calls, ticket, 0}``: the key is drawn ONCE from torch's generator of the device at construction (so
    ``torch.manual_seed`` before it fixes the run) or taken from ``seed``, and every call -- eager or replayed -- advances ``calls`` by one on
    the device.  Row i of call c draws Philox4x32-10(counter (i, c), key): ``get_state()`` / ``set_state(key, calls)`` are what a checkpoint
    stores to resume with the values the uninterrupted run would have drawn.  Constructing one inside a stream capture raises (the key would
    be drawn by a captured launch into the capture's private pool: every replay the same key).

    ``aug(eig)`` returns a new tensor; ``aug(eig, out=buf)`` writes ``buf`` (``eig`` itself is allowed) and bumps its version counter, so a
    ``DGNGraph`` that cached edge weights for ``buf`` computes them again.

    Not covered: the superpixel loop's ``--distortion`` (its line 48 adds the whole ``[N, K]`` tensor to a column and raises in the reference;
    ``dgn_amd.eig.distort`` ships the evident intent, and that needs a batch-wide mean of |column| -- a reduction, not a per-row kernel)."""

    def __init__(self, rotate_deg: float = 0.0, flip=None, device=None, seed: Optional[int] = None):
        self.rotate_deg = float(rotate_deg)
        if not math.isfinite(self.rotate_deg):
            raise ValueError(f"EigAugment: rotate_deg must be finite, got {rotate_deg}")
        self.flip_mask = _flip_mask(flip)
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 63):
            raise ValueError(f"EigAugment: seed must be an int in [0, 2^63), got {seed!r}")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise _lib.DgnError("EigAugment: CUDA devices only (dgn_amd has no CPU path)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("EigAugment: construct it outside a stream capture (its state would live in the capture's private pool and "
                               "its key be drawn by a captured launch: every replay the same key)")
        self.device = dev
        self.state = torch.zeros(4, dtype=torch.int64, device=dev)
        if seed is None:
            self.state[:1] = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=dev)
        else:
            self.state[0] = seed

    @classmethod
    def molecules(cls, **kw) -> "EigAugment":
        """``--flip`` of the molecule loop: a random sign per entry."""
        return cls(rotate_deg=0.0, flip="all", **kw)

    @classmethod
    def superpixels(cls, augmentation: float = 0.0, flip: bool = False, **kw) -> "EigAugment":
        """``--augmentation`` / ``--flip`` of the superpixel loop: the rotation (off at or below 1e-7 degrees, as there), then the sign of column 2."""
        return cls(rotate_deg=float(augmentation) if augmentation > 1e-7 else 0.0, flip=2 if flip else None, **kw)

    def __call__(self, eig: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        from .ops import eig_augment
        return eig_augment(eig, self.state, self.rotate_deg, self.flip_mask, out=out)

    def get_state(self):
        """``(key, calls so far)`` as Python ints (one read-back)."""
        key, calls = self.state[:2].tolist()
        return key, calls

    def set_state(self, key: int, calls: int = 0) -> None:
        """Continue from ``(key, calls)``: what ``get_state`` returned (a checkpoint), or a chosen point of the stream."""
        key, calls = int(key), int(calls)
        if not (-2 ** 63 <= key < 2 ** 63 and 0 <= calls < 2 ** 63):
            raise ValueError("EigAugment.set_state: key and calls must fit an int64, calls >= 0")
        self.state.copy_(torch.tensor([key, calls, 0, 0], dtype=torch.int64))

    def __repr__(self):
        return f"EigAugment(rotate_deg={self.rotate_deg}, flip_mask={self.flip_mask:#x}, device='{self.device}')"
