"""The 65-192-node eigensolver's host side, without a GPU: the size functions and argument validation of ``dgn_eig_mid`` (nothing touches
the device before it), ``batch_eig``'s routing of the graphs by their host sizes, and the numpy model of the kernel (tests/eig_mid_model.py:
packed storage, tile map, rotation log, backward replay) against the dense oracle with the GPU test's tolerances."""
import ctypes as C

import numpy as np
import pytest
import torch

import eig_mid_model as M

K = 6
ENTRY = 8                                                        # a log entry: the rotation's tangent, fp64


@pytest.fixture(scope="module")
def lib():
    from dgn_amd import _lib
    return _lib.load()


def test_eig_mid_sizes(lib):
    assert lib.dgn_eig_mid_max_nodes() == 192 and lib.dgn_eig_small_max_nodes() == 64
    ws = lib.dgn_eig_mid_workspace_bytes
    assert ws(0, 30) == 0 and ws(3, 0) == 0
    for slots, sweeps in ((1, 1), (3, 30), (128, 30), (41127, 30)):
        assert ws(slots, sweeps) == slots * sweeps * 191 * 96 * ENTRY
        assert ws(slots + 1, sweeps) > ws(slots, sweeps) < ws(slots, sweeps + 1)
    assert ws(128, 30) == 563281920                               # 4.4 MB per graph: 563 MB for 128 graphs at the default cap


def test_eig_mid_validates_before_any_device_work(lib):
    from dgn_amd import _lib
    err = lambda: lib.dgn_last_error().decode()
    a = 1 << 12                                                  # dummy non-null pointer, never dereferenced
    g = _lib.DgnGraph()
    g.n_nodes, g.n_edges = 10, 20
    need = lib.dgn_eig_mid_workspace_bytes(3, 30)
    call = lambda graph=C.byref(g), off=a, G=3, ids=None, n_ids=0, k=6, norm=0, sweeps=30, vec=a, val=a, status=a, ws=a, ws_bytes=need: \
        lib.dgn_eig_mid(graph, off, G, ids, n_ids, k, norm, sweeps, vec, val, status, ws, ws_bytes, None)
    assert call() == -1 and "null CSR" in err()                  # indptr / src missing
    assert call(graph=None) == -1 and "null CSR" in err()
    g.indptr = g.src = a
    assert call(off=None) == -1 and "null" in err()
    assert call(vec=None) == -1 and "null" in err()
    assert call(status=None) == -1 and "null" in err()
    assert call(k=0) == -1 and "k = 0" in err()
    assert call(k=33) == -1 and "k = 33" in err()
    assert call(norm=3) == -1 and "norm" in err()
    assert call(norm=-1) == -1 and "norm" in err()
    assert call(G=-1) == -1 and "n_graphs" in err()
    assert call(sweeps=0) == -1 and "max_sweeps" in err()
    assert call(ids=a, n_ids=-1) == -1 and "n_ids" in err()
    assert call(n_ids=-1) == -1 and "n_ids" in err()             # (checked with or without a list)
    assert call(ws=None) < 0 and "workspace" in err()
    assert call(ws_bytes=need - 1) == -2 and "workspace" in err()      # DGN_ERR_WORKSPACE: the log slots do not hold max_sweeps sweeps
    assert call(ws_bytes=lib.dgn_eig_mid_workspace_bytes(3, 29)) == -2 and "workspace" in err()
    assert call(ids=a, n_ids=4, ws_bytes=need) == -2 and "workspace" in err()      # four listed graphs need four slots
    assert call(G=0, val=None, ws=None, ws_bytes=0) == 0         # no graphs: nothing to do
    assert call(ids=a, n_ids=0, ws=None, ws_bytes=0) == 0        # an empty list: nothing to do
    assert call(G=0, k=0) == -1                                  # (the arguments are still checked)


def test_python_side_rejects_bad_norm():
    from dgn_amd import eig as E
    with pytest.raises(ValueError):
        E.batch_eig(object(), [3], 4, norm="rw", mid=True)
    with pytest.raises(ValueError):
        E.laplacian_eig_mid(object(), torch.zeros(2, dtype=torch.int64), 4, norm="rw")


def test_batch_eig_routes_by_host_sizes(monkeypatch):
    """Sizes [10, 64, 65, 128, 129, 192, 193]: graphs 2 .. 5 go to the mid launch (one slot each, taken from the host sizes), graph 6 keeps
    -1 and goes to the bucketed eigh; ``mid=False`` or ``check=False`` alone sends none to the mid launch."""
    import dgn_amd
    from dgn_amd import eig as E
    sizes = [10, 64, 65, 128, 129, 192, 193]
    graph = dgn_amd.DGNGraph.__new__(dgn_amd.DGNGraph)
    graph.num_nodes, graph.device = sum(sizes), torch.device("cpu")
    seen = {}

    def small(g, off, k, norm="none", *, max_sweeps=30):
        n = off[1:] - off[:-1]
        seen["off"] = off.tolist()
        return (torch.zeros(int(off[-1]), k), torch.full((n.numel(), k), float("nan"), dtype=torch.float64),
                torch.where(n <= 64, 5, -1).to(torch.int32))

    def mid(g, off, k, norm="none", *, graph_ids=None, out=None, values=None, status=None, workspace=None, max_sweeps=30):
        assert graph_ids.dtype == torch.int32 and workspace is None and out is not None and values is not None
        seen.setdefault("mid", []).append(graph_ids.tolist())
        status[graph_ids.long()] = 7
        return out, values, status

    def fallback(g, off, big, k, norm, eig, values):
        seen["fallback"] = list(big)

    monkeypatch.setattr(E, "laplacian_eig_small", small)
    monkeypatch.setattr(E, "laplacian_eig_mid", mid)
    monkeypatch.setattr(E, "_eigh_fallback", fallback)
    for kw, want_mid, want_fallback in ((dict(), [[2, 3, 4, 5]], [6]),
                                        (dict(mid=True), [[2, 3, 4, 5]], [6]),
                                        (dict(mid=False), None, [2, 3, 4, 5, 6]),
                                        (dict(check=False), None, None),
                                        (dict(check=False, mid=False), None, None),
                                        (dict(check=False, mid=True), [[2, 3, 4, 5]], None)):
        seen.clear()
        E.batch_eig(graph, sizes, K, "sym", **kw)
        assert seen.get("mid") == want_mid and seen.get("fallback") == want_fallback, (kw, seen)
        assert seen["off"] == [0, 10, 74, 139, 267, 396, 588, 781]
    seen.clear()
    E.batch_eig(graph, sizes[:2] + [sum(sizes[2:])], K)          # nothing of 65 .. 192 nodes: no mid launch at all
    assert "mid" not in seen and seen["fallback"] == [2]


def test_tile_map_covers_every_pair_of_pairs_once():
    for npairs in (33, 64, 65, 96):
        P, Q = M.tile_map(npairs)
        assert len({(min(p, q), max(p, q)) for p, q in zip(P.tolist(), Q.tolist())}) == npairs * (npairs - 1) // 2 == P.size
        assert np.all(P != Q)


GRAPHS = dict(M.mid_graphs())


@pytest.mark.parametrize("norm", ["none", "sym"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_model_vs_oracle(name, norm):
    """The kernel's arithmetic in numpy against the dense oracle: eigenvalues 1e-10, residuals of the fp32 columns 5e-5, cluster projectors
    2e-5 (clusters by the 1e-6 rule), 1 <= sweeps < 30 -- the GPU test's limits."""
    from oracle import eig_oracle
    src, dst, n = GRAPHS[name]
    (w, v), = eig_oracle.eigvecs(src, dst, [n], K, norm)
    M.assert_unambiguous_clusters(w, K)
    vec, val, sweeps = M.eig_mid(src, dst, n, K, norm)
    print(f"eig_mid model sweeps: {name} {norm} {sweeps}")
    assert 1 <= sweeps < 30 and (sweeps == 1) == (name == "edgeless70")
    blk = vec.astype(np.float64)
    np.testing.assert_allclose(val, w[:K], rtol=0, atol=1e-10)
    L = eig_oracle.graph_laplacian(src, dst, n, norm)
    for c in range(K):
        np.testing.assert_allclose(L @ blk[:, c], w[c] * blk[:, c], atol=5e-5)
    j = 0
    while j < K:
        e = j + 1
        while e < n and abs(w[e] - w[j]) < 1e-6:
            e += 1
        if e <= K:
            np.testing.assert_allclose(blk[:, j:e] @ blk[:, j:e].T, v[:, j:e] @ v[:, j:e].T, atol=2e-5)
        j = e


def test_model_self_loop_matches_the_square():
    """Packed storage has one cell per {i, j}: a self-loop adds -2w to it, which is what the full square and the oracle's (A + A^T) / 2 hold."""
    from oracle import eig_oracle
    src, dst, n = GRAPHS["loop66"]
    for norm in ("none", "sym"):
        A, _ = M.build_packed(src, dst, n, norm)
        L = eig_oracle.graph_laplacian(src, dst, n, norm)
        i, j = np.tril_indices(n)
        np.testing.assert_allclose(A[M.pidx(i, j)], L[i, j], rtol=0, atol=1e-15)
