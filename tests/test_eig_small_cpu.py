"""The small-graph eigensolver's host side, without a GPU: argument validation of ``dgn_eig_small`` (nothing touches the device before it),
``eig_multiplicity`` on hand-made tables, ``positional_encoding``'s slicing, and the g14 fixture's own consistency."""
import ctypes as C

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from dgn_amd import _lib
    return _lib.load()


def test_eig_small_validates_before_any_device_work(lib):
    from dgn_amd import _lib
    err = lambda: lib.dgn_last_error().decode()
    a = 1 << 12                                                  # dummy non-null pointer, never dereferenced
    g = _lib.DgnGraph()
    g.n_nodes, g.n_edges = 10, 20
    call = lambda graph=C.byref(g), off=a, G=3, k=6, norm=0, sweeps=30, vec=a, val=a, status=a: \
        lib.dgn_eig_small(graph, off, G, k, norm, sweeps, vec, val, status, None)
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
    assert call(G=0, val=None) == 0                              # no graphs: nothing to do, the eigenvalues are optional
    assert call(G=0, k=0) == -1                                  # (the arguments are still checked)


def test_eig_small_max_nodes(lib):
    assert lib.dgn_eig_small_max_nodes() == 64


def test_eig_multiplicity():
    from dgn_amd import eig_multiplicity
    nan = float("nan")
    v = torch.tensor([[0.0, 1.0, 1.25, 9.0],                      # a gap of exactly 0.25 (exact in binary)
                      [0.0, 1.0, 1.5, 9.0],                       # distinct
                      [0.0, 1.0, 1.0, 9.0],                       # a double eigenvalue
                      [0.0, 1.0, nan, nan],                       # a 2-node graph: NaN slots count as not distinct
                      [0.0, 2.0, 1.0, 9.0]], dtype=torch.float64)      # |.|: the order of the two does not matter
    assert eig_multiplicity(v, tol=0.25) == (2 / 5, 2, 5)         # strictly greater than tol, as multiplicity_eig.py:53
    assert eig_multiplicity(v) == (3 / 5, 3, 5)                   # the defaults: first=1, second=2, tol=1e-3
    assert eig_multiplicity(v, first=0, second=3) == (4 / 5, 4, 5)
    assert eig_multiplicity(v[:, :2], first=0, second=1, tol=1.5) == (1 / 5, 1, 5)
    assert eig_multiplicity(torch.zeros(0, 4, dtype=torch.float64)) == (0.0, 0, 0)
    assert eig_multiplicity(v.float(), tol=0.25)[1:] == (2, 5)    # any float dtype, CPU tensors


def test_positional_encoding_slices_batch_eig(monkeypatch):
    from dgn_amd import eig as E
    seen = {}

    def fake(graph, sizes=None, k=6, norm="none", check=True):
        seen.update(graph=graph, sizes=sizes, k=k, norm=norm, check=check)
        return torch.arange(7 * k, dtype=torch.float32).reshape(7, k), torch.zeros(2, k, dtype=torch.float64)

    monkeypatch.setattr(E, "batch_eig", fake)
    pe = E.positional_encoding("G", [3, 4], 4)
    assert seen == dict(graph="G", sizes=[3, 4], k=5, norm="sym", check=True)
    assert pe.shape == (7, 4) and torch.equal(pe, torch.arange(35, dtype=torch.float32).reshape(7, 5)[:, 1:])


def test_python_side_rejects_bad_arguments():
    from dgn_amd import eig as E
    with pytest.raises(ValueError):
        E.batch_eig(object(), [3], 4, norm="rw")
    with pytest.raises(ValueError):
        E.laplacian_eig_small(object(), torch.zeros(2, dtype=torch.int64), 4, norm="rw")


def test_g14_fixture_is_self_consistent(golden):
    g = golden("g14_pos_enc")
    k = int(g["pos_enc_dim"])
    assert int(g["n_graphs"]) == 5
    for i in range(5):
        n, L, w, pe = int(g[f"g{i}/n"]), g[f"g{i}/L"], g[f"g{i}/eigval"], g[f"g{i}/pos_enc"].astype(np.float64)
        assert 5 <= n <= 40 and L.shape == (n, n) and w.shape == (n,) and pe.shape == (n, k) and g[f"g{i}/pos_enc"].dtype == np.float32
        src, dst = g[f"g{i}/src"], g[f"g{i}/dst"]
        assert sorted(zip(src.tolist(), dst.tolist())) == sorted(zip(dst.tolist(), src.tolist()))      # symmetric edge list
        np.testing.assert_allclose(L, L.T, atol=0)
        np.testing.assert_allclose(w, np.sort(np.linalg.eigvalsh(L)), atol=1e-12)
        assert abs(w[0]) < 1e-12 and w[1] > 1e-6                                                       # connected
        for c in range(k):                                                                             # stored fp32 columns: L v = lambda v
            np.testing.assert_allclose(L @ pe[:, c], w[c + 1] * pe[:, c], atol=1e-6)
