"""Superpixel graphs without a GPU: the numpy restatement (tests/superpixels_oracle.py) against fixture G15 -- the unmodified reference's
``compute_adjacency_matrix_images`` / ``compute_edges_list`` / ``sort_eig`` --, the rank gaps of the GPU tests' inputs, the edge counts, the
host-side validation of the two entry points and the refusal to compute on CPU tensors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import superpixels_inputs as spi
import superpixels_oracle as so


@pytest.fixture(scope="module")
def lib():
    from dgn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _graphs(g):
    for i in range(int(g["n_graphs"])):
        C_ = int(g[f"g{i}/channels"])
        yield i, int(g[f"g{i}/n"]), g[f"g{i}/coord"], (g[f"g{i}/feat"] if C_ else None)


def test_adjacency_matches_the_reference(golden):
    """A at rtol 1e-13: the operations and their order are the reference's; only the order of sigma's 9-term sum is its own (np.partition
    leaves it unspecified)."""
    g = golden("g15_superpixels")
    seen = set()
    for i, n, coord, feat in _graphs(g):
        A = so.adjacency(coord, feat)
        ref = g[f"g{i}/A"] if f"g{i}/A" in g.files else g[f"g{i}/A_head"]
        np.testing.assert_allclose(A[:ref.shape[0]], ref, rtol=1e-13, atol=0, err_msg=f"graph {i} ({n} nodes)")
        seen.add((n, 0 if feat is None else feat.shape[1]))
    assert {n for n, _ in seen} == {1, 2, 8, 9, 10, 11, 40, 75, 150} and {c for _, c in seen} == {0, 1, 3}


def test_neighbours_are_ranks_1_to_8_of_the_reference(golden):
    """Every row of the reference's knns, as a set, is ranks 1 .. 8 of the restatement -- the most similar node is left out --, its values
    those of A; fully connected up to 9 nodes, one self-loop for a single node."""
    g = golden("g15_superpixels")
    for i, n, coord, feat in _graphs(g):
        A = so.adjacency(coord, feat)
        dst, val = so.neighbours(A, 8, skip_nearest=True)
        knns, values = g[f"g{i}/knns"], g[f"g{i}/knn_values"]
        assert knns.shape == dst.shape == ((1, 1) if n == 1 else (n, n - 1) if n <= 9 else (n, 8)), i
        assert dst.size == so.edge_count(n)
        for r in range(n):
            assert set(knns[r].tolist()) == set(dst[r].tolist()), (i, r)
            order = np.argsort(knns[r], kind="stable")
            mine = np.argsort(dst[r], kind="stable")
            np.testing.assert_allclose(val[r][mine], values[r][order], rtol=1e-13, atol=0, err_msg=f"graph {i} row {r}")
        if n > 9:
            top = so.ranked(A)[:, 0]
            assert not any(top[r] in knns[r] for r in range(n)), i                  # the nearest node is NOT a neighbour
            plain, _ = so.neighbours(A, 8, skip_nearest=False)
            assert all(plain[r, 0] == top[r] and set(plain[r, 1:]) < set(dst[r]) for r in range(n))
        elif n > 1:
            assert all(dst[r].tolist() == [j for j in range(n) if j != r] for r in range(n))
        else:
            assert dst.tolist() == [[0]] and val.tolist() == [[0.0]]


def test_sort_eig_matches_the_reference_on_every_arm(golden):
    g = golden("g15_superpixels")
    arms = set()
    for i in range(int(g["n_sort"])):
        eig, x, y = g[f"s{i}/eig"], g[f"s{i}/x"], g[f"s{i}/y"]
        arms.add(so.sort_eig_branch(eig, x, y))
        got = so.sort_eig(eig, x, y, [eig.shape[0]])
        assert np.array_equal(got, g[f"s{i}/sorted"]), i
        assert np.array_equal(got[:, 0], eig[:, 0]) and np.array_equal(got[:, 3:], eig[:, 3:])
    assert arms == {0, 1, 2, 3}


@pytest.mark.parametrize("channels", [0, 1, 3])
@pytest.mark.parametrize("k,skip", [(8, True), (8, False), (3, True)])
def test_gpu_test_inputs_have_rank_gaps(channels, k, skip):
    """The GPU tests compare neighbour SETS with no row left out, so no decision of their inputs may hang on the last digits: every
    relative gap between rank 0 and 1 and between the last kept and the first dropped rank is at least 1e-9 (fp64 evaluations of the same
    formula differ by ~1e-14)."""
    coord, feat, sizes = spi.batch(channels)
    off = 0
    for n in sizes:
        A = so.adjacency(coord[off:off + n], None if feat is None else feat[off:off + n], k)
        first, tail = so.rank_gaps(A, k, skip)
        assert first.min() >= 1e-9 and tail.min() >= 1e-9, (n, first.min(), tail.min())
        off += n


def test_edge_counts():
    import dgn_amd
    k = 8
    assert dgn_amd.knn_edge_counts([1, 2, k + 1, k + 2, 150], k).tolist() == [1, 2, (k + 1) * k, (k + 2) * k, 150 * k]
    assert dgn_amd.knn_edge_counts(torch.tensor([1, 2, 4, 5, 150]), 3).tolist() == [1, 2, 12, 15, 450]
    assert [so.edge_count(n, k) for n in (1, 2, k + 1, k + 2, 150)] == [1, 2, (k + 1) * k, (k + 2) * k, 150 * k]
    assert dgn_amd.knn_edge_counts([], k).tolist() == []
    for bad in ([0], [5, 0, 3], [-1]):
        with pytest.raises(ValueError):
            dgn_amd.knn_edge_counts(bad, k)
    with pytest.raises(ValueError):
        dgn_amd.knn_edge_counts([5], 0)
    with pytest.raises(ValueError):
        dgn_amd.knn_edge_counts([5], 33)


def test_knn_graph_validates_before_any_device_work(lib):
    err = lambda: lib.dgn_last_error().decode()
    a = 1 << 12                                                                       # dummy aligned pointer, never dereferenced
    call = lambda coord=a, feat=None, n_feat=0, n_nodes=10, goff=a, eoff=a, G=1, k=8, skip=1, E=80, src=a, dst=a, val=a, st=a: \
        lib.dgn_knn_graph(coord, feat, n_feat, n_nodes, goff, eoff, G, k, skip, E, src, dst, val, st, None)
    assert lib.dgn_knn_graph_max_nodes() == 256
    assert call(k=0) == -1 and "k = 0" in err()
    assert call(k=33) == -1 and "k = 33" in err()
    assert call(feat=a, n_feat=0) == -1 and "n_feat" in err()
    assert call(feat=a, n_feat=9) == -1 and "n_feat" in err()
    assert call(feat=None, n_feat=3) == -1 and "n_feat" in err()
    assert call(skip=2) == -1 and "skip_nearest" in err()
    assert call(G=-1) == -1 and "negative" in err()
    assert call(n_nodes=-1) == -1 and "negative" in err()
    assert call(E=-1) == -1 and "negative" in err()
    for name in ("coord", "goff", "eoff", "src", "dst", "val", "st"):
        assert call(**{name: None}) == -1 and "null" in err(), name
    assert call(G=0) == 0                                                             # no graphs: nothing to do


def test_sort_eig_validates_before_any_device_work(lib):
    err = lambda: lib.dgn_last_error().decode()
    a = 1 << 12
    call = lambda eig=a, ld=7, cols=7, x=a, y=a, n_nodes=10, goff=a, G=1: lib.dgn_superpixel_sort_eig(eig, ld, cols, x, y, n_nodes, goff, G, None)
    assert call(cols=2, ld=2) == -1 and "n_cols = 2" in err()
    assert call(ld=6) == -1 and "ld_eig" in err()
    assert call(G=-1) == -1 and "negative" in err()
    assert call(n_nodes=-1) == -1 and "negative" in err()
    for name in ("eig", "x", "y", "goff"):
        assert call(**{name: None}) == -1 and "null" in err(), name
    assert call(G=0) == 0


def test_no_cpu_fallback():
    import dgn_amd
    coord = torch.rand(12, 2)
    with pytest.raises(dgn_amd._lib.DgnError):
        dgn_amd.knn_graph(coord, [12])
    with pytest.raises(dgn_amd._lib.DgnError):
        dgn_amd.sort_eig(torch.randn(12, 7), coord, [12])
    assert dgn_amd.coord_encoding(coord).shape == (12, 3)                             # (a concatenation: no kernel of the library)
    enc = dgn_amd.coord_encoding(coord)
    assert torch.equal(enc[:, 0], torch.zeros(12)) and torch.equal(enc[:, 1:], coord) and enc.dtype == torch.float32
