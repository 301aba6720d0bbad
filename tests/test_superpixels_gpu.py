"""``dgn_knn_graph`` and ``dgn_superpixel_sort_eig`` on the GPU against the numpy restatement (tests/superpixels_oracle.py, pinned to the
reference by fixture G15 in test_superpixels_cpu.py) and against the fixture itself.

Tolerances.  The kernel and the restatement evaluate the same fp64 formula; they differ in the order of sigma's k + 1 terms and in exp's last
bit, ~1e-14 relative on the values that are kept (1e-13 in the far tail).  Rounded to fp32 that moves a value by at most one ulp; the tests
allow two.  Neighbour SETS are compared with no row left out: test_superpixels_cpu.py asserts that every rank gap of these inputs is at
least 1e-9.  On the regular grid, where distances tie exactly, validity is asserted instead, with an absolute 1e-12 (A <= 1)."""
import functools
import warnings

import numpy as np
import pytest
import torch

import superpixels_inputs as spi
import superpixels_oracle as so

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(a, dtype=dtype).cuda()


def _knn(coord, sizes, feat=None, k=8, skip=True, **kw):
    """knn_graph on numpy inputs -> (src, dst, value) numpy"""
    import dgn_amd
    out = dgn_amd.knn_graph(_dev(coord), sizes, _dev(feat), k=k, skip_nearest=skip, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


@functools.lru_cache(maxsize=None)
def _reference(channels, k, skip):
    coord, feat, sizes = spi.batch(channels)
    return so.knn_graph(coord, sizes, feat, k, skip)


def _ulps(a, b):
    """distance in fp32 ulps of two arrays of non-negative floats"""
    return np.abs(a.astype(np.float32).view(np.int32).astype(np.int64) - b.astype(np.float32).view(np.int32).astype(np.int64))


def _rows(sizes, k):
    """(graph, node offset, edge offset, n, per_node) of every graph"""
    n0 = e0 = 0
    for g, n in enumerate(sizes):
        per = 1 if n == 1 else (n - 1 if n <= k + 1 else k)
        yield g, n0, e0, n, per
        n0, e0 = n0 + n, e0 + n * per


def _check_against(src, dst, val, sizes, k, As, ref_dst):
    """src as specified, per-row neighbour sets == the restatement's, values within 2 fp32 ulps of float32(A_ref), ranked rows non-increasing"""
    assert src.dtype == dst.dtype == np.int64 and val.dtype == np.float32
    assert src.size == sum(so.edge_count(n, k) for n in sizes) == ref_dst.size
    worst = 0
    for g, n0, e0, n, per in _rows(sizes, k):
        s, d, v = (t[e0:e0 + n * per].reshape(n, per) for t in (src, dst, val))
        assert np.array_equal(s, np.repeat(np.arange(n0, n0 + n), per).reshape(n, per)), g
        r = ref_dst[e0:e0 + n * per].reshape(n, per)
        assert np.array_equal(np.sort(d, axis=1), np.sort(r, axis=1)), f"graph {g} ({n} nodes): neighbour sets differ"
        a_ref = np.take_along_axis(As[g], d - n0, axis=1)
        worst = max(worst, int(_ulps(v, a_ref).max()))
        if n >= k + 2:
            assert np.all(v[:, :-1] >= v[:, 1:]), f"graph {g}: a row's values increase"
        elif n > 1:
            assert np.array_equal(d - n0, np.array([[j for j in range(n) if j != i] for i in range(n)])), g
        else:
            assert d[0, 0] == n0 and v[0, 0] == 0.0
    print("largest fp32 ulp distance:", worst)
    assert worst <= 2


@pytest.mark.parametrize("channels", [0, 1, 3])
@pytest.mark.parametrize("k,skip", [(8, True), (8, False), (3, True)])
def test_batch_against_restatement(channels, k, skip):
    coord, feat, sizes = spi.batch(channels)
    _, ref_dst, _, As = _reference(channels, k, skip)
    src, dst, val = _knn(coord, sizes, feat, k, skip)
    _check_against(src, dst, val, sizes, k, As, ref_dst)


def test_fp32_inputs_give_the_same_bits():
    coord, feat, sizes = spi.batch(3)
    import dgn_amd
    a = dgn_amd.knn_graph(_dev(coord), sizes, _dev(feat))
    b = dgn_amd.knn_graph(_dev(coord, torch.float32), sizes, _dev(feat, torch.float32))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_golden_inputs_give_the_reference_neighbours(golden):
    """The fixture's graphs through the device, one batch per channel count: every row's neighbour set is the reference's knns row."""
    g = golden("g15_superpixels")
    by_c = {}
    for i in range(int(g["n_graphs"])):
        by_c.setdefault(int(g[f"g{i}/channels"]), []).append(i)
    assert set(by_c) == {0, 1, 3}
    for c, ids in by_c.items():
        sizes = [int(g[f"g{i}/n"]) for i in ids]
        coord = np.concatenate([g[f"g{i}/coord"] for i in ids])
        feat = np.concatenate([g[f"g{i}/feat"] for i in ids]) if c else None
        src, dst, val = _knn(coord, sizes, feat)
        for (_, n0, e0, n, per), i in zip(_rows(sizes, 8), ids):
            knns, values = g[f"g{i}/knns"], g[f"g{i}/knn_values"]
            d = dst[e0:e0 + n * per].reshape(n, per) - n0
            v = val[e0:e0 + n * per].reshape(n, per)
            assert knns.shape == d.shape, i
            assert np.array_equal(np.sort(d, axis=1), np.sort(knns, axis=1)), f"fixture graph {i} ({n} nodes, {c} channels)"
            mine, theirs = np.argsort(d, axis=1, kind="stable"), np.argsort(knns, axis=1, kind="stable")
            assert _ulps(np.take_along_axis(v, mine, axis=1), np.take_along_axis(values, theirs, axis=1)).max() <= 2, i


@pytest.mark.parametrize("skip", [True, False])
def test_exact_ties_on_a_regular_grid(skip):
    """144 nodes on a 12 x 12 grid: ranks tie exactly, so any valid choice passes -- every kept value >= every value neither kept nor
    dropped, the dropped (most similar) one >= every kept one, each to 1e-12; k distinct neighbours per row, never the node itself."""
    k, tol = 8, 1e-12
    coord = spi.grid(12)
    n = coord.shape[0]
    src, dst, val = _knn(coord, [n], None, k, skip)
    A = so.adjacency(coord, None, k)
    d = dst.reshape(n, k)
    assert np.array_equal(src.reshape(n, k), np.repeat(np.arange(n), k).reshape(n, k))
    assert _ulps(val.reshape(n, k), np.take_along_axis(A, d, axis=1)).max() <= 2
    for i in range(n):
        kept = set(d[i].tolist())
        assert len(kept) == k and i not in kept and all(0 <= j < n for j in kept), i
        rest = np.array([j for j in range(n) if j != i and j not in kept])
        low = A[i, d[i]].min()
        if skip:
            dropped = rest[np.argmax(A[i, rest])]
            assert A[i, dropped] >= A[i, d[i]].max() - tol, i
            rest = rest[rest != dropped]
        assert low >= A[i, rest].max() - tol, i


def test_a_graph_has_the_same_bits_in_any_batch():
    coord, feat, sizes = spi.batch(3)
    off = np.concatenate([[0], np.cumsum(sizes)])
    pick = sizes.index(150)
    c1, f1 = coord[off[pick]:off[pick + 1]], feat[off[pick]:off[pick + 1]]
    _, d_alone, v_alone = _knn(c1, [150], f1)
    others = [g for g in range(len(sizes)) if g != pick]
    co, fo = (np.concatenate([a[off[g]:off[g + 1]] for g in others]) for a in (coord, feat))
    so_sizes = [sizes[g] for g in others]
    _, d_first, v_first = _knn(np.concatenate([c1, co]), [150] + so_sizes, np.concatenate([f1, fo]))
    _, d_last, v_last = _knn(np.concatenate([co, c1]), so_sizes + [150], np.concatenate([fo, f1]))
    E, n_before = 150 * 8, int(sum(so_sizes))
    assert np.array_equal(d_first[:E], d_alone) and np.array_equal(v_first[:E].view(np.int32), v_alone.view(np.int32))
    assert np.array_equal(d_last[-E:] - n_before, d_alone) and np.array_equal(v_last[-E:].view(np.int32), v_alone.view(np.int32))


def test_oversize_graph_in_the_middle_of_a_batch():
    """257 nodes: status -1, its edge range keeps the sentinel, the graphs around it are built; check=True raises and names it, check=False
    reads nothing back."""
    import dgn_amd
    sizes, k = [20, 257, 30], 8
    coord, _ = spi.points(sizes, 0, seed=7)
    counts = dgn_amd.knn_edge_counts(sizes, k).tolist()
    assert counts == [160, 257 * 8, 240]
    E = sum(counts)
    out = (torch.full((E,), -7, dtype=torch.int64, device="cuda"), torch.full((E,), -7, dtype=torch.int64, device="cuda"),
           torch.full((E,), -7.0, dtype=torch.float32, device="cuda"))
    status = torch.full((3,), 5, dtype=torch.int32, device="cuda")
    c = _dev(coord)
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            res = dgn_amd.knn_graph(c, sizes, k=k, check=False, out=out, status=status)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    syncs = [str(w.message) for w in seen if "synchronizing" in str(w.message) and "prototype feature" not in str(w.message)]
    assert not syncs, syncs                                                            # (set_sync_debug_mode itself warns that it is a prototype)
    assert all(a is b for a, b in zip(res, out))
    torch.cuda.synchronize()
    assert status.tolist() == [0, -1, 0]
    src, dst, val = (t.cpu().numpy() for t in out)
    lo, hi = counts[0], counts[0] + counts[1]
    assert np.all(src[lo:hi] == -7) and np.all(dst[lo:hi] == -7) and np.all(val[lo:hi] == -7.0)
    for g, n0, e0 in ((0, 0, 0), (2, 277, hi)):
        n = sizes[g]
        A = so.adjacency(coord[n0:n0 + n], None, k)
        want, _ = so.neighbours(A, k, True)
        got = dst[e0:e0 + n * k].reshape(n, k) - n0
        assert np.array_equal(np.sort(got, axis=1), np.sort(want, axis=1)), g
        assert np.array_equal(src[e0:e0 + n * k], np.repeat(np.arange(n0, n0 + n), k))
        assert _ulps(val[e0:e0 + n * k].reshape(n, k), np.take_along_axis(A, got, axis=1)).max() <= 2
    with pytest.raises(dgn_amd._lib.DgnError, match="graph 1 has more than 256 nodes"):
        dgn_amd.knn_graph(c, sizes, k=k, check=True)


def test_wrong_edge_offsets_are_refused():
    """An `out` whose length is not the rule's edge count (device sizes: E is taken from it): status -2, nothing written."""
    import dgn_amd
    sizes = [12, 40]
    coord, _ = spi.points(sizes, 0, seed=9)
    E = int(dgn_amd.knn_edge_counts(sizes).sum())
    out = (torch.full((E - 8,), -7, dtype=torch.int64, device="cuda"), torch.full((E - 8,), -7, dtype=torch.int64, device="cuda"),
           torch.full((E - 8,), -7.0, dtype=torch.float32, device="cuda"))
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    dgn_amd.knn_graph(_dev(coord), torch.tensor(sizes, device="cuda"), check=False, out=out, status=status)
    torch.cuda.synchronize()
    assert status.tolist() == [0, -2]                                                  # (the last graph's range ends beyond the arrays)
    assert bool((out[1][12 * 8:] == -7).all()) and bool((out[1][:12 * 8] >= 0).all())


def _sort_inputs(sizes, seed, cols=7):
    rng = np.random.default_rng(seed)
    N = int(sum(sizes))
    return rng.standard_normal((N, cols)).astype(np.float32), rng.random((N, 2), dtype=np.float32)


def test_capture_and_replay():
    """knn_graph(check=False) and sort_eig captured on one stream: after the inputs are overwritten the replay gives the eager call's bits."""
    import dgn_amd
    sizes = [85, 150, 12, 100]
    N, E = sum(sizes), int(dgn_amd.knn_edge_counts(sizes).sum())
    sizes_dev = torch.tensor(sizes, device="cuda")
    coord_buf = torch.zeros(N, 2, dtype=torch.float64, device="cuda")
    feat_buf = torch.zeros(N, 3, dtype=torch.float64, device="cuda")
    eig_buf = torch.zeros(N, 7, dtype=torch.float32, device="cuda")
    out = (torch.zeros(E, dtype=torch.int64, device="cuda"), torch.zeros(E, dtype=torch.int64, device="cuda"),
           torch.zeros(E, dtype=torch.float32, device="cuda"))
    status = torch.zeros(len(sizes), dtype=torch.int32, device="cuda")

    def load(seed):
        coord, feat = spi.points(sizes, 3, seed=seed)
        eig, _ = _sort_inputs(sizes, seed)
        coord_buf.copy_(_dev(coord)); feat_buf.copy_(_dev(feat)); eig_buf.copy_(_dev(eig))
        return coord, feat, eig

    def step():
        dgn_amd.knn_graph(coord_buf, sizes_dev, feat_buf, check=False, out=out, status=status)
        dgn_amd.sort_eig(eig_buf, coord_buf, sizes_dev)

    load(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                      # warm-up outside the capture
        step()
    torch.cuda.current_stream().wait_stream(side)
    load(1)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        step()
    for seed in (2, 3):
        coord, feat, eig = load(seed)
        status.fill_(9)
        cg.replay()
        torch.cuda.synchronize()
        want = dgn_amd.knn_graph(_dev(coord), sizes, _dev(feat))
        want_eig = dgn_amd.sort_eig(_dev(eig), _dev(coord), sizes)
        torch.cuda.synchronize()
        assert status.tolist() == [0] * len(sizes)
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1]) and torch.equal(out[2].view(torch.int32), want[2].view(torch.int32))
        assert torch.equal(eig_buf.view(torch.int32), want_eig.view(torch.int32))
        assert np.array_equal(want_eig.cpu().numpy(), so.sort_eig(eig, coord[:, 0], coord[:, 1], sizes))


def test_sort_eig_golden_cases(golden):
    """The fixture's cases as one batch: exactly what the reference's sort_eig left, on every arm of its if-chain."""
    import dgn_amd
    g = golden("g15_superpixels")
    ids = range(int(g["n_sort"]))
    eig = np.concatenate([g[f"s{i}/eig"] for i in ids])
    xy = np.stack([np.concatenate([g[f"s{i}/x"] for i in ids]), np.concatenate([g[f"s{i}/y"] for i in ids])], axis=1)
    sizes = [g[f"s{i}/eig"].shape[0] for i in ids]
    assert {so.sort_eig_branch(g[f"s{i}/eig"], g[f"s{i}/x"], g[f"s{i}/y"]) for i in ids} == {0, 1, 2, 3}
    e = _dev(eig)
    got = dgn_amd.sort_eig(e, _dev(xy), sizes)
    torch.cuda.synchronize()
    assert got is e
    assert np.array_equal(got.cpu().numpy(), np.concatenate([g[f"s{i}/sorted"] for i in ids]))


@pytest.mark.parametrize("strided", [False, True])
def test_sort_eig_random_batch(strided):
    """70 graphs of 3 .. 150 nodes against the restatement, exactly; column 0 and the columns from 3 on are not touched."""
    import dgn_amd
    sizes = np.random.default_rng(70).integers(3, 151, 70).tolist()
    eig, xy = _sort_inputs(sizes, 71)
    want = so.sort_eig(eig, xy[:, 0], xy[:, 1], sizes)
    arms = set()
    off = 0
    for n in sizes:
        arms.add(so.sort_eig_branch(eig[off:off + n], xy[off:off + n, 0], xy[off:off + n, 1]))
        off += n
    assert arms == {0, 1, 2, 3}
    if strided:
        wide = torch.full((eig.shape[0], 10), 3.5, dtype=torch.float32, device="cuda")
        e = wide[:, 1:8]
        e.copy_(_dev(eig))
    else:
        e = _dev(eig)
    dgn_amd.sort_eig(e, _dev(xy), torch.tensor(sizes) if strided else sizes)
    torch.cuda.synchronize()
    got = e.cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(got[:, 0], eig[:, 0]) and np.array_equal(got[:, 3:], eig[:, 3:])
    if strided:
        assert bool((wide[:, 0] == 3.5).all()) and bool((wide[:, 8:] == 3.5).all())


def test_raw_data_to_a_layer_input():
    """6 graphs of 85 .. 150 nodes: knn_graph -> DGNGraph -> superpixel_eig (batch_eig's own check passes: every solve converged) -> one
    DGNLayer forward."""
    import dgn_amd
    sizes = [85, 100, 117, 128, 140, 150]
    coord, feat = spi.points(sizes, 3, seed=11)
    N = sum(sizes)
    c, f = _dev(coord, torch.float32), _dev(feat, torch.float32)
    src, dst, val = dgn_amd.knn_graph(c, sizes, f)
    assert src.numel() == N * 8 and val.dtype == torch.float32
    graph = dgn_amd.DGNGraph(src, dst, N)
    enc = dgn_amd.superpixel_eig(graph, c, sizes, coord_eig=True)
    assert enc.shape == (N, 3) and torch.equal(enc[:, 1:], c) and not bool(enc[:, 0].any())
    eig = dgn_amd.superpixel_eig(graph, c, sizes, coord_eig=False)
    assert eig.shape == (N, 7) and eig.dtype == torch.float32 and bool(torch.isfinite(eig).all())
    raw, _ = dgn_amd.batch_eig(graph, sizes, k=7, norm="sym")
    want = so.sort_eig(raw.cpu().numpy(), coord[:, 0].astype(np.float32), coord[:, 1].astype(np.float32), sizes)
    assert np.array_equal(eig.cpu().numpy(), want)
    graph.ndata["eig"] = eig
    torch.manual_seed(0)
    layer = dgn_amd.DGNLayer(65, 65, 0.0, True, True, "mean dir1-dx dir2-dx", "identity", {"log": torch.tensor(2.2)}, "simple", True).model.cuda()
    h = torch.randn(N, 65, device="cuda")
    snorm = torch.cat([torch.full((n, 1), n ** -0.5) for n in sizes]).cuda()
    y = layer(graph, h, None, snorm)
    torch.cuda.synchronize()
    assert y.shape == (N, 65) and bool(torch.isfinite(y).all())
