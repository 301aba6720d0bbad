"""Host side of the device-resident datasets (dgn_amd/data.py), without a GPU: tests/collate_ref.py against the reference's own
``collate`` methods (fixture g19_collate, tests/golden/make_golden_collate.py), and ``PackedGraphs``' pointers, pack-time errors,
capacities, epochs, offset tables and graph-norm values."""
import numpy as np
import pytest
import torch

import collate_ref as cr


@pytest.mark.parametrize("dataset", cr.DATASETS)
def test_restatement_equals_the_reference_collate(golden, dataset):
    g = golden("g19_collate")
    assert list(g["datasets"]) == list(cr.DATASETS)
    batched, labels, snorm_n, snorm_e = cr.collate(dataset, cr.fake_samples(dataset, int(g[f"{dataset}/seed"])))
    same = lambda a, b: a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert same(labels, g[f"{dataset}/labels"]), (labels.dtype, labels.shape, g[f"{dataset}/labels"].dtype, g[f"{dataset}/labels"].shape)
    assert same(snorm_n, g[f"{dataset}/snorm_n"]) and same(snorm_e, g[f"{dataset}/snorm_e"])
    assert same(batched["src"], g[f"{dataset}/src"]) and same(batched["dst"], g[f"{dataset}/dst"])
    assert batched["num_nodes"] == int(g[f"{dataset}/num_nodes"]) == snorm_n.shape[0]
    keys = [k for k in g.files if k.startswith(f"{dataset}/ndata::") or k.startswith(f"{dataset}/edata::")]
    assert len(keys) == len(batched["ndata"]) + len(batched["edata"]) == 3
    for k in keys:
        kind, name = k.split("/")[1].split("::")
        assert same(batched[kind][name], g[k]), k


def _graphs(sizes, seed=0, edgeless=()):
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(sizes):
        e = 0 if (n == 1 or i in edgeless) else int(rng.integers(1, 3 * n))
        out.append(dict(src=rng.integers(0, n, e), dst=rng.integers(0, n, e), num_nodes=n,
                        node=dict(feat=rng.integers(0, 9, n), eig=rng.standard_normal((n, 3)).astype(np.float32)),
                        edge=dict(feat=rng.integers(0, 4, e)), graph=dict(label=np.float32(rng.standard_normal()))))
    return out


def test_pointers_columns_and_pads():
    from dgn_amd import PackedGraphs
    graphs = _graphs([1, 4, 2, 7, 3], edgeless=(2,))
    ds = PackedGraphs.from_graphs(graphs)
    assert len(ds) == 5 and ds.device is None and ds.graph is None
    assert ds.node_ptr.tolist() == [0, 1, 5, 7, 14, 17]
    assert ds.edge_ptr.tolist() == np.concatenate([[0], np.cumsum([len(g["src"]) for g in graphs])]).tolist()
    assert ds.edge_ptr[1] == 0 and ds.edge_ptr[3] == ds.edge_ptr[2]              # the single node and the edgeless graph
    assert (ds.num_nodes, ds.num_edges) == (17, int(ds.edge_ptr[-1]))
    for g, lo, hi, m in zip(graphs, ds.node_ptr[:-1], ds.node_ptr[1:], ds.max_in_degree):
        assert m == (np.bincount(g["dst"], minlength=g["num_nodes"]).max() if len(g["dst"]) else 0)
    assert torch.equal(ds.columns["node"]["feat"], torch.cat([torch.as_tensor(g["node"]["feat"]) for g in graphs]))
    assert ds.columns["graph"]["label"].shape == (5,) and ds.columns["graph"]["label"].dtype == torch.float32
    assert ds.pads[("node", "feat")] == 0 and ds.pads[("node", "eig")] == 0 and np.isnan(ds.pads[("graph", "label")])
    # the same dataset from concatenated arrays; class labels pad with -1, and a pad value can be chosen
    b = cr.dgl_batch([dict(g, ndata=g["node"], edata=g["edge"]) for g in graphs])
    ds2 = PackedGraphs.from_packed(b["src"], b["dst"], b["batch_num_nodes"], b["batch_num_edges"], node=dict(b["ndata"], label=np.zeros(17, dtype=np.int64)),
                                   graph=dict(label=np.arange(5)), pads={("node", "feat"): 8})
    assert ds2.node_ptr.tolist() == ds.node_ptr.tolist() and ds2.edge_ptr.tolist() == ds.edge_ptr.tolist()
    assert ds2.pads[("node", "label")] == -1 and ds2.pads[("graph", "label")] == -1 and ds2.pads[("node", "feat")] == 8
    assert torch.equal(ds2._src, ds._src) and torch.equal(ds2._dst, ds._dst)


def test_pack_time_errors():
    from dgn_amd import PackedGraphs
    from dgn_amd.graph import HUB_THRESHOLD
    ok = _graphs([3, 4])
    with pytest.raises(ValueError, match="outside the graph"):
        PackedGraphs.from_graphs([ok[0], dict(ok[1], src=np.array([0, 4]), dst=np.array([1, 0]), edge=dict(feat=np.zeros(2, dtype=np.int64)))])
    with pytest.raises(ValueError, match="outside the graph"):                    # a global id of the NEXT graph in from_packed
        PackedGraphs.from_packed([0, 3], [1, 2], [3, 2], [1, 1])
    with pytest.raises(ValueError, match="outside the graph"):
        PackedGraphs.from_packed([0, -1], [1, 0], [3, 2], [2, 0])
    with pytest.raises(ValueError, match="no nodes"):
        PackedGraphs.from_packed([0], [1], [3, 0, 2], [1, 0, 0])
    with pytest.raises(ValueError, match="int32"):
        PackedGraphs.from_packed([], [], [2 ** 30, 2 ** 30], [0, 0])
    hub = HUB_THRESHOLD + 1
    with pytest.raises(ValueError, match="in-degree"):
        PackedGraphs.from_packed(np.arange(1, hub + 1), np.zeros(hub, dtype=np.int64), [hub + 1], [hub])
    PackedGraphs.from_packed(np.arange(1, hub), np.zeros(hub - 1, dtype=np.int64), [hub], [hub - 1])      # exactly the threshold: taken
    with pytest.raises(ValueError, match="rows"):
        PackedGraphs.from_packed([0], [1], [3], [1], node=dict(feat=np.zeros(4)))
    with pytest.raises(ValueError, match="int64 or float32"):
        PackedGraphs.from_packed([0], [1], [3], [1], node=dict(feat=np.zeros(3, dtype=np.complex64)))
    with pytest.raises(ValueError, match="at most 2"):
        PackedGraphs.from_packed([0], [1], [3], [1], graph={f"c{i}": np.zeros(1) for i in range(3)})
    with pytest.raises(ValueError, match="unknown column"):
        PackedGraphs.from_packed([0], [1], [3], [1], pads={("node", "feat"): 1})


def test_capacity_and_batches():
    from dgn_amd import PackedGraphs
    sizes = [5, 1, 9, 3, 7, 2, 8]
    ds = PackedGraphs.from_graphs(_graphs(sizes, seed=3))
    ne = np.diff(ds.edge_ptr)
    assert ds.capacity(3) == (9 + 8 + 7, int(np.sort(ne)[-3:].sum()), 9, int(ne.max()))
    assert ds.capacity(100) == (sum(sizes), int(ne.sum()), 9, int(ne.max()))
    # every batch of an epoch fits the capacity, whatever the order
    for shuffle, gen in ((False, None), (True, 5), (True, np.random.default_rng(1)), (True, torch.Generator().manual_seed(2))):
        seen = []
        for ids in ds.batches(3, shuffle=shuffle, generator=gen):
            assert ids.dtype == np.int64 and 1 <= ids.size <= 3
            p = ds.plan(ids)
            assert p.N <= ds.capacity(3)[0] and p.E <= ds.capacity(3)[1]
            seen += ids.tolist()
        assert sorted(seen) == list(range(7)) and (shuffle or seen == list(range(7)))
    assert [b.tolist() for b in ds.batches(3, drop_last=True)] == [[0, 1, 2], [3, 4, 5]]
    assert [b.tolist() for b in ds.batches(3, shuffle=True, generator=9)] == [b.tolist() for b in ds.batches(3, shuffle=True, generator=9)]
    with pytest.raises(ValueError):
        next(ds.batches(0))


def test_offset_table_for_repeated_and_unsorted_ids():
    from dgn_amd import PackedGraphs
    from dgn_amd.data import MAX_BATCH_GRAPHS
    sizes = [5, 1, 9, 3]
    ds = PackedGraphs.from_graphs(_graphs(sizes, seed=4))
    ne = np.diff(ds.edge_ptr)
    ids = [2, 0, 2, 1, 3, 1]
    for given in (ids, np.asarray(ids), torch.tensor(ids), tuple(ids)):
        p = ds.plan(given)
        assert p.table.dtype == np.int32 and p.table.shape == (5, 7)
        assert p.table[0].tolist() == [0, 9, 14, 23, 24, 27, 28] and (p.G, p.N) == (6, 28)
        assert p.table[1].tolist() == np.concatenate([[0], np.cumsum(ne[ids])]).tolist() and p.E == int(ne[ids].sum())
        assert p.table[2, :6].tolist() == [ds.node_ptr[i] for i in ids] and p.table[3, :6].tolist() == [ds.edge_ptr[i] for i in ids]
        assert p.table[4, :6].tolist() == ids
        assert p.sizes.tolist() == [sizes[i] for i in ids] and p.max_in_degree == int(ds.max_in_degree[ids].max())
    empty = ds.plan([])
    assert (empty.G, empty.N, empty.E, empty.max_in_degree) == (0, 0, 0, 0) and empty.table.shape == (5, 1) and not empty.table.any()
    with pytest.raises(IndexError):
        ds.plan([0, 4])
    with pytest.raises(IndexError):
        ds.plan([-1])
    with pytest.raises(ValueError, match="at most"):
        ds.plan(np.zeros(MAX_BATCH_GRAPHS + 1, dtype=np.int64))
    assert ds.plan(np.zeros(MAX_BATCH_GRAPHS, dtype=np.int64)).N == 5 * MAX_BATCH_GRAPHS


def test_graph_norm_is_the_reference_expression_bit_for_bit():
    from dgn_amd import PackedGraphs
    from dgn_amd.data import graph_norm
    sizes = np.arange(1, 4097)
    got = graph_norm(sizes)
    want = torch.cat([torch.FloatTensor(1, 1).fill_(1. / float(size)) for size in sizes]).sqrt().reshape(-1)      # data/molecules.py:224-225
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32))
    small = np.arange(1, 200)                                                   # (and per ROW, as the restatement spreads them)
    assert np.array_equal(np.repeat(got[:199].numpy(), small).view(np.int32), cr.snorm(small)[:, 0].view(np.int32))
    assert graph_norm([0, 1, 0]).tolist() == [0.0, 1.0, 0.0]                    # a graph without edges has no snorm_e rows
    ds = PackedGraphs.from_graphs(_graphs([1, 4, 2, 7], seed=6))
    assert torch.equal(ds.snorm_n, graph_norm([1, 4, 2, 7])) and torch.equal(ds.snorm_e, graph_norm(np.diff(ds.edge_ptr)))


def test_collating_needs_the_device():
    import dgn_amd
    ds = dgn_amd.PackedGraphs.from_graphs(_graphs([3, 4]))
    with pytest.raises(dgn_amd._lib.DgnError, match="host only"):
        ds.collate([0])
    with pytest.raises(dgn_amd._lib.DgnError, match="GPU only"):
        ds.to("cpu")


def test_collate_refuses_more_columns_than_the_kernel_takes():
    """DGN_ERR_INVALID through the C ABI, before anything touches the device."""
    import ctypes as C
    from dgn_amd import _lib
    lib = _lib.load()
    for field, limit in (("n_node_cols", _lib.DGN_COLLATE_MAX_NODE_COLS), ("n_edge_cols", _lib.DGN_COLLATE_MAX_EDGE_COLS),
                         ("n_graph_cols", _lib.DGN_COLLATE_MAX_GRAPH_COLS)):
        c = _lib.DgnCollate()
        setattr(c, field, limit + 1)
        assert lib.dgn_collate(C.byref(c), None) == _lib.DGN_ERR_INVALID and b"columns" in lib.dgn_last_error()
        setattr(c, field, limit)
        assert lib.dgn_collate(C.byref(c), None) == _lib.DGN_OK                   # (no outputs wanted: nothing launched)
    assert _lib.DGN_COLLATE_MAX_NODE_COLS >= 8 and _lib.DGN_COLLATE_MAX_EDGE_COLS >= 4 and _lib.DGN_COLLATE_MAX_GRAPH_COLS >= 2
    c = _lib.DgnCollate()
    c.n_graphs = _lib.DGN_COLLATE_MAX_GRAPHS + 1
    assert lib.dgn_collate(C.byref(c), None) == _lib.DGN_ERR_INVALID
    c.n_graphs, c.n_nodes, c.n_rows_out = 1, 5, 4
    assert lib.dgn_collate(C.byref(c), None) == _lib.DGN_ERR_INVALID and b"exceeds" in lib.dgn_last_error()
    c.n_rows_out, c.g_rows_out, c.n_node_cols, c.table = 5, 1, 1, 4096      # (dummy addresses: never dereferenced)
    c.node_in[0], c.node_out[0], c.node_row_bytes[0] = 4096, 4096, 6
    assert lib.dgn_collate(C.byref(c), None) == _lib.DGN_ERR_INVALID and b"multiple of 4" in lib.dgn_last_error()
