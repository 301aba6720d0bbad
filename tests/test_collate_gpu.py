"""The device-resident dataset on the GPU (dgn_amd/data.py, csrc/dgn_collate.hip): ``PackedGraphs.collate`` / ``gather`` against the
restatement of the reference's ``collate`` (tests/collate_ref.py), ``DGNGraph.load_packed`` against ``rebuild`` on the restated edge
list, the nets on a collated batch against the nets on a graph built from that edge list, and the captured steps fed by ``load_packed``
against the same steps fed by ``load``.  EVERY comparison is exact: integer equality, float bit patterns through an int32 view (NaN
labels compare)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import collate_ref as cr

pytestmark = pytest.mark.gpu

K = 3      # positional encodings of the nets below: eig[:, 1:K + 1]


def _bits(t):
    t = torch.as_tensor(t).detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def _restate(graphs, ids):
    """What the reference's collate leaves of the graphs ``ids``: dgl.batch's concatenation, the stacked graph columns, the graph norms."""
    picked = [graphs[int(i)] for i in ids]
    b = cr.dgl_batch([dict(g, ndata=g["node"], edata=g["edge"]) for g in picked]) if picked else None
    if b is None:
        return None
    b["graph"] = {k: np.stack([np.asarray(g["graph"][k]) for g in picked]) for k in picked[0]["graph"]}
    b["snorm_n"], b["snorm_e"] = cr.snorm(b["batch_num_nodes"]), cr.snorm([e for e in b["batch_num_edges"] if e])
    b["graph_id"] = np.repeat(np.arange(len(picked), dtype=np.int32), b["batch_num_nodes"])
    return b


def _random_graphs(sizes, seed, edgeless=()):
    """Graphs with the nine columns of the gather test: node int64 [N] / int64 [N, 9] / float32 [N, 3] (12-byte rows) / float32 [N, 6] /
    int64 labels, edge int64 [E] / float32 [E, 1], graph float32 [D, 5] with NaNs / int64 [D]."""
    rng = np.random.default_rng(seed)
    graphs = []
    for i, n in enumerate(sizes):
        e = 0 if (n == 1 or i in edgeless) else int(rng.integers(1, 3 * n + 1))
        y = rng.standard_normal(5).astype(np.float32)
        y[rng.random(5) < 0.4] = np.nan
        graphs.append(dict(src=rng.integers(0, n, e), dst=rng.integers(0, n, e), num_nodes=n,
                           node=dict(feat=rng.integers(0, 28, n), atoms=rng.integers(0, 2 ** 40, (n, 9)), eig=rng.standard_normal((n, 3)).astype(np.float32),
                                     wide=rng.standard_normal((n, 6)).astype(np.float32), label=rng.integers(0, 6, n)),
                           edge=dict(feat=rng.integers(0, 4, e), w=rng.standard_normal((e, 1)).astype(np.float32)),
                           graph=dict(label=y, cls=np.int64(rng.integers(0, 10)))))
    return graphs


SIZES = [1, 2, 3, 63, 64, 65, 9, 37, 5, 1, 30, 12, 2, 21]      # a single node with no edge first, both sides of the wave boundary
PADS = {("graph", "cls"): -1}


@pytest.fixture(scope="module")
def gather_ds():
    from dgn_amd import PackedGraphs
    graphs = _random_graphs(SIZES, seed=11, edgeless=(8,))
    return graphs, PackedGraphs.from_graphs(graphs, "cuda", pads=PADS)


BATCHES = {"all": list(range(14)), "one": [6], "unsorted": [7, 2, 13, 4, 0, 11], "twice": [3, 5, 3, 10], "single_node_first_and_last": [0, 4, 8, 6, 9],
           "edgeless_only": [0, 9, 8]}


@pytest.mark.parametrize("capacity", [False, True])
@pytest.mark.parametrize("batch", list(BATCHES))
def test_gather_equals_the_restated_collate(gather_ds, batch, capacity):
    graphs, ds = gather_ds
    dev, ids = ds.device, BATCHES[batch]
    ref = _restate(graphs, ids)
    N, E, G = ref["num_nodes"], len(ref["src"]), len(ids)
    n_out, e_out, g_out = (N + 70, E + 3, G + 16) if capacity else (N, E, G)
    rows = {"node": n_out, "edge": e_out, "graph": g_out}
    junk = lambda shape, dtype: torch.full(shape, 85, dtype=dtype, device=dev)          # (no output may keep what it held)
    outs = {dom: {k: junk((rows[dom],) + tuple(v.shape[1:]), v.dtype) for k, v in ds.columns[dom].items()} for dom in rows}
    snorm_n, snorm_e = junk((n_out,), torch.float32), junk((e_out,), torch.float32)
    graph_id, src, dst = junk((n_out,), torch.int32), junk((e_out,), torch.int64), junk((e_out,), torch.int64)
    p = ds.gather(ids, n_rows_out=n_out, e_rows_out=e_out, g_rows_out=g_out, node=outs["node"], edge=outs["edge"], graph=outs["graph"],
                  snorm_n=snorm_n, snorm_e=snorm_e, graph_id=graph_id, src=src, dst=dst)
    assert (p.G, p.N, p.E) == (G, N, E)
    count = {"node": N, "edge": E, "graph": G}
    want = {"node": ref["ndata"], "edge": ref["edata"], "graph": ref["graph"]}
    for dom in rows:
        assert list(outs[dom]) == list(want[dom]) and len(outs[dom]) in (5, 2)
        for name, out in outs[dom].items():
            col = ds.columns[dom][name]
            assert _same(out[:count[dom]], torch.from_numpy(np.ascontiguousarray(want[dom][name])).to(col.dtype)), (dom, name)
            pad = torch.full_like(out[count[dom]:], ds.pads[(dom, name)])                       # every row behind the batch
            assert _same(out[count[dom]:], pad), (dom, name, "pad rows")
    assert _same(snorm_n[:N], ref["snorm_n"][:, 0]) and _same(snorm_e[:E], ref["snorm_e"][:, 0])
    assert bool((snorm_n[N:] == 0).all()) and bool((snorm_e[E:] == 0).all())
    assert _same(graph_id[:N], ref["graph_id"]) and bool((graph_id[N:] == -1).all())
    assert _same(src[:E], ref["src"]) and _same(dst[:E], ref["dst"]) and bool((src[E:] == 0).all()) and bool((dst[E:] == 0).all())
    if not capacity:
        # the eager collate: the reference's tuple, the columns in ndata / edata, the graph adopted without a sort
        b = ds.collate(ids)
        g, labels, sn, se = b
        assert _same(labels, ref["graph"]["label"]) and _same(sn, ref["snorm_n"]) and _same(se, ref["snorm_e"].reshape(-1, 1))
        assert _same(b.src, ref["src"]) and _same(b.dst, ref["dst"]) and g.batch_num_nodes == ref["batch_num_nodes"].tolist()
        assert g.batch_num_edges == ref["batch_num_edges"].tolist() and (g.num_nodes, g.num_edges) == (N, E)
        assert _same(g.ndata["graph_id"], ref["graph_id"]) and _same(g.edata["feat"], ref["edata"]["feat"])
        for name in ("feat", "atoms", "eig", "wide", "label"):
            assert _same(g.ndata[name], ref["ndata"][name]), name


def test_many_graphs_cross_the_offset_chunks():
    """1 500 graphs of 1 to 3 nodes in one batch -- 700 single nodes without an edge in a row, 200 three-node graphs, then mixed --, so that a
    workgroup's bracket of graphs is both below and above the chunk the offset search keeps in LDS; then a 1 025-graph slice."""
    import dgn_amd
    rng = np.random.default_rng(5)
    sizes = [1] * 700 + [3] * 200 + [int(x) for x in rng.integers(1, 4, 600)]
    graphs = []
    for n in sizes:
        e = 0 if n == 1 else int(rng.integers(0, 2 * n + 1))
        graphs.append(dict(src=rng.integers(0, n, e), dst=rng.integers(0, n, e), num_nodes=n,
                           node=dict(feat=rng.integers(0, 2 ** 40, n), eig=rng.standard_normal((n, 3)).astype(np.float32)),
                           edge=dict(feat=rng.integers(0, 4, e)), graph=dict(label=np.int64(rng.integers(0, 10)))))
    ds = dgn_amd.PackedGraphs.from_graphs(graphs, "cuda")
    for ids in (np.arange(1500), np.arange(300, 1325), rng.permutation(1500)[:1025]):
        ref = _restate(graphs, ids)
        b = ds.collate(ids)
        N, E = ref["num_nodes"], len(ref["src"])
        assert (b.num_nodes, b.num_edges, b.num_graphs) == (N, E, len(ids))
        assert _same(b.src, ref["src"]) and _same(b.dst, ref["dst"]) and _same(b.labels, ref["graph"]["label"])
        assert _same(b.node["feat"], ref["ndata"]["feat"]) and _same(b.node["eig"], ref["ndata"]["eig"]) and _same(b.edge["feat"], ref["edata"]["feat"])
        assert _same(b.snorm_n, ref["snorm_n"]) and _same(b.snorm_e, ref["snorm_e"].reshape(-1, 1)) and _same(b.graph.ndata["graph_id"], ref["graph_id"])
        built = dgn_amd.DGNGraph(b.src, b.dst, N)
        built.ensure_csc()
        for name in ("indptr", "src", "dst_csr", "eid", "in_degree", "log_deg", "csc_ptr", "csc_pos", "csc_order"):
            assert _same(getattr(b.graph, name), getattr(built, name)), name
        assert b.graph.max_in_degree == built.max_in_degree and b.graph.n_hub == 0


CSR_ROWS = ("indptr", "in_degree", "log_deg", "csc_ptr", "eid")            # compared in full
CSR_SLOTS = ("src", "dst_csr", "csc_pos", "_csc_order")                    # compared over the batch's edges


def test_load_packed_leaves_the_arrays_rebuild_leaves(gather_ds):
    """One padded graph filled by ``load_packed``, a second one by ``rebuild`` on the restated edge list; then a SMALLER batch into the
    same two objects (stale tails)."""
    from dgn_amd import DGNGraph
    graphs, ds = gather_ds
    dev = ds.device
    n_cap, e_cap, _, _ = ds.capacity(len(graphs))
    n_cap, e_cap = n_cap + 70, e_cap + 3
    packed, rebuilt = DGNGraph.padded(n_cap, e_cap, dev, eig_dim=3), DGNGraph.padded(n_cap, e_cap, dev, eig_dim=3)
    for ids in (BATCHES["all"], BATCHES["unsorted"], BATCHES["twice"], BATCHES["edgeless_only"], BATCHES["one"]):
        ref = _restate(graphs, ids)
        N, E = ref["num_nodes"], len(ref["src"])
        p = packed.load_packed(ds, ids)
        rebuilt.rebuild(torch.from_numpy(ref["src"]).to(dev), torch.from_numpy(ref["dst"]).to(dev), N, torch.from_numpy(ref["ndata"]["eig"]).to(dev),
                        graph_sizes=ref["batch_num_nodes"])
        assert (p.N, p.E, packed.batch_nodes, packed.batch_edges) == (N, E, rebuilt.batch_nodes, rebuilt.batch_edges)
        for name in CSR_ROWS:
            assert _same(getattr(packed, name), getattr(rebuilt, name)), (name, ids)
        for name in CSR_SLOTS:
            assert _same(getattr(packed, name)[:E], getattr(rebuilt, name)[:E]), (name, ids)
        assert _same(packed.n_valid, rebuilt.n_valid) and int(packed.n_valid) == N
        assert _same(packed._stats[:2], rebuilt._stats[:2]) and packed._stats[:2].tolist() == [p.max_in_degree, 0]
        assert _same(packed.ndata["eig"], rebuilt.ndata["eig"])
        assert packed.max_in_degree == rebuilt.max_in_degree == 0
        packed.check_deferred()
        rebuilt.check_deferred()


def _mol_graphs(n_graphs, seed):
    from dgn_amd import synth
    b = synth.molecule_batch(n_graphs, seed=seed, laplacian_eig=False, eig_dim=K + 1)
    return _split(b, seed, lambda rng, n: dict(feat=rng.integers(0, 9, n)), lambda rng: dict(label=rng.standard_normal(1).astype(np.float32)))


def _split(b, seed, node_cols, graph_cols):
    """The graphs of a synth batch as per-graph dicts (local ids), with eig, pos_enc = eig[:, 1:K + 1] and the given columns."""
    from dgn_amd import synth
    rng = np.random.default_rng(seed)
    sizes, edges = b["sizes"].numpy(), synth.edges_per_graph(b).numpy()
    off, eoff = np.concatenate([[0], np.cumsum(sizes)]), np.concatenate([[0], np.cumsum(edges)])
    graphs = []
    for i, n in enumerate(sizes):
        eig = b["eig"][off[i]:off[i + 1]].numpy()
        graphs.append(dict(src=b["src"][eoff[i]:eoff[i + 1]].numpy() - off[i], dst=b["dst"][eoff[i]:eoff[i + 1]].numpy() - off[i], num_nodes=int(n),
                           node=dict(node_cols(rng, int(n)), eig=eig, pos_enc=np.ascontiguousarray(eig[:, 1:K + 1])), edge={}, graph=graph_cols(rng)))
    return graphs


def _net_params(type_net, hidden, L=2, **extra):
    return dict(dict(hidden_dim=hidden, out_dim=hidden, in_feat_dropout=0.0, dropout=0.0, L=L, type_net=type_net, pos_enc_dim=K, readout="mean",
                     graph_norm=True, batch_norm=True, aggregators="mean max min dir1-av dir1-dx", scalers="identity amplification attenuation",
                     avg_d={"log": torch.tensor(1.1)}, residual=True, edge_feat=False, edge_dim=0, pretrans_layers=1, posttrans_layers=1,
                     device="cuda"), **extra)


def _zinc_net(dev):
    from dgn_amd.nets import DGNNet
    return DGNNet(_net_params("towers", 20, num_atom_type=9, num_bond_type=4)).to(dev).train()


def _node_net(dev):
    from dgn_amd.nets import DGNNodeNet
    net = DGNNodeNet(_net_params("complex", 20, in_dim=3, n_classes=2, aggregators="mean dir1-dx dir2-dx")).to(dev).train()
    with torch.no_grad():
        for fc in net.MLP_layer.FC_layers:
            fc.weight.normal_(0.0, (2.0 / fc.weight.shape[1]) ** 0.5)
    return net


def _sbm_graphs(n_graphs, seed):
    from dgn_amd import synth
    b = synth.sbm_batch(n_graphs=n_graphs, seed=seed, n_lo=44, n_hi=60, eig_dim=K + 1)
    return _split(b, seed, lambda rng, n: dict(feat=rng.integers(0, 3, n), label=rng.integers(0, 2, n)), lambda rng: {})


def _knn_graphs(n_graphs, seed, in_dim=5):
    from dgn_amd import synth
    b = synth.knn_batch(n_graphs, seed=seed, n_lo=12, n_hi=30)
    return _split(b, seed, lambda rng, n: dict(feat=rng.random((n, in_dim)).astype(np.float32)), lambda rng: dict(label=np.int64(rng.integers(0, 10))))


@pytest.mark.parametrize("kind", ["graph_regression", "node_classification"])
def test_eager_net_on_a_collated_batch_is_bit_equal(kind):
    """The net on ``ds.collate(ids)`` against the same net on ``DGNGraph(src, dst, N, eig)`` built from the restatement's edge list (both
    graphs carry dgl.batch's ``batch_num_nodes``): scores and every parameter gradient."""
    import dgn_amd
    dev = torch.device("cuda")
    mol = kind == "graph_regression"
    graphs = _mol_graphs(12, 21) if mol else _sbm_graphs(5, 22)
    ds = dgn_amd.PackedGraphs.from_graphs(graphs, dev)
    ids = [7, 2, 9, 2, 0, 11] if mol else [3, 0, 4]
    ref = _restate(graphs, ids)
    torch.manual_seed(3)
    net = _zinc_net(dev) if mol else _node_net(dev)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def run(graph, feat, snorm, labels):
        net.zero_grad(set_to_none=True)
        scores = net(graph, feat, None, snorm, None)
        loss = net.loss(scores, labels)
        loss.backward()
        return scores.detach().clone(), loss.detach().clone(), {k: q.grad.clone() for k, q in net.named_parameters()}

    g = dgn_amd.DGNGraph(dv(ref["src"]), dv(ref["dst"]), ref["num_nodes"], eig=dv(ref["ndata"]["eig"]))
    g.batch_num_nodes = ref["batch_num_nodes"].tolist()
    g.ndata["pos_enc"] = dv(ref["ndata"]["pos_enc"])
    labels = dv(ref["graph"]["label"]) if mol else dv(ref["ndata"]["label"])
    want = run(g, dv(ref["ndata"]["feat"]), dv(ref["snorm_n"]), labels)
    b = ds.collate(ids)
    assert _same(b.labels, labels) and b.graph.ndata["pos_enc"].shape == (ref["num_nodes"], K)
    got = run(b.graph, b.graph.ndata["feat"], b.snorm_n, b.labels)
    assert _same(got[0], want[0]), "scores"
    assert _same(got[1], want[1]), "loss"
    assert len(got[2]) == len(want[2]) > 10
    for k in want[2]:
        assert _same(got[2][k], want[2][k]), k


def _two_steps(make_net, make_step, dev):
    from dgn_amd.hipgraph import rewrap_parameters
    torch.manual_seed(3)
    net_a = make_net(dev)
    net_b = copy.deepcopy(net_a)
    steps = []
    for net in (net_a, net_b):
        rewrap_parameters(net)
        steps.append(make_step(net, torch.optim.SGD(net.parameters(), lr=1e-2)))
    return steps


def _run_both(by_load, by_packed, ds, graphs, batches, load):
    """Three batches of different sizes through ONE capture each; the loss after every step and the parameters at the end, bit for bit."""
    first = batches[0]
    load(by_load, _restate(graphs, first))
    by_packed.load_packed(ds, first)
    by_load.capture(warmup=2)
    by_packed.capture(warmup=2)
    for ids in batches:
        load(by_load, _restate(graphs, ids))
        by_packed.load_packed(ds, ids)
        out_a, out_b = by_load.step(), by_packed.step()
        out_a, out_b = (out_a, out_b) if isinstance(out_a, tuple) else ((out_a,), (out_b,))
        for a, b in zip(out_a, out_b):
            assert _same(a, b), ("step output", len(ids))
        assert bool(torch.isfinite(out_a[0]))
    for (k, a), (_, b) in zip(by_load.net.state_dict().items(), by_packed.net.state_dict().items()):
        assert _same(a, b), k
    by_load.pb.graph.check_deferred()
    by_packed.pb.graph.check_deferred()
    assert _same(by_load.snorm, by_packed.snorm) and _same(by_load.pb.graph.ndata["eig"], by_packed.pb.graph.ndata["eig"])


def test_captured_net_step_fed_by_load_packed_equals_load(monkeypatch):
    import dgn_amd
    from dgn_amd.hipgraph import CapturedNetStep
    monkeypatch.setattr(dgn_amd.ops, "BLOCK_LAYER_MAX_NODES", 32768)       # (the static block table of ds.capacity(): the graph-block route)
    dev = torch.device("cuda")
    graphs = _mol_graphs(40, 31)
    ds = dgn_amd.PackedGraphs.from_graphs(graphs, dev)
    n_cap, e_cap, max_nodes, max_edges = ds.capacity(16)
    make = lambda net, opt: CapturedNetStep(net, n_cap, e_cap, g_cap=17, eig_dim=K + 1, optimizer=opt, max_graph_nodes=max_nodes, max_graph_edges=max_edges)
    by_load, by_packed = _two_steps(_zinc_net, make, dev)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    load = lambda cs, r: cs.load(dv(r["src"]), dv(r["dst"]), r["num_nodes"], dv(r["ndata"]["eig"]), dv(r["ndata"]["feat"]), dv(r["snorm_n"]),
                                 r["batch_num_nodes"].tolist(), dv(r["graph"]["label"]), pos_enc=dv(r["ndata"]["pos_enc"]))
    batches = [list(range(16)), [39, 3, 17, 3, 20, 8, 1], list(range(20, 33))]
    _run_both(by_load, by_packed, ds, graphs, batches, load)
    G = len(batches[-1])
    assert _same(by_load.atoms, by_packed.atoms) and _same(by_load.targets, by_packed.targets) and bool(torch.isnan(by_packed.targets[G:]).all())
    assert _same(by_load.pb.node["pos_enc"], by_packed.pb.node["pos_enc"]) and _same(by_load.rg.indptr, by_packed.rg.indptr)


def test_captured_superpixel_step_fed_by_load_packed_equals_load():
    import dgn_amd
    from dgn_amd.hipgraph import CapturedSuperpixelStep
    from dgn_amd.nets import DGNSuperpixelNet
    from test_superpixel_net_oracle_vs_golden import superpixel_net_params
    dev = torch.device("cuda")
    graphs = _knn_graphs(20, 41)
    ds = dgn_amd.PackedGraphs.from_graphs(graphs, dev)
    assert ds.pads[("graph", "label")] == -1
    n_cap, e_cap, _, _ = ds.capacity(8)

    def make_net(dev):
        net = DGNSuperpixelNet(superpixel_net_params("simple", 20, 5, "mean dir1-dx dir2-dx", "identity", "mean", False, L=2)).to(dev).train()
        with torch.no_grad():
            for fc in net.MLP_layer.FC_layers:
                fc.weight.normal_(0.0, (2.0 / fc.weight.shape[1]) ** 0.5)
        return net

    make = lambda net, opt: CapturedSuperpixelStep(net, n_cap, e_cap, g_cap=9, eig_dim=3, optimizer=opt)
    by_load, by_packed = _two_steps(make_net, make, dev)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    load = lambda cs, r: cs.load(dv(r["src"]), dv(r["dst"]), r["num_nodes"], dv(r["ndata"]["eig"]), dv(r["ndata"]["feat"]), dv(r["snorm_n"]),
                                 r["batch_num_nodes"].tolist(), dv(r["graph"]["label"]))
    batches = [list(range(8)), [19, 4, 4, 11], list(range(9, 15))]
    _run_both(by_load, by_packed, ds, graphs, batches, load)
    assert _same(by_load.atoms, by_packed.atoms) and _same(by_load.targets, by_packed.targets) and bool((by_packed.targets[6:] == -1).all())


def test_captured_mol_step_fed_by_load_packed_equals_load():
    """The OGB molecule step: [n_cap, 9] atom columns (72-byte rows), 128 label columns with NaN = not measured."""
    import dgn_amd
    from dgn_amd import synth
    from dgn_amd.hipgraph import CapturedMolStep
    from dgn_amd.nets import OGB_ATOM_DIMS, DGNPCBANet
    from test_mol_net_gpu import HIV_JSON
    dev = torch.device("cuda")

    def labels(rng):
        y = rng.integers(0, 2, 128).astype(np.float32)
        y[rng.random(128) < 0.6] = np.nan
        return dict(label=y)

    graphs = _split(synth.molecule_batch(14, seed=71, laplacian_eig=False, eig_dim=3), 71,
                    lambda rng, n: dict(feat=np.stack([rng.integers(0, d, n) for d in OGB_ATOM_DIMS], 1)), labels)
    ds = dgn_amd.PackedGraphs.from_graphs(graphs, dev)
    n_cap, e_cap, _, _ = ds.capacity(6)
    params = dict(HIV_JSON, avg_d={"log": torch.tensor(1.1)}, device="cuda", L=2, hidden_dim=20, out_dim=20, decreasing_dim=True, virtual_node=None)
    make_net = lambda dev: DGNPCBANet(params).to(dev).train()
    make = lambda net, opt: CapturedMolStep(net, n_cap, e_cap, g_cap=7, eig_dim=3, optimizer=opt)
    by_load, by_packed = _two_steps(make_net, make, dev)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    load = lambda cs, r: cs.load(dv(r["src"]), dv(r["dst"]), r["num_nodes"], dv(r["ndata"]["eig"]), dv(r["ndata"]["feat"]), dv(r["snorm_n"]),
                                 r["batch_num_nodes"].tolist(), dv(r["graph"]["label"]))
    batches = [list(range(6)), [13, 2, 2], [7, 12, 9, 3, 10]]
    _run_both(by_load, by_packed, ds, graphs, batches, load)
    assert by_packed.atoms.shape == (n_cap, 9) and by_packed.targets.shape == (by_packed.g_rows, 128)
    assert _same(by_load.atoms, by_packed.atoms) and _same(by_load.targets, by_packed.targets) and bool(torch.isnan(by_packed.targets[5:]).all())


def test_captured_node_step_fed_by_load_packed_equals_load():
    import dgn_amd
    from dgn_amd.hipgraph import CapturedNodeStep
    dev = torch.device("cuda")
    graphs = _sbm_graphs(9, 51)
    ds = dgn_amd.PackedGraphs.from_graphs(graphs, dev)
    n_cap, e_cap, _, _ = ds.capacity(4)
    make = lambda net, opt: CapturedNodeStep(net, n_cap, e_cap, eig_dim=K + 1, optimizer=opt)
    by_load, by_packed = _two_steps(_node_net, make, dev)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    load = lambda cs, r: cs.load(dv(r["src"]), dv(r["dst"]), r["num_nodes"], dv(r["ndata"]["eig"]), dv(r["ndata"]["feat"]), dv(r["snorm_n"]),
                                 dv(r["ndata"]["label"]), r["batch_num_nodes"].tolist(), pos_enc=dv(r["ndata"]["pos_enc"]))
    batches = [[0, 1, 2, 3], [8, 5], [4, 6, 4]]
    _run_both(by_load, by_packed, ds, graphs, batches, load)
    N = int(sum(graphs[i]["num_nodes"] for i in batches[-1]))
    assert _same(by_load.feats, by_packed.feats) and _same(by_load.labels, by_packed.labels) and bool((by_packed.labels[N:] == -1).all())


def test_refusals_leave_the_buffers_as_they_were(gather_ds):
    import dgn_amd
    from dgn_amd import DGNGraph, _lib
    from dgn_amd.hipgraph import CapturedNetStep
    graphs, ds = gather_ds
    dev = ds.device
    fits = [6, 8, 2]                                                    # 9 + 5 + 3 nodes
    ref = _restate(graphs, fits)
    pg = DGNGraph.padded(ref["num_nodes"] + 1, len(ref["src"]) + 4, dev, eig_dim=3)
    pg.load_packed(ds, fits)
    arrays = ("indptr", "src", "dst_csr", "eid", "in_degree", "log_deg", "csc_ptr", "csc_pos", "_csc_order", "n_valid", "_stats")
    before = {k: getattr(pg, k).clone() for k in arrays}
    eig = pg.ndata["eig"].clone()
    with pytest.raises(ValueError, match="exceeds the capacity"):
        pg.load_packed(ds, [5])                                         # 65 nodes
    with pytest.raises(ValueError, match="exceeds the capacity"):
        pg.load_packed(ds, fits + [12])                                 # two nodes too many
    with pytest.raises(ValueError, match="no node column"):
        pg.load_packed(ds, fits, node={"nope": eig})
    with pytest.raises(ValueError, match="shape"):
        pg.load_packed(ds, fits, node={"wide": eig})                    # [n_cap, 3] for a [N, 6] column
    with pytest.raises(ValueError, match="torch.int64"):
        pg.load_packed(ds, fits, node={"feat": torch.zeros(pg._pad["n_cap"], device=dev)})
    for k in arrays:
        assert _same(getattr(pg, k), before[k]), k
    assert _same(pg.ndata["eig"], eig) and (pg.batch_nodes, pg.batch_edges) == (ref["num_nodes"], len(ref["src"]))
    # a captured step: more graphs than graph rows
    mol = _mol_graphs(6, 61)
    mds = dgn_amd.PackedGraphs.from_graphs(mol, dev)
    n_cap, e_cap, _, _ = mds.capacity(6)
    cs = CapturedNetStep(_zinc_net(dev), n_cap, e_cap, g_cap=4, eig_dim=K + 1)
    cs.load_packed(mds, [0, 1, 2])
    targets, atoms, indptr = cs.targets.clone(), cs.atoms.clone(), cs.pb.graph.indptr.clone()
    with pytest.raises(ValueError, match="graph rows"):
        cs.load_packed(mds, [0, 1, 2, 3])
    assert _same(cs.targets, targets) and _same(cs.atoms, atoms) and _same(cs.pb.graph.indptr, indptr)
    # more columns than the kernel takes: DGN_ERR_INVALID through the C ABI
    c = _lib.DgnCollate()
    c.n_node_cols = _lib.DGN_COLLATE_MAX_NODE_COLS + 1
    assert _lib.load().dgn_collate(C.byref(c), _lib.stream_ptr(dev)) == _lib.DGN_ERR_INVALID
