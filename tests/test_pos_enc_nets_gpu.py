"""The nets with positional encodings on the device: fixture G18 (the reference's own nets with ``pos_enc_dim = 3``) through
``dgn_amd.nets.DGNNet`` / ``DGNNodeNet`` -- ``h0`` within the forward bound of tests/test_node_input_gpu.py, everything else at the
tolerances of tests/test_net_gpu.py::test_net_vs_reference_fixture -- and ``hipgraph.CapturedNetStep`` / ``CapturedNodeStep`` with
positional encodings against eager training on the unpadded batches (the construction and tolerances of
tests/test_net_gpu.py::test_captured_net_step_equals_eager_training and its node-net counterpart)."""
import copy

import numpy as np
import pytest
import torch

import input_stage_oracle as iso
from test_input_stage_oracle_vs_golden import CASES, pos_enc_net

pytestmark = pytest.mark.gpu

K = 3


def _spy(monkeypatch):
    import dgn_amd
    calls = []
    real = dgn_amd.ops.node_input
    monkeypatch.setattr(dgn_amd.ops, "node_input", lambda *a, **k: calls.append(a[0].shape[0]) or real(*a, **k))
    return calls


@pytest.mark.parametrize("case", CASES)
def test_pos_enc_net_vs_reference_fixture(golden, monkeypatch, case):
    import dgn_amd
    g = golden("g18_pos_enc_nets")
    dev = torch.device("cuda")
    calls = _spy(monkeypatch)
    net, sd, kind = pos_enc_net(g, case, "cuda")
    assert set(sd) == set(net.state_dict())
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train(True)
    N = int(g["N"])
    eig = torch.from_numpy(g["eig"]).to(dev)
    graph = dgn_amd.DGNGraph(torch.from_numpy(g["src"]).to(dev), torch.from_numpy(g["dst"]).to(dev), N, eig=eig)
    graph.batch_num_nodes = [int(s) for s in g["sizes"]]
    graph.ndata["pos_enc"] = eig[:, 1:K + 1]
    feats = torch.from_numpy(g["atoms" if kind == "mol" else "feats"]).to(dev)
    snorm = torch.from_numpy(g["snorm"]).to(dev)
    seen = {}
    handle = net.layers[0].register_forward_pre_hook(lambda m, args: seen.__setitem__("h0", args[1].detach().clone()))
    scores = net(graph, feats, None, snorm, None)
    handle.remove()
    assert calls == [N], "the input stage did not take ops.node_input"
    # h0: the forward bound (C + K + 1) 2^-23 (|T| + |b| + sum_k |W pe|) against the fp64 restatement, C = 1
    table, w, b = g[f"{case}/sd::embedding_h.weight"], g[f"{case}/sd::embedding_pos_enc.weight"], g[f"{case}/sd::embedding_pos_enc.bias"]
    idx, pe = g["atoms" if kind == "mol" else "feats"], g["eig"][:, 1:K + 1]
    r64 = iso.input_stage(idx, [table], pe, w, b, np.float64)
    bound = (1 + K + 1) * 2.0 ** -23 * iso.input_stage_magnitude(idx, [table], pe, w, b)
    assert bool((np.abs(seen["h0"].cpu().numpy().astype(np.float64) - r64) <= bound).all())
    np.testing.assert_allclose(seen["h0"].cpu().numpy(), g[f"{case}/h0"], rtol=1e-5, atol=1e-6)
    loss = net.loss(scores, torch.from_numpy(g["targets"]).to(dev)) if kind == "mol" else net.loss(scores, torch.from_numpy(g["labels"]).to(dev))
    np.testing.assert_allclose(scores.detach().cpu().numpy(), g[f"{case}/scores"], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(loss.item(), float(g[f"{case}/loss"]), rtol=1e-5)
    loss.backward()
    n_checked = 0
    for k, q in net.named_parameters():
        key = f"{case}/gp::{k}"
        if key in g:
            ref = g[key]
            np.testing.assert_allclose(q.grad.cpu().numpy(), ref, rtol=2e-3, atol=2e-4 * max(1e-2, float(np.abs(ref).max())), err_msg=k)
            n_checked += 1
    assert n_checked >= 15 and net.embedding_pos_enc.weight.grad is not None
    for k, v in net.state_dict().items():
        if "running" in k:
            np.testing.assert_allclose(v.cpu().numpy(), g[f"{case}/after::{k}"], rtol=1e-4, atol=1e-5, err_msg=k)


def _mol_batches(dev):
    from dgn_amd import synth
    gen = torch.Generator().manual_seed(5)
    batches = []
    for i, n_graphs in enumerate((24, 31, 17, 28)):
        b = synth.molecule_batch(n_graphs, seed=60 + i, laplacian_eig=False)
        N = int(b["num_nodes"])
        batches.append(dict(src=b["src"].to(dev), dst=b["dst"].to(dev), N=N, eig=b["eig"].to(dev), sizes=[int(s) for s in b["sizes"]],
                            atoms=torch.randint(0, 9, (N,), generator=gen).to(dev), snorm=b["snorm_n"].to(dev),
                            y=torch.randn(n_graphs, 1, generator=gen).to(dev)))
    return batches


def _zinc_net(dev):
    from dgn_amd.nets import DGNNet
    params = dict(num_atom_type=9, num_bond_type=4, hidden_dim=20, out_dim=20, in_feat_dropout=0.0, dropout=0.0, L=3, type_net="towers",
                  pos_enc_dim=K, readout="mean", graph_norm=True, batch_norm=True, aggregators="mean max min dir1-av dir1-dx",
                  scalers="identity amplification attenuation", avg_d={"log": torch.tensor(1.1)}, residual=True, edge_feat=False, edge_dim=0,
                  pretrans_layers=1, posttrans_layers=1, device="cuda")
    return DGNNet(params).to(dev).train()


@pytest.mark.parametrize("block_route", [False, True])
def test_captured_net_step_with_pos_enc_equals_eager_training(monkeypatch, block_route):
    """``CapturedNetStep`` on a net with ``pos_enc_dim = 3`` (static ``[n_cap, 3]`` buffer in ``ndata['pos_enc']``, filled from the
    ``eig[:, 1:4]`` slice as it is; NaN targets behind the batch masked by the loss kernel) against eager training on the unpadded
    batches: four batches of 17 to 31 molecules, plain SGD on both sides, the tolerances of the test this one is built after."""
    import dgn_amd
    from dgn_amd.hipgraph import CapturedNetStep, rewrap_parameters
    taken = []
    if block_route:
        monkeypatch.setattr(dgn_amd.ops, "BLOCK_LAYER_MAX_NODES", 32768)
        real = dgn_amd.ops.block_layer
        monkeypatch.setattr(dgn_amd.ops, "block_layer", lambda *a, **k: taken.append(a[0]) or real(*a, **k))
    calls = _spy(monkeypatch)
    dev = torch.device("cuda")
    torch.manual_seed(3)
    net_e = _zinc_net(dev)
    net_c = copy.deepcopy(net_e)
    batches = _mol_batches(dev)
    order = [0, 0, 1, 2, 3, 1]                                  # (the first two = the capture's warm-up steps on batch 0)
    opt = torch.optim.SGD(net_e.parameters(), lr=1e-2)
    losses_e = []
    for i in order:
        b = batches[i]
        g = dgn_amd.DGNGraph(b["src"], b["dst"], b["N"], eig=b["eig"])
        g.batch_num_nodes = b["sizes"]
        g.ndata["pos_enc"] = b["eig"][:, 1:K + 1]
        opt.zero_grad(set_to_none=True)
        loss = net_e.loss(net_e(g, b["atoms"], None, b["snorm"], None), b["y"])
        loss.backward()
        opt.step()
        losses_e.append(float(loss))
    assert calls == [batches[i]["N"] for i in order]
    n_cap = max(b["N"] for b in batches) + 40
    e_cap = max(b["src"].numel() for b in batches) + 64
    rewrap_parameters(net_c)
    caps = dict(max_graph_nodes=max(max(b["sizes"]) for b in batches), max_graph_edges=4 * max(max(b["sizes"]) for b in batches)) if block_route else {}
    cs = CapturedNetStep(net_c, n_cap, e_cap, g_cap=40, eig_dim=batches[0]["eig"].shape[1], optimizer=torch.optim.SGD(net_c.parameters(), lr=1e-2), **caps)
    assert cs.pb.graph.ndata["pos_enc"] is cs.pb.node["pos_enc"] and tuple(cs.pb.node["pos_enc"].shape) == (n_cap, K)
    load = lambda b: cs.load(b["src"], b["dst"], b["N"], b["eig"], b["atoms"], b["snorm"], b["sizes"], b["y"], pos_enc=b["eig"][:, 1:K + 1])
    load(batches[0])
    cs.capture(warmup=2)
    assert calls[len(order):] == [n_cap] * 3                    # two warm-up steps and the captured one, on the padded batch
    losses_c = []
    for i in order[2:]:
        load(batches[i])
        losses_c.append(float(cs.step()))
        assert bool((cs.pb.node["pos_enc"][batches[i]["N"]:] == 0).all()) and bool(torch.isnan(cs.targets[len(batches[i]["sizes"]):]).all())
    np.testing.assert_allclose(losses_c, losses_e[2:], rtol=2e-4, atol=1e-5)
    if block_route:
        assert any(getattr(g, "_pad", None) is not None for g in taken), "the captured step did not take the graph-block route"
        cs.pb.graph.check_deferred()
    for (k, a), (_, b) in zip(net_c.named_parameters(), net_e.named_parameters()):
        np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(), rtol=1e-4, atol=2e-5, err_msg=k)
    for (k, a), (_, b) in zip(net_c.state_dict().items(), net_e.state_dict().items()):
        if "running" in k:
            np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-3, atol=1e-5, err_msg=k)


def _sbm_batches(dev, n_classes, graph_counts, seed0):
    from dgn_amd import synth
    gen = torch.Generator().manual_seed(5)
    batches = []
    for i, n_graphs in enumerate(graph_counts):
        b = synth.sbm_batch(n_graphs=n_graphs, seed=seed0 + i, n_lo=44, n_hi=60, eig_dim=K + 1)
        N = int(b["num_nodes"])
        batches.append(dict(src=b["src"].to(dev), dst=b["dst"].to(dev), N=N, eig=b["eig"].to(dev), sizes=[int(s) for s in b["sizes"]],
                            feats=torch.randint(0, 3, (N,), generator=gen).to(dev), snorm=b["snorm_n"].to(dev),
                            y=torch.randint(0, n_classes, (N,), generator=gen).to(dev)))
    return batches


def _pattern_net(dev):
    from dgn_amd.nets import DGNNodeNet
    net = DGNNodeNet(dict(in_dim=3, hidden_dim=47, out_dim=47, n_classes=2, in_feat_dropout=0.0, dropout=0.0, L=3, type_net="complex",
                          pos_enc_dim=K, readout="mean", graph_norm=True, batch_norm=True, aggregators="mean dir1-dx dir2-dx",
                          scalers="identity amplification attenuation", avg_d={"log": torch.tensor(1.1)}, residual=True, edge_feat=False,
                          edge_dim=0, pretrans_layers=1, posttrans_layers=1, device="cuda")).to(dev).train()
    with torch.no_grad():                                       # (wider than the stock gain = 1 / in_size head: scores away from 0)
        for fc in net.MLP_layer.FC_layers:
            fc.weight.normal_(0.0, (2.0 / fc.weight.shape[1]) ** 0.5)
    return net


def test_captured_node_step_with_pos_enc_equals_eager_training(monkeypatch):
    """``CapturedNodeStep`` likewise, on PATTERN-like batches of 6 graphs of 44 to 60 nodes (``synth.sbm_batch``), hidden 47."""
    import dgn_amd
    from dgn_amd.hipgraph import CapturedNodeStep, rewrap_parameters
    calls = _spy(monkeypatch)
    dev = torch.device("cuda")
    torch.manual_seed(3)
    net_e = _pattern_net(dev)
    net_c = copy.deepcopy(net_e)
    batches = _sbm_batches(dev, 2, (6, 6, 6, 6), 70)
    order = [0, 0, 1, 2, 3, 1]
    opt = torch.optim.SGD(net_e.parameters(), lr=1e-2)
    losses_e = []
    for i in order:
        b = batches[i]
        g = dgn_amd.DGNGraph(b["src"], b["dst"], b["N"], eig=b["eig"])
        g.batch_num_nodes = b["sizes"]
        g.ndata["pos_enc"] = b["eig"][:, 1:K + 1]
        opt.zero_grad(set_to_none=True)
        loss = net_e.loss(net_e(g, b["feats"], None, b["snorm"], None), b["y"])
        loss.backward()
        opt.step()
        losses_e.append(float(loss))
    assert calls == [batches[i]["N"] for i in order]
    n_cap = max(b["N"] for b in batches) + 40
    e_cap = max(b["src"].numel() for b in batches) + 64
    rewrap_parameters(net_c)
    cs = CapturedNodeStep(net_c, n_cap, e_cap, eig_dim=batches[0]["eig"].shape[1], optimizer=torch.optim.SGD(net_c.parameters(), lr=1e-2))
    load = lambda b: cs.load(b["src"], b["dst"], b["N"], b["eig"], b["feats"], b["snorm"], b["y"], b["sizes"], pos_enc=b["eig"][:, 1:K + 1])
    load(batches[0])
    cs.capture(warmup=2)
    losses_c = []
    for i in order[2:]:
        load(batches[i])
        loss, cm = cs.step()
        losses_c.append(float(loss))
        assert int(cm.sum()) == batches[i]["N"]                   # the padding rows are counted nowhere
    np.testing.assert_allclose(losses_c, losses_e[2:], rtol=2e-4, atol=1e-5)
    for (k, a), (_, b_) in zip(net_c.named_parameters(), net_e.named_parameters()):
        np.testing.assert_allclose(a.detach().cpu().numpy(), b_.detach().cpu().numpy(), rtol=1e-4, atol=2e-5, err_msg=k)
    for (k, a), (_, b_) in zip(net_c.state_dict().items(), net_e.state_dict().items()):
        if "running" in k:
            np.testing.assert_allclose(a.cpu().numpy(), b_.cpu().numpy(), rtol=1e-3, atol=1e-5, err_msg=k)


def test_load_checks_pos_enc():
    """A net with positional encodings needs ``pos_enc`` at ``load``; a net without takes none."""
    from dgn_amd.hipgraph import CapturedNetStep, CapturedNodeStep
    from dgn_amd.nets import DGNNet
    dev = torch.device("cuda")
    torch.manual_seed(0)
    b = _mol_batches(dev)[2]
    with_pe = CapturedNetStep(_zinc_net(dev), b["N"] + 40, b["src"].numel() + 64, g_cap=40, eig_dim=b["eig"].shape[1])
    args = (b["src"], b["dst"], b["N"], b["eig"], b["atoms"], b["snorm"], b["sizes"], b["y"])
    with pytest.raises(ValueError, match="pos_enc"):
        with_pe.load(*args)
    with pytest.raises(ValueError, match="pos_enc"):
        with_pe.load(*args, pos_enc=b["eig"][:, 1:K + 2])          # the wrong width
    with_pe.load(*args, pos_enc=b["eig"][:, 1:K + 1])
    params = dict(num_atom_type=9, num_bond_type=4, hidden_dim=20, out_dim=20, in_feat_dropout=0.0, dropout=0.0, L=2, type_net="simple",
                  pos_enc_dim=0, readout="mean", graph_norm=True, batch_norm=True, aggregators="mean max", scalers="identity",
                  avg_d={"log": torch.tensor(1.1)}, residual=True, edge_feat=False, edge_dim=0, pretrans_layers=1, posttrans_layers=1, device="cuda")
    without = CapturedNetStep(DGNNet(params).to(dev).train(), b["N"] + 40, b["src"].numel() + 64, g_cap=40, eig_dim=b["eig"].shape[1])
    with pytest.raises(ValueError, match="pos_enc"):
        without.load(*args, pos_enc=b["eig"][:, 1:K + 1])
    without.load(*args)
    (s,) = _sbm_batches(dev, 2, (6,), 90)
    node = CapturedNodeStep(_pattern_net(dev), s["N"] + 40, s["src"].numel() + 64, eig_dim=s["eig"].shape[1])
    with pytest.raises(ValueError, match="pos_enc"):
        node.load(s["src"], s["dst"], s["N"], s["eig"], s["feats"], s["snorm"], s["y"], s["sizes"])
    node.load(s["src"], s["dst"], s["N"], s["eig"], s["feats"], s["snorm"], s["y"], s["sizes"], pos_enc=s["eig"][:, 1:K + 1])
