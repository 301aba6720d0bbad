"""The superpixel graph-classification net (dgn_amd.nets.DGNSuperpixelNet) against fixture G16 -- the reference's own MNIST / CIFAR10 net
(nets/superpixels_graph_classification/dgn_net.py) on the same batch with the same weights: scores, cross-entropy, hit count, every
parameter gradient, BatchNorm running statistics --, the whole preparation chain (knn_graph -> DGNGraph -> superpixel_eig) into the net
against the same modules composed by hand with F.linear / F.cross_entropy, and hipgraph.CapturedSuperpixelStep against eager training.
Tolerances: those of tests/test_node_net_gpu.py for the same quantities of the node-classification net."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import superpixel_net_oracle as spo
from test_superpixel_net_oracle_vs_golden import fixture_net_params, superpixel_net_params

gpu = pytest.mark.gpu


def _assert_net_quantities(tag, scores, loss, net, ref_scores, ref_loss, ref_grads, ref_running, min_grads):
    """scores, loss, parameter gradients and running statistics of ``net`` against references given as numpy arrays keyed by name."""
    np.testing.assert_allclose(scores.detach().cpu().numpy(), ref_scores, rtol=2e-4, atol=2e-5, err_msg=tag)
    np.testing.assert_allclose(loss.item(), float(ref_loss), rtol=1e-5, err_msg=tag)
    n_checked = 0
    for k, q in net.named_parameters():
        if k in ref_grads:
            ref = ref_grads[k]
            np.testing.assert_allclose(q.grad.cpu().numpy(), ref, rtol=2e-3, atol=2e-4 * max(1e-2, float(np.abs(ref).max())), err_msg=f"{tag} {k}")
            n_checked += 1
    assert n_checked >= min_grads, (tag, n_checked)
    for k, v in net.state_dict().items():
        if "running" in k:
            np.testing.assert_allclose(v.cpu().numpy(), ref_running[k], rtol=1e-4, atol=1e-5, err_msg=f"{tag} {k}")


@gpu
@pytest.mark.parametrize("case", ["simple", "towers", "complex"])
def test_superpixel_net_vs_reference_fixture(golden, case):
    import dgn_amd
    from dgn_amd.nets import DGNSuperpixelNet, accuracy_mnist_cifar
    g = golden("g16_superpixel_net")
    dev = torch.device("cuda")
    p = fixture_net_params(g, case)
    net = DGNSuperpixelNet(p)
    sd = {k.split("sd::", 1)[1]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith(f"{case}/sd::")}
    assert set(sd) == set(net.state_dict()), set(sd) ^ set(net.state_dict())
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train(True)
    N = int(g["N"])
    graph = dgn_amd.DGNGraph(torch.from_numpy(g["src"]).to(dev), torch.from_numpy(g["dst"]).to(dev), N, eig=torch.from_numpy(g["eig"]).to(dev))
    graph.batch_num_nodes = [int(s) for s in g["sizes"]]
    feats = torch.from_numpy(g["feats"]).to(dev)[:, :p["in_dim"]]            # (a column slice: row stride 5 for in_dim 3)
    e = torch.from_numpy(g["evals"]).to(dev) if p["edge_feat"] else None
    snorm, labels = torch.from_numpy(g["snorm"]).to(dev), torch.from_numpy(g[f"{case}/labels"]).to(dev)
    assert dgn_amd.ops.feature_embedding_supported(feats, net.embedding_h.weight)
    scores = net(graph, feats, e, snorm, None)
    assert tuple(scores.shape) == (len(g["sizes"]), 10)
    loss, hits = net.loss(scores, labels, hits=True)
    assert net.loss(scores, labels).item() == loss.item()
    loss.backward()
    _assert_net_quantities(case, scores, loss, net, g[f"{case}/scores"], g[f"{case}/loss"],
                           {k: g[f"{case}/gp::{k}"] for k, _ in net.named_parameters() if f"{case}/gp::{k}" in g},
                           {k: g[f"{case}/after::{k}"] for k in net.state_dict() if "running" in k}, 15)
    assert net.embedding_h.weight.grad is not None and (not p["edge_feat"] or net.embedding_e.weight.grad is not None)
    # the fixture's top-two gaps are >= 1e-3 (asserted by its generator), far above the scores' tolerance: same predictions
    assert hits.is_cuda and hits.dim() == 0 and int(hits) == int(g[f"{case}/hits"]) == int(accuracy_mnist_cifar(scores, labels))


def _superpixel_batch(dev, n_graphs, seed, with_px=1):
    """Seeded coordinates and mean pixel values of ``n_graphs`` graphs of 12-30 nodes through the preparation chain on the device."""
    import dgn_amd
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.randint(12, 31, (n_graphs,), generator=gen).tolist()
    N = sum(sizes)
    coord, px = torch.rand(N, 2, generator=gen).to(dev), torch.rand(N, with_px, generator=gen).to(dev)
    src, dst, value = dgn_amd.knn_graph(coord, sizes, feat=px)
    eig = dgn_amd.superpixel_eig(dgn_amd.DGNGraph(src, dst, N), coord, sizes)
    graph = dgn_amd.DGNGraph(src, dst, N, eig=eig)
    graph.batch_num_nodes = sizes
    snorm = torch.cat([torch.full((n, 1), 1.0 / n) for n in sizes]).sqrt().to(dev)
    return graph, torch.cat([px, coord], dim=1), value.unsqueeze(1), snorm, sizes


@gpu
@pytest.mark.parametrize("type_net,edge_feat,mode", [("simple", False, "mean"), ("complex", True, "sum")])
def test_preparation_chain_into_the_net_equals_the_hand_composition(type_net, edge_feat, mode):
    """knn_graph -> DGNGraph -> superpixel_eig -> net -> loss -> backward against F.linear, the same layer modules, readout, the same head
    and F.cross_entropy on the same weights."""
    from dgn_amd.nets import DGNSuperpixelNet
    from dgn_amd.readout import readout
    dev = torch.device("cuda")
    torch.manual_seed(2)
    net = DGNSuperpixelNet(superpixel_net_params(type_net, 20, 3, "mean dir1-dx dir2-dx", "identity amplification", mode, edge_feat))
    with torch.no_grad():                                       # (wider than the stock gain = 1 / in_size head: scores away from 0)
        for fc in net.MLP_layer.FC_layers:
            fc.weight.normal_(0.0, (2.0 / fc.weight.shape[1]) ** 0.5)
    net = net.to(dev).train()
    hand = copy.deepcopy(net)
    graph, feats, evals, snorm, sizes = _superpixel_batch(dev, 6, seed=12)
    labels = torch.randint(0, 10, (6,), generator=torch.Generator().manual_seed(1)).to(dev)
    h = F.linear(feats, hand.embedding_h.weight, hand.embedding_h.bias)
    e = F.linear(evals, hand.embedding_e.weight, hand.embedding_e.bias) if edge_feat else None
    for conv in hand.layers:
        h = conv(graph, h, e, snorm)
    ref_scores = hand.MLP_layer(readout(graph, h, mode))
    ref_loss = F.cross_entropy(ref_scores, labels)
    ref_loss.backward()
    scores = net(graph, feats, evals if edge_feat else None, snorm, None)
    loss, hits = net.loss(scores, labels, hits=True)
    loss.backward()
    assert float(ref_scores.detach().std()) > 0.1
    _assert_net_quantities(type_net, scores, loss, net, ref_scores.detach().cpu().numpy(), ref_loss.item(),
                           {k: q.grad.cpu().numpy() for k, q in hand.named_parameters() if q.grad is not None},
                           {k: v.cpu().numpy() for k, v in hand.state_dict().items() if "running" in k}, 15)
    gap = spo.top_gap(ref_scores.detach().cpu(), labels.cpu())
    print(f"chain {type_net}: top-two gap of the hand composition {gap:.2e}")
    if gap > 1e-3:                                              # (above the scores' tolerance: same predictions)
        assert int(hits) == spo.hits(ref_scores.detach().cpu(), labels.cpu())


CIFAR_SMALL = dict(type_net="simple", hidden=65, in_dim=5, aggs="mean dir1-dx dir2-dx", scalers="identity", readout="mean")


def _knn_batches(dev, graph_counts, seed0, in_dim):
    from dgn_amd import synth
    gen = torch.Generator().manual_seed(5)
    batches = []
    for i, n_graphs in enumerate(graph_counts):
        b = synth.knn_batch(n_graphs, seed=seed0 + i, n_lo=12, n_hi=30)
        N = int(b["num_nodes"])
        batches.append(dict(src=b["src"].to(dev), dst=b["dst"].to(dev), N=N, eig=b["eig"].to(dev), sizes=[int(s) for s in b["sizes"]],
                            feats=torch.rand(N, in_dim, generator=gen).to(dev), snorm=b["snorm_n"].to(dev),
                            y=torch.randint(0, 10, (n_graphs,), generator=gen).to(dev)))
    return batches


@gpu
def test_captured_superpixel_step_equals_eager_training():
    """hipgraph.CapturedSuperpixelStep (forward, cross-entropy + hit count, backward, optimizer as ONE HIP graph over capacity-padded static
    buffers, label -1 on the graph rows behind the batch) against eager training on the unpadded batches: per-step losses, hit counts,
    parameters and running statistics after four batches of different sizes through one capacity.  Plain SGD on both sides (see
    tests/test_net_gpu.py).  The shipped CIFAR10 layer in small: simple, hidden 65, in_dim 5, one scaler."""
    import dgn_amd
    from dgn_amd.hipgraph import CapturedSuperpixelStep, rewrap_parameters
    from dgn_amd.nets import DGNSuperpixelNet
    dev = torch.device("cuda")
    torch.manual_seed(3)
    c = CIFAR_SMALL
    net_e = DGNSuperpixelNet(superpixel_net_params(c["type_net"], c["hidden"], c["in_dim"], c["aggs"], c["scalers"], c["readout"], False))
    net_e = net_e.to(dev).train()
    with torch.no_grad():
        for fc in net_e.MLP_layer.FC_layers:
            fc.weight.normal_(0.0, (2.0 / fc.weight.shape[1]) ** 0.5)
    net_c = copy.deepcopy(net_e)
    batches = _knn_batches(dev, (6, 9, 4, 8), 80, c["in_dim"])
    order = [0, 0, 1, 2, 3, 1]                                  # (the first two = the capture's warm-up steps on batch 0)
    opt = torch.optim.SGD(net_e.parameters(), lr=1e-2)
    losses_e, hits_e, gaps_e = [], [], []
    for i in order:
        b = batches[i]
        g = dgn_amd.DGNGraph(b["src"], b["dst"], b["N"], eig=b["eig"])
        g.batch_num_nodes = b["sizes"]
        opt.zero_grad(set_to_none=True)
        scores = net_e(g, b["feats"], None, b["snorm"], None)
        loss, hits = net_e.loss(scores, b["y"], hits=True)
        loss.backward()
        opt.step()
        losses_e.append(loss.item())
        hits_e.append(int(hits))
        gaps_e.append(spo.top_gap(scores.detach().cpu(), b["y"].cpu()))
    n_cap = max(b["N"] for b in batches) + 40
    e_cap = max(b["src"].numel() for b in batches) + 64
    rewrap_parameters(net_c)
    cs = CapturedSuperpixelStep(net_c, n_cap, e_cap, g_cap=12, eig_dim=batches[0]["eig"].shape[1],
                                optimizer=torch.optim.SGD(net_c.parameters(), lr=1e-2))
    assert cs.atoms.shape == (n_cap, c["in_dim"]) and cs.atoms.dtype == torch.float32
    assert cs.targets.dtype == torch.int64 and cs.targets.shape == (cs.g_rows,) and bool((cs.targets == -1).all())
    load = lambda b: cs.load(b["src"], b["dst"], b["N"], b["eig"], b["feats"], b["snorm"], b["sizes"], b["y"])
    load(batches[0])
    cs.capture(warmup=2)
    losses_c, hits_c = [], []
    for i in order[2:]:
        load(batches[i])
        n_graphs = len(batches[i]["sizes"])
        assert bool((cs.targets[n_graphs:] == -1).all()) and bool((cs.atoms[batches[i]["N"]:] == 0).all())
        loss, hits = cs.step()
        assert loss.is_cuda and hits.is_cuda and hits.dtype == torch.int64
        losses_c.append(float(loss))
        hits_c.append(int(hits))
    np.testing.assert_allclose(losses_c, losses_e[2:], rtol=2e-4, atol=1e-5)
    for j, (a, b_) in enumerate(zip(hits_c, hits_e[2:])):
        assert 0 <= a <= len(batches[order[2 + j]]["sizes"])      # the padding rows are counted nowhere
        if gaps_e[2 + j] > 1e-4:
            print(f"captured superpixel step {j}: eager top-two gap {gaps_e[2 + j]:.2e} > 1e-4: hit counts compared exactly")
            assert a == b_, (j, a, b_)
        else:
            print(f"captured superpixel step {j}: eager top-two gap {gaps_e[2 + j]:.2e} <= 1e-4: hit counts within one")
            assert abs(a - b_) <= 1, (j, a, b_)
    for (k, a), (_, b_) in zip(net_c.named_parameters(), net_e.named_parameters()):
        np.testing.assert_allclose(a.detach().cpu().numpy(), b_.detach().cpu().numpy(), rtol=1e-4, atol=2e-5, err_msg=k)
    for (k, a), (_, b_) in zip(net_c.state_dict().items(), net_e.state_dict().items()):
        if "running" in k:
            np.testing.assert_allclose(a.cpu().numpy(), b_.cpu().numpy(), rtol=1e-3, atol=1e-5, err_msg=k)


@gpu
def test_captured_superpixel_step_refuses_edge_features():
    from dgn_amd.hipgraph import CapturedSuperpixelStep
    from dgn_amd.nets import DGNSuperpixelNet
    net = DGNSuperpixelNet(superpixel_net_params("complex", 19, 3, "mean dir1-dx", "identity", "mean", True)).cuda()
    before = [id(q) for q in net.parameters()]
    with pytest.raises(ValueError, match="CapturedSuperpixelStep: nets with edge_feat=True are not supported"):
        CapturedSuperpixelStep(net, 256, 2048, g_cap=8, eig_dim=3)
    assert [id(q) for q in net.parameters()] == before           # a refused construction leaves the net's Parameter objects alone
