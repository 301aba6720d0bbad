"""The node-classification net (dgn_amd.nets.DGNNodeNet) against fixture G11 -- the reference's own PATTERN / CLUSTER net
(nets/SBMs_node_classification/dgn_net.py) on the same batch with the same weights: scores, balanced cross-entropy, every parameter
gradient, BatchNorm running statistics, accuracy_SBM -- and hipgraph.CapturedNodeStep against eager training.  Tolerances: those of
tests/test_net_gpu.py for the same quantities of the graph-regression net."""
import copy

import numpy as np
import pytest
import torch

import node_ce_oracle as nco
from test_node_ce_oracle_vs_golden import node_net_params

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("case", ["complex", "simple"])
def test_node_net_vs_reference_fixture(golden, case):
    import dgn_amd
    from dgn_amd.nets import DGNNodeNet, accuracy_sbm
    g = golden("g11_node_net")
    dev = torch.device("cuda")
    type_net, hidden, aggs, scalers, n_classes = [str(x) for x in g[f"{case}/cfg"]]
    net = DGNNodeNet(node_net_params(type_net, int(hidden), aggs, scalers, int(n_classes), "cuda"))
    sd = {k.split("sd::", 1)[1]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith(f"{case}/sd::")}
    assert set(sd) == set(net.state_dict()), set(sd) ^ set(net.state_dict())
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train(True)
    N = int(g["N"])
    graph = dgn_amd.DGNGraph(torch.from_numpy(g["src"]).to(dev), torch.from_numpy(g["dst"]).to(dev), N, eig=torch.from_numpy(g["eig"]).to(dev))
    graph.batch_num_nodes = [int(s) for s in g["sizes"]]
    feats, snorm = torch.from_numpy(g["feats"]).to(dev), torch.from_numpy(g["snorm"]).to(dev)
    labels = torch.from_numpy(g[f"{case}/labels"]).to(dev)
    scores = net(graph, feats, None, snorm, None)
    assert tuple(scores.shape) == (N, int(n_classes))
    loss, cm = net.loss(scores, labels, confusion=True)
    assert net.loss(scores, labels).item() == loss.item()
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
    assert n_checked >= 15
    for k, v in net.state_dict().items():
        if "running" in k:
            np.testing.assert_allclose(v.cpu().numpy(), g[f"{case}/after::{k}"], rtol=1e-4, atol=1e-5, err_msg=k)
    # the fixture's prediction gaps are >= 1e-3 (asserted by its generator), far above the scores' tolerance: same predictions
    ref_scores, ref_labels = torch.from_numpy(g[f"{case}/scores"]), torch.from_numpy(g[f"{case}/labels"])
    assert torch.equal(cm.cpu(), nco.confusion_matrix(ref_scores, ref_labels, int(n_classes)))
    assert abs(float(accuracy_sbm(cm)) - float(g[f"{case}/acc"])) <= 1e-4
    if case == "simple":
        assert int(cm[3].sum()) == 0                                  # the class absent from the labels


def _sbm_batches(dev, n_classes, graph_counts, seed0):
    from dgn_amd import synth
    gen = torch.Generator().manual_seed(5)
    batches = []
    for i, n_graphs in enumerate(graph_counts):
        b = synth.sbm_batch(n_graphs, seed=seed0 + i)
        N = int(b["num_nodes"])
        batches.append(dict(src=b["src"].to(dev), dst=b["dst"].to(dev), N=N, eig=b["eig"].to(dev), sizes=[int(s) for s in b["sizes"]],
                            feats=torch.randint(0, 3, (N,), generator=gen).to(dev), snorm=b["snorm_n"].to(dev),
                            y=torch.randint(0, n_classes, (N,), generator=gen).to(dev)))
    return batches


PATTERN_SMALL = dict(type_net="complex", hidden=47, aggs="mean dir1-dx dir2-dx", scalers="identity amplification attenuation", n_classes=2)


@gpu
def test_captured_node_step_equals_eager_training():
    """hipgraph.CapturedNodeStep (forward, balanced cross-entropy + confusion matrix, backward, optimizer as ONE HIP graph over
    capacity-padded static buffers, label -1 behind the batch) against eager training on the unpadded batches: per-step losses, confusion
    matrices, parameters and running statistics after four batches of different sizes through one capacity.  Plain SGD on both sides (see
    tests/test_net_gpu.py).  PATTERN's layer in small: complex, odd hidden size 47, three scalers."""
    import dgn_amd
    from dgn_amd.hipgraph import CapturedNodeStep, rewrap_parameters
    from dgn_amd.nets import DGNNodeNet, accuracy_sbm
    dev = torch.device("cuda")
    torch.manual_seed(3)
    C = PATTERN_SMALL["n_classes"]
    net_e = DGNNodeNet(node_net_params(PATTERN_SMALL["type_net"], PATTERN_SMALL["hidden"], PATTERN_SMALL["aggs"], PATTERN_SMALL["scalers"], C, "cuda"))
    net_e = net_e.to(dev).train()
    with torch.no_grad():                                       # (wider than the stock gain = 1 / in_size head: scores away from 0)
        for fc in net_e.MLP_layer.FC_layers:
            fc.weight.normal_(0.0, (2.0 / fc.weight.shape[1]) ** 0.5)
    net_c = copy.deepcopy(net_e)
    batches = _sbm_batches(dev, C, (6, 9, 4, 8), 70)
    order = [0, 0, 1, 2, 3, 1]                                  # (the first two = the capture's warm-up steps on batch 0)
    opt = torch.optim.SGD(net_e.parameters(), lr=1e-2)
    losses_e, cms_e, gaps_e = [], [], []
    for i in order:
        b = batches[i]
        g = dgn_amd.DGNGraph(b["src"], b["dst"], b["N"], eig=b["eig"])
        g.batch_num_nodes = b["sizes"]
        opt.zero_grad(set_to_none=True)
        scores = net_e(g, b["feats"], None, b["snorm"], None)
        loss, cm = net_e.loss(scores, b["y"], confusion=True)
        loss.backward()
        opt.step()
        losses_e.append(float(loss))
        cms_e.append(cm.cpu())
        gaps_e.append(nco.prediction_gap(scores.detach().cpu(), b["y"].cpu()))
    n_cap = max(b["N"] for b in batches) + 40
    e_cap = max(b["src"].numel() for b in batches) + 64
    rewrap_parameters(net_c)
    cs = CapturedNodeStep(net_c, n_cap, e_cap, eig_dim=batches[0]["eig"].shape[1], optimizer=torch.optim.SGD(net_c.parameters(), lr=1e-2))
    load = lambda b: cs.load(b["src"], b["dst"], b["N"], b["eig"], b["feats"], b["snorm"], b["y"], b["sizes"])
    load(batches[0])
    cs.capture(warmup=2)
    losses_c, cms_c = [], []
    for i in order[2:]:
        load(batches[i])
        loss, cm = cs.step()
        assert loss.is_cuda and cm.is_cuda
        losses_c.append(float(loss))
        cms_c.append(cm.cpu().clone())
    np.testing.assert_allclose(losses_c, losses_e[2:], rtol=2e-4, atol=1e-5)
    for j, (a, b_) in enumerate(zip(cms_c, cms_e[2:])):
        assert int(a.sum()) == batches[order[2 + j]]["N"]         # the padding rows are counted nowhere
        if gaps_e[2 + j] > 1e-4:
            print(f"captured node step {j}: eager prediction gap {gaps_e[2 + j]:.2e} > 1e-4: confusion matrices compared exactly")
            assert torch.equal(a, b_), (j, a, b_)
        else:
            print(f"captured node step {j}: eager prediction gap {gaps_e[2 + j]:.2e} <= 1e-4: accuracies compared with the loss tolerance")
            np.testing.assert_allclose(float(accuracy_sbm(a)), float(accuracy_sbm(b_)), rtol=2e-4, atol=1e-5)
    for (k, a), (_, b_) in zip(net_c.named_parameters(), net_e.named_parameters()):
        np.testing.assert_allclose(a.detach().cpu().numpy(), b_.detach().cpu().numpy(), rtol=1e-4, atol=2e-5, err_msg=k)
    for (k, a), (_, b_) in zip(net_c.state_dict().items(), net_e.state_dict().items()):
        if "running" in k:
            np.testing.assert_allclose(a.cpu().numpy(), b_.cpu().numpy(), rtol=1e-3, atol=1e-5, err_msg=k)


@gpu
def test_captured_node_step_default_optimizer_trains():
    """The default construction (parameters re-wrapped, fused capturable Adam): the loss of a fixed batch goes down over 60 replays."""
    from dgn_amd.hipgraph import CapturedNodeStep
    from dgn_amd.nets import DGNNodeNet
    dev = torch.device("cuda")
    torch.manual_seed(0)
    net = DGNNodeNet(node_net_params("complex", 47, PATTERN_SMALL["aggs"], PATTERN_SMALL["scalers"], 2, "cuda", L=2)).to(dev).train()
    (b,) = _sbm_batches(dev, 2, (8,), 90)
    b["y"] = (b["feats"] > 0).long()                              # a learnable target: the class follows the node type
    cs = CapturedNodeStep(net, b["N"] + 50, b["src"].numel() + 50, eig_dim=b["eig"].shape[1], lr=5e-3)
    cs.load(b["src"], b["dst"], b["N"], b["eig"], b["feats"], b["snorm"], b["y"], b["sizes"])
    cs.capture(warmup=2)
    first = float(cs.step()[0])
    for _ in range(60):
        last = float(cs.step()[0])
    assert np.isfinite(last) and last < 0.7 * first, (first, last)
    assert int(cs.step()[1].sum()) == b["N"]
