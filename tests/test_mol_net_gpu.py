"""The OGB molecule nets (dgn_amd.nets.DGNHIVNet / DGNPCBANet) against fixture G13 -- the reference's own nets
(nets/HIV_graph_classification/dgn_net.py, nets/PCBA_graph_classification/dgn_net.py) on the same batch with the same weights: scores,
masked binary cross-entropy, every parameter gradient, BatchNorm running statistics -- and hipgraph.CapturedMolStep against eager
training.  Tolerances: those of tests/test_node_net_gpu.py for the same quantities of the node-classification net."""
import copy

import numpy as np
import pytest
import torch

from test_mol_oracle_vs_golden import mol_net_params, mol_state_dict

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("case", ["hiv_simple", "pcba_towers_vn", "hiv_complex_edge"])
def test_mol_net_vs_reference_fixture(golden, case):
    import dgn_amd
    from dgn_amd.nets import DGNHIVNet, DGNPCBANet
    g = golden("g13_mol_nets")
    dev = torch.device("cuda")
    which, params = mol_net_params(g[f"{case}/cfg"], "cuda")
    net = (DGNHIVNet if which == "hiv" else DGNPCBANet)(params)
    sd = mol_state_dict(g, case)
    assert set(sd) == set(net.state_dict()), set(sd) ^ set(net.state_dict())
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train(True)
    N = int(g["N"])
    graph = dgn_amd.DGNGraph(torch.from_numpy(g["src"]).to(dev), torch.from_numpy(g["dst"]).to(dev), N, eig=torch.from_numpy(g["eig"]).to(dev))
    graph.batch_num_nodes = [int(s) for s in g["sizes"]]
    graph.ndata["pos_enc"] = torch.from_numpy(g["pos_enc"]).to(dev)
    atoms, snorm = torch.from_numpy(g["atoms"]).to(dev), torch.from_numpy(g["snorm"]).to(dev)
    bonds = torch.from_numpy(g["bonds"]).to(dev) if params["edge_feat"] else None
    labels = torch.from_numpy(g[f"{case}/labels"]).to(dev)
    # the encoders alone: bit-equal to the reference's
    assert net.embedding_h(atoms).detach().cpu().numpy().tobytes() == g[f"{case}/h0"].tobytes()
    if params["edge_feat"]:
        assert net.embedding_e(bonds).detach().cpu().numpy().tobytes() == g[f"{case}/e0"].tobytes()
        feats = net.embedding_e.edge_type_features(bonds, graph)
        assert isinstance(feats, dgn_amd.EdgeTypeFeatures) and tuple(feats.table.shape) == (60, params["edge_dim"])
        assert feats.dense().detach().cpu().numpy().tobytes() == g[f"{case}/e0"].tobytes()
        assert net.embedding_e.combined_types(bonds, graph) is feats.types               # computed once per batch, cached on the graph
    scores = net(graph, atoms, bonds, snorm, None)
    assert tuple(scores.shape) == (len(g["sizes"]), 1 if which == "hiv" else 128)
    loss = net.loss(scores, labels)
    np.testing.assert_allclose(scores.detach().cpu().numpy(), g[f"{case}/scores"], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(loss.item(), float(g[f"{case}/loss"]), rtol=1e-5)
    if which == "pcba":                                          # the reference loop's form: 1-D, selected by the boolean index
        lab = labels == labels
        np.testing.assert_allclose(net.loss(scores[lab], labels[lab]).item(), float(g[f"{case}/loss"]), rtol=1e-5)
    loss.backward()
    n_checked = 0
    for k, q in net.named_parameters():
        key = f"{case}/gp::{k}"
        if key in g:
            ref = g[key]
            np.testing.assert_allclose(q.grad.cpu().numpy(), ref, rtol=2e-3, atol=2e-4 * max(1e-2, float(np.abs(ref).max())), err_msg=k)
            n_checked += 1
    assert n_checked >= 24                                       # nine atom tables, at least three layers' and the head's tensors
    for i in range(9):
        assert f"{case}/gp::embedding_h.atom_embedding_list.{i}.weight" in g
    for k, v in net.state_dict().items():
        if "running" in k:
            np.testing.assert_allclose(v.cpu().numpy(), g[f"{case}/after::{k}"], rtol=1e-4, atol=1e-5, err_msg=k)


HIV_JSON = dict(L=4, hidden_dim=70, out_dim=70, type_net="simple", residual=True, edge_feat=False, readout="mean", in_feat_dropout=0.0,
                dropout=0.0, graph_norm=False, batch_norm=True, aggregators="mean max min dir1-dx dir1-av", scalers="identity", towers=5,
                divide_input_first=False, divide_input_last=True, edge_dim=0, pretrans_layers=1, posttrans_layers=1, pos_enc_dim=0)


def _mol_batches(dev, graph_counts, seed0):
    from dgn_amd import synth
    from dgn_amd.nets import OGB_ATOM_DIMS
    gen = torch.Generator().manual_seed(5)
    batches = []
    for i, n_graphs in enumerate(graph_counts):
        b = synth.molecule_batch(n_graphs, seed=seed0 + i, laplacian_eig=False)
        N = int(b["num_nodes"])
        atoms = torch.stack([torch.randint(0, d, (N,), generator=gen) for d in OGB_ATOM_DIMS], 1)
        batches.append(dict(src=b["src"].to(dev), dst=b["dst"].to(dev), N=N, eig=b["eig"].to(dev), sizes=[int(s) for s in b["sizes"]],
                            atoms=atoms.to(dev), snorm=b["snorm_n"].to(dev), y=torch.randint(0, 2, (n_graphs,), generator=gen).to(dev)))
    return batches


@gpu
def test_captured_mol_step_equals_eager_training():
    """hipgraph.CapturedMolStep (AtomEncoder, layers, readout, head, masked BCE, backward, optimizer as ONE HIP graph over capacity-padded
    static buffers, NaN labels behind the batch) against eager training on the unpadded batches: per-step losses, parameters and running
    statistics after three batches of different sizes through one capture at a 128-graph capacity.  The shipped HIV json's net
    parameters with dropout 0; plain SGD on both sides (see tests/test_net_gpu.py).

    The head is re-drawn at variance 0.5 / fan-in: wider than the stock gain, so that the scores reach ~1.5 and the sigmoid leaves its
    linear part, and no wider, because the comparison is only as sharp as the training run is well conditioned.  The weights in front of
    a BatchNorm are scale invariant, so their gradient grows as their norm shrinks; at variance 2 / fan-in the first step at lr 1e-2 moves
    them by ten times their norm (|grad| 36 against |w| 0.03), and from there EAGER training against ITSELF, with every parameter
    changed by one ulp after the first step, is 1e-3 apart in the loss and 3e-2 in the parameters four steps later (measured on the
    MI355X) -- while the padded step's gradients from identical parameters are within 5e-7 of the eager ones at each of the five steps.
    At 0.5 / fan-in the same one-ulp experiment stays at rounding level, so a difference beyond the tolerances is the step's own."""
    import dgn_amd
    from dgn_amd.hipgraph import CapturedMolStep, rewrap_parameters
    from dgn_amd.nets import DGNHIVNet
    dev = torch.device("cuda")
    torch.manual_seed(3)
    net_e = DGNHIVNet(dict(HIV_JSON, avg_d={"log": torch.tensor(1.1)}, device="cuda")).to(dev).train()
    with torch.no_grad():                                       # (see the docstring)
        for fc in net_e.MLP_layer.FC_layers:
            fc.weight.normal_(0.0, (0.5 / fc.weight.shape[1]) ** 0.5)
    net_c = copy.deepcopy(net_e)
    batches = _mol_batches(dev, (128, 97, 113), 80)
    order = [0, 0, 1, 2, 0]                                     # (the first two = the capture's warm-up steps on batch 0)
    opt = torch.optim.SGD(net_e.parameters(), lr=1e-2)
    losses_e = []
    for i in order:
        b = batches[i]
        g = dgn_amd.DGNGraph(b["src"], b["dst"], b["N"], eig=b["eig"])
        g.batch_num_nodes = b["sizes"]
        opt.zero_grad(set_to_none=True)
        loss = net_e.loss(net_e(g, b["atoms"], None, b["snorm"], None), b["y"])
        loss.backward()
        opt.step()
        losses_e.append(float(loss))
    n_cap = max(b["N"] for b in batches) + 40
    e_cap = max(b["src"].numel() for b in batches) + 64
    rewrap_parameters(net_c)
    cs = CapturedMolStep(net_c, n_cap, e_cap, g_cap=129, eig_dim=batches[0]["eig"].shape[1], optimizer=torch.optim.SGD(net_c.parameters(), lr=1e-2))
    assert tuple(cs.atoms.shape) == (n_cap, 9) and tuple(cs.targets.shape) == (cs.g_rows, 1) and bool(torch.isnan(cs.targets).all())
    load = lambda b: cs.load(b["src"], b["dst"], b["N"], b["eig"], b["atoms"], b["snorm"], b["sizes"], b["y"])
    load(batches[0])
    cs.capture(warmup=2)
    losses_c = []
    for i in order[2:]:
        load(batches[i])
        G = len(batches[i]["sizes"])
        assert bool(torch.isnan(cs.targets[G:]).all()) and not bool(torch.isnan(cs.targets[:G]).any())
        loss = cs.step()
        assert loss.is_cuda
        losses_c.append(float(loss))
    np.testing.assert_allclose(losses_c, losses_e[2:], rtol=2e-4, atol=1e-5)
    for (k, a), (_, b_) in zip(net_c.named_parameters(), net_e.named_parameters()):
        np.testing.assert_allclose(a.detach().cpu().numpy(), b_.detach().cpu().numpy(), rtol=1e-4, atol=2e-5, err_msg=k)
    for (k, a), (_, b_) in zip(net_c.state_dict().items(), net_e.state_dict().items()):
        if "running" in k:
            np.testing.assert_allclose(a.cpu().numpy(), b_.cpu().numpy(), rtol=1e-3, atol=1e-5, err_msg=k)


@gpu
def test_captured_mol_step_refusals():
    from dgn_amd.hipgraph import CapturedMolStep
    from dgn_amd.nets import DGNHIVNet, DGNPCBANet
    dev = torch.device("cuda")
    base = dict(HIV_JSON, avg_d={"log": torch.tensor(1.1)}, device="cuda", L=2, hidden_dim=20, out_dim=20)
    with pytest.raises(ValueError, match="edge_feat"):
        CapturedMolStep(DGNHIVNet(dict(base, type_net="complex", edge_feat=True, edge_dim=6)).to(dev), 512, 2048, g_cap=17, eig_dim=3)
    with pytest.raises(ValueError, match="virtual_node"):
        CapturedMolStep(DGNPCBANet(dict(base, decreasing_dim=True, virtual_node="sum")).to(dev), 512, 2048, g_cap=17, eig_dim=3)
    with pytest.raises(ValueError, match="pos_enc_dim"):
        CapturedMolStep(DGNHIVNet(dict(base, pos_enc_dim=2)).to(dev), 512, 2048, g_cap=17, eig_dim=3)
    # without a virtual node the PCBA net is captured like the HIV one: 128 label columns
    cs = CapturedMolStep(DGNPCBANet(dict(base, decreasing_dim=True, virtual_node=None)).to(dev), 512, 2048, g_cap=17, eig_dim=3)
    assert tuple(cs.targets.shape) == (cs.g_rows, 128)
