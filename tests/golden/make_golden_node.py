#!/usr/bin/env python3
"""Generate the node-classification fixtures by IMPORTING the reference (see make_golden.py for the stubs and the rules: arrays and
short config strings only, no reference source or bytecode).

    python tests/golden/make_golden_node.py            # rewrites g11_node_net.npz and g12_node_ce.npz

* ``g12_node_ce``: the reference's own ``DGNNet.loss`` (nets/SBMs_node_classification/dgn_net.py:67-81, called unbound on a namespace that
  carries ``n_classes`` and ``device``) and ``accuracy_SBM`` (train/metrics.py:37-54; scikit-learn's ``confusion_matrix``) on seeded
  scores (std 3) and labels.  Rows whose two best ``scores[n, c] - logsumexp_n scores[:, c]`` are closer than 4e-4 are nudged apart, so
  that fp32 and fp64 evaluations agree on every prediction.  Every finite case has each class id below C among its labels or
  predictions: only then is scikit-learn's matrix the full C x C one that the reference's ``CM[r, r]`` indexing assumes.
* ``g11_node_net``: the unmodified node-classification net in training mode on ``make_test_graph``.  The MLP head's weights are re-drawn
  wider than the reference's ``gain = 1 / in_size`` initialisation (stored in the fixture): with the stock initialisation every score is
  ~0 and the loss is ln C whatever the code under test does.
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))          # tests/: node_ce_oracle (the nudge)

import numpy as np
import torch

from make_golden import FakeGraph, _install_stubs, make_test_graph

torch.set_num_threads(1)


def _reference_tail():
    from nets.SBMs_node_classification.dgn_net import DGNNet
    from train.metrics import accuracy_SBM
    return DGNNet, accuracy_SBM


def _labels(gen, N, C, present):
    """N labels over the classes ``present``, each of them at least once (as far as N allows)."""
    present = torch.tensor(present)
    y = present[torch.randint(0, len(present), (N,), generator=gen)]
    k = min(N, len(present))
    y[:k] = present[:k]
    return y[torch.randperm(N, generator=gen)]


def g12_node_ce(out):
    import node_ce_oracle as nco
    DGNNet, accuracy_SBM = _reference_tail()
    cases = [("n2_c2", 2, 2, [0, 1]), ("n63_c2", 63, 2, [0, 1]), ("n64_c2", 64, 2, [0, 1]), ("n65_c6", 65, 6, list(range(6))),
             ("n1000_c6", 1000, 6, list(range(6))), ("n3001_c2", 3001, 2, [0, 1]),
             ("missing_n500_c6", 500, 6, [0, 2, 3, 5]),           # two of six classes absent from the labels: weights 0 there, finite loss
             ("single_n50_c3", 50, 3, [1])]                       # one class only: every weight 0, nan
    out["cases"] = np.array([c[0] for c in cases])
    for i, (name, N, C, present) in enumerate(cases):
        for attempt in range(50):          # (a draw without a single hit has no accuracy: the reference divides by zero -- unpinned)
            gen = torch.Generator().manual_seed(100 + i + 1000 * attempt)
            labels = _labels(gen, N, C, present)
            scores = nco.nudge_scores(3.0 * torch.randn(N, C, generator=gen), labels)
            if bool((nco.predictions(scores, labels) == labels).any()):
                break
        assert nco.prediction_gap(scores, labels) >= 1e-4 and nco.prediction_gap(scores.double(), labels) >= 1e-4
        x = scores.clone().requires_grad_(True)
        loss = DGNNet.loss(types.SimpleNamespace(n_classes=C, device="cpu"), x, labels)
        (grad,) = torch.autograd.grad(loss, x)
        out[f"{name}/scores"], out[f"{name}/labels"], out[f"{name}/C"] = scores.numpy(), labels.numpy(), np.array(C)
        out[f"{name}/loss"], out[f"{name}/grad"] = loss.detach().numpy(), grad.numpy()
        if len(present) == 1:
            assert bool(torch.isnan(loss)) and bool(torch.isnan(grad).all())
            continue
        assert bool(torch.isfinite(loss))
        pred = nco.predictions(scores, labels)
        assert set(labels.tolist()) | set(pred.tolist()) == set(range(C)), name
        out[f"{name}/acc"] = np.array(float(accuracy_SBM(scores, labels)))
        assert np.isfinite(out[f"{name}/acc"]), name


def g11_node_net(out):
    import node_ce_oracle as nco
    DGNNet, accuracy_SBM = _reference_tail()
    src, dst, N, sizes = make_test_graph(seed=8)
    out["src"], out["dst"], out["N"], out["sizes"] = src, dst, np.array(N), np.array(sizes)
    gen = torch.Generator().manual_seed(33)
    eig = torch.randn(N, 4, generator=gen)
    feats = torch.randint(0, 3, (N,), generator=gen)
    snorm = torch.rand(N, 1, generator=gen) + 0.5
    out["eig"], out["feats"], out["snorm"] = eig.numpy(), feats.numpy(), snorm.numpy()
    # (name, type_net, hidden, aggregators, scalers, n_classes, classes present among the labels)
    cases = [("complex", "complex", 19, "mean dir1-dx dir2-dx", "identity amplification attenuation", 2, [0, 1]),
             ("simple", "simple", 20, "mean max dir1-av dir1-dx", "identity amplification", 6, [0, 1, 2, 4, 5])]
    out["cases"] = np.array([c[0] for c in cases])
    for i, (name, type_net, hidden, aggs, scalers, C, present) in enumerate(cases):
        torch.manual_seed(11 + i)
        params = dict(in_dim=3, hidden_dim=hidden, out_dim=hidden, n_classes=C, in_feat_dropout=0.0, dropout=0.0, L=3, type_net=type_net,
                      pos_enc_dim=0, readout="mean", graph_norm=True, batch_norm=True, aggregators=aggs, scalers=scalers,
                      avg_d={"log": torch.tensor(1.1)}, residual=True, edge_feat=False, edge_dim=0, pretrans_layers=1, posttrans_layers=1,
                      device="cpu")
        net = DGNNet(params)
        net.train(True)
        with torch.no_grad():
            for fc in net.MLP_layer.FC_layers:
                fc.weight.copy_(torch.randn(fc.weight.shape, generator=gen) * (2.0 / fc.weight.shape[1]) ** 0.5)
                fc.bias.copy_(0.1 * torch.randn(fc.bias.shape, generator=gen))
        labels = _labels(gen, N, C, present)
        for k, v in net.state_dict().items():
            out[f"{name}/sd::{k}"] = v.detach().numpy().copy()
        g = FakeGraph(src, dst, N)
        g.batch_num_nodes = list(sizes)
        g.ndata["eig"] = eig
        scores = net(g, feats, None, snorm, None)
        assert float(scores.detach().std()) >= 0.5, name
        assert nco.prediction_gap(scores.detach(), labels) >= 1e-3, name
        loss = net.loss(scores, labels)
        names = [k for k, q in net.named_parameters()]
        grads = torch.autograd.grad(loss, [q for _, q in net.named_parameters()], allow_unused=True)
        pred = nco.predictions(scores.detach(), labels)
        assert set(labels.tolist()) | set(pred.tolist()) == set(range(C)), name
        out[f"{name}/cfg"] = np.array([type_net, str(hidden), aggs, scalers, str(C)])
        out[f"{name}/labels"] = labels.numpy()
        out[f"{name}/scores"], out[f"{name}/loss"] = scores.detach().numpy(), loss.detach().numpy()
        out[f"{name}/acc"] = np.array(float(accuracy_SBM(scores.detach(), labels)))
        for k, gr in zip(names, grads):
            if gr is not None:
                out[f"{name}/gp::{k}"] = gr.numpy()
        for k, v in net.state_dict().items():
            if "running" in k:
                out[f"{name}/after::{k}"] = v.detach().numpy().copy()


def main():
    _install_stubs()
    only = sys.argv[1:]
    for fname, fn in (("g11_node_net", g11_node_net), ("g12_node_ce", g12_node_ce)):
        if only and fname not in only:
            continue
        out = {}
        fn(out)
        path = os.path.join(HERE, fname + ".npz")
        np.savez_compressed(path, **out)
        print(f"{fname}: {len(out)} arrays, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
