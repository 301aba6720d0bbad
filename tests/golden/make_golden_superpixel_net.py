#!/usr/bin/env python3
"""Generate the superpixel graph-classification fixtures by IMPORTING the reference (see make_golden.py for the stubs and the rules:
arrays and short config strings only, no reference source or bytecode).

    python tests/golden/make_golden_superpixel_net.py            # rewrites g16_superpixel_net.npz and g17_class_ce.npz

* ``g17_class_ce``: the reference's own ``DGNNet.loss`` (nets/superpixels_graph_classification/dgn_net.py:75-78, called unbound: it does
  not read ``self``) and ``accuracy_MNIST_CIFAR`` (train/metrics.py:25-28) on seeded scores (std 3) and labels.  Rows whose two best
  scores are closer than 4e-4 are nudged apart, so that fp32 and fp64 evaluations agree on every prediction (asserted: gap >= 1e-4 in both);
  one case has scores around +-80; the case ``ties`` instead places EXACT ties on purpose -- between two columns that are not the label,
  between the label and a later column (a hit under the first-maximum rule) and between an earlier column and the label (a miss).
* ``g16_superpixel_net``: the unmodified net in training mode on ``make_test_graph``, dropout 0.  The MLP head's weights are re-drawn wider
  than the reference's ``gain = 1 / in_size`` initialisation (stored in the fixture): with the stock initialisation every score is ~0 and
  the loss is ln C whatever the code under test does.  The labels are chosen after the forward pass: the first two graphs carry their
  predicted class, the last one the class after it (two hits of three).
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))          # tests/: superpixel_net_oracle (the nudge)

import numpy as np
import torch

from make_golden import FakeGraph, _install_stubs, make_test_graph

torch.set_num_threads(1)


def _reference_tail():
    from nets.superpixels_graph_classification.dgn_net import DGNNet
    from train.metrics import accuracy_MNIST_CIFAR
    return DGNNet, accuracy_MNIST_CIFAR


def _tie_case(gen):
    """12 rows of 10 classes: rows 0-3 tie two non-label columns at the top, rows 4-7 tie the label with a LATER column (hits), rows 8-11
    tie an EARLIER column with the label (misses)."""
    import superpixel_net_oracle as spo
    G, C = 12, 10
    scores = spo.nudge_scores(3.0 * torch.randn(G, C, generator=gen))
    labels = torch.tensor([0, 9, 4, 5, 0, 3, 6, 8, 1, 4, 7, 9])
    others = [(2, 7), (1, 3), (5, 9), (0, 8), (0, 4), (3, 9), (6, 7), (8, 9), (0, 1), (2, 4), (3, 7), (8, 9)]
    for r, (a, b) in enumerate(others):
        top = float(scores[r].max()) + 1.0
        scores[r, a] = scores[r, b] = top
    assert all(labels[r] not in others[r] for r in range(4))
    assert all(int(labels[r]) == others[r][0] for r in range(4, 8)) and all(int(labels[r]) == others[r][1] for r in range(8, 12))
    return scores, labels


def g17_class_ce(out):
    import superpixel_net_oracle as spo
    DGNNet, accuracy = _reference_tail()
    shapes = [(1, 2), (2, 10), (63, 10), (64, 10), (65, 10), (257, 10), (1000, 3), (130, 64)]
    cases = [(f"g{G}_c{C}", G, C, "plain") for G, C in shapes] + [("big_g64_c10", 64, 10, "big"), ("ties", 12, 10, "ties")]
    out["cases"] = np.array([c[0] for c in cases])
    for i, (name, G, C, kind) in enumerate(cases):
        gen = torch.Generator().manual_seed(1700 + i)
        if kind == "ties":
            scores, labels = _tie_case(gen)
            assert spo.top_gap(scores, labels) == 0.0
        else:
            labels = torch.randint(0, C, (G,), generator=gen)
            scores = 3.0 * torch.randn(G, C, generator=gen)
            if kind == "big":                      # scores around +-80: the row maximum has to be taken out before the exponentials
                scores = scores / 3.0 + 80.0 * torch.sign(torch.randn(G, C, generator=gen))
            scores = spo.nudge_scores(scores)
            assert spo.top_gap(scores, labels) >= 1e-4 and spo.top_gap(scores.double(), labels) >= 1e-4, name
        x = scores.clone().requires_grad_(True)
        loss = DGNNet.loss(types.SimpleNamespace(), x, labels)
        (grad,) = torch.autograd.grad(loss, x)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()), name
        hits = accuracy(scores, labels)
        assert hits == spo.hits(scores, labels) == spo.hits(scores.double(), labels), name
        out[f"{name}/scores"], out[f"{name}/labels"] = scores.numpy(), labels.numpy()
        out[f"{name}/loss"], out[f"{name}/grad"], out[f"{name}/hits"] = loss.detach().numpy(), grad.numpy(), np.array(int(hits))
    assert int(out["ties/hits"]) == 4


def g16_superpixel_net(out):
    import superpixel_net_oracle as spo
    DGNNet, accuracy = _reference_tail()
    src, dst, N, sizes = make_test_graph(seed=16)
    out["src"], out["dst"], out["N"], out["sizes"] = src, dst, np.array(N), np.array(sizes)
    gen = torch.Generator().manual_seed(61)
    eig = torch.randn(N, 4, generator=gen)
    feats = torch.rand(N, 5, generator=gen)            # (mean pixel values and coordinates lie in [0, 1]; a case takes its first in_dim columns)
    evals = torch.rand(len(src), 1, generator=gen)     # (the k-NN similarity of an edge lies in (0, 1])
    snorm = torch.rand(N, 1, generator=gen) + 0.5
    out["eig"], out["feats"], out["evals"], out["snorm"] = eig.numpy(), feats.numpy(), evals.numpy(), snorm.numpy()
    # (name, type_net, hidden, in_dim, aggregators, scalers, readout, edge_feat)
    cases = [("simple", "simple", 20, 3, "mean max dir1-av dir1-dx", "identity amplification", "mean", False),
             ("towers", "towers", 20, 5, "mean dir1-dx dir2-dx", "identity", "sum", False),
             ("complex", "complex", 19, 3, "mean dir1-dx dir2-dx", "identity amplification attenuation", "max", True)]
    out["cases"] = np.array([c[0] for c in cases])
    C = 10
    for i, (name, type_net, hidden, in_dim, aggs, scalers, mode, edge_feat) in enumerate(cases):
        torch.manual_seed(16 + i)
        params = dict(in_dim=in_dim, in_dim_edge=1, hidden_dim=hidden, out_dim=hidden, n_classes=C, in_feat_dropout=0.0, dropout=0.0, L=3,
                      type_net=type_net, readout=mode, graph_norm=True, batch_norm=True, residual=True, aggregators=aggs, scalers=scalers,
                      avg_d={"log": torch.tensor(1.1)}, edge_feat=edge_feat, edge_dim=6 if edge_feat else 0, pretrans_layers=1,
                      posttrans_layers=1)
        net = DGNNet(params)
        net.train(True)
        with torch.no_grad():
            for fc in net.MLP_layer.FC_layers:
                fc.weight.copy_(torch.randn(fc.weight.shape, generator=gen) * (2.0 / fc.weight.shape[1]) ** 0.5)
                fc.bias.copy_(0.1 * torch.randn(fc.bias.shape, generator=gen))
        for k, v in net.state_dict().items():
            out[f"{name}/sd::{k}"] = v.detach().numpy().copy()
        g = FakeGraph(src, dst, N)
        g.batch_num_nodes = list(sizes)
        g.ndata["eig"] = eig
        scores = net(g, feats[:, :in_dim], evals if edge_feat else None, snorm, None)
        assert tuple(scores.shape) == (len(sizes), C)
        assert float(scores.detach().std()) >= 0.5, (name, float(scores.detach().std()))
        pred = spo.predictions(scores.detach())
        labels = pred.clone()
        labels[-1] = (pred[-1] + 1) % C
        assert spo.top_gap(scores.detach(), labels) >= 1e-3, (name, spo.top_gap(scores.detach(), labels))
        loss = net.loss(scores, labels)
        names = [k for k, q in net.named_parameters()]
        grads = torch.autograd.grad(loss, [q for _, q in net.named_parameters()], allow_unused=True)
        hits = accuracy(scores, labels)
        assert hits == len(sizes) - 1
        out[f"{name}/cfg"] = np.array([type_net, str(hidden), str(in_dim), aggs, scalers, mode, str(int(edge_feat))])
        out[f"{name}/labels"] = labels.numpy()
        out[f"{name}/scores"], out[f"{name}/loss"], out[f"{name}/hits"] = scores.detach().numpy(), loss.detach().numpy(), np.array(int(hits))
        for k, gr in zip(names, grads):
            if gr is not None:
                out[f"{name}/gp::{k}"] = gr.numpy()
        for k, v in net.state_dict().items():
            if "running" in k:
                out[f"{name}/after::{k}"] = v.detach().numpy().copy()


def main():
    _install_stubs()
    only = sys.argv[1:]
    for fname, fn in (("g16_superpixel_net", g16_superpixel_net), ("g17_class_ce", g17_class_ce)):
        if only and fname not in only:
            continue
        out = {}
        fn(out)
        path = os.path.join(HERE, fname + ".npz")
        np.savez_compressed(path, **out)
        print(f"{fname}: {len(out)} arrays, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
