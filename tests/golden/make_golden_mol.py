#!/usr/bin/env python3
"""Generate the fixtures of the OGB molecule nets by IMPORTING the reference (see make_golden.py for the stubs and the rules: arrays and
short config strings only, no reference source or bytecode).

    python tests/golden/make_golden_mol.py            # rewrites g13_mol_nets.npz and g14_mol_loss_metrics.npz

The reference's two nets import ``ogb.graphproppred.mol_encoder``.  ogb is a third-party package that is not installed here; a stub module
of that name is registered whose two encoders are RESTATED below from their public definition (one ``nn.Embedding`` per feature column,
xavier-uniform weights, ``x_embedding = 0; x_embedding += emb_i(x[:, i])``), with the feature widths of the ogb releases before 1.3.0.

* ``g13_mol_nets``: the unmodified nets (nets/HIV_graph_classification/dgn_net.py, nets/PCBA_graph_classification/dgn_net.py) in
  training mode on ``make_test_graph``, dropout 0, the MLP head re-drawn wider than the reference's ``gain = 1 / in_size`` initialisation
  (as in G11: with the stock head every score is ~0).  Atom columns are drawn within their widths and skewed (three atoms in four carry
  one type per column).  Losses: PCBA's through the reference loop's own two masking lines (train/train_PCBA_graph_classification.py:
  32-33) in front of the net's ``loss``.  The HIV net's ``loss`` hard-codes ``.to('cuda')`` and cannot run here: the PCBA net's ``loss`` --
  the identical ``BCEWithLogitsLoss()`` -- is called on ``labels.float().unsqueeze(-1)``, the tensor the HIV line forms.
* ``g14_mol_loss_metrics``: seeded (scores, labels) cases; loss and gradient from torch in fp32 and fp64 through that same path (masking
  lines + PCBA ``loss``), ROC-AUC and average precision from scikit-learn applied per task by ogb's evaluator rule (labelled rows of a
  task that has a positive and a negative; the mean over those tasks; nan where there is none).  NaN shares 0 (the single-task cases), 0.4
  and 1; logits at +-100; scores quantised to 0.5 (ties); in every 128-task case task 3 has one class only and, with NaNs, task 5 is
  unmeasured.  The scikit-learn version is recorded in the file.
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch
import torch.nn as nn

from make_golden import FakeGraph, _install_stubs, make_test_graph

torch.set_num_threads(1)

ATOM_DIMS = [119, 4, 12, 12, 10, 6, 6, 2, 2]
BOND_DIMS = [5, 6, 2]


def _install_ogb_stub():
    class _Encoder(nn.Module):
        def __init__(self, emb_dim, dims, name):
            super().__init__()
            embs = nn.ModuleList()
            for dim in dims:
                emb = nn.Embedding(dim, emb_dim)
                nn.init.xavier_uniform_(emb.weight.data)
                embs.append(emb)
            setattr(self, name, embs)
            self._name = name

        def forward(self, x):
            x_embedding = 0
            for i in range(x.shape[1]):
                x_embedding += getattr(self, self._name)[i](x[:, i])
            return x_embedding

    class AtomEncoder(_Encoder):
        def __init__(self, emb_dim):
            super().__init__(emb_dim, ATOM_DIMS, "atom_embedding_list")

    class BondEncoder(_Encoder):
        def __init__(self, emb_dim):
            super().__init__(emb_dim, BOND_DIMS, "bond_embedding_list")

    for name in ("ogb", "ogb.graphproppred", "ogb.graphproppred.mol_encoder"):
        sys.modules.setdefault(name, types.ModuleType(name))
    mod = sys.modules["ogb.graphproppred.mol_encoder"]
    mod.AtomEncoder, mod.BondEncoder = AtomEncoder, BondEncoder


def _reference_nets():
    from nets.HIV_graph_classification.dgn_net import DGNNet as HIVNet
    from nets.PCBA_graph_classification.dgn_net import DGNNet as PCBANet
    return HIVNet, PCBANet


def _masked_reference_loss(PCBANet, scores, labels):
    """train/train_PCBA_graph_classification.py:32-33, then the net's own loss"""
    is_labeled = labels == labels
    return PCBANet.loss(None, scores[is_labeled], labels.float()[is_labeled]) if scores.dtype == torch.float32 else \
        PCBANet.loss(None, scores[is_labeled], labels.double()[is_labeled])


def _skewed_columns(gen, n, dims):
    """n rows of integer features within ``dims``; three rows in four carry each column's most common value"""
    cols = []
    for d in dims:
        common = int(torch.randint(0, d, (1,), generator=gen))
        draw = torch.randint(0, d, (n,), generator=gen)
        cols.append(torch.where(torch.rand(n, generator=gen) < 0.75, torch.full((n,), common), draw))
    return torch.stack(cols, 1)


def g13_mol_nets(out):
    HIVNet, PCBANet = _reference_nets()
    src, dst, N, sizes = make_test_graph(seed=13)
    out["src"], out["dst"], out["N"], out["sizes"] = src, dst, np.array(N), np.array(sizes)
    gen = torch.Generator().manual_seed(131)
    eig = torch.randn(N, 4, generator=gen)
    atoms = _skewed_columns(gen, N, ATOM_DIMS)
    bonds = _skewed_columns(gen, len(src), BOND_DIMS)
    snorm = torch.rand(N, 1, generator=gen) + 0.5
    pos_enc = torch.randn(N, 2, generator=gen)
    G = len(sizes)
    out["eig"], out["atoms"], out["bonds"], out["snorm"], out["pos_enc"] = eig.numpy(), atoms.numpy(), bonds.numpy(), snorm.numpy(), pos_enc.numpy()
    out["atom_dims"], out["bond_dims"] = np.array(ATOM_DIMS), np.array(BOND_DIMS)
    # (name, net, type_net, hidden, aggregators, scalers, extra net parameters)
    cases = [("hiv_simple", "hiv", "simple", 19, "mean max min dir1-dx dir1-av", "identity", dict(pos_enc_dim=2, edge_feat=False, edge_dim=0)),
             ("pcba_towers_vn", "pcba", "towers", 20, "mean max dir1-av dir1-dx", "identity amplification",
              dict(towers=5, virtual_node="mean", decreasing_dim=True, edge_feat=False, edge_dim=0)),
             ("hiv_complex_edge", "hiv", "complex", 20, "mean dir1-dx dir2-dx", "identity amplification attenuation",
              dict(pos_enc_dim=0, edge_feat=True, edge_dim=6))]
    out["cases"] = np.array([c[0] for c in cases])
    for i, (name, which, type_net, hidden, aggs, scalers, extra) in enumerate(cases):
        torch.manual_seed(13 + i)
        params = dict(hidden_dim=hidden, out_dim=hidden, in_feat_dropout=0.0, dropout=0.0, L=3, type_net=type_net, readout="mean", graph_norm=True,
                      batch_norm=True, aggregators=aggs, scalers=scalers, avg_d={"log": torch.tensor(1.1)}, residual=True, pretrans_layers=1,
                      posttrans_layers=1, device="cpu", **extra)
        net = (HIVNet if which == "hiv" else PCBANet)(params)
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
        g.ndata["pos_enc"] = pos_enc
        with torch.no_grad():
            out[f"{name}/h0"] = net.embedding_h(atoms).numpy()
            if params["edge_feat"]:
                out[f"{name}/e0"] = net.embedding_e(bonds).numpy()
        scores = net(g, atoms, bonds if params["edge_feat"] else None, snorm, None)
        if which == "hiv":
            labels = torch.randint(0, 2, (G,), generator=gen)
            labels[:2] = torch.tensor([0, 1])
            loss = PCBANet.loss(None, scores, labels.float().unsqueeze(-1))
        else:
            labels = torch.randint(0, 2, (G, 128), generator=gen).float()
            labels[torch.rand(G, 128, generator=gen) < 0.6] = float("nan")
            labels[:, 7] = float("nan")                             # a task nobody was measured on
            assert 0.5 < float(torch.isnan(labels).float().mean()) < 0.7
            loss = _masked_reference_loss(PCBANet, scores, labels)
        assert tuple(scores.shape) == (G, 1 if which == "hiv" else 128) and float(scores.detach().abs().max()) >= 0.1, name       # (scores away from 0)
        names = [k for k, q in net.named_parameters()]
        grads = torch.autograd.grad(loss, [q for _, q in net.named_parameters()], allow_unused=True)
        out[f"{name}/cfg"] = np.array([which, type_net, str(hidden), aggs, scalers, str(int(params["edge_feat"])), str(params["edge_dim"]),
                                       str(params.get("pos_enc_dim", 0)), str(params.get("virtual_node", "none"))])
        out[f"{name}/labels"] = labels.numpy()
        out[f"{name}/scores"], out[f"{name}/loss"] = scores.detach().numpy(), loss.detach().numpy()
        for k, gr in zip(names, grads):
            if gr is not None:
                out[f"{name}/gp::{k}"] = gr.numpy()
        for k, v in net.state_dict().items():
            if "running" in k:
                out[f"{name}/after::{k}"] = v.detach().numpy().copy()


def _ogb_metric(fn, scores, labels):
    """ogb's evaluator rule around a scikit-learn metric (the mean over the scorable tasks; nan where ogb raises)"""
    vals = []
    for t in range(labels.shape[1]):
        y = labels[:, t]
        if (y == 1).sum() > 0 and (y == 0).sum() > 0:
            lab = y == y
            vals.append(fn(y[lab], scores[lab, t]))
    return float(np.mean(vals)) if vals else float("nan")


def g14_mol_loss_metrics(out):
    import sklearn
    from sklearn.metrics import average_precision_score, roc_auc_score
    _, PCBANet = _reference_nets()
    out["sklearn_version"] = np.array(sklearn.__version__)
    # (name, G, T, share of NaN labels, score transform)
    cases = [("g1_t1", 1, 1, 0.0, None), ("g63_t1", 63, 1, 0.0, None), ("g64_t1_nan", 64, 1, 0.4, None), ("g65_t128_nan", 65, 128, 0.4, None),
             ("g300_t128_nan", 300, 128, 0.4, None), ("allnan_g65_t128", 65, 128, 1.0, None),
             ("extreme_g64_t1", 64, 1, 0.0, "extreme"), ("extreme_g65_t128_nan", 65, 128, 0.4, "extreme"),
             ("ties_g300_t128_nan", 300, 128, 0.4, "ties"), ("ties_g63_t1", 63, 1, 0.0, "ties")]
    out["cases"] = np.array([c[0] for c in cases])
    for i, (name, G, T, nan_share, how) in enumerate(cases):
        gen = torch.Generator().manual_seed(1400 + i)
        scores = 2.0 * torch.randn(G, T, generator=gen)
        if how == "extreme":
            scores[torch.rand(G, T, generator=gen) < 0.1] = 100.0
            scores[torch.rand(G, T, generator=gen) < 0.1] = -100.0
        if how == "ties":
            scores = torch.round(scores * 2.0) / 2.0
        labels = (torch.rand(G, T, generator=gen) < 0.3).float()
        if T > 1:
            labels[:, 3] = 1.0                                      # a task of a single class: no metric, but it counts in the loss
        if 0.0 < nan_share < 1.0:
            labels[torch.rand(G, T, generator=gen) < nan_share] = float("nan")
            if T > 1:
                labels[:, 5] = float("nan")                         # a task nobody was measured on
        elif nan_share >= 1.0:
            labels[:] = float("nan")
        out[f"{name}/scores"], out[f"{name}/labels"] = scores.numpy(), labels.numpy()
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            x = scores.to(dtype).clone().requires_grad_(True)
            loss = _masked_reference_loss(PCBANet, x, labels)
            (grad,) = torch.autograd.grad(loss, x)
            out[f"{name}/loss{tag}"] = loss.detach().numpy()
            if tag == "32" or G * T <= 65 * 128:                   # (the fp64 gradient of a 300 x 128 case is 300 KB: tests/mol_oracle.py, pinned to
                out[f"{name}/grad{tag}"] = grad.numpy()            #  the fp64 gradients of the smaller cases, restates it)
            if nan_share >= 1.0:
                assert bool(torch.isnan(loss)) and bool((grad == 0).all())
            else:
                assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
                assert bool((grad[torch.isnan(labels)] == 0).all())
        s, y = scores.numpy(), labels.numpy()
        out[f"{name}/rocauc"] = np.array(_ogb_metric(roc_auc_score, s, y))
        out[f"{name}/ap"] = np.array(_ogb_metric(average_precision_score, s, y))
        print(f"  {name}: loss {float(out[name + '/loss64']):.6f} rocauc {float(out[name + '/rocauc']):.6f} ap {float(out[name + '/ap']):.6f}")


def main():
    _install_stubs()
    _install_ogb_stub()
    only = sys.argv[1:]
    for fname, fn in (("g13_mol_nets", g13_mol_nets), ("g14_mol_loss_metrics", g14_mol_loss_metrics)):
        if only and fname not in only:
            continue
        out = {}
        fn(out)
        path = os.path.join(HERE, fname + ".npz")
        np.savez_compressed(path, **out)
        print(f"{fname}: {len(out)} arrays, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
