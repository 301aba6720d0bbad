#!/usr/bin/env python3
"""Generate the positional-encoding fixture by IMPORTING the reference (see make_golden.py for the stubs and the rules: arrays and short
config strings only, no reference source or bytecode).

    python tests/golden/make_golden_pos_enc.py            # rewrites g18_pos_enc_nets.npz

``g18_pos_enc_nets``: the unmodified graph-regression net (nets/molecules_graph_regression/dgn_net.py; towers and simple) and the
unmodified node-classification net (nets/SBMs_node_classification/dgn_net.py; complex) with ``pos_enc_dim = 3``, hidden 20, L = 2, in
training mode on one batch of ten small molecule-like graphs, ``g.ndata['pos_enc'] = eig[:, 1:4]``.  Per case: the ``state_dict``,
``h0`` -- the input stage's output, ``embedding_h(h) + embedding_pos_enc(pos_enc)``, taken by a hook in front of the first layer -- and
the loss' gradient with respect to it (``g_h0``: the upstream gradient of the input stage), scores, loss, every parameter gradient and
the BatchNorm running statistics after the step.  The node net's MLP head is re-drawn wider, as in make_golden_node.py.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

from make_golden import FakeGraph, _install_stubs

torch.set_num_threads(1)

POS_ENC_DIM, HIDDEN, LAYERS = 3, 20, 2


def _batch(seed=18, n_graphs=10):
    """Ten molecule-like graphs of 7 .. 15 nodes: a random spanning tree plus two ring bonds, symmetric directed edges."""
    rng = np.random.default_rng(seed)
    src, dst, sizes, off = [], [], [], 0
    for _ in range(n_graphs):
        n = int(rng.integers(7, 16))
        und = set()
        for v in range(1, n):
            und.add((int(rng.integers(0, v)), v))
        while len(und) < n + 1:
            a, b = rng.integers(0, n, 2)
            if a != b:
                und.add((int(min(a, b)), int(max(a, b))))
        for a, b in sorted(und):
            src += [a + off, b + off]
            dst += [b + off, a + off]
        sizes.append(n)
        off += n
    return np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64), off, sizes


def _run(out, name, net, g, feats, snorm, loss_of):
    net.train(True)
    for k, v in net.state_dict().items():
        out[f"{name}/sd::{k}"] = v.detach().numpy().copy()
    seen = {}

    def hook(module, args):
        seen["h0"] = args[1]
        args[1].retain_grad()

    handle = net.layers[0].register_forward_pre_hook(hook)
    scores = net(g, feats, None, snorm, None)
    handle.remove()
    loss = loss_of(scores)
    names = [k for k, _ in net.named_parameters()]
    loss.backward()
    out[f"{name}/h0"], out[f"{name}/g_h0"] = seen["h0"].detach().numpy().copy(), seen["h0"].grad.numpy().copy()
    out[f"{name}/scores"], out[f"{name}/loss"] = scores.detach().numpy(), loss.detach().numpy()
    for k, q in net.named_parameters():
        if q.grad is not None:
            out[f"{name}/gp::{k}"] = q.grad.numpy().copy()
    assert f"{name}/gp::embedding_pos_enc.weight" in out and f"{name}/gp::embedding_h.weight" in out, names
    for k, v in net.state_dict().items():
        if "running" in k:
            out[f"{name}/after::{k}"] = v.detach().numpy().copy()


def g18_pos_enc_nets(out):
    from nets.molecules_graph_regression.dgn_net import DGNNet as MolNet
    from nets.SBMs_node_classification.dgn_net import DGNNet as NodeNet
    src, dst, N, sizes = _batch()
    out["src"], out["dst"], out["N"], out["sizes"] = src, dst, np.array(N), np.array(sizes)
    gen = torch.Generator().manual_seed(118)
    eig = torch.randn(N, POS_ENC_DIM + 2, generator=gen)
    atoms = torch.randint(0, 6, (N,), generator=gen)
    feats = torch.randint(0, 3, (N,), generator=gen)
    snorm = torch.rand(N, 1, generator=gen) + 0.5
    targets = torch.randn(len(sizes), 1, generator=gen)
    labels = torch.randint(0, 2, (N,), generator=gen)
    labels[:2] = torch.tensor([0, 1])
    out["eig"], out["atoms"], out["feats"], out["snorm"] = eig.numpy(), atoms.numpy(), feats.numpy(), snorm.numpy()
    out["targets"], out["labels"] = targets.numpy(), labels.numpy()
    out["pos_enc_dim"] = np.array(POS_ENC_DIM)

    def graph():
        g = FakeGraph(src, dst, N)
        g.batch_num_nodes = list(sizes)
        g.ndata["eig"] = eig
        g.ndata["pos_enc"] = eig[:, 1:POS_ENC_DIM + 1]
        return g

    common = dict(hidden_dim=HIDDEN, out_dim=HIDDEN, in_feat_dropout=0.0, dropout=0.0, L=LAYERS, pos_enc_dim=POS_ENC_DIM, graph_norm=True,
                  batch_norm=True, avg_d={"log": torch.tensor(1.1)}, residual=True, edge_feat=False, edge_dim=0, pretrans_layers=1,
                  posttrans_layers=1, device="cpu")
    # (name, net, type_net, readout, aggregators, scalers)
    cases = [("zinc_towers", "mol", "towers", "mean", "mean max dir1-av dir1-dx", "identity amplification"),
             ("zinc_simple", "mol", "simple", "sum", "mean max dir1-av dir1-dx", "identity amplification"),
             ("sbm_complex", "node", "complex", "mean", "mean dir1-dx dir2-dx", "identity amplification attenuation")]
    out["cases"] = np.array([c[0] for c in cases])
    for i, (name, kind, type_net, mode, aggs, scalers) in enumerate(cases):
        torch.manual_seed(180 + i)
        if kind == "mol":
            net = MolNet(dict(common, num_atom_type=6, num_bond_type=4, type_net=type_net, readout=mode, aggregators=aggs, scalers=scalers))
            _run(out, name, net, graph(), atoms, snorm, lambda s: net.loss(s, targets))
        else:
            net = NodeNet(dict(common, in_dim=3, n_classes=2, type_net=type_net, readout=mode, aggregators=aggs, scalers=scalers))
            with torch.no_grad():
                for fc in net.MLP_layer.FC_layers:
                    fc.weight.copy_(torch.randn(fc.weight.shape, generator=gen) * (2.0 / fc.weight.shape[1]) ** 0.5)
                    fc.bias.copy_(0.1 * torch.randn(fc.bias.shape, generator=gen))
            _run(out, name, net, graph(), feats, snorm, lambda s: net.loss(s, labels))
            assert float(torch.from_numpy(out[f"{name}/scores"]).std()) >= 0.3, name
        out[f"{name}/cfg"] = np.array([kind, type_net, mode, aggs, scalers])


def main():
    _install_stubs()
    out = {}
    g18_pos_enc_nets(out)
    path = os.path.join(HERE, "g18_pos_enc_nets.npz")
    np.savez_compressed(path, **out)
    print(f"g18_pos_enc_nets: {len(out)} arrays, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
