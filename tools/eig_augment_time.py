#!/usr/bin/env python3
"""What the eigenvector augmentation costs on the captured route (measured, asserted by nothing).

A synthetic ZINC-like dataset (synth.molecule_batch: 9-37 atoms per graph), 128 graphs per batch, the shipped ZINC net (towers, hidden 70,
4 layers) as ``hipgraph.CapturedNetStep`` on the graph-block route, fed by ``load_packed``.  Three forms of one training step with the
reference's ``--flip`` (train/train_molecules_graph_regression.py:29-33):

  (a) no augmentation       ``load_packed`` + replay
  (b) host-issued flip      ``load_packed``, then ``eig.flip_sign`` of the static eig buffer written back into it with torch ops, then the
                            replay -- the only way before ``augment=``
  (c) augment=              ``CapturedNetStep(..., augment=EigAugment.molecules())``: ``load_packed`` + replay, the signs drawn by the first
                            kernel of the captured graph

Per form: the wall time per batch of load + step and of the replay alone (windows of PASSES epochs ended by a device synchronise; the
forms are warmed and alternate inside this one process; median and spread over the windows), and the device launches and copies of one
load + step (torch.profiler, in a pass of its own).
Usage: eig_augment_time.py [n_graphs=4096] [batch=128] [repeats=9]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dgn_amd  # noqa: E402
from dgn_amd import eig as eig_mod  # noqa: E402
from dgn_amd import synth  # noqa: E402
from dgn_amd.hipgraph import CapturedNetStep, rewrap_parameters  # noqa: E402
from dgn_amd.nets import DGNNet  # noqa: E402

n_graphs = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
batch = int(sys.argv[2]) if len(sys.argv) > 2 else 128
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 9
dev = torch.device("cuda")
K = 6
PASSES = 8          # epochs per timed window: 256 batches at the defaults, a fraction of a second


def dataset():
    b = synth.molecule_batch(n_graphs, seed=7, laplacian_eig=False, eig_dim=K)
    rng = np.random.default_rng(7)
    sizes, edges = b["sizes"].numpy(), synth.edges_per_graph(b).numpy()
    off, eoff = np.concatenate([[0], np.cumsum(sizes)]), np.concatenate([[0], np.cumsum(edges)])
    src, dst, eig = b["src"].numpy(), b["dst"].numpy(), b["eig"].numpy()
    samples = []
    for i, n in enumerate(sizes):
        samples.append(dict(src=src[eoff[i]:eoff[i + 1]] - off[i], dst=dst[eoff[i]:eoff[i + 1]] - off[i], num_nodes=int(n),
                            node=dict(feat=rng.integers(0, 28, int(n)), eig=eig[off[i]:off[i + 1]]), edge={},
                            graph=dict(label=rng.standard_normal(1).astype(np.float32))))
    return dgn_amd.PackedGraphs.from_graphs(samples, dev)


def make_step(ds, augment=None):
    torch.manual_seed(0)
    net = DGNNet(dict(num_atom_type=28, num_bond_type=4, hidden_dim=70, out_dim=70, in_feat_dropout=0.0, dropout=0.0, L=4, type_net="towers",
                      pos_enc_dim=0, readout="mean", graph_norm=True, batch_norm=True, aggregators="mean max min dir1-av dir1-dx",
                      scalers="identity amplification attenuation", avg_d={"log": torch.tensor(1.1)}, residual=True, edge_feat=False, edge_dim=0,
                      pretrans_layers=1, posttrans_layers=1, device="cuda")).to(dev).train()
    rewrap_parameters(net)
    n_cap, e_cap, max_nodes, max_edges = ds.capacity(batch)
    return CapturedNetStep(net, n_cap, e_cap, g_cap=batch + 1, eig_dim=K, max_graph_nodes=max_nodes, max_graph_edges=max_edges, augment=augment)


def spread(ts):
    ts = sorted(ts)
    return f"median {ts[len(ts) // 2]:.1f} us  (min {ts[0]:.1f}, max {ts[-1]:.1f}; {len(ts)} windows)"


def device_activities(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name() for e in prof.profiler.kineto_results.events() if str(e.device_type()).endswith("CUDA")]
    copies = sum(1 for n in names if "memcpy" in n.lower() or "memset" in n.lower())
    return len(names) - copies, copies


def main():
    ds = dataset()
    plain, hosted, fused = make_step(ds), make_step(ds), make_step(ds, augment=dgn_amd.EigAugment.molecules(device=dev, seed=1))
    epoch = [ids.tolist() for ids in ds.batches(batch, shuffle=True, generator=3, drop_last=True)]

    def host_flip():
        buf = hosted.pb.graph.ndata["eig"]
        buf.copy_(eig_mod.flip_sign(buf))

    forms = (("(a) no augmentation ", plain, None), ("(b) host-issued flip", hosted, host_flip), ("(c) augment=        ", fused, None))
    for _, step, _ in forms:
        step.load_packed(ds, epoch[0])
        step.capture()
    print(f"{torch.cuda.get_device_name(0)}: {n_graphs} ZINC-like graphs ({ds.num_nodes} nodes, {ds.num_edges} directed edges), {batch} per batch, "
          f"{len(epoch)} batches per epoch, {repeats} alternating windows of {PASSES} epochs per figure", flush=True)

    def window(step, between, load=True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(PASSES):
            for ids in epoch:
                if load:
                    step.load_packed(ds, ids)
                    if between is not None:
                        between()
                step.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (PASSES * len(epoch)) * 1e6

    for what, load in (("load_packed + step", True), ("replay alone (no load, nothing between)", False)):
        ts = {name: [] for name, _, _ in forms}
        for name, step, between in forms:                      # warm all
            window(step, between, load)
        for _ in range(repeats):                               # alternate
            for name, step, between in forms:
                if load or between is None:                    # (the host-issued form has no replay of its own: it is (a)'s)
                    ts[name].append(window(step, between, load))
        print(f"{what}, per batch:", flush=True)
        for name, t in ts.items():
            if t:
                print(f"  {name}: {spread(t)}", flush=True)
    for name, step, between in forms:
        def one():
            step.load_packed(ds, epoch[1])
            if between is not None:
                between()
            step.step()
        k, c = device_activities(one)
        kl, cl = device_activities(lambda: step.load_packed(ds, epoch[1]))
        print(f"device activities of one load + step {name}: {k} kernels + {c} copies / fills ({kl} + {cl} of them the load's)", flush=True)
    print(f"state of the augmenting step's stream: {fused.augment.get_state()}", flush=True)
    for _, step, _ in forms:
        step.pb.graph.check_deferred()


if __name__ == "__main__":
    main()
