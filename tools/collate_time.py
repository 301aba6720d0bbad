#!/usr/bin/env python3
"""Timing of the input side of a captured training step (measured, asserted by nothing).

A synthetic ZINC-like dataset (synth.molecule_batch: 9-37 atoms per graph), 128 graphs per batch, the shipped ZINC net (towers, hidden 70,
4 layers) as ``hipgraph.CapturedNetStep`` on the graph-block route.  Two ways to put a batch into the step's static buffers:

  (a) host collate + load   a numpy restatement of the reference's collate (data/molecules.py:219-230: the samples' arrays concatenated
                            with shifted node ids as dgl.batch does, labels, the per-node graph norm) followed by ``CapturedNetStep.load``
                            of the concatenated host arrays -- the path without a device-resident dataset
  (b) load_packed           ``PackedGraphs`` on the device, ``CapturedNetStep.load_packed(ds, ids)``: one gather launch

Per batch: the host wall time of the load alone (a window of PASSES epochs ended by a device synchronise), the device launches and copies
of one load (torch.profiler, in a pass of its own), and epochs of load + captured step both ways.  Both paths are warmed, alternate inside
this one process, and every figure comes with its spread over the windows (median, min - max).
Usage: collate_time.py [n_graphs=4096] [batch=128] [repeats=9]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dgn_amd  # noqa: E402
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
    """Per-graph host samples (what a Dataset's __getitem__ hands the reference's collate) and the same graphs packed."""
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
    return samples, dgn_amd.PackedGraphs.from_graphs(samples, dev)


def host_collate(samples, ids):
    """The reference's collate, restated on numpy: dgl.batch's concatenation, labels, snorm_n."""
    picked = [samples[i] for i in ids]
    sizes = np.asarray([g["num_nodes"] for g in picked], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)])
    src = np.concatenate([g["src"] + off[i] for i, g in enumerate(picked)])
    dst = np.concatenate([g["dst"] + off[i] for i, g in enumerate(picked)])
    feat = np.concatenate([g["node"]["feat"] for g in picked])
    eig = np.concatenate([g["node"]["eig"] for g in picked])
    labels = np.stack([g["graph"]["label"] for g in picked])
    snorm = torch.cat([torch.FloatTensor(int(n), 1).fill_(1. / float(n)) for n in sizes]).sqrt()
    return src, dst, int(off[-1]), eig, feat, snorm, sizes, labels


def make_step(ds):
    torch.manual_seed(0)
    net = DGNNet(dict(num_atom_type=28, num_bond_type=4, hidden_dim=70, out_dim=70, in_feat_dropout=0.0, dropout=0.0, L=4, type_net="towers",
                      pos_enc_dim=0, readout="mean", graph_norm=True, batch_norm=True, aggregators="mean max min dir1-av dir1-dx",
                      scalers="identity amplification attenuation", avg_d={"log": torch.tensor(1.1)}, residual=True, edge_feat=False, edge_dim=0,
                      pretrans_layers=1, posttrans_layers=1, device="cuda")).to(dev).train()
    rewrap_parameters(net)
    n_cap, e_cap, max_nodes, max_edges = ds.capacity(batch)
    return CapturedNetStep(net, n_cap, e_cap, g_cap=batch + 1, eig_dim=K, max_graph_nodes=max_nodes, max_graph_edges=max_edges)


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
    samples, ds = dataset()
    step_a, step_b = make_step(ds), make_step(ds)
    epoch = [ids.tolist() for ids in ds.batches(batch, shuffle=True, generator=3, drop_last=True)]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)

    def load_a(ids):
        src, dst, N, eig, feat, snorm, sizes, labels = host_collate(samples, ids)
        step_a.load(to(src), to(dst), N, to(eig), to(feat), snorm.to(dev, non_blocking=True), sizes, to(labels))

    def load_b(ids):
        step_b.load_packed(ds, ids)

    load_a(epoch[0])
    load_b(epoch[0])
    step_a.capture()
    step_b.capture()
    print(f"{torch.cuda.get_device_name(0)}: {n_graphs} ZINC-like graphs ({ds.num_nodes} nodes, {ds.num_edges} directed edges), {batch} per batch, "
          f"{len(epoch)} batches per epoch, {repeats} alternating windows of {PASSES} epochs per figure", flush=True)

    def window(load, step=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(PASSES):
            for ids in epoch:
                load(ids)
                if step is not None:
                    step.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (PASSES * len(epoch)) * 1e6

    for what, sa, sb in (("load alone", None, None), ("load + captured step", step_a, step_b)):
        window(load_a, sa), window(load_b, sb)                 # warm both
        ta, tb = [], []
        for _ in range(repeats):                               # alternate
            ta.append(window(load_a, sa))
            tb.append(window(load_b, sb))
        print(f"{what}, per batch:\n  (a) host collate + load: {spread(ta)}\n  (b) load_packed:         {spread(tb)}", flush=True)
    ka, ca = device_activities(lambda: load_a(epoch[1]))
    kb, cb = device_activities(lambda: load_b(epoch[1]))
    print(f"device activities of one load: (a) {ka} kernels + {ca} copies / fills, (b) {kb} kernels + {cb} copies / fills", flush=True)
    t = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(PASSES * len(epoch)):
            step_b.step()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) / (PASSES * len(epoch)) * 1e6)
    print(f"captured step alone (no load): {spread(t)}", flush=True)
    step_a.pb.graph.check_deferred()
    step_b.pb.graph.check_deferred()


if __name__ == "__main__":
    main()
