#!/usr/bin/env python3
"""Timing of the node-classification tail and step (measured, asserted by nothing).

1. Loss + metric of one PATTERN-sized batch (synth.sbm_batch(128): ~15 k nodes, 2 classes), forward + backward: the reference's
   formulation against ops.balanced_cross_entropy + nets.accuracy_sbm.  The reference's formulation is spelled out here in this
   project's own words WITH its read-backs: bincount, nonzero, unique, indexed assignment, weighted cross_entropy on the device; then
   for the metric the scores go to the host, softmax over the nodes, arg-max over the classes and a host-side confusion matrix
   (numpy; the reference calls scikit-learn's) on every batch.  A device-only rewrite would time something else.
2. The whole training step at the shipped PATTERN json (4 complex layers, hidden 47, mean dir1-dx dir2-dx x 3 scalers, Adam): eager with
   nets.DGNNodeNet, and hipgraph.CapturedNodeStep replay.

Conventions: 30 warm-up steps (the device's clock ramp, see bench.py), then the median over groups of steps timed wall-clock around a
device synchronisation; device-kernel counts from torch.profiler.
Usage: node_step_time.py [steps=200] [n_graphs=128]"""
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dgn_amd  # noqa: E402
from dgn_amd import ops, synth  # noqa: E402
from dgn_amd.hipgraph import CapturedNodeStep  # noqa: E402
from dgn_amd.nets import DGNNodeNet, accuracy_sbm  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
n_graphs = int(sys.argv[2]) if len(sys.argv) > 2 else 128
WARMUP, GROUP = 30, 10
dev = torch.device("cuda")


def timed(step, sync_inside=False):
    """Median / p10 / p90 in microseconds per step over groups of GROUP steps."""
    for _ in range(WARMUP):
        step()
    torch.cuda.synchronize()
    t = []
    for _ in range(max(steps // GROUP, 3)):
        t0 = time.perf_counter()
        for _ in range(GROUP):
            step()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) / GROUP * 1e6)
    t.sort()
    return t[len(t) // 2], t[len(t) // 10], t[(len(t) * 9) // 10]


def device_kernels(step):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return len([e for e in prof.profiler.kineto_results.events() if str(e.device_type()).endswith("CUDA")])


def report(name, step):
    med, p10, p90 = timed(step)
    print(f"{name}: median {med:.1f} us  (p10 {p10:.1f}, p90 {p90:.1f})  device activities per step: {device_kernels(step)}", flush=True)
    return med


b = synth.sbm_batch(n_graphs)
N = int(b["num_nodes"])
gen = torch.Generator().manual_seed(0)
C = 2
labels = torch.randint(0, C, (N,), generator=gen).to(dev)
scores = (3.0 * torch.randn(N, C, generator=gen)).to(dev).requires_grad_(True)
print(f"batch: {n_graphs} SBM graphs, {N} nodes, {b['src'].numel()} directed edges; {torch.cuda.get_device_name(0)}; {steps} steps after {WARMUP}")


def reference_formulation():
    # the loss, as the reference forms it (two read-backs: nonzero, unique)
    V = labels.size(0)
    count = torch.bincount(labels)
    count = count[count.nonzero()].squeeze()
    sizes = torch.zeros(C, dtype=torch.long, device=dev)
    sizes[torch.unique(labels)] = count
    weight = (V - sizes).float() / V
    weight *= (sizes > 0).float()
    loss = F.cross_entropy(scores, labels, weight=weight)
    scores.grad = None
    loss.backward()
    # the metric, as the reference forms it: everything on the host
    S = labels.cpu().numpy()
    pred = np.argmax(torch.softmax(scores, dim=0).detach().cpu().numpy(), axis=1)
    cm = np.bincount(S * C + pred, minlength=C * C).reshape(C, C).astype(np.float32)
    hits, present = 0, np.zeros(C)
    for r in range(C):
        n_r = int((S == r).sum())
        if n_r:
            present[r] = cm[r, r] / float(n_r)
            hits += int(cm[r, r] > 0)
    return loss, 100.0 * present.sum() / max(hits, 1)


def new_op():
    loss, cm = ops.balanced_cross_entropy(scores, labels, C, confusion=True)
    scores.grad = None
    loss.backward()
    return loss, accuracy_sbm(cm)


print("-- 1. loss + metric, forward + backward")
t_ref = report("reference formulation (device loss with read-backs, host metric)", reference_formulation)
t_new = report("balanced_cross_entropy + accuracy_sbm (device only)", new_op)
print(f"ratio {t_ref / t_new:.2f}x; accuracy {reference_formulation()[1]:.4f} (reference formulation) vs {float(new_op()[1]):.4f}")

print("-- 2. whole training step, shipped PATTERN json (4 complex layers, hidden 47, Adam)")
avg_log = float(torch.log(torch.bincount(b["dst"], minlength=N).float() + 1).mean())
params = dict(in_dim=3, hidden_dim=47, out_dim=47, n_classes=C, in_feat_dropout=0.0, dropout=0.0, L=4, type_net="complex", pos_enc_dim=0,
              readout="mean", graph_norm=True, batch_norm=True, aggregators="mean dir1-dx dir2-dx", scalers="identity amplification attenuation",
              avg_d={"log": torch.tensor(avg_log)}, residual=True, edge_feat=False, edge_dim=0, pretrans_layers=1, posttrans_layers=1, device="cuda")
torch.manual_seed(0)
feats = torch.randint(0, 3, (N,), generator=gen).to(dev)
src, dst, eig, snorm = b["src"].to(dev), b["dst"].to(dev), b["eig"].to(dev), b["snorm_n"].to(dev)
sizes = [int(s) for s in b["sizes"]]

net = DGNNodeNet(params).to(dev).train()
opt = torch.optim.Adam(net.parameters(), lr=1e-3)
graph = dgn_amd.DGNGraph(src, dst, N, eig=eig)
graph.batch_num_nodes = sizes


def eager_step():
    opt.zero_grad(set_to_none=True)
    graph.invalidate_caches()
    loss, cm = net.loss(net(graph, feats, None, snorm, None), labels, confusion=True)
    loss.backward()
    opt.step()


t_eager = report("eager step (DGNNodeNet, Adam)", eager_step)

net_c = DGNNodeNet(params).to(dev).train()
cs = CapturedNodeStep(net_c, N + 256, src.numel() + 256, eig_dim=eig.shape[1], lr=1e-3)
cs.load(src, dst, N, eig, feats, snorm, labels, sizes)
cs.capture(warmup=3)
t_cap = report("CapturedNodeStep replay", cs.step)
print(f"eager / captured {t_eager / t_cap:.2f}x; last captured loss {float(cs.step()[0]):.5f}")
