#!/usr/bin/env python3
"""Timing of the superpixel graph-classification net's own pieces and step (measured, asserted by nothing).  One process; the comparison
is always the torch composition on the same tensors, never the kernels against themselves.

(a) The input embedding, forward + backward (weight and bias gradient), ops.feature_embedding against F.linear: the CIFAR10 batch (128
    graphs of synth.knn_batch, K 5, F 65), the MNIST batch (n_lo=60, n_hi=75, K 3, F 65) and the edge embedding of the CIFAR10 batch
    (K 1, one row per edge, F 6).
(b) The loss tail at G 128, C 10, forward + backward: ops.class_cross_entropy(hits=True) against F.cross_entropy + argmax / eq / sum.
(c) The whole training step of the shipped CIFAR10 json (L 4, hidden 65, mean dir1-dx dir2-dx, identity, dropout 0.3, Adam) as type_net
    simple (bench.py's c3) and towers: eager with nets.DGNSuperpixelNet, and hipgraph.CapturedSuperpixelStep replay.

Conventions: 30 warm-up steps per version (the device's clock ramp, see bench.py), then groups of steps timed wall-clock around a device
synchronisation; the two versions of a comparison take turns group by group, so that a drift of the shared host hits both; median with
p10 / p90 as the spread; device activities per step from torch.profiler in a step of its own.
Usage: superpixel_step_time.py [steps=400] [n_graphs=128]"""
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dgn_amd  # noqa: E402
from dgn_amd import ops, synth  # noqa: E402
from dgn_amd.hipgraph import CapturedSuperpixelStep  # noqa: E402
from dgn_amd.nets import DGNSuperpixelNet  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 400
n_graphs = int(sys.argv[2]) if len(sys.argv) > 2 else 128
WARMUP, GROUP = 30, 10
dev = torch.device("cuda")


def timed_together(versions):
    """{name: (median, p10, p90)} in microseconds per step; the versions' groups of GROUP steps alternate."""
    for step in versions.values():
        for _ in range(WARMUP):
            step()
    torch.cuda.synchronize()
    t = {name: [] for name in versions}
    for _ in range(max(steps // GROUP, 5)):
        for name, step in versions.items():
            t0 = time.perf_counter()
            for _ in range(GROUP):
                step()
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) / GROUP * 1e6)
    out = {}
    for name, v in t.items():
        v.sort()
        out[name] = (v[len(v) // 2], v[len(v) // 10], v[(len(v) * 9) // 10])
    return out


def device_kernels(step):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return len([e for e in prof.profiler.kineto_results.events() if str(e.device_type()).endswith("CUDA")])


def compare(title, versions):
    res = timed_together(versions)
    print(f"-- {title}")
    for name, (med, p10, p90) in res.items():
        print(f"   {name}: median {med:.1f} us  (p10 {p10:.1f}, p90 {p90:.1f})  device activities per step: {device_kernels(versions[name])}", flush=True)
    (a, ra), (b, rb) = list(res.items())[:2]
    print(f"   {b} / {a}: {rb[0] / ra[0]:.2f}x")
    return res


print(f"{torch.cuda.get_device_name(0)}; {steps} steps per version after {WARMUP}, groups of {GROUP}")
gen = torch.Generator().manual_seed(0)
cifar = synth.knn_batch(n_graphs)
mnist = synth.knn_batch(n_graphs, n_lo=60, n_hi=75)

# ---- (a) the embedding, forward + backward ------------------------------------------------------------------------------------------


def embedding_versions(R, K, Fo):
    x = torch.rand(R, K, generator=gen).to(dev)
    fc = torch.nn.Linear(K, Fo).to(dev)
    ct = torch.randn(R, Fo, generator=gen).to(dev)

    def run(fn):
        def step():
            fc.weight.grad = fc.bias.grad = None
            fn(x, fc.weight, fc.bias).backward(ct)
        return step
    assert ops.feature_embedding_supported(x, fc.weight)
    return {"ops.feature_embedding": run(ops.feature_embedding), "F.linear": run(F.linear)}


for tag, R, K, Fo in (("CIFAR10 nodes", int(cifar["num_nodes"]), 5, 65), ("MNIST nodes", int(mnist["num_nodes"]), 3, 65),
                      ("CIFAR10 edges", cifar["src"].numel(), 1, 6)):
    compare(f"(a) embedding forward + backward, {tag}: R {R}, K {K}, F {Fo}", embedding_versions(R, K, Fo))

# ---- (b) the loss tail, forward + backward ------------------------------------------------------------------------------------------

G, C = n_graphs, 10
scores = (3.0 * torch.randn(G, C, generator=gen)).to(dev).requires_grad_(True)
labels = torch.randint(0, C, (G,), generator=gen).to(dev)


def tail_kernel():
    loss, hits = ops.class_cross_entropy(scores, labels, hits=True)
    scores.grad = None
    loss.backward()
    return hits


def tail_torch():
    loss = F.cross_entropy(scores, labels)
    hits = (scores.detach().argmax(dim=1) == labels).sum()
    scores.grad = None
    loss.backward()
    return hits


compare(f"(b) loss + hit count forward + backward, G {G}, C {C} (no read-back on either side)",
        {"ops.class_cross_entropy(hits=True)": tail_kernel, "F.cross_entropy + argmax / eq / sum": tail_torch})
assert int(tail_kernel()) == int(tail_torch())

# ---- (c) the whole training step --------------------------------------------------------------------------------------------------------

N = int(cifar["num_nodes"])
src, dst, eig, snorm = cifar["src"].to(dev), cifar["dst"].to(dev), cifar["eig"].to(dev), cifar["snorm_n"].to(dev)
sizes = [int(s) for s in cifar["sizes"]]
feats = torch.rand(N, 5, generator=gen).to(dev)
y = torch.randint(0, C, (n_graphs,), generator=gen).to(dev)
avg_log = float(torch.log(torch.bincount(cifar["dst"], minlength=N).float() + 1).mean())
print(f"(c) batch: {n_graphs} 8-NN graphs, {N} nodes, {src.numel()} directed edges")
for type_net in ("simple", "towers"):
    params = dict(in_dim=5, in_dim_edge=1, hidden_dim=65, out_dim=65, n_classes=C, in_feat_dropout=0.0, dropout=0.3, L=4, type_net=type_net,
                  readout="mean", graph_norm=True, batch_norm=True, residual=True, aggregators="mean dir1-dx dir2-dx", scalers="identity",
                  avg_d={"log": torch.tensor(avg_log)}, edge_feat=False, edge_dim=0, pretrans_layers=1, posttrans_layers=1)
    torch.manual_seed(0)
    net = DGNSuperpixelNet(params).to(dev).train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    graph = dgn_amd.DGNGraph(src, dst, N, eig=eig)
    graph.batch_num_nodes = sizes

    def eager_step():
        opt.zero_grad(set_to_none=True)
        graph.invalidate_caches()
        loss, hits = net.loss(net(graph, feats, None, snorm, None), y, hits=True)
        loss.backward()
        opt.step()

    net_c = DGNSuperpixelNet(params).to(dev).train()
    cs = CapturedSuperpixelStep(net_c, N + 256, src.numel() + 256, g_cap=n_graphs + 1, eig_dim=eig.shape[1], lr=1e-3)
    cs.load(src, dst, N, eig, feats, snorm, sizes, y)
    cs.capture(warmup=3)
    compare(f"(c) training step, CIFAR10 json as {type_net} (L 4, hidden 65, dropout 0.3, Adam)",
            {"CapturedSuperpixelStep replay": cs.step, "eager step (DGNSuperpixelNet)": eager_step})
    loss_c, hits_c = cs.step()
    print(f"   last captured loss {float(loss_c):.5f}, hits {int(hits_c)} of {n_graphs}")
