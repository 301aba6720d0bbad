#!/usr/bin/env python3
"""Timing of the nets' MLPReadout head: ops.mlp_head (one launch forward, two backward) against the torch composition of the same
nn.Linear modules (ops.FUSED_MLP_HEAD = False) -- measured, asserted by nothing.

1. The head alone, forward + backward (input gradient included), at 15 361 x (47, 23, 11, 2) [PATTERN, every node], 128 x (45, 22, 11, 1)
   [ZINC], 128 x (70, 35, 17, 1) [HIV] and 2 048 x (70, 70, 70, 128) [PCBA].
2. hipgraph.CapturedNodeStep replay at the shipped PATTERN json (what tools/node_step_time.py builds), captured with the switch off and on.
3. hipgraph.CapturedNetStep replay at the shipped ZINC json (bench.py's net batch), captured with the switch off and on.

Conventions (tools/mol_step_time.py): 30 warm-up steps, then the median (p10, p90) over groups of 10 steps timed wall-clock around a
device synchronisation; the two forms of a comparison are measured in alternating windows; device-activity counts from torch.profiler.
Usage: mlp_head_time.py [steps=300]"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dgn_amd import ops, synth  # noqa: E402
from dgn_amd.hipgraph import CapturedNetStep, CapturedNodeStep, bucket_capacity  # noqa: E402
from dgn_amd.nets import DGNNet, DGNNodeNet, MLPReadout  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
WARMUP, GROUP, WINDOWS = 30, 10, 3
dev = torch.device("cuda")


def window(step, n_groups):
    t = []
    for _ in range(n_groups):
        t0 = time.perf_counter()
        for _ in range(GROUP):
            step()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) / GROUP * 1e6)
    return t


def timed_pair(a, b):
    """Medians (p10, p90) in microseconds per step of two step functions measured in alternating windows."""
    for f in (a, b):
        for _ in range(WARMUP):
            f()
    torch.cuda.synchronize()
    ta, tb = [], []
    per = max(steps // GROUP // WINDOWS, 2)
    for _ in range(WINDOWS):
        ta += window(a, per)
        tb += window(b, per)
    stat = lambda t: (sorted(t)[len(t) // 2], sorted(t)[len(t) // 10], sorted(t)[(len(t) * 9) // 10])
    return stat(ta), stat(tb)


def device_kernels(step):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return len([e for e in prof.profiler.kineto_results.events() if str(e.device_type()).endswith("CUDA")])


def compare(title, name_a, a, name_b, b, count=True):
    (ma, la, ha), (mb, lb, hb) = timed_pair(a, b)
    acts = (lambda f: f", device activities {device_kernels(f)}") if count else (lambda f: "")
    spread = max(ha - la, hb - lb)
    print(f"{title}\n   {name_a}: median {ma:.1f} us (p10 {la:.1f}, p90 {ha:.1f}){acts(a)}\n"
          f"   {name_b}: median {mb:.1f} us (p10 {lb:.1f}, p90 {hb:.1f}){acts(b)}\n"
          f"   ratio {ma / mb:.2f}x; difference {mb - ma:+.1f} us against a p10-p90 spread of {spread:.1f} us", flush=True)
    return ma, mb, spread


def with_switch(on, build):
    """``build()`` under ops.FUSED_MLP_HEAD = on (a captured step keeps the route it was captured with)"""
    keep = ops.FUSED_MLP_HEAD
    ops.FUSED_MLP_HEAD = on
    try:
        return build()
    finally:
        ops.FUSED_MLP_HEAD = keep


print(f"{torch.cuda.get_device_name(0)}; {steps} steps after {WARMUP} warm-up steps per form")
print("== 1. the head alone, forward + backward")
slower = []
for rows, dims, decreasing in ((15361, (47, 23, 11, 2), True), (128, (45, 22, 11, 1), True), (128, (70, 35, 17, 1), True), (2048, (70, 70, 70, 128), False)):
    torch.manual_seed(0)
    head = MLPReadout(dims[0], dims[-1], decreasing_dim=decreasing).to(dev)
    assert tuple([head.FC_layers[0].in_features] + [fc.out_features for fc in head.FC_layers]) == dims
    with torch.no_grad():
        for fc in head.FC_layers:
            fc.weight.normal_(0.0, (2.0 / fc.weight.shape[1]) ** 0.5)
    x = torch.randn(rows, dims[0], device=dev).requires_grad_(True)
    cot = torch.randn(rows, dims[-1], device=dev)

    def run(on):
        def step():
            ops.FUSED_MLP_HEAD = on
            head.zero_grad(set_to_none=True)
            x.grad = None
            head(x).backward(cot)
        return step
    t_torch, t_fused, _ = compare(f"-- {rows} x {dims}", "torch composition", run(False), "ops.mlp_head", run(True))
    if t_fused >= t_torch:
        slower.append((rows, dims))
    ops.FUSED_MLP_HEAD = True
print("   the fused head is faster at all four sizes" if not slower else f"   the fused head is NOT faster at {slower}", flush=True)

print("== 2. CapturedNodeStep replay, shipped PATTERN json (4 complex layers, hidden 47, Adam), 128 SBM graphs")
b = synth.sbm_batch(128)
N = int(b["num_nodes"])
gen = torch.Generator().manual_seed(0)
labels = torch.randint(0, 2, (N,), generator=gen).to(dev)
feats = torch.randint(0, 3, (N,), generator=gen).to(dev)
avg_log = float(torch.log(torch.bincount(b["dst"], minlength=N).float() + 1).mean())
params = dict(in_dim=3, hidden_dim=47, out_dim=47, n_classes=2, in_feat_dropout=0.0, dropout=0.0, L=4, type_net="complex", pos_enc_dim=0,
              readout="mean", graph_norm=True, batch_norm=True, aggregators="mean dir1-dx dir2-dx", scalers="identity amplification attenuation",
              avg_d={"log": torch.tensor(avg_log)}, residual=True, edge_feat=False, edge_dim=0, pretrans_layers=1, posttrans_layers=1, device="cuda")
src, dst, eig, snorm = b["src"].to(dev), b["dst"].to(dev), b["eig"].to(dev), b["snorm_n"].to(dev)
sizes = [int(s) for s in b["sizes"]]


def node_step():
    torch.manual_seed(0)
    cs = CapturedNodeStep(DGNNodeNet(params).to(dev).train(), N + 256, src.numel() + 256, eig_dim=eig.shape[1], lr=1e-3)
    cs.load(src, dst, N, eig, feats, snorm, labels, sizes)
    cs.capture(warmup=3)
    return cs


off, on = with_switch(False, node_step), with_switch(True, node_step)
print(f"   {N} nodes, {src.numel()} directed edges")
compare("-- replay", "head on torch's GEMMs", off.step, "head as ops.mlp_head", on.step, count=False)
print(f"   last captured losses {float(off.step()[0]):.5f} / {float(on.step()[0]):.5f}", flush=True)
del off, on

print("== 3. CapturedNetStep replay, shipped ZINC json (4 towers layers, hidden 70, Adam), 128 molecules")
b = synth.molecule_batch(n_graphs=128, seed=41, extra_bonds=3.9, eig_dim=6)
N = int(b["num_nodes"])
avg_log = float(torch.log(torch.bincount(b["dst"], minlength=N).float() + 1).mean())
params = dict(num_atom_type=28, num_bond_type=4, hidden_dim=70, out_dim=70, in_feat_dropout=0.0, dropout=0.0, L=4, type_net="towers",
              pos_enc_dim=0, readout="mean", graph_norm=True, batch_norm=True, aggregators="mean max min dir1-av dir1-dx",
              scalers="identity amplification attenuation", avg_d={"log": torch.tensor(avg_log)}, residual=True, edge_feat=False, edge_dim=0,
              pretrans_layers=1, posttrans_layers=1, device="cuda")
src, dst, eig, snorm = b["src"].to(dev), b["dst"].to(dev), b["eig"].to(dev), b["snorm_n"].to(dev)
sizes = [int(s) for s in b["sizes"]]
cuts = torch.cumsum(torch.tensor([0] + sizes), 0)
max_edges = int(torch.bincount(torch.searchsorted(cuts, b["dst"], right=True) - 1, minlength=len(sizes)).max())      # of one graph
atoms, y = torch.randint(0, 28, (N,), generator=gen).to(dev), torch.randn(128, 1, generator=gen).to(dev)


def net_step():
    torch.manual_seed(0)
    n_cap, e_cap = bucket_capacity(N, src.numel())
    cs = CapturedNetStep(DGNNet(params).to(dev).train(), n_cap, e_cap, g_cap=129, eig_dim=eig.shape[1], lr=1e-3, max_graph_nodes=max(sizes),
                         max_graph_edges=max_edges)
    cs.load(src, dst, N, eig, atoms, snorm, sizes, y)
    cs.capture(warmup=3)
    return cs


off, on = with_switch(False, net_step), with_switch(True, net_step)
print(f"   {N} nodes, {src.numel()} directed edges")
compare("-- replay", "head on torch's GEMMs", off.step, "head as ops.mlp_head", on.step, count=False)
print(f"   last captured losses {float(off.step()):.5f} / {float(on.step()):.5f}", flush=True)
