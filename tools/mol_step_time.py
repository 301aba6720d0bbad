#!/usr/bin/env python3
"""Timing of the OGB molecule nets' encoder, loss and training step (measured, asserted by nothing).

For batches of 128 and of 2048 molecule-like graphs (synth.molecule_batch: ~3 k and ~47 k nodes), with the shipped HIV json's net (4 simple
layers, hidden 70, mean max min dir1-dx dir1-av, dropout 0.3):
1. AtomEncoder forward + backward: ops.multi_embedding against the torch composition of the same nine nn.Embedding weights
   (``h = 0; h += emb_c(x[:, c])``, torch's sort-based embedding backward).
2. The loss on [G, 128] scores with 60 % NaN labels, forward + backward: ops.masked_bce_with_logits against the reference loop's
   boolean-index form (train/train_PCBA_graph_classification.py:32-33: a device-to-host read-back per call).
3. The whole training step (Adam): eager with nets.DGNHIVNet, and hipgraph.CapturedMolStep replay.

Conventions: 30 warm-up steps, then the median (p10, p90) over groups of 10 steps timed wall-clock around a device synchronisation; the
two forms of a comparison are measured in alternating windows; device-kernel counts from torch.profiler.
Usage: mol_step_time.py [steps=200]"""
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dgn_amd  # noqa: E402
from dgn_amd import ops, synth  # noqa: E402
from dgn_amd.hipgraph import CapturedMolStep  # noqa: E402
from dgn_amd.nets import OGB_ATOM_DIMS, AtomEncoder, DGNHIVNet  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
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


def compare(title, name_a, a, name_b, b):
    (ma, la, ha), (mb, lb, hb) = timed_pair(a, b)
    print(f"{title}\n   {name_a}: median {ma:.1f} us (p10 {la:.1f}, p90 {ha:.1f}), device activities {device_kernels(a)}\n"
          f"   {name_b}: median {mb:.1f} us (p10 {lb:.1f}, p90 {hb:.1f}), device activities {device_kernels(b)}\n"
          f"   ratio {ma / mb:.2f}x", flush=True)


HIV = dict(L=4, hidden_dim=70, out_dim=70, type_net="simple", residual=True, edge_feat=False, readout="mean", in_feat_dropout=0.0, dropout=0.3,
           graph_norm=False, batch_norm=True, aggregators="mean max min dir1-dx dir1-av", scalers="identity", towers=5, edge_dim=0,
           pretrans_layers=1, posttrans_layers=1, pos_enc_dim=0, device="cuda")

print(f"{torch.cuda.get_device_name(0)}; {steps} steps after {WARMUP} warm-up steps per form")
for n_graphs in (128, 2048):
    b = synth.molecule_batch(n_graphs, laplacian_eig=False)
    N = int(b["num_nodes"])
    gen = torch.Generator().manual_seed(0)
    print(f"== {n_graphs} graphs, {N} nodes, {b['src'].numel()} directed edges")
    atoms = torch.stack([torch.randint(0, d, (N,), generator=gen) for d in OGB_ATOM_DIMS], 1).to(dev)
    torch.manual_seed(0)
    enc = AtomEncoder(70).to(dev)
    cot = torch.randn(N, 70, device=dev)

    def enc_fused():
        enc.zero_grad(set_to_none=True)
        enc(atoms).backward(cot)

    def enc_torch():
        enc.zero_grad(set_to_none=True)
        h = 0
        for c, emb in enumerate(enc.atom_embedding_list):
            h = h + emb(atoms[:, c])
        h.backward(cot)

    compare("-- 1. AtomEncoder (nine tables, hidden 70), forward + backward", "torch composition", enc_torch, "ops.multi_embedding", enc_fused)

    scores = (2.0 * torch.randn(n_graphs, 128, generator=gen)).to(dev).requires_grad_(True)
    labels = (torch.rand(n_graphs, 128, generator=gen) < 0.3).float()
    labels[torch.rand(n_graphs, 128, generator=gen) < 0.6] = float("nan")
    labels = labels.to(dev)

    def loss_index():
        scores.grad = None
        is_labeled = labels == labels
        F.binary_cross_entropy_with_logits(scores[is_labeled], labels.float()[is_labeled]).backward()

    def loss_fused():
        scores.grad = None
        ops.masked_bce_with_logits(scores, labels).backward()

    compare("-- 2. loss on [G, 128] scores, 60 % NaN labels, forward + backward", "boolean-index form", loss_index, "ops.masked_bce_with_logits",
            loss_fused)

    avg_log = float(torch.log(torch.bincount(b["dst"], minlength=N).float() + 1).mean())
    params = dict(HIV, avg_d={"log": torch.tensor(avg_log)})
    src, dst, eig, snorm = b["src"].to(dev), b["dst"].to(dev), b["eig"].to(dev), b["snorm_n"].to(dev)
    sizes = [int(s) for s in b["sizes"]]
    y = torch.randint(0, 2, (n_graphs,), generator=gen).to(dev)
    torch.manual_seed(0)
    net = DGNHIVNet(params).to(dev).train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    graph = dgn_amd.DGNGraph(src, dst, N, eig=eig)
    graph.batch_num_nodes = sizes

    def eager_step():
        opt.zero_grad(set_to_none=True)
        graph.invalidate_caches()
        net.loss(net(graph, atoms, None, snorm, None), y).backward()
        opt.step()

    torch.manual_seed(0)
    net_c = DGNHIVNet(params).to(dev).train()
    cs = CapturedMolStep(net_c, N + 256, src.numel() + 256, g_cap=n_graphs + 1, eig_dim=eig.shape[1], lr=1e-3)
    cs.load(src, dst, N, eig, atoms, snorm, sizes, y)
    cs.capture(warmup=3)
    compare("-- 3. whole training step, shipped HIV json (4 simple layers, hidden 70, dropout 0.3, Adam)", "eager step (DGNHIVNet)", eager_step,
            "CapturedMolStep replay", cs.step)
    print(f"   last captured loss {float(cs.step()):.5f}", flush=True)
