#!/usr/bin/env python3
"""Timing of the nets' input stage with positional encodings, of the masked L1 loss and of the captured steps around them (measured,
asserted by nothing).

At 128 and 2048 graphs of synth.molecule_batch (~3 k and ~47 k nodes) and at a 128-graph synth.sbm_batch (~15 k nodes):
(a) input stage forward + backward: ops.node_input against the composition it replaces -- nets.small_table_embedding (28 atom types;
    ops.multi_embedding of the nine OGB tables for the HIV net), then nn.Linear(K, hidden), then the add;
(b) loss forward + backward on [G, 1] scores: ops.masked_l1_loss against F.l1_loss and against the five-op masked composition the
    captured step carried before, ((s - t).abs() * mask).sum() / n;
(c) the captured ZINC-json training step (4 complex layers, hidden 45, mean dir1-dx dir1-av x 3 scalers, graph-block route, Adam) at
    pos_enc_dim 0 and 8, the latter also against the same net's eager step;
(d) the captured PATTERN-json training step (4 complex layers, hidden 47, mean dir1-dx dir2-dx x 3 scalers, Adam) at pos_enc_dim 0 and 2,
    likewise.

Conventions (those of tools/mol_step_time.py): 30 warm-up steps, then the median (p10, p90) over groups of 10 steps timed wall-clock
around a device synchronisation; the two forms of a comparison are measured in alternating windows of one process; device-activity
counts from torch.profiler.  A comparison "meets the bar" when the fused form's median is below the other's by more than the wider of
the two p10-p90 spreads.  ``--replays-only`` prints the pos_enc_dim = 0 replays of (c) and (d) alone: the lines to compare between two
commits (it uses nothing a commit without the fused input stage lacks).
Usage: input_stage_time.py [steps=200] [--replays-only]"""
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dgn_amd  # noqa: E402
from dgn_amd import nets, ops, synth  # noqa: E402
from dgn_amd.hipgraph import CapturedNetStep, CapturedNodeStep, bucket_capacity  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
REPLAYS_ONLY = "--replays-only" in sys.argv[1:]
steps = int(args[0]) if args else 200
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


def timed(*fns):
    """Medians (p10, p90) in microseconds per step of the step functions, measured in alternating windows."""
    for f in fns:
        for _ in range(WARMUP):
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    per = max(steps // GROUP // WINDOWS, 2)
    for _ in range(WINDOWS):
        for t, f in zip(ts, fns):
            t += window(f, per)
    return [(sorted(t)[len(t) // 2], sorted(t)[len(t) // 10], sorted(t)[(len(t) * 9) // 10]) for t in ts]


def device_kernels(step):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return len([e for e in prof.profiler.kineto_results.events() if str(e.device_type()).endswith("CUDA")])


def compare(title, fused, *others):
    """``fused`` and ``others``: (name, step) pairs; the fused form's bar is judged against every other form."""
    stats = timed(*[f for _, f in (fused,) + others])
    print(title)
    for (name, f), (m, lo, hi) in zip((fused,) + others, stats):
        print(f"   {name}: median {m:.1f} us (p10 {lo:.1f}, p90 {hi:.1f}), device activities {device_kernels(f)}")
    (m0, lo0, hi0) = stats[0]
    for (name, _), (m, lo, hi) in zip(others, stats[1:]):
        spread = max(hi0 - lo0, hi - lo)
        print(f"   {fused[0]} vs {name}: {m / m0:.2f}x, {m - m0:+.1f} us against a spread of {spread:.1f} us: "
              f"{'meets the bar' if m - m0 > spread else 'does NOT meet the bar'}")
    sys.stdout.flush()


def input_stage(label, N, tables_module, idx, K, hidden):
    """(a): tables_module is an nn.Embedding (idx [N]) or an AtomEncoder (idx [N, 9])."""
    torch.manual_seed(0)
    fc = torch.nn.Linear(K, hidden).to(dev)
    eig = torch.randn(N, K + 2, device=dev)
    pe = eig[:, 1:K + 1]
    cot = torch.randn(N, hidden, device=dev)
    single = isinstance(tables_module, torch.nn.Embedding)
    tables = [tables_module.weight] if single else tables_module.weights
    params = list(tables) + [fc.weight, fc.bias]

    def zero():
        for q in params:
            q.grad = None

    def fused():
        zero()
        ops.node_input(idx, tables, pe, fc.weight, fc.bias).backward(cot)

    def composition():
        zero()
        h = nets.small_table_embedding(tables_module, idx) if single else tables_module(idx)
        (h + fc(pe)).backward(cot)

    compare(f"-- (a) input stage, {label}, K = {K}, hidden {hidden}, forward + backward", ("ops.node_input", fused),
            ("lookup + nn.Linear + add", composition))


def l1_loss(G):
    gen = torch.Generator().manual_seed(1)
    scores = torch.randn(G, 1, generator=gen).to(dev).requires_grad_(True)
    targets = torch.randn(G, 1, generator=gen).to(dev)
    mask, n = torch.ones(G, 1, device=dev), torch.full((1,), float(G), device=dev)

    def fused():
        scores.grad = None
        ops.masked_l1_loss(scores, targets).backward()

    def plain():
        scores.grad = None
        F.l1_loss(scores, targets).backward()

    def five_op():
        scores.grad = None
        (((scores - targets).abs() * mask).sum() / n).backward()

    compare(f"-- (b) L1 loss on [{G}, 1] scores, forward + backward", ("ops.masked_l1_loss", fused), ("F.l1_loss", plain),
            ("five-op masked composition", five_op))


def zinc_step(b, K):
    """(c): captured (and, with K > 0, eager) ZINC-json step; returns the (name, step) pairs."""
    N, n_graphs = int(b["num_nodes"]), len(b["sizes"])
    gen = torch.Generator().manual_seed(0)
    avg_log = float(torch.log(torch.bincount(b["dst"], minlength=N).float() + 1).mean())
    params = dict(num_atom_type=28, num_bond_type=4, hidden_dim=45, out_dim=45, in_feat_dropout=0.0, dropout=0.0, L=4, type_net="complex",
                  pos_enc_dim=K, readout="mean", graph_norm=True, batch_norm=True, aggregators="mean dir1-dx dir1-av",
                  scalers="identity amplification attenuation", avg_d={"log": torch.tensor(avg_log)}, residual=True, edge_feat=False, edge_dim=0,
                  pretrans_layers=1, posttrans_layers=1, device="cuda")
    src, dst, eig, snorm = b["src"].to(dev), b["dst"].to(dev), b["eig"].to(dev), b["snorm_n"].to(dev)
    if eig.shape[1] < K + 1:
        eig = torch.cat([eig, torch.randn(N, K + 1 - eig.shape[1], device=dev)], 1)
    sizes = [int(s) for s in b["sizes"]]
    atoms = torch.randint(0, 28, (N,), generator=gen).to(dev)
    y = torch.randn(n_graphs, 1, generator=gen).to(dev)
    pos = dict(pos_enc=eig[:, 1:K + 1]) if K > 0 else {}
    torch.manual_seed(0)
    net_c = nets.DGNNet(params).to(dev).train()
    n_cap, e_cap = bucket_capacity(N, src.numel())
    deg = torch.bincount(torch.repeat_interleave(torch.arange(n_graphs), torch.tensor(sizes))[b["dst"]], minlength=n_graphs)
    cs = CapturedNetStep(net_c, n_cap, e_cap, g_cap=n_graphs + 1, eig_dim=eig.shape[1], lr=1e-3, max_graph_nodes=max(sizes),
                         max_graph_edges=int(deg.max()))
    cs.load(src, dst, N, eig, atoms, snorm, sizes, y, **pos)
    cs.capture(warmup=3)
    out = [(f"CapturedNetStep replay, pos_enc_dim {K}", cs.step)]
    if K > 0:
        torch.manual_seed(0)
        net = nets.DGNNet(params).to(dev).train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        graph = dgn_amd.DGNGraph(src, dst, N, eig=eig)
        graph.batch_num_nodes = sizes
        graph.ndata["pos_enc"] = pos["pos_enc"]

        def eager_step():
            opt.zero_grad(set_to_none=True)
            graph.invalidate_caches()
            net.loss(net(graph, atoms, None, snorm, None), y).backward()
            opt.step()

        out.append((f"eager step, pos_enc_dim {K}", eager_step))
    return out


def pattern_step(b, K):
    """(d): captured (and, with K > 0, eager) PATTERN-json step."""
    N = int(b["num_nodes"])
    gen = torch.Generator().manual_seed(0)
    avg_log = float(torch.log(torch.bincount(b["dst"], minlength=N).float() + 1).mean())
    params = dict(in_dim=3, hidden_dim=47, out_dim=47, n_classes=2, in_feat_dropout=0.0, dropout=0.0, L=4, type_net="complex", pos_enc_dim=K,
                  readout="mean", graph_norm=True, batch_norm=True, aggregators="mean dir1-dx dir2-dx", scalers="identity amplification attenuation",
                  avg_d={"log": torch.tensor(avg_log)}, residual=True, edge_feat=False, edge_dim=0, pretrans_layers=1, posttrans_layers=1, device="cuda")
    src, dst, eig, snorm = b["src"].to(dev), b["dst"].to(dev), b["eig"].to(dev), b["snorm_n"].to(dev)
    sizes = [int(s) for s in b["sizes"]]
    feats = torch.randint(0, 3, (N,), generator=gen).to(dev)
    y = torch.randint(0, 2, (N,), generator=gen).to(dev)
    pos = dict(pos_enc=eig[:, 1:K + 1]) if K > 0 else {}
    torch.manual_seed(0)
    net_c = nets.DGNNodeNet(params).to(dev).train()
    n_cap, e_cap = bucket_capacity(N, src.numel())
    cs = CapturedNodeStep(net_c, n_cap, e_cap, eig_dim=eig.shape[1], lr=1e-3)
    cs.load(src, dst, N, eig, feats, snorm, y, sizes, **pos)
    cs.capture(warmup=3)
    out = [(f"CapturedNodeStep replay, pos_enc_dim {K}", cs.step)]
    if K > 0:
        torch.manual_seed(0)
        net = nets.DGNNodeNet(params).to(dev).train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        graph = dgn_amd.DGNGraph(src, dst, N, eig=eig)
        graph.batch_num_nodes = sizes
        graph.ndata["pos_enc"] = pos["pos_enc"]

        def eager_step():
            opt.zero_grad(set_to_none=True)
            graph.invalidate_caches()
            net.loss(net(graph, feats, None, snorm, None), y).backward()
            opt.step()

        out.append((f"eager step, pos_enc_dim {K}", eager_step))
    return out


def replay_line(title, name, step):
    ((m, lo, hi),) = timed(step)
    print(f"{title}\n   {name}: median {m:.1f} us (p10 {lo:.1f}, p90 {hi:.1f}), device activities {device_kernels(step)}", flush=True)


print(f"{torch.cuda.get_device_name(0)}; {steps} steps after {WARMUP} warm-up steps per form")
mol128 = synth.molecule_batch(128, extra_bonds=3.9, eig_dim=9, laplacian_eig=False)
sbm128 = synth.sbm_batch(128)
if REPLAYS_ONLY:
    replay_line("-- (c) captured ZINC-json step, 128 molecules", *zinc_step(mol128, 0)[0])
    replay_line("-- (d) captured PATTERN-json step, 128 graphs", *pattern_step(sbm128, 0)[0])
    sys.exit(0)

for n_graphs in (128, 2048):
    b = mol128 if n_graphs == 128 else synth.molecule_batch(n_graphs, extra_bonds=3.9, eig_dim=9, laplacian_eig=False)
    N = int(b["num_nodes"])
    print(f"== {n_graphs} molecule graphs, {N} nodes, {b['src'].numel()} directed edges")
    gen = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    input_stage("ZINC atoms (28 types)", N, torch.nn.Embedding(28, 70).to(dev), torch.randint(0, 28, (N,), generator=gen).to(dev), 8, 70)
    atoms9 = torch.stack([torch.randint(0, d, (N,), generator=gen) for d in nets.OGB_ATOM_DIMS], 1).to(dev)
    input_stage("OGB atoms (nine tables)", N, nets.AtomEncoder(70).to(dev), atoms9, 3, 70)
    l1_loss(n_graphs)
N = int(sbm128["num_nodes"])
print(f"== 128 SBM graphs, {N} nodes, {sbm128['src'].numel()} directed edges")
torch.manual_seed(0)
input_stage("PATTERN node types (3)", N, torch.nn.Embedding(3, 47).to(dev), torch.randint(0, 3, (N,)).to(dev), 2, 47)

print("== captured steps")
(name0, replay0), = zinc_step(mol128, 0)
replay_line("-- (c) captured ZINC-json step, 128 molecules", name0, replay0)
(name8, replay8), eager8 = zinc_step(mol128, 8)
compare("-- (c) ZINC-json step with positional encodings, 128 molecules", (name8, replay8), eager8)
(name0, replay0), = pattern_step(sbm128, 0)
replay_line("-- (d) captured PATTERN-json step, 128 graphs", name0, replay0)
(name2, replay2), eager2 = pattern_step(sbm128, 2)
compare("-- (d) PATTERN-json step with positional encodings, 128 graphs", (name2, replay2), eager2)
