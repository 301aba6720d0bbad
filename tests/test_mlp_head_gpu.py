"""The fused MLPReadout head (csrc/dgn_mlp_head.hip, ``ops.mlp_head``) on the GPU.

Ground truth is the same ``nn.Linear`` / ReLU composition in float64 on the device -- the reference module's whole definition
(nets/mlp_readout_layer.py:24-30); the reference's own numbers reach the head through fixtures G10, G11 and G13 in the net tests.
Tolerance: the rule of tests/test_mol_io_gpu.py, no constant of this file's own.  For the output, ``g_x``, every ``g_W`` and every ``g_b``:
the kernel's error against fp64, relative to the tensor's largest magnitude, is at most ``max(4 x the torch fp32 composition's error
against the same fp64, 1e-6)`` (4 = the project's margin for a different summation order); both errors go to the parity report.
Shapes: the kernels' tile is 32 rows (so 31 / 32 / 33 are the tile and its neighbours), a workgroup per tile up to 256 workgroups
(15 361 rows = 481 tiles: two tiles per workgroup, the slot's load-add-store path)."""
import copy

import numpy as np
import pytest
import torch

import parity_util

pytestmark = pytest.mark.gpu

WIDTHS = [(47, 23, 11, 2), (45, 22, 11, 1), (70, 35, 17, 1), (70, 70, 70, 128), (20, 10, 5, 1), (128, 64, 32, 32), (7, 1), (5, 3, 2)]
ROWS = [1, 31, 32, 33, 1000]
PATTERN, PATTERN_ROWS = (47, 23, 11, 2), 15361


def _params(dims, seed, dev, dtype=torch.float32):
    """weights of standard deviation sqrt(2 / fan_in) (ReLUs fire both ways), biases of 0.1"""
    gen = torch.Generator().manual_seed(seed)
    ws = [torch.randn(o, i, generator=gen) * (2.0 / i) ** 0.5 for i, o in zip(dims[:-1], dims[1:])]
    bs = [0.1 * torch.randn(o, generator=gen) for o in dims[1:]]
    return [w.to(dev, dtype) for w in ws], [b.to(dev, dtype) for b in bs]


def _composition(x, ws, bs):
    for w, b in zip(ws[:-1], bs[:-1]):
        x = torch.relu(torch.nn.functional.linear(x, w, b))
    return torch.nn.functional.linear(x, ws[-1], bs[-1])


def _run(fn, x, ws, bs, cot, dtype=torch.float32, x_grad=True):
    """(y, g_x or None, g_W..., g_b...) of ``fn`` on fresh leaves of ``dtype``"""
    x = x.detach().to(dtype).requires_grad_(x_grad)
    ws, bs = [w.detach().to(dtype).requires_grad_(True) for w in ws], [b.detach().to(dtype).requires_grad_(True) for b in bs]
    y = fn(x, ws, bs)
    grads = torch.autograd.grad(y, ([x] if x_grad else []) + ws + bs, cot.to(dtype))
    return [y.detach()] + ([] if x_grad else [None]) + list(grads)


def _names(n_lin):
    return ["y", "g_x"] + [f"g_W{l}" for l in range(n_lin)] + [f"g_b{l}" for l in range(n_lin)]


def _judge(mine, r32, r64, what):
    for name, a, b, c in zip(_names((len(mine) - 2) // 2), mine, r32, r64):
        scale = float(c.abs().max())
        if scale == 0.0:                                                       # (every ReLU in front of it closed: exact zeros on all sides)
            assert not bool(a.any()), (what, name)
            continue
        e_ref, e_mine = float((b.double() - c).abs().max()) / scale, float((a.double() - c).abs().max()) / scale
        parity_util.note(f"mlp_head {what} {name}: torch fp32 {e_ref:.2e}  kernel {e_mine:.2e}")
        assert e_mine <= max(4 * e_ref, 1e-6), (what, name, e_mine, e_ref)


def _case(dims, N, dev, seed=0):
    gen = torch.Generator().manual_seed(1000 * seed + N)
    ws, bs = _params(dims, seed + len(dims), dev)
    return torch.randn(N, dims[0], generator=gen).to(dev), ws, bs, torch.randn(N, dims[-1], generator=gen).to(dev)


@pytest.fixture(scope="module")
def pattern_case():
    """15 361 x (47, 23, 11, 2): the inputs and the fp32 / fp64 compositions, computed once"""
    dev = torch.device("cuda")
    x, ws, bs, cot = _case(PATTERN, PATTERN_ROWS, dev)
    return x, ws, bs, cot, _run(_composition, x, ws, bs, cot), _run(_composition, x, ws, bs, cot, torch.float64)


@pytest.mark.parametrize("dims", WIDTHS, ids=lambda d: "-".join(map(str, d)))
def test_value_and_gradient_parity(dims):
    from dgn_amd import ops
    dev = torch.device("cuda")
    for N in ROWS:
        x, ws, bs, cot = _case(dims, N, dev)
        assert ops.mlp_head_supported(x, ws)
        mine = _run(ops.mlp_head, x, ws, bs, cot)
        assert tuple(mine[0].shape) == (N, dims[-1]) and tuple(mine[1].shape) == (N, dims[0])
        _judge(mine, _run(_composition, x, ws, bs, cot), _run(_composition, x, ws, bs, cot, torch.float64), f"{dims} N={N}")


def test_value_and_gradient_parity_at_the_pattern_batch(pattern_case):
    from dgn_amd import ops
    x, ws, bs, cot, r32, r64 = pattern_case
    _judge(_run(ops.mlp_head, x, ws, bs, cot), r32, r64, f"{PATTERN} N={PATTERN_ROWS}")


def test_two_runs_are_bit_equal(pattern_case):
    from dgn_amd import ops
    x, ws, bs, cot = pattern_case[:4]
    for a, b in zip(_run(ops.mlp_head, x, ws, bs, cot), _run(ops.mlp_head, x, ws, bs, cot)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dims,N", [((47, 23, 11, 2), 1000), ((70, 70, 70, 128), 33), ((7, 1), 65)], ids=["pattern", "pcba", "single"])
def test_column_slice_input_and_non_contiguous_cotangent(dims, N):
    """x = big[:, 1:1 + d0]: row stride above d0, base 4 bytes off a 16-byte boundary; g_y the ``.t()`` of a transposed buffer."""
    from dgn_amd import ops
    dev = torch.device("cuda")
    x, ws, bs, cot = _case(dims, N, dev, seed=1)
    big = torch.full((N, dims[0] + 5), float("nan"), device=dev)
    big[:, 1:1 + dims[0]] = x
    view = big[:, 1:1 + dims[0]]
    assert view.stride(0) > dims[0] and view.data_ptr() % 16 == 4 and ops.mlp_head_supported(view, ws)
    cot_t = cot.t().contiguous().t()
    assert not cot_t.is_contiguous() or min(cot.shape) == 1
    r32, r64 = _run(_composition, x, ws, bs, cot), _run(_composition, x, ws, bs, cot, torch.float64)
    _judge(_run(ops.mlp_head, x, ws, bs, cot_t), r32, r64, f"{dims} N={N} transposed g_y")
    # through the view itself: the gradient of the wide leaf is zero outside the slice
    leaf = big.clone().requires_grad_(True)
    w2, b2 = [w.clone().requires_grad_(True) for w in ws], [b.clone().requires_grad_(True) for b in bs]
    y = ops.mlp_head(leaf[:, 1:1 + dims[0]], w2, b2)
    grads = torch.autograd.grad(y, [leaf] + w2 + b2, cot_t)
    assert bool((grads[0][:, :1] == 0).all()) and bool((grads[0][:, 1 + dims[0]:] == 0).all())
    _judge([y.detach(), grads[0][:, 1:1 + dims[0]]] + list(grads[1:]), r32, r64, f"{dims} N={N} column slice")


def test_no_rows():
    from dgn_amd import ops
    dev = torch.device("cuda")
    x, ws, bs, _ = _case(PATTERN, 0, dev)
    mine = _run(ops.mlp_head, x, ws, bs, torch.zeros(0, 2, device=dev))
    assert tuple(mine[0].shape) == (0, 2) and tuple(mine[1].shape) == (0, 47)
    for g, p in zip(mine[2:], ws + bs):
        assert g.shape == p.shape and not bool(g.any())


def test_relu_passes_nothing_at_an_activation_of_exactly_zero():
    from dgn_amd import ops
    dev = torch.device("cuda")
    dims = (20, 10, 5, 1)
    x, ws, bs, cot = _case(dims, 65, dev, seed=2)
    ws[0][3].zero_()
    bs[0][3] = 0.0
    ws[1][:, 3] = 1.0                                                          # (the unit's outgoing weights are not what stops its gradient)
    y, g_x, gw0, gw1, gw2, gb0, gb1, gb2 = _run(ops.mlp_head, x, ws, bs, cot)
    assert not bool(gw0[3].any()) and float(gb0[3]) == 0.0 and not bool(gw1[:, 3].any())
    assert bool(gw0.any()) and bool(gw1.any()) and bool(gb0.any())
    _judge([y, g_x, gw0, gw1, gw2, gb0, gb1, gb2], _run(_composition, x, ws, bs, cot), _run(_composition, x, ws, bs, cot, torch.float64), "zero unit")


def test_needs_input_grad_and_no_grad():
    from dgn_amd import ops
    dev = torch.device("cuda")
    x, ws, bs, cot = _case(PATTERN, 1000, dev, seed=3)
    full = _run(ops.mlp_head, x, ws, bs, cot)
    params_only = _run(ops.mlp_head, x, ws, bs, cot, x_grad=False)
    assert params_only[1] is None and torch.equal(full[0], params_only[0])
    for a, b in zip(full[2:], params_only[2:]):
        assert torch.equal(a, b)
    with torch.no_grad():
        y = ops.mlp_head(x, [w.requires_grad_(True) for w in ws], bs)
    assert not y.requires_grad and torch.equal(y, full[0])
    # only some parameters ask for a gradient
    w0 = ws[0].detach().clone().requires_grad_(True)
    frozen = [w0] + [w.detach() for w in ws[1:]]
    (g,) = torch.autograd.grad(ops.mlp_head(x, frozen, [b.detach() for b in bs]), [w0], cot)
    assert torch.equal(g, full[2])


def _device_events(step):
    """Names of the device activities of one step, one entry per launch (the pattern of tests/test_mol_io_gpu.py)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    evs = prof.profiler.kineto_results.events()
    return [e.name() for e in evs if str(e.device_type()).endswith("CUDA")]


def test_launch_counts():
    from dgn_amd import ops
    dev = torch.device("cuda")
    x, ws, bs, cot = _case(PATTERN, 1000, dev)
    x.requires_grad_(True)
    leaves = [x] + [t.requires_grad_(True) for t in ws + bs]
    torch.autograd.grad(ops.mlp_head(x, ws, bs), leaves, cot)                  # (first call: library load, allocator, LDS attribute)
    out = []
    names = _device_events(lambda: out.append(ops.mlp_head(x, ws, bs)))
    assert len(names) == 1 and "mlp_head_forward" in names[0], names
    names = _device_events(lambda: torch.autograd.grad(out[0], leaves, cot))
    assert 1 <= len(names) <= 2 and all("mlp_head_" in n for n in names), names


def _net_case(which, dev):
    """(net, forward-and-loss closure) of a small net on a few synthetic graphs"""
    import dgn_amd
    from dgn_amd import synth
    from dgn_amd.nets import OGB_ATOM_DIMS, DGNNet, DGNNodeNet, DGNPCBANet
    gen = torch.Generator().manual_seed(11)
    avg_d = {"log": torch.tensor(1.1)}
    if which == "zinc":
        b = synth.molecule_batch(7, seed=31, laplacian_eig=False)
        net = DGNNet(dict(num_atom_type=9, num_bond_type=4, hidden_dim=20, out_dim=20, in_feat_dropout=0.0, dropout=0.0, L=2, type_net="towers",
                          pos_enc_dim=0, readout="mean", graph_norm=True, batch_norm=True, aggregators="mean max min dir1-av dir1-dx",
                          scalers="identity amplification attenuation", avg_d=avg_d, residual=True, edge_feat=False, edge_dim=0,
                          pretrans_layers=1, posttrans_layers=1, device="cuda"))
        N = int(b["num_nodes"])
        feats, y = torch.randint(0, 9, (N,), generator=gen).to(dev), torch.randn(7, 1, generator=gen).to(dev)
    elif which == "pattern":
        b = synth.sbm_batch(6, seed=32)
        net = DGNNodeNet(dict(in_dim=3, hidden_dim=47, out_dim=47, n_classes=2, in_feat_dropout=0.0, dropout=0.0, L=2, type_net="complex",
                              pos_enc_dim=0, readout="mean", graph_norm=True, batch_norm=True, aggregators="mean dir1-dx dir2-dx",
                              scalers="identity amplification attenuation", avg_d=avg_d, residual=True, edge_feat=False, edge_dim=0,
                              pretrans_layers=1, posttrans_layers=1, device="cuda"))
        N = int(b["num_nodes"])
        feats, y = torch.randint(0, 3, (N,), generator=gen).to(dev), torch.randint(0, 2, (N,), generator=gen).to(dev)
    else:
        b = synth.molecule_batch(9, seed=33, laplacian_eig=False)
        net = DGNPCBANet(dict(L=2, hidden_dim=70, out_dim=70, type_net="simple", residual=True, edge_feat=False, readout="mean", in_feat_dropout=0.0,
                              dropout=0.0, graph_norm=False, batch_norm=True, aggregators="mean max min dir1-dx dir1-av", scalers="identity", towers=5,
                              edge_dim=0, pretrans_layers=1, posttrans_layers=1, decreasing_dim=False, virtual_node=None, avg_d=avg_d, device="cuda"))
        N = int(b["num_nodes"])
        feats = torch.stack([torch.randint(0, d, (N,), generator=gen) for d in OGB_ATOM_DIMS], 1).to(dev)
        y = (torch.rand(9, 128, generator=gen) < 0.3).float()
        y[torch.rand(9, 128, generator=gen) < 0.4] = float("nan")
        y = y.to(dev)
    torch.manual_seed(3)
    net = net.to(dev).train()
    with torch.no_grad():                                                      # (wider than the stock gain = 1 / in_size head: scores away from 0)
        for fc in net.MLP_layer.FC_layers:
            fc.weight.normal_(0.0, (2.0 / fc.weight.shape[1]) ** 0.5)

    def step(model):
        g = dgn_amd.DGNGraph(b["src"].to(dev), b["dst"].to(dev), N, eig=b["eig"].to(dev))
        g.batch_num_nodes = [int(s) for s in b["sizes"]]
        scores = model(g, feats, None, b["snorm_n"].to(dev), None)
        model.loss(scores, y).backward()
        return scores.detach()
    return net, step


@pytest.mark.parametrize("which", ["zinc", "pattern", "pcba"])
def test_the_nets_take_the_fused_head(monkeypatch, which):
    """DGNNet / DGNNodeNet / DGNPCBANet call ``ops.mlp_head`` once per forward; with the switch off they do not, and scores and gradients
    agree within the net tests' tolerances (tests/test_node_net_gpu.py: scores rtol 2e-4 / atol 2e-5, gradients rtol 2e-3 / atol 2e-4 of
    the tensor's largest magnitude, floor 1e-2)."""
    from dgn_amd import ops
    dev = torch.device("cuda")
    net, step = _net_case(which, dev)
    twin = copy.deepcopy(net)
    calls = []
    real = ops.mlp_head
    monkeypatch.setattr(ops, "mlp_head", lambda *a, **k: calls.append(tuple(a[0].shape)) or real(*a, **k))
    assert ops.FUSED_MLP_HEAD
    scores = step(net)
    assert len(calls) == 1 and calls[0][1] == net.MLP_layer.FC_layers[0].in_features, calls
    monkeypatch.setattr(ops, "FUSED_MLP_HEAD", False)
    scores_t = step(twin)
    assert len(calls) == 1, calls                                              # the other side stayed on torch's composition
    np.testing.assert_allclose(scores.cpu().numpy(), scores_t.cpu().numpy(), rtol=2e-4, atol=2e-5)
    n_checked = 0
    for (k, p), (_, q) in zip(net.named_parameters(), twin.named_parameters()):
        assert (p.grad is None) == (q.grad is None), k
        if p.grad is not None:
            ref = q.grad.cpu().numpy()
            np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=2e-3, atol=2e-4 * max(1e-2, float(np.abs(ref).max())), err_msg=k)
            n_checked += 1
    assert n_checked >= 12 and all(fc.weight.grad is not None and fc.bias.grad is not None for fc in net.MLP_layer.FC_layers)


def test_capture_and_replay_equal_eager_calls():
    from dgn_amd import ops
    dev = torch.device("cuda")
    dims, N = PATTERN, 1000
    x, ws, bs, cot = _case(dims, N, dev, seed=4)
    others = [_case(dims, N, dev, seed=s)[0] for s in (5, 6)]
    sx = x.clone().requires_grad_(True)
    leaves = [sx] + [t.clone().requires_grad_(True) for t in ws + bs]

    def work():
        y = ops.mlp_head(sx, leaves[1:1 + len(ws)], leaves[1 + len(ws):])
        return [y] + list(torch.autograd.grad(y, leaves, cot))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = work()
    for other in others:
        with torch.no_grad():
            sx.copy_(other)
        graph.replay()
        torch.cuda.synchronize()
        eager = _run(ops.mlp_head, other, ws, bs, cot)
        for a, b in zip(static, eager):
            assert torch.equal(a.detach(), b)
