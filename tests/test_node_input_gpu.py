"""The input-stage kernels (csrc/dgn_node_input.hip: dgn_node_input_*) on the GPU through ``ops.node_input`` against the fp64 restatement
(tests/input_stage_oracle.py).

Forward: an output is C table terms, K fused multiply-adds from the bias on and one last add: C + K + 1 roundings, each at most 2^-24 of
a partial sum that the sum of the terms' magnitudes bounds.  The test asserts twice that:
``|ours - r64| <= (C + K + 1) 2^-23 (sum_c |T_c| + |b| + sum_k |W pe|)`` per entry.  Gradients (sums over the batch's rows):
``parity_util.check_reduced`` at its defaults, r32 = the CPU fp32 autograd of nn.Embedding + nn.Linear + add, r64 the same composition
in fp64."""
import types

import numpy as np
import pytest
import torch

import input_stage_oracle as iso
from parity_util import check_reduced

pytestmark = pytest.mark.gpu

FWD_ROWS = 64             # kFwdRows: rows per forward workgroup
MIN_ROWS = 64             # kMinRows: rows of one backward workgroup's range while there are fewer than MAX_GROUPS ranges
MAX_GROUPS = 256          # kMaxGroups
OGB_ATOM_DIMS = [119, 4, 12, 12, 10, 6, 6, 2, 2]
CASES = [(1, [3], 2, 47), (1, [28], 8, 45), (1, [7], 1, 1), (1, [6], 40, 70), (9, OGB_ATOM_DIMS, 3, 70), (2, [5, 2], 20, 75)]
ROWS = [1, 63, 65, 197, MIN_ROWS * 3 + 5, 20000]      # (20 000 > MIN_ROWS * MAX_GROUPS: a full set of slots, ranges of 79 rows)


def _case(N, dims, K, F, seed=0, bias=True):
    gen = torch.Generator().manual_seed(seed + 7 * N + 1000 * K + F)
    idx = torch.stack([torch.randint(0, d, (N,), generator=gen) for d in dims], dim=1)
    tables = [torch.randn(d, F, generator=gen) for d in dims]
    eig = torch.randn(N, K + 2, generator=gen)
    w = torch.randn(F, K, generator=gen) / K ** 0.5
    b = torch.randn(F, generator=gen) if bias else None
    gy = torch.randn(N, F, generator=gen)
    return idx, tables, eig, w, b, gy


def _composition(idx, tables, pe, w, b, gy, dtype):
    """CPU autograd of nn.Embedding + nn.Linear + add (dgn_net.py:58-62): the output and the gradients of the tables, W and b."""
    ts = [t.to(dtype).clone().requires_grad_(True) for t in tables]
    wd = w.to(dtype).clone().requires_grad_(True)
    bd = b.to(dtype).clone().requires_grad_(True) if b is not None else None
    h = 0
    for c, t in enumerate(ts):
        h = h + torch.nn.functional.embedding(idx[:, c], t)
    h = h + torch.nn.functional.linear(pe.to(dtype), wd, bd)
    h.backward(gy.to(dtype))
    return h.detach(), [t.grad for t in ts], wd.grad, bd.grad if b is not None else None


def _run(idx, tables, pe, w, b, gy):
    """forward + backward through the op on the device (idx / pe as given: device tensors, possibly views)."""
    from dgn_amd import ops
    dev = torch.device("cuda")
    ts = [t.to(dev).requires_grad_(True) for t in tables]
    wd = w.to(dev).requires_grad_(True)
    bd = b.to(dev).requires_grad_(True) if b is not None else None
    assert ops.node_input_supported(ts, pe, wd)
    h = ops.node_input(idx, ts, pe, wd, bd)
    assert tuple(h.shape) == (idx.shape[0], w.shape[0]) and h.is_contiguous()
    h.backward(gy.to(dev))
    torch.cuda.synchronize()
    return h.detach().cpu(), [t.grad.cpu() for t in ts], wd.grad.cpu(), bd.grad.cpu() if b is not None else None


def _check(name, idx, tables, pe, w, b, gy, got):
    h, g_tables, g_w, g_b = got
    C, K = len(tables), w.shape[1]
    np_tables = [t.numpy() for t in tables]
    nb = b.numpy() if b is not None else None
    r64 = iso.input_stage(idx.numpy(), np_tables, pe.numpy(), w.numpy(), nb, np.float64)
    bound = (C + K + 1) * 2.0 ** -23 * iso.input_stage_magnitude(idx.numpy(), np_tables, pe.numpy(), w.numpy(), nb)
    err = np.abs(h.numpy().astype(np.float64) - r64)
    assert bool((err <= bound).all()), (name, float((err - bound).max()))
    _, t32, w32, b32 = _composition(idx, tables, pe, w, b, gy, torch.float32)
    _, t64, w64, b64 = _composition(idx, tables, pe, w, b, gy, torch.float64)
    for c in range(C):
        check_reduced(g_tables[c], t32[c], t64[c], f"{name} table {c}")
    check_reduced(g_w, w32, w64, f"{name} dW")
    if b is not None:
        check_reduced(g_b, b32, b64, f"{name} db")
    if idx.shape[0] <= 1000:                     # the restatement's gradients and the fp64 autograd agree (small batches: it walks the rows)
        o64, ow64, ob64 = iso.input_stage_grads(idx.numpy(), [t.shape[0] for t in tables], pe.numpy(), gy.numpy(), np.float64)
        for c in range(C):
            np.testing.assert_allclose(t64[c].numpy(), o64[c], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(w64.numpy(), ow64, rtol=1e-9, atol=1e-9)
        if b is not None:
            np.testing.assert_allclose(b64.numpy(), ob64, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("C,dims,K,F", CASES)
def test_forward_and_gradients_vs_fp64(C, dims, K, F):
    assert C == len(dims)
    for N in sorted(set(ROWS)):
        idx, tables, eig, w, b, gy = _case(N, dims, K, F)
        pe = eig[:, :K].contiguous()
        flat = idx[:, 0] if C == 1 else idx                                  # one table: idx [N], as the nets pass it
        got = _run(flat.cuda(), tables, pe.cuda(), w, b, gy)
        _check(f"node_input C={C} K={K} F={F} N={N}", idx, tables, pe, w, b, gy, got)


@pytest.mark.parametrize("C,dims,K,F,N", [(1, [28], 8, 45, 197), (9, OGB_ATOM_DIMS, 3, 70, 131), (2, [5, 2], 20, 75, 65), (1, [7], 1, 1, 63)])
def test_strided_unaligned_views_and_no_bias(C, dims, K, F, N):
    """``pos_enc`` as ``eig[:, 1:K+1]`` of a ``[N, K + 2]`` tensor (row stride K + 2, base 4 bytes past the allocation's alignment) and
    ``idx`` as a column slice of a wider tensor: only their own columns are read (the others hold NaN / a huge index), and the numbers are
    those of the contiguous call.  Without bias the linear terms start at zero and no bias gradient exists."""
    idx, tables, eig, w, b, gy = _case(N, dims, K, F, seed=5)
    eig[:, 0], eig[:, K + 1] = float("nan"), float("nan")
    pe_view = eig.cuda()[:, 1:K + 1]
    assert pe_view.stride(0) == K + 2 and pe_view.data_ptr() % 16 == 4
    wide = torch.full((N, C + 2), 2 ** 40, dtype=torch.int64)
    wide[:, 1:C + 1] = idx
    idx_view = wide.cuda()[:, 1:C + 1]
    assert idx_view.stride(0) == C + 2
    pe = eig[:, 1:K + 1].contiguous()
    got = _run(idx_view, tables, pe_view, w, b, gy)
    _check(f"node_input views C={C} K={K} F={F} N={N}", idx, tables, pe, w, b, gy, got)
    ref = _run(idx.cuda(), tables, pe.cuda(), w, b, gy)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2]) and torch.equal(got[3], ref[3])
    assert all(torch.equal(a, r) for a, r in zip(got[1], ref[1]))
    nb = _run(idx.cuda(), tables, pe.cuda(), w, None, gy)
    assert nb[3] is None and torch.equal(nb[2], ref[2]) and all(torch.equal(a, r) for a, r in zip(nb[1], ref[1]))
    _check(f"node_input no bias C={C} K={K} F={F} N={N}", idx, tables, pe, w, None, gy, nb)


def test_out_of_range_indices_are_clamped():
    """An index outside its table is clamped into it in both directions (memory-safe by construction, as ``multi_embedding``): the
    numbers are those of the clamped indices."""
    dims, K, F, N = [5, 2], 3, 47, 130
    idx, tables, eig, w, b, gy = _case(N, dims, K, F, seed=9)
    bad = idx.clone()
    bad[::7, 0] = -3
    bad[3::11, 1] = 2 + 5
    bad[5::13, 0] = 2 ** 40
    clamped = torch.stack([bad[:, c].clamp(0, d - 1) for c, d in enumerate(dims)], dim=1)
    pe = eig[:, 1:K + 1].contiguous()
    got, ref = _run(bad.cuda(), tables, pe.cuda(), w, b, gy), _run(clamped.cuda(), tables, pe.cuda(), w, b, gy)
    assert torch.equal(got[0], ref[0]) and all(torch.equal(a, r) for a, r in zip(got[1], ref[1]))
    _check("node_input clamped", clamped, tables, pe, w, b, gy, got)


@pytest.mark.parametrize("C,dims,K,F,N", [(1, [28], 8, 45, 20000), (9, OGB_ATOM_DIMS, 3, 70, 1000)])
def test_gradients_are_bit_equal_across_two_runs(C, dims, K, F, N):
    idx, tables, eig, w, b, gy = _case(N, dims, K, F, seed=3)
    pe = eig.cuda()[:, 1:K + 1]
    a, c = _run(idx.cuda(), tables, pe, w, b, gy), _run(idx.cuda(), tables, pe, w, b, gy)
    for p, q in zip([a[0], *a[1], a[2], a[3]], [c[0], *c[1], c[2], c[3]]):
        assert p.numpy().tobytes() == q.numpy().tobytes()


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
    idx, tables, eig, w, b, gy = _case(3001, [28], 8, 70, seed=1)
    ts = [t.to(dev).requires_grad_(True) for t in tables]
    wd, bd, cot = w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True), gy.to(dev)
    idx, pe = idx[:, 0].to(dev), eig.to(dev)[:, 1:9]
    params = ts + [wd, bd]
    torch.autograd.grad(ops.node_input(idx, ts, pe, wd, bd), params, cot)        # (first call: library load, allocator, LDS attribute)
    out = []
    names = _device_events(lambda: out.append(ops.node_input(idx, ts, pe, wd, bd)))
    assert len(names) == 1 and "node_input_forward" in names[0], names
    names = _device_events(lambda: torch.autograd.grad(out[0], params, cot))
    assert len(names) == 2 and all("node_input_backward" in n for n in names), names


def test_empty_batch():
    from dgn_amd import ops
    dev = torch.device("cuda")
    idx, tables, eig, w, b, gy = _case(0, [6], 3, 20)
    ts = [t.to(dev).requires_grad_(True) for t in tables]
    wd, bd = w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    h = ops.node_input(idx[:, 0].to(dev), ts, eig.to(dev)[:, 1:4], wd, bd)
    assert tuple(h.shape) == (0, 20)
    h.sum().backward()
    assert bool((ts[0].grad == 0).all()) and bool((wd.grad == 0).all()) and bool((bd.grad == 0).all())


@pytest.mark.parametrize("dims,K,F,p,why", [([6], 41, 20, 0.0, "K = 41"), ([600], 3, 70, 0.0, "604 x 70 floats over the LDS budget"),
                                            ([6], 3, 20, 0.5, "in_feat_dropout active between the two terms")])
def test_outside_the_domain_the_nets_take_the_composition(monkeypatch, dims, K, F, p, why):
    """Shapes the kernels do not take, a ``pos_enc`` that asks for a gradient, and an active dropout: the op says so, and the nets' input
    stage runs nn.Embedding + nn.Linear + add."""
    from dgn_amd import nets, ops
    dev = torch.device("cuda")
    N = 150
    idx, tables, eig, w, b, gy = _case(N, dims, K, F, seed=11)
    emb = torch.nn.Embedding(dims[0], F).to(dev)
    fc = torch.nn.Linear(K, F).to(dev)
    with torch.no_grad():
        emb.weight.copy_(tables[0])
        fc.weight.copy_(w)
        fc.bias.copy_(b)
    net = types.SimpleNamespace(embedding_pos_enc=fc, in_feat_dropout=torch.nn.Dropout(p).train())
    pe = eig.to(dev)[:, 1:K + 1]
    graph = types.SimpleNamespace(ndata={"pos_enc": pe})
    if p == 0.0:
        assert not ops.node_input_supported([emb.weight], pe, fc.weight), why
        with pytest.raises(ValueError, match="not supported"):
            ops.node_input(idx[:, 0].to(dev), [emb.weight], pe, fc.weight, fc.bias)
    else:
        assert ops.node_input_supported([emb.weight], pe, fc.weight)
    called = []
    monkeypatch.setattr(ops, "node_input", lambda *a, **k: called.append(1))
    h = nets._input_with_pos_enc(net, [emb.weight], idx[:, 0].to(dev), emb, graph)
    assert not called and tuple(h.shape) == (N, F), why
    if p == 0.0:
        r64 = iso.input_stage(idx.numpy(), [tables[0].numpy()], eig[:, 1:K + 1].numpy(), w.numpy(), b.numpy(), np.float64)
        np.testing.assert_allclose(h.detach().cpu().numpy(), r64, rtol=1e-4, atol=1e-4)      # (the library GEMM may run reduced precision)
        h.backward(gy.to(dev))
        assert emb.weight.grad is not None and fc.weight.grad is not None


def test_pos_enc_that_asks_for_a_gradient_is_not_supported():
    from dgn_amd import ops
    dev = torch.device("cuda")
    idx, tables, eig, w, b, gy = _case(50, [6], 3, 20, seed=13)
    ts, wd = [tables[0].to(dev)], w.to(dev)
    pe = eig.to(dev)[:, 1:4].clone().requires_grad_(True)
    assert not ops.node_input_supported(ts, pe, wd) and ops.node_input_supported(ts, pe.detach(), wd)
    with pytest.raises(ValueError, match="not supported"):
        ops.node_input(idx[:, 0].to(dev), ts, pe, wd, None)
