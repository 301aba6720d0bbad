"""``ops.masked_l1_loss`` (csrc/dgn_mol_io.hip: the bce_stats / bce_rows pair on the L1 term, dgn_masked_mae_*) on the GPU against the
fp64 restatement (tests/input_stage_oracle.py::masked_l1).

Loss: the kernel rounds each ``s - t`` once (2^-24 relative on that term, so on the sum of the terms' magnitudes), sums the fp32 terms in
fp64 (errors far below) and rounds the quotient once to fp32 (2^-24): 2^-23 in all, asserted with a factor 2 of margin as 2^-22 relative.
Gradient: exactly ``float32(sign(s - t) / count)``, exactly 0 at the masked entries and at ties."""
import numpy as np
import pytest
import torch

import input_stage_oracle as iso

pytestmark = pytest.mark.gpu

STATS_ELEMS = 2048        # kBceMinElems: elements of one stats workgroup's range while there are fewer than 256 ranges
GS = [1, 63, 64, 65, 1000, STATS_ELEMS + 5]      # (the last: past a single stats range for T = 1, three ranges for T = 3)


def _case(G, T, seed=0):
    """T = 3: about 40 % of the targets NaN; T = 1: none.  15 % planted ties either way."""
    gen = torch.Generator().manual_seed(seed + 31 * G + T)
    s = torch.randn(G, T, generator=gen)
    t = torch.randn(G, T, generator=gen)
    ties = torch.rand(G, T, generator=gen) < 0.15                      # planted ties: s == t exactly
    t[ties] = s[ties]
    if T == 3:
        t[torch.rand(G, T, generator=gen) < 0.4] = float("nan")
    return s, t


def _check(s, t, loss, grad):
    l64, _ = iso.masked_l1(s.numpy(), t.numpy(), np.float64)
    _, g32 = iso.masked_l1(s.numpy(), t.numpy(), np.float32)
    keep = ~torch.isnan(t)
    count = int(keep.sum())
    if count == 0:
        assert np.isnan(loss) and bool((grad == 0).all())
        return
    assert abs(loss - float(l64)) <= 2.0 ** -22 * abs(float(l64)), (loss, float(l64))
    sign = torch.sign(torch.where(keep, s - torch.nan_to_num(t), torch.zeros_like(s))).numpy()
    expect = (sign * np.float32(1.0 / count)).astype(np.float32)
    assert grad.numpy().tobytes() == np.where(sign == 0, np.float32(0), expect).astype(np.float32).tobytes()
    assert grad.numpy().tobytes() == g32.tobytes()                      # the restatement's fp32 form, bit for bit
    assert bool((grad[~keep] == 0).all()) and bool((grad[(s == t)] == 0).all())


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("G", GS)
def test_loss_and_gradient_vs_fp64(G, T):
    from dgn_amd import ops
    s, t = _case(G, T)
    sd = s.cuda().requires_grad_(True)
    loss = ops.masked_l1_loss(sd, t.cuda())
    assert loss.dim() == 0 and loss.is_cuda
    loss.backward()
    _check(s, t, float(loss), sd.grad.cpu())
    if T == 1:                                                         # 1-D scores and targets, as a loop may pass them
        s1 = s[:, 0].cuda().requires_grad_(True)
        l1 = ops.masked_l1_loss(s1, t[:, 0].cuda())
        l1.backward()
        assert float(l1) == float(loss) and torch.equal(s1.grad.cpu(), sd.grad.cpu()[:, 0])
        if not bool(torch.isnan(t).any()):                              # no NaN: nn.L1Loss() itself
            ref = torch.nn.L1Loss()(s.double(), t.double())
            assert abs(float(loss) - float(ref)) <= 2.0 ** -22 * abs(float(ref))


def test_upstream_gradient_scales_the_saved_one():
    from dgn_amd import ops
    s, t = _case(300, 3, seed=2)
    sd = s.cuda().requires_grad_(True)
    (2.5 * ops.masked_l1_loss(sd, t.cuda())).backward()
    _, g32 = iso.masked_l1(s.numpy(), t.numpy(), np.float32)
    assert sd.grad.cpu().numpy().tobytes() == (g32 * np.float32(2.5)).astype(np.float32).tobytes()


def test_all_targets_nan():
    from dgn_amd import ops
    s, t = _case(70, 3, seed=3)
    t[:] = float("nan")
    sd = s.cuda().requires_grad_(True)
    loss = ops.masked_l1_loss(sd, t.cuda())
    loss.backward()
    assert bool(torch.isnan(loss)) and bool((sd.grad == 0).all())


def test_strided_scores_and_other_target_dtypes():
    from dgn_amd import ops
    s, t = _case(131, 3, seed=4)
    wide = torch.full((131, 5), float("nan"))
    wide[:, 1:4] = s
    view = wide.cuda()[:, 1:4].requires_grad_(True)
    assert view.stride(0) == 5
    loss = ops.masked_l1_loss(view, t.cuda())
    (g,) = torch.autograd.grad(loss, view)
    _check(s, t, float(loss), g.cpu())
    s1, t1 = _case(64, 1, seed=5)
    ti = (t1 * 3).round().to(torch.int64)                              # integer targets: any dtype is taken
    sd = s1.cuda().requires_grad_(True)
    loss = ops.masked_l1_loss(sd, ti.cuda())
    loss.backward()
    _check(s1, ti.float(), float(loss), sd.grad.cpu())


def test_no_grad_allocates_no_gradient_buffer():
    from dgn_amd import ops
    s, t = _case(1 << 18, 3, seed=6)
    sd, td = s.cuda(), t.cuda()
    with torch.no_grad():
        ops.masked_l1_loss(sd, td)                                     # (first call: library load, workspace blocks in the allocator)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss = ops.masked_l1_loss(sd, td)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    assert not loss.requires_grad
    assert peak < s.numel() * 4 // 2, peak                             # a [G, T] fp32 gradient would be 3 MiB
    l64, _ = iso.masked_l1(s.numpy(), t.numpy(), np.float64)
    assert abs(float(loss) - float(l64)) <= 2.0 ** -22 * abs(float(l64))


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
    s, t = _case(3000, 3, seed=7)
    x, y = s.cuda().requires_grad_(True), t.cuda()
    ops.masked_l1_loss(x, y).backward()
    out = []
    names = _device_events(lambda: out.append(ops.masked_l1_loss(x, y)))
    assert len(names) == 2 and all("bce_" in n and "L1Term" in n for n in names), names
    one = torch.ones((), device="cuda")
    names = _device_events(lambda: torch.autograd.grad(out[0], x, grad_outputs=one))
    assert len(names) == 1 and "bce_scale" in names[0], names


def test_dgn_net_loss_routes():
    """``DGNNet.loss``: ``ops.masked_l1_loss`` on device tensors, ``F.l1_loss`` on CPU tensors."""
    from dgn_amd.nets import DGNNet
    s, t = _case(40, 1, seed=8)
    cpu = DGNNet.loss(None, s, t)
    assert float(cpu) == float(torch.nn.functional.l1_loss(s, t))
    t_nan = t.clone()
    t_nan[30:] = float("nan")                                           # the rows behind a captured batch
    dev = DGNNet.loss(None, s.cuda(), t_nan.cuda())
    ref = torch.nn.functional.l1_loss(s[:30].double(), t[:30].double())
    assert dev.is_cuda and abs(float(dev) - float(ref)) <= 2.0 ** -22 * abs(float(ref))
