"""The one gradient policy of the four losses (``ops._wants_grad``): under ``torch.no_grad()`` a score tensor that REQUIRES a gradient gets
no gradient buffer -- ``ctx.needs_input_grad`` would say it wants one, since it reports ``requires_grad`` whatever the grad mode -- and the
loss is the grad-mode loss bit for bit (the same launches on the same inputs; only the gradient store differs).

The memory criterion is that of tests/test_masked_l1_gpu.py::test_no_grad_allocates_no_gradient_buffer: the peak over the call stays
below half a gradient buffer (0.75 MiB here; the call's own allocations are the loss, the 4 - 30 KiB workspace and the small outputs)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

G = 1 << 16


def _scores(width):
    gen = torch.Generator().manual_seed(width)
    return torch.randn(G, width, generator=gen), gen


def _balanced_ce():
    from dgn_amd import ops
    s, gen = _scores(4)
    y = torch.randint(-1, 4, (G,), generator=gen).cuda()               # (-1: padding rows)
    return s, lambda x: ops.balanced_cross_entropy(x, y, 4)


def _class_ce():
    from dgn_amd import ops
    s, gen = _scores(4)
    y = torch.randint(-1, 4, (G,), generator=gen).cuda()
    return s, lambda x: ops.class_cross_entropy(x, y)


def _masked_bce():
    from dgn_amd import ops
    s, gen = _scores(3)
    y = (torch.rand(G, 3, generator=gen) < 0.5).float()
    y[torch.rand(G, 3, generator=gen) < 0.4] = float("nan")            # not measured
    y = y.cuda()
    return s, lambda x: ops.masked_bce_with_logits(x, y)


def _masked_l1():
    from dgn_amd import ops
    s, gen = _scores(3)
    t = torch.randn(G, 3, generator=gen)
    t[torch.rand(G, 3, generator=gen) < 0.4] = float("nan")
    t = t.cuda()
    return s, lambda x: ops.masked_l1_loss(x, t)


@pytest.mark.parametrize("case", [_balanced_ce, _class_ce, _masked_bce, _masked_l1], ids=lambda f: f.__name__.strip("_"))
def test_no_grad_writes_no_gradient_buffer_for_a_leaf_that_requires_grad(case):
    s, loss_of = case()
    sd = s.cuda().requires_grad_(True)
    with_grad = loss_of(sd)                                             # (first call: library load, workspace blocks in the allocator)
    assert with_grad.requires_grad
    with torch.no_grad():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss = loss_of(sd)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    assert not loss.requires_grad
    assert peak < s.numel() * 4 // 2, peak
    assert torch.equal(loss.detach().view(torch.int32), with_grad.detach().view(torch.int32)), (float(loss), float(with_grad))
