"""The class cross-entropy / hit-count kernels (csrc/dgn_graph_cls.hip: dgn_class_ce_*) on the GPU: through the C ABI against fixture G17
(the reference's own fp32 results) and against the fp64 restatement (tests/superpixel_net_oracle.py), padding rows, row strides, the
autograd op, reproducibility.

Tolerance against fp64: the rule of tests/test_node_ce_gpu.py for the same quantities of its kernel (the arithmetic is the same kind: fp32
exp / log per row, fp64 sums across rows) -- the kernel is allowed four times the distance of the REFERENCE's fp32 result (the fixture)
from the fp64 restatement, with a floor of 1e-6 relative; loss: |x - x64| / |x64|, gradient: max |g - g64| / max |g64|.  The hit count must
be EXACTLY the fixture's and the restatement's."""
import numpy as np
import pytest
import torch

import superpixel_net_oracle as spo

pytestmark = pytest.mark.gpu


def _run(scores, labels, strided=False, want_grad=True, want_hits=True):
    """dgn_class_ce_forward through ctypes; returns loss, hits, grad as CPU tensors."""
    from dgn_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda")
    G, C = scores.shape
    ld, ld_g = (C + 3, C + 1) if strided else (C, C)
    buf = torch.full((max(G, 1), ld), float("nan"), device=dev)
    buf[:G, :C] = scores.to(dev)
    lab = labels.to(dev)
    loss = torch.full((1,), -7.0, device=dev)
    hits = torch.full((1,), -7, dtype=torch.int64, device=dev) if want_hits else None
    g = torch.full((max(G, 1), ld_g), 123.0, device=dev) if want_grad else None
    need = lib.dgn_class_ce_workspace_bytes(G, C)
    assert need > 0
    ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
    rc = lib.dgn_class_ce_forward(G, C, buf.data_ptr(), ld, lab.data_ptr(), loss.data_ptr(), hits.data_ptr() if want_hits else None,
                                  g.data_ptr() if want_grad else None, ld_g, ws.data_ptr(), need, _lib.stream_ptr(dev))
    _lib.check(rc, "dgn_class_ce_forward")
    torch.cuda.synchronize()
    if want_grad and strided:
        assert bool((g[:, C:] == 123.0).all()), "wrote outside the gradient rows' C columns"
    return loss[0].cpu(), int(hits[0]) if want_hits else None, g[:G, :C].cpu() if want_grad else None


def _check(tag, scores, labels, loss, hits, grad, ref_loss, ref_grad):
    """``ref_loss`` / ``ref_grad``: the reference op's fp32 result on the valid rows (gradient rows of the padding: zero)."""
    loss64, grad64 = spo.loss_and_grad(scores.double(), labels)
    l64, gmax = float(loss64), float(grad64.abs().max())
    d_ref, d_mine = abs(float(ref_loss) - l64) / abs(l64), abs(float(loss) - l64) / abs(l64)
    dg_ref = float((ref_grad.double() - grad64).abs().max()) / gmax
    dg_mine = float((grad.double() - grad64).abs().max()) / gmax
    print(f"class_ce {tag}: loss {l64:.9g}  reference fp32 {d_ref:.2e}  kernel {d_mine:.2e} | gradient reference fp32 {dg_ref:.2e}  kernel {dg_mine:.2e}")
    assert d_mine <= max(4 * d_ref, 1e-6), (tag, d_mine, d_ref)
    assert dg_mine <= max(4 * dg_ref, 1e-6), (tag, dg_mine, dg_ref)
    assert bool((grad[labels < 0] == 0).all()), tag
    assert hits == spo.hits(scores.double(), labels) == spo.hits(scores, labels), tag


def _reference_fp32(scores, labels):
    """The op the reference calls (dgn_net.py:76-77) on the CPU in fp32; padding rows dropped first."""
    valid = labels >= 0
    x = scores[valid].clone().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(x, labels[valid])
    (gx,) = torch.autograd.grad(loss, x)
    grad = torch.zeros_like(scores)
    grad[valid] = gx
    return loss.detach(), grad


def _fixture_case(g, name):
    return torch.from_numpy(g[f"{name}/scores"]), torch.from_numpy(g[f"{name}/labels"])


@pytest.mark.parametrize("strided", [False, True])
def test_kernel_vs_reference_fixture(golden, strided):
    g = golden("g17_class_ce")
    for name in [str(c) for c in g["cases"]]:
        scores, labels = _fixture_case(g, name)
        loss, hits, grad = _run(scores, labels, strided=strided)
        _check(f"g17/{name}", scores, labels, loss, hits, grad, torch.from_numpy(g[f"{name}/loss"]), torch.from_numpy(g[f"{name}/grad"]))
        assert hits == int(g[f"{name}/hits"]), name
    assert int(g["ties/hits"]) == 4              # (label first among the tied: hit; second: miss -- the kernel agreed above)


@pytest.mark.parametrize("name", ["g65_c10", "g257_c10", "g1000_c3", "g130_c64", "ties"])
def test_padding_rows_interleaved_and_at_the_tail(golden, name):
    g = golden("g17_class_ce")
    scores, labels = _fixture_case(g, name)
    G, C = scores.shape
    gen = torch.Generator().manual_seed(G)
    pad_mid, pad_tail = max(G // 3, 1), 37
    keep = torch.sort(torch.randperm(G + pad_mid, generator=gen)[:G]).values
    scores_p = 5.0 * torch.randn(G + pad_mid + pad_tail, C, generator=gen)
    labels_p = torch.full((G + pad_mid + pad_tail,), -1, dtype=torch.int64)
    scores_p[keep], labels_p[keep] = scores, labels
    labels_p[-1] = -5                                            # any negative label is padding
    loss, hits, grad = _run(scores_p, labels_p)
    ref_loss, ref_grad = _reference_fp32(scores_p, labels_p)
    _check(f"padded {name}", scores_p, labels_p, loss, hits, grad, ref_loss, ref_grad)
    assert hits == int(g[f"{name}/hits"])
    _, _, grad0 = _run(scores, labels)
    assert torch.equal(grad[keep], grad0)                        # a row's gradient depends on the row and on V alone


@pytest.mark.parametrize("G", [300, 0])
def test_no_valid_row_and_no_row(G):
    scores, labels = torch.randn(G, 10), torch.full((G,), -1, dtype=torch.int64)
    loss, hits, grad = _run(scores, labels)
    assert bool(torch.isnan(loss)) and hits == 0 and bool((grad == 0).all()) and grad.shape[0] == G
    loss, hits, _ = _run(scores, labels, want_grad=False)
    assert bool(torch.isnan(loss)) and hits == 0


def test_label_beyond_the_class_range_and_nan_score():
    gen = torch.Generator().manual_seed(4)
    scores, labels = 3.0 * torch.randn(70, 10, generator=gen), torch.randint(0, 10, (70,), generator=gen)
    ok_loss, ok_hits, ok_grad = _run(scores, labels)
    assert bool(torch.isfinite(ok_loss))
    bad = labels.clone()
    bad[5], bad[40] = 10, 10 ** 12                               # (10: inside the register row of 16, outside the 10 classes)
    was_hit = int(scores[5].argmax() == labels[5]) + int(scores[40].argmax() == labels[40])
    loss, hits, grad = _run(scores, bad, strided=True)
    assert bool(torch.isnan(loss)) and hits == ok_hits - was_hit
    rows = torch.ones(70, dtype=torch.bool)
    rows[[5, 40]] = False
    assert bool(torch.isnan(grad[~rows]).all()) and torch.equal(grad[rows], ok_grad[rows])      # V is the same: the other rows are untouched
    nan_scores = scores.clone()
    nan_scores[12, 3] = float("nan")
    loss, hits, grad = _run(nan_scores, labels)
    assert bool(torch.isnan(loss)) and bool(torch.isnan(grad[12]).all()) and bool(torch.isfinite(grad[rows & (torch.arange(70) != 12)]).all())
    assert hits == spo.hits(nan_scores, labels)                  # (a NaN is the largest score for torch.argmax and numpy.argmax alike)


@pytest.mark.parametrize("name", ["g257_c10", "g1000_c3", "g130_c64"])
def test_two_calls_give_identical_bits(golden, name):
    g = golden("g17_class_ce")
    scores, labels = _fixture_case(g, name)
    labels = labels.clone()
    labels[::9] = -1
    a, b = _run(scores, labels), _run(scores, labels)
    assert a[0].numpy().tobytes() == b[0].numpy().tobytes() and a[1] == b[1] and a[2].numpy().tobytes() == b[2].numpy().tobytes()
    loss_only = _run(scores, labels, want_grad=False, want_hits=False)[0]             # the optional outputs do not change the loss
    assert loss_only.numpy().tobytes() == a[0].numpy().tobytes()


def test_autograd_op_strides_incoming_gradient_and_no_grad(golden):
    from dgn_amd import ops
    from dgn_amd._lib import DgnError
    dev = torch.device("cuda")
    g = golden("g17_class_ce")
    scores, labels = _fixture_case(g, "g257_c10")
    labels = labels.clone()
    labels[250:] = -1
    ref_loss, ref_hits, ref_grad = _run(scores, labels)
    x, y = scores.to(dev).requires_grad_(True), labels.to(dev)
    loss, hits = ops.class_cross_entropy(x, y, hits=True)
    assert loss.dim() == 0 and hits.dim() == 0 and hits.dtype == torch.int64 and hits.is_cuda and not hits.requires_grad
    assert loss.item() == float(ref_loss) and int(hits) == ref_hits
    (g1,) = torch.autograd.grad(loss, x, retain_graph=True)
    assert g1.cpu().numpy().tobytes() == ref_grad.numpy().tobytes()              # unit incoming gradient: the saved rows themselves
    (3 * loss).backward()
    assert torch.equal(x.grad.cpu(), ref_grad * 3)                               # one rounding per element on both sides
    # a column slice of a wider tensor (ld > C), without the hit count
    wide = torch.zeros(257, 15, device=dev)
    wide[:, 2:12] = scores.to(dev)
    xv = wide.requires_grad_(True)
    loss_v = ops.class_cross_entropy(xv[:, 2:12], y)
    assert torch.is_tensor(loss_v) and loss_v.item() == loss.item()
    loss_v.backward()
    assert torch.equal(xv.grad[:, 2:12].cpu(), ref_grad) and bool((xv.grad[:, :2] == 0).all()) and bool((xv.grad[:, 12:] == 0).all())
    # under no_grad no gradient buffer is allocated
    torch.cuda.synchronize()
    with torch.no_grad():
        ops.class_cross_entropy(x, y, hits=True)                                 # (allocator warm)
        torch.cuda.synchronize()
        big_x, big_y = torch.randn(200000, 10, device=dev).requires_grad_(True), torch.zeros(200000, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        out = ops.class_cross_entropy(big_x, big_y, hits=True)
        torch.cuda.synchronize()
        assert torch.cuda.max_memory_allocated() - held < big_x.numel() * 4 // 2, "a [G, C] buffer was allocated under no_grad"
        assert not out[0].requires_grad
        assert float(ops.class_cross_entropy(x, y)) == float(ref_loss)
    with pytest.raises(ValueError):
        ops.class_cross_entropy(x, y[:-1])
    with pytest.raises(ValueError):
        ops.class_cross_entropy(torch.zeros(4, 65, device=dev), torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(DgnError):
        ops.class_cross_entropy(scores, labels)


def _device_events(step):
    """Names of the device activities of one step, one entry per launch (the pattern of tests/test_node_ce_gpu.py)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    evs = prof.profiler.kineto_results.events()
    return [e.name() for e in evs if str(e.device_type()).endswith("CUDA")]


def test_forward_is_at_most_two_launches_and_backward_one():
    from dgn_amd import ops
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(1)
    x = (3.0 * torch.randn(128, 10, generator=gen)).to(dev).requires_grad_(True)
    y = torch.randint(0, 10, (128,), generator=gen).to(dev)
    ops.class_cross_entropy(x, y, hits=True)[0].backward()                        # (first call: library load, allocator)
    out = []
    names = _device_events(lambda: out.append(ops.class_cross_entropy(x, y, hits=True)))
    assert names, "the profiler saw no device kernel"
    assert len(names) <= 2 and all("gcls" in n for n in names), names
    loss = out[0][0]
    one = torch.ones((), device=dev)
    names = _device_events(lambda: torch.autograd.grad(loss, x, grad_outputs=one))
    assert len(names) == 1, names
