"""The balanced cross-entropy / SBM confusion-matrix kernels (csrc/dgn_node_ce.hip) on the GPU: through the C ABI against fixture G12
(the reference's own fp32 results) and against the fp64 restatement (tests/node_ce_oracle.py), bitwise reproducibility, the autograd
op, stream capture and the launch count.

Tolerance against fp64 (no precedent in this project, so it is derived per case, not picked): the distance of the REFERENCE's fp32
result from the fp64 restatement -- for the G12 cases the fixture is that fp32 result; for the larger sizes it is
``torch.nn.functional.cross_entropy(weight=...)`` on the CPU with the restated weights, the very op the reference calls, tied to the
reference by the G12 cases.  The kernel is allowed four times that distance (it sums in another order; four leaves room for one more
level of a reduction tree without admitting a wrong term), with a floor of 1e-6 relative where the reference happens to round exactly.
Gradient: the same rule on the largest element error relative to max |g|.  The confusion matrix must be EXACTLY the fp64
restatement's; the inputs are nudged so that every row's two best margins are >= 1e-4 apart in the fp32 restatement (a condition on the
inputs, asserted in the test).  Weights: (V - count) / V is one correctly rounded fp32 division on both sides; 1e-6 relative allows
for a division that is 1-2 ulp off.

Measured distances from the fp64 restatement, relative (loss: |x - x64| / |x64|; gradient: max |g - g64| / max |g64|), dense case of
each size -- reference fp32 / kernel:

    case                 loss: reference   kernel     gradient: reference   kernel
    g12 n2_c2                  1.66e-08      1.66e-08             7.68e-08      7.68e-08
    g12 n63_c2                 6.04e-08      3.28e-09             1.37e-07      1.16e-07
    g12 n64_c2                 8.27e-08      1.07e-08             1.03e-07      1.63e-07
    g12 n65_c6                 3.82e-08      3.82e-08             8.48e-08      1.00e-07
    g12 n1000_c6               1.10e-08      1.10e-08             3.06e-07      2.49e-07
    g12 n3001_c2               9.82e-09      9.82e-09             1.85e-07      1.78e-07
    g12 missing_n500_c6        1.26e-08      1.26e-08             1.95e-07      1.95e-07
    N=2 C=2                    1.44e-08      1.44e-08             3.83e-08      3.83e-08
    N=64 C=2                   1.01e-07      8.63e-09             9.64e-08      1.06e-07
    N=65 C=6                   4.50e-08      4.50e-08             1.73e-07      1.65e-07
    N=15257 C=2                1.57e-08      1.57e-08             2.08e-07      2.01e-07
    N=15257 C=6                5.89e-09      5.89e-09             2.79e-07      2.86e-07
    N=300001 C=10              9.49e-08      1.29e-09             4.34e-07      4.24e-07
    N=1000 C=32                4.59e-08      2.19e-08             2.52e-07      3.65e-07

Every one of them is below the 1e-6 floor, so the floor is what binds: the loss partials are summed in fp64 and rounded once, and an
element of the gradient is a handful of fp32 operations on either side.
"""
import numpy as np
import pytest
import torch

import node_ce_oracle as nco

pytestmark = pytest.mark.gpu

SIZES = [(2, 2), (64, 2), (65, 6), (15257, 2), (15257, 6), (300001, 10), (1000, 32)]
MODES = ["dense", "strided", "padded", "missing"]


def _inputs(N, n_classes, mode, seed=0):
    """Seeded scores (std 3) and labels with every class present (``missing``: the last class absent, C > 2 only), ``padded``: ~10 % of
    the rows carry the label -1; nudged to prediction gaps of >= 1e-4 (asserted on the fp32 restatement)."""
    gen = torch.Generator().manual_seed(1000 * n_classes + N % 997 + seed)
    hi = n_classes - 1 if mode == "missing" else n_classes
    labels = torch.randint(0, hi, (N,), generator=gen)
    k = min(N, hi)
    labels[torch.randperm(N, generator=gen)[:k]] = torch.arange(k)
    if mode == "padded" and N > 16:
        labels[torch.rand(N, generator=gen) < 0.1] = -1
    scores = nco.nudge_scores(3.0 * torch.randn(N, n_classes, generator=gen), labels)
    assert nco.prediction_gap(scores, labels) >= 1e-4
    return scores, labels


def _run(scores, labels, n_classes, strided=False, want_grad=True, want_cm=True):
    """dgn_node_ce_forward through ctypes; returns loss, weight, grad, confusion as CPU tensors."""
    from dgn_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda")
    N = scores.shape[0]
    ld, ld_g = (n_classes + 3, n_classes + 1) if strided else (n_classes, n_classes)
    buf = torch.full((max(N, 1), ld), float("nan"), device=dev)
    buf[:N, :n_classes] = scores.to(dev)
    lab = labels.to(dev)
    out = torch.full((1 + n_classes,), -7.0, device=dev)
    g = torch.full((max(N, 1), ld_g), 123.0, device=dev) if want_grad else None
    cm = torch.full((n_classes, n_classes), -1, dtype=torch.int64, device=dev) if want_cm else None
    need = lib.dgn_node_ce_workspace_bytes(N, n_classes)
    ws = torch.empty(max(need // 8, 1), dtype=torch.float64, device=dev)
    rc = lib.dgn_node_ce_forward(N, n_classes, buf.data_ptr(), ld, lab.data_ptr(), out.data_ptr(), out.data_ptr() + 4,
                                 g.data_ptr() if want_grad else None, ld_g, cm.data_ptr() if want_cm else None, ws.data_ptr(), need,
                                 _lib.stream_ptr(dev))
    _lib.check(rc, "dgn_node_ce_forward")
    torch.cuda.synchronize()
    if want_grad and strided:
        assert bool((g[:, n_classes:] == 123.0).all()), "wrote outside the gradient rows' n_classes columns"
    return (out[0].cpu(), out[1:].cpu(), g[:N, :n_classes].cpu() if want_grad else None, cm.cpu() if want_cm else None)


def _reference_fp32(scores, labels, n_classes):
    """The op the reference calls (dgn_net.py:78-79) on the CPU in fp32 with the restated weights; padding rows dropped first."""
    valid = labels >= 0
    x = scores[valid].clone().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(x, labels[valid], weight=nco.class_weights(labels, n_classes, torch.float32))
    (gx,) = torch.autograd.grad(loss, x)
    grad = torch.zeros_like(scores)
    grad[valid] = gx
    return loss.detach(), grad


def _check_against_fp64(tag, scores, labels, n_classes, loss, weight, grad, cm, ref_loss, ref_grad):
    loss64, grad64 = nco.loss_and_grad(scores.double(), labels, n_classes)
    l64, gmax = float(loss64), float(grad64.abs().max())
    d_ref, d_mine = abs(float(ref_loss) - l64) / abs(l64), abs(float(loss) - l64) / abs(l64)
    dg_ref = float((ref_grad.double() - grad64).abs().max()) / gmax
    dg_mine = float((grad.double() - grad64).abs().max()) / gmax
    print(f"node_ce {tag}: loss {l64:.9g}  reference fp32 {d_ref:.2e}  kernel {d_mine:.2e} | gradient reference fp32 {dg_ref:.2e}  kernel {dg_mine:.2e}")
    assert d_mine <= max(4 * d_ref, 1e-6), (tag, d_mine, d_ref)
    assert dg_mine <= max(4 * dg_ref, 1e-6), (tag, dg_mine, dg_ref)
    assert bool((grad[labels < 0] == 0).all()), tag
    np.testing.assert_allclose(weight.numpy(), nco.class_weights(labels, n_classes, torch.float32).numpy(), rtol=1e-6, atol=0, err_msg=tag)
    assert torch.equal(cm, nco.confusion_matrix(scores.double(), labels, n_classes)), tag
    assert torch.equal(cm, nco.confusion_matrix(scores, labels, n_classes)), tag


def test_kernel_vs_reference_fixture(golden):
    g = golden("g12_node_ce")
    for name in [str(c) for c in g["cases"]]:
        scores, labels, n_classes = torch.from_numpy(g[f"{name}/scores"]), torch.from_numpy(g[f"{name}/labels"]), int(g[f"{name}/C"])
        loss, weight, grad, cm = _run(scores, labels, n_classes)
        if name.startswith("single"):
            assert np.isnan(float(g[f"{name}/loss"])) and bool(torch.isnan(loss)) and bool(torch.isnan(grad).all()) and bool((weight == 0).all())
            continue
        _check_against_fp64("g12/" + name, scores, labels, n_classes, loss, weight, grad, cm, torch.from_numpy(g[f"{name}/loss"]),
                            torch.from_numpy(g[f"{name}/grad"]))
        from dgn_amd.nets import accuracy_sbm
        acc = accuracy_sbm(cm.cuda())
        assert acc.is_cuda and acc.dim() == 0
        assert abs(float(acc) - float(g[f"{name}/acc"])) <= 1e-4, (name, float(acc), float(g[f"{name}/acc"]))


# (two classes with one of them missing is the single-class case: test_single_class_is_nan_and_padding_rows_stay_zero)
@pytest.mark.parametrize("N,n_classes,mode", [(N, C, m) for (N, C) in SIZES for m in MODES if not (m == "missing" and C == 2)])
def test_kernel_vs_fp64_restatement(N, n_classes, mode):
    scores, labels = _inputs(N, n_classes, mode)
    loss, weight, grad, cm = _run(scores, labels, n_classes, strided=(mode == "strided"))
    ref_loss, ref_grad = _reference_fp32(scores, labels, n_classes)
    _check_against_fp64(f"N={N} C={n_classes} {mode}", scores, labels, n_classes, loss, weight, grad, cm, ref_loss, ref_grad)
    if mode == "missing":
        assert float(weight[-1]) == 0.0 and int(cm[-1].sum()) == 0


@pytest.mark.parametrize("N,n_classes", [(2, 2), (1000, 6), (15257, 2)])
def test_single_class_is_nan_and_padding_rows_stay_zero(N, n_classes):
    gen = torch.Generator().manual_seed(3)
    scores = 3.0 * torch.randn(N, n_classes, generator=gen)
    labels = torch.full((N,), n_classes - 1, dtype=torch.int64)
    if N > 2:
        labels[::5] = -1
    loss, weight, grad, cm = _run(scores, labels, n_classes)
    assert bool(torch.isnan(loss)) and bool((weight == 0).all())
    assert bool(torch.isnan(grad[labels >= 0]).all()) and bool((grad[labels < 0] == 0).all())
    assert int(cm.sum()) == int((labels >= 0).sum()) and int(cm[n_classes - 1].sum()) == int(cm.sum())


def test_no_valid_row_and_no_row():
    scores, labels = torch.randn(300, 4), torch.full((300,), -1, dtype=torch.int64)
    loss, weight, grad, cm = _run(scores, labels, 4)
    assert float(loss) == 0.0 and bool((grad == 0).all()) and bool((cm == 0).all()) and bool((weight == 0).all())
    loss, weight, grad, cm = _run(torch.zeros(0, 4), torch.zeros(0, dtype=torch.int64), 4)
    assert float(loss) == 0.0 and bool((cm == 0).all()) and bool((weight == 0).all())


def test_labels_beyond_the_class_range_are_ignored_like_padding():
    scores, labels = _inputs(500, 6, "dense")
    bad = labels.clone()
    bad[::7] = 6 + (torch.arange(bad[::7].numel()) % 3) * 1000
    pad = labels.clone()
    pad[::7] = -1
    a, b = _run(scores, bad, 6), _run(scores, pad, 6)
    for x, y in zip(a, b):
        assert x.numpy().tobytes() == y.numpy().tobytes()


@pytest.mark.parametrize("N,n_classes", [(15257, 2), (300001, 10), (1000, 32)])
def test_two_calls_give_identical_bits(N, n_classes):
    scores, labels = _inputs(N, n_classes, "padded")
    a, b = _run(scores, labels, n_classes), _run(scores, labels, n_classes)
    for x, y in zip(a, b):
        assert x.numpy().tobytes() == y.numpy().tobytes()
    assert bool((a[2][labels < 0] == 0).all())
    loss_only = _run(scores, labels, n_classes, want_grad=False, want_cm=False)[0]           # the optional outputs do not change the loss
    assert loss_only.numpy().tobytes() == a[0].numpy().tobytes()


def test_autograd_op_and_incoming_gradient():
    from dgn_amd import ops
    dev = torch.device("cuda")
    scores, labels = _inputs(15257, 6, "padded")
    _, _, grad, cm_ref = _run(scores, labels, 6)
    x = scores.to(dev).requires_grad_(True)
    loss, cm = ops.balanced_cross_entropy(x, labels.to(dev), 6, confusion=True)
    assert loss.dim() == 0 and cm.dtype == torch.int64 and not cm.requires_grad and torch.equal(cm.cpu(), cm_ref)
    (g1,) = torch.autograd.grad(loss, x, retain_graph=True)
    assert g1.cpu().numpy().tobytes() == grad.numpy().tobytes()                  # unit incoming gradient: the saved rows themselves
    (g2,) = torch.autograd.grad(loss * -2.5, x)
    assert torch.equal(g2.cpu(), grad * -2.5)                                    # one rounding per element on both sides
    # through a non-contiguous view, and without the confusion matrix
    wide = torch.zeros(15257, 9, device=dev)
    wide[:, 2:8] = scores.to(dev)
    xv = wide.requires_grad_(True)
    loss_v = ops.balanced_cross_entropy(xv[:, 2:8], labels.to(dev), 6)
    assert loss_v.item() == loss.item()
    loss_v.backward()
    assert torch.equal(xv.grad[:, 2:8].cpu(), grad) and bool((xv.grad[:, :2] == 0).all())
    with torch.no_grad():
        assert float(ops.balanced_cross_entropy(x, labels.to(dev), 6)) == float(loss)
    with pytest.raises(ValueError):
        ops.balanced_cross_entropy(x, labels.to(dev), 5)


def _device_events(step):
    """Names of the device activities of one step, one entry per launch (the ``_device_kernels`` pattern of tests/test_bench_sizes_gpu.py)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    evs = prof.profiler.kineto_results.events()
    return [e.name() for e in evs if str(e.device_type()).endswith("CUDA")]


def test_forward_is_at_most_three_launches_and_backward_one():
    from dgn_amd import ops
    dev = torch.device("cuda")
    scores, labels = _inputs(15257, 2, "dense")
    x, y = scores.to(dev).requires_grad_(True), labels.to(dev)
    ops.balanced_cross_entropy(x, y, 2, confusion=True)[0].backward()             # (first call: library load, allocator)
    out = []
    names = _device_events(lambda: out.append(ops.balanced_cross_entropy(x, y, 2, confusion=True)))
    assert names, "the profiler saw no device kernel"
    assert len(names) <= 3 and all("node_ce" in n for n in names), names
    loss = out[0][0]
    one = torch.ones((), device=dev)
    names = _device_events(lambda: torch.autograd.grad(loss, x, grad_outputs=one))
    assert names, "the profiler saw no device kernel"
    assert len(names) == 1 and "node_ce" in names[0], names
    with torch.no_grad():
        names = _device_events(lambda: ops.balanced_cross_entropy(x, y, 2))
    assert names and len(names) <= 3 and all("node_ce" in n for n in names), names


def test_op_inside_a_captured_graph_follows_its_buffers():
    """Forward + backward captured once; replayed after scores and labels were overwritten it equals the eager call on the new contents
    (nothing in the op reads the device back, or the capture would fail)."""
    from dgn_amd import ops
    from dgn_amd.hipgraph import capture
    dev = torch.device("cuda")
    N, n_classes = 4000, 6
    s0, l0 = _inputs(N, n_classes, "padded")
    x = s0.to(dev).requires_grad_(True)
    y = l0.to(dev)
    st_loss, st_cm, st_g = torch.zeros((), device=dev), torch.zeros(n_classes, n_classes, dtype=torch.int64, device=dev), torch.zeros(N, n_classes, device=dev)

    def step():
        loss, cm = ops.balanced_cross_entropy(x, y, n_classes, confusion=True)
        (g,) = torch.autograd.grad(loss, x)
        st_loss.copy_(loss.detach())
        st_cm.copy_(cm)
        st_g.copy_(g)

    graph = capture(step, warmup=2)
    s1, l1 = _inputs(N, n_classes, "missing", seed=9)
    with torch.no_grad():
        x.copy_(s1.to(dev))
        y.copy_(l1.to(dev))
    graph.replay()
    torch.cuda.synchronize()
    loss, _, grad, cm = _run(s1, l1, n_classes)
    assert float(st_loss) == float(loss) and torch.equal(st_cm.cpu(), cm) and torch.equal(st_g.cpu(), grad)
    assert not torch.equal(cm, _run(s0, l0, n_classes)[3])
