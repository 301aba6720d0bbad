"""The encoder and loss kernels of the OGB molecule nets (csrc/dgn_mol_io.hip) and the evaluator metrics (dgn_amd.nets) on the GPU.

* Multi-column embedding sum, forward: BIT-equal to the torch composition (``h = 0; h = h + emb_c(idx[:, c])``) -- the kernel does the
  same fp32 adds in the same order.
* Backward: every table's gradient through ``parity_util.check_reduced`` at its defaults -- judged against the fp64 evaluation of the
  torch composition, the allowance being the fp32 composition's own error on that tensor, measured inside the call (no new number);
  two runs are bit-equal (no floating-point atomics).
* Masked BCE with logits: the G14 cases (the reference loop's masking lines + ``BCEWithLogitsLoss`` in fp32 and fp64).  Tolerances as in
  tests/test_node_ce_gpu.py for the same two quantities: the kernel may sit four times as far from the fp64 result as the reference's own
  fp32 result does, with a floor of 1e-6 relative (loss: |x - x64| / |x64|; gradient: max |g - g64| / max |g64|).  The fp64 gradient of
  the 300 x 128 cases is tests/mol_oracle.py's (pinned to the fixture's fp64 gradients of the smaller cases).
* Metrics: the recorded scikit-learn values to 1e-6 absolute (rank statistics: exact up to the fp64 rounding of a mean)."""
import numpy as np
import pytest
import torch

import mol_oracle as mo
import parity_util

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 64, 65, 513, 3001]
WIDTHS = [1, 19, 70, 75, 128]
TABLES = {1: [28], 3: [5, 6, 2], 9: [119, 4, 12, 12, 10, 6, 6, 2, 2]}


def _tables(dims, F, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(d, F, generator=gen) for d in dims]


def _indices(dims, N, seed):
    """skewed: three rows in four carry each column's most common value"""
    gen = torch.Generator().manual_seed(seed)
    cols = []
    for d in dims:
        common = int(torch.randint(0, d, (1,), generator=gen))
        cols.append(torch.where(torch.rand(N, generator=gen) < 0.75, torch.full((N,), common), torch.randint(0, d, (N,), generator=gen)))
    return torch.stack(cols, 1)


def _composition(weights, idx):
    h = 0
    for c, w in enumerate(weights):
        h = h + torch.nn.functional.embedding(idx[:, c], w)
    return h


def _composition_grads(weights, idx, cot, dtype):
    ws = [w.to(dtype).clone().requires_grad_(True) for w in weights]
    return torch.autograd.grad(_composition(ws, idx), ws, cot.to(dtype))


def _fused(weights, idx, cot=None):
    """ops.multi_embedding on the device; (output, gradients) as CPU tensors"""
    from dgn_amd import ops
    dev = torch.device("cuda")
    ws = [w.to(dev).requires_grad_(True) for w in weights]
    out = ops.multi_embedding(ws, idx)
    grads = torch.autograd.grad(out, ws, cot.to(dev)) if cot is not None else None
    return out.detach().cpu(), None if grads is None else [g.cpu() for g in grads]


@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("C", [1, 3, 9])
def test_embedding_forward_is_bit_equal_to_the_torch_composition(F, C):
    from dgn_amd import ops
    dev = torch.device("cuda")
    dims = TABLES[C]
    weights = _tables(dims, F, seed=10 * F + C)
    assert ops.multi_embedding_supported(weights)
    for N in ROWS:
        idx = _indices(dims, N, seed=N + C)
        ref = _composition(weights, idx)
        out, _ = _fused(weights, idx.to(dev))
        assert out.numpy().tobytes() == ref.numpy().tobytes(), (N, F, C)
        assert torch.equal(out, _composition([w.to(dev) for w in weights], idx.to(dev)).cpu())
        wide = torch.full((N, C + 3), -7, dtype=torch.int64)               # a strided view (values outside every table around it)
        wide[:, 1:C + 1] = idx
        out_v, _ = _fused(weights, wide.to(dev)[:, 1:C + 1])
        assert out_v.numpy().tobytes() == ref.numpy().tobytes(), (N, F, C, "strided")
        one = idx[:1].expand(N, C).contiguous()                            # all rows on one index
        out_1, _ = _fused(weights, one.to(dev))
        assert out_1.numpy().tobytes() == _composition(weights, one).numpy().tobytes(), (N, F, C, "one index")


@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("C", [1, 3, 9])
def test_embedding_backward_vs_fp64_composition(F, C):
    dev = torch.device("cuda")
    dims = TABLES[C]
    weights = _tables(dims, F, seed=10 * F + C)
    for N in ROWS:
        for mode in ("skewed", "one index"):
            idx = _indices(dims, N, seed=N + C)
            if mode == "one index":
                idx = idx[:1].expand(N, C).contiguous()
            cot = torch.randn(N, F, generator=torch.Generator().manual_seed(N))
            r32, r64 = _composition_grads(weights, idx, cot, torch.float32), _composition_grads(weights, idx, cot, torch.float64)
            _, grads = _fused(weights, idx.to(dev), cot)
            for c in range(C):
                parity_util.check_reduced(grads[c], r32[c], r64[c], f"multi_embedding N={N} F={F} C={C} {mode} table {c}")
            assert all(bool((g[torch.bincount(idx[:, c], minlength=dims[c]) == 0] == 0).all()) for c, g in enumerate(grads))
        _, again = _fused(weights, idx.to(dev), cot)
        for a, b in zip(grads, again):
            assert a.numpy().tobytes() == b.numpy().tobytes(), (N, F, C)


def test_embedding_backward_through_a_strided_index_view_and_two_runs_at_the_largest_size():
    dev = torch.device("cuda")
    dims, F, N = TABLES[9], 70, 52001                                      # more than 256 x 64 rows: every workgroup walks > 64 rows
    weights = _tables(dims, F, seed=1)
    idx = _indices(dims, N, seed=2)
    cot = torch.randn(N, F, generator=torch.Generator().manual_seed(3))
    r32, r64 = _composition_grads(weights, idx, cot, torch.float32), _composition_grads(weights, idx, cot, torch.float64)
    wide = torch.zeros(N, 12, dtype=torch.int64)
    wide[:, 2:11] = idx
    _, a = _fused(weights, wide.to(dev)[:, 2:11], cot)
    _, b = _fused(weights, idx.to(dev), cot)
    for c in range(9):
        parity_util.check_reduced(a[c], r32[c], r64[c], f"multi_embedding N={N} F={F} C=9 strided table {c}")
        assert a[c].numpy().tobytes() == b[c].numpy().tobytes()


def test_embedding_backward_above_64_kb_of_lds_on_a_second_device_of_the_process():
    """173 x 96 floats = 66 432 bytes of dynamic LDS, the smallest OGB-atom case above the 64 KB a kernel may use without its per-device
    attribute; 65 rows = two partial-table slots.  The same call on cuda:0 and then on cuda:1 of one process: bit-equal outputs and
    gradients (both deterministic), each against the torch composition as in the backward test above."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices in one process")
    dims, F, N = TABLES[9], 96, 65
    weights = _tables(dims, F, seed=12)
    idx = _indices(dims, N, seed=13)
    cot = torch.randn(N, F, generator=torch.Generator().manual_seed(14))
    ref = _composition(weights, idx)
    r32, r64 = _composition_grads(weights, idx, cot, torch.float32), _composition_grads(weights, idx, cot, torch.float64)
    runs = []
    for d in (0, 1):
        with torch.cuda.device(d):                                         # (torch.device("cuda") in _fused = the current device)
            out, grads = _fused(weights, idx.to(torch.device("cuda", d)), cot)
        assert out.numpy().tobytes() == ref.numpy().tobytes(), d
        for c in range(len(dims)):
            parity_util.check_reduced(grads[c], r32[c], r64[c], f"multi_embedding N={N} F={F} C=9 cuda:{d} table {c}")
        runs.append((out, grads))
    assert runs[0][0].numpy().tobytes() == runs[1][0].numpy().tobytes()
    for a, b in zip(runs[0][1], runs[1][1]):
        assert a.numpy().tobytes() == b.numpy().tobytes()


def test_embedding_out_of_range_indices_are_clamped_and_validate_raises():
    from dgn_amd import ops
    dev = torch.device("cuda")
    dims, F, N = TABLES[9], 19, 513
    weights = _tables(dims, F, seed=4)
    idx = _indices(dims, N, seed=5)
    bad = idx.clone()
    bad[::7, 0], bad[3::11, 4], bad[5::13, 8] = 119 + 1000, -1, 2 ** 40
    clamped = torch.minimum(bad.clamp_min(0), torch.tensor(dims) - 1)
    cot = torch.randn(N, F, generator=torch.Generator().manual_seed(6))
    out_b, g_b = _fused(weights, bad.to(dev), cot)
    out_c, g_c = _fused(weights, clamped.to(dev), cot)
    assert out_b.numpy().tobytes() == out_c.numpy().tobytes() == _composition(weights, clamped).numpy().tobytes()
    for a, b in zip(g_b, g_c):
        assert a.numpy().tobytes() == b.numpy().tobytes()
    untouched = (bad == idx).all(1)
    out_i, _ = _fused(weights, idx.to(dev))
    assert torch.equal(out_b[untouched], out_i[untouched])                  # the other rows are what they were
    ws = [w.to(dev) for w in weights]
    with pytest.raises(IndexError):
        ops.multi_embedding_validate(ws, bad.to(dev))
    ops.multi_embedding_validate(ws, idx.to(dev))


@pytest.mark.parametrize("dims,F", [(TABLES[9], 256), ([3] * 17, 8)])
def test_embedding_shapes_outside_the_kernels_take_the_torch_composition(dims, F):
    """173 rows x 256 floats exceed the LDS budget of the backward; 17 columns exceed the column limit: decided by shape, same numbers."""
    from dgn_amd import ops
    dev = torch.device("cuda")
    N = 513
    weights = _tables(dims, F, seed=7)
    assert not ops.multi_embedding_supported(weights)
    idx = _indices(dims, N, seed=8)
    cot = torch.randn(N, F, generator=torch.Generator().manual_seed(9))
    out, grads = _fused(weights, idx.to(dev), cot)
    assert out.numpy().tobytes() == _composition(weights, idx).numpy().tobytes()
    r32, r64 = _composition_grads(weights, idx, cot, torch.float32), _composition_grads(weights, idx, cot, torch.float64)
    for c in range(len(dims)):
        parity_util.check_reduced(grads[c], r32[c], r64[c], f"multi_embedding fallback F={F} C={len(dims)} table {c}")


# ---- masked BCE with logits ------------------------------------------------------------------------------------------------------------

def _bce(scores, labels, strided=False, cot=None):
    """ops.masked_bce_with_logits on the device -> (loss, gradient) as CPU tensors"""
    from dgn_amd import ops
    dev = torch.device("cuda")
    if strided:
        wide = torch.full((scores.shape[0], scores.shape[1] + 5), float("nan"), device=dev)
        wide[:, 2:2 + scores.shape[1]] = scores.to(dev)
        leaf = wide.requires_grad_(True)
        x = leaf[:, 2:2 + scores.shape[1]]
    else:
        leaf = x = scores.to(dev).requires_grad_(True)
    loss = ops.masked_bce_with_logits(x, labels.to(dev))
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (g,) = torch.autograd.grad(loss if cot is None else loss * cot, leaf)
    if strided:
        assert bool((g[:, :2] == 0).all()) and bool((g[:, 2 + scores.shape[1]:] == 0).all())
        g = g[:, 2:2 + scores.shape[1]]
    return loss.detach().cpu(), g.cpu()


def _g14_cases():
    return ["g1_t1", "g63_t1", "g64_t1_nan", "g65_t128_nan", "g300_t128_nan", "allnan_g65_t128", "extreme_g64_t1", "extreme_g65_t128_nan",
            "ties_g300_t128_nan", "ties_g63_t1"]


def test_the_case_list_is_the_fixtures(golden):
    assert _g14_cases() == [str(c) for c in golden("g14_mol_loss_metrics")["cases"]]


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("name", _g14_cases())
def test_masked_bce_vs_reference_fixture(golden, name, strided):
    g = golden("g14_mol_loss_metrics")
    scores, labels = torch.from_numpy(g[f"{name}/scores"]), torch.from_numpy(g[f"{name}/labels"])
    loss, grad = _bce(scores, labels, strided)
    again = _bce(scores, labels, strided)
    assert loss.numpy().tobytes() == again[0].numpy().tobytes() and grad.numpy().tobytes() == again[1].numpy().tobytes()   # run to run
    unlabelled = torch.isnan(labels)
    assert bool((grad[unlabelled] == 0).all()), name
    if name.startswith("allnan"):
        assert np.isnan(float(g[f"{name}/loss32"])) and bool(torch.isnan(loss)) and bool((grad == 0).all())
        return
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()), name          # (also at logits of +-100)
    l64, l32 = float(g[f"{name}/loss64"]), float(g[f"{name}/loss32"])
    g32 = torch.from_numpy(g[f"{name}/grad32"]).double()
    g64 = torch.from_numpy(g[f"{name}/grad64"]) if f"{name}/grad64" in g.files else mo.masked_bce(scores.double(), labels)[1]
    gmax = float(g64.abs().max())
    d_ref, d_mine = abs(l32 - l64) / abs(l64), abs(float(loss) - l64) / abs(l64)
    dg_ref, dg_mine = float((g32 - g64).abs().max()) / gmax, float((grad.double() - g64).abs().max()) / gmax
    parity_util.note(f"masked_bce {name}{' strided' if strided else ''}: loss {l64:.9g}  reference fp32 {d_ref:.2e}  kernel {d_mine:.2e} | "
                     f"gradient reference fp32 {dg_ref:.2e}  kernel {dg_mine:.2e}")
    assert d_mine <= max(4 * d_ref, 1e-6), (name, d_mine, d_ref)
    assert dg_mine <= max(4 * dg_ref, 1e-6), (name, dg_mine, dg_ref)


def test_masked_bce_incoming_gradient_shapes_and_no_grad(golden):
    from dgn_amd import ops
    dev = torch.device("cuda")
    g = golden("g14_mol_loss_metrics")
    scores, labels = torch.from_numpy(g["g65_t128_nan/scores"]), torch.from_numpy(g["g65_t128_nan/labels"])
    loss, grad = _bce(scores, labels)
    _, scaled = _bce(scores, labels, cot=-2.5)
    assert torch.equal(scaled, grad * -2.5)                                  # one rounding per element on both sides
    x = scores.to(dev).requires_grad_(True)
    half = ops.masked_bce_with_logits(x, labels.to(dev)) * 0.5 + ops.masked_bce_with_logits(x, labels.to(dev)) * 0.25
    (g2,) = torch.autograd.grad(half, x)
    assert torch.equal(g2.cpu(), grad * 0.5 + grad * 0.25)
    with torch.no_grad():
        assert float(ops.masked_bce_with_logits(x, labels.to(dev))) == float(loss)
    # 1-D (what the reference loop's boolean index leaves) = the labelled entries as one column; integer labels
    lab = ~torch.isnan(labels)
    flat = ops.masked_bce_with_logits(scores[lab].to(dev), labels[lab].to(dev))
    np.testing.assert_allclose(float(flat), float(loss), rtol=1e-6)
    s1, y1 = torch.from_numpy(g["g63_t1/scores"]), torch.from_numpy(g["g63_t1/labels"])
    as_int = ops.masked_bce_with_logits(s1.to(dev), y1.long().to(dev))
    assert float(as_int) == float(_bce(s1, y1)[0])
    with pytest.raises(ValueError):
        ops.masked_bce_with_logits(x, labels[:, :5].to(dev))


def test_masked_bce_at_the_benchmarked_batch_of_2048_graphs():
    """2048 x 128 entries = 128 workgroups: the cross-workgroup fold, against the fp64 restatement and torch's fp32 op on the selection."""
    gen = torch.Generator().manual_seed(11)
    scores = 2.0 * torch.randn(2048, 128, generator=gen)
    labels = (torch.rand(2048, 128, generator=gen) < 0.3).float()
    labels[torch.rand(2048, 128, generator=gen) < 0.6] = float("nan")
    loss, grad = _bce(scores, labels)
    l64, g64 = mo.masked_bce(scores.double(), labels)
    lab = ~torch.isnan(labels)
    x = scores.clone().requires_grad_(True)
    l32 = torch.nn.functional.binary_cross_entropy_with_logits(x[lab], labels[lab])
    (g32,) = torch.autograd.grad(l32, x)
    d_ref, d_mine = abs(float(l32) - float(l64)) / float(l64), abs(float(loss) - float(l64)) / float(l64)
    gmax = float(g64.abs().max())
    dg_ref, dg_mine = float((g32.double() - g64).abs().max()) / gmax, float((grad.double() - g64).abs().max()) / gmax
    parity_util.note(f"masked_bce 2048x128: reference fp32 {d_ref:.2e} kernel {d_mine:.2e} | gradient reference fp32 {dg_ref:.2e} kernel {dg_mine:.2e}")
    assert d_mine <= max(4 * d_ref, 1e-6) and dg_mine <= max(4 * dg_ref, 1e-6)
    assert bool((grad[~lab] == 0).all())


def _device_events(step):
    """Names of the device activities of one step, one entry per launch (the pattern of tests/test_node_ce_gpu.py)."""
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
    dims, F, N = TABLES[9], 70, 3001
    ws = [w.to(dev).requires_grad_(True) for w in _tables(dims, F, seed=1)]
    idx = _indices(dims, N, seed=2).to(dev)
    cot = torch.randn(N, F, device=dev)
    torch.autograd.grad(ops.multi_embedding(ws, idx), ws, cot)              # (first call: library load, allocator, LDS attribute)
    out = []
    names = _device_events(lambda: out.append(ops.multi_embedding(ws, idx)))
    assert len(names) == 1 and "emb_forward" in names[0], names
    names = _device_events(lambda: torch.autograd.grad(out[0], ws, cot))
    assert len(names) == 2 and all("emb_backward" in n for n in names), names
    x = torch.randn(300, 128, device=dev).requires_grad_(True)
    y = (torch.rand(300, 128, device=dev) < 0.3).float()
    y[torch.rand(300, 128, device=dev) < 0.4] = float("nan")
    ops.masked_bce_with_logits(x, y).backward()
    out = []
    names = _device_events(lambda: out.append(ops.masked_bce_with_logits(x, y)))
    assert len(names) == 2 and all("bce_" in n for n in names), names
    one = torch.ones((), device=dev)
    names = _device_events(lambda: torch.autograd.grad(out[0], x, grad_outputs=one))
    assert len(names) == 1 and "bce_scale" in names[0], names


# ---- metrics -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", _g14_cases())
def test_metrics_vs_scikit_learn(golden, name):
    from dgn_amd.nets import ap_ogb, rocauc_ogb
    dev = torch.device("cuda")
    g = golden("g14_mol_loss_metrics")
    scores, labels = torch.from_numpy(g[f"{name}/scores"]).to(dev), torch.from_numpy(g[f"{name}/labels"]).to(dev)
    for key, op in (("rocauc", rocauc_ogb), ("ap", ap_ogb)):
        ref, mine = float(g[f"{name}/{key}"]), op(scores, labels)
        assert mine.is_cuda and mine.dim() == 0 and mine.dtype == torch.float64
        if np.isnan(ref):
            assert bool(torch.isnan(mine)), (name, key)
        else:
            assert abs(float(mine) - ref) <= 1e-6, (name, key, float(mine), ref)
