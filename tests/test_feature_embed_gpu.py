"""The feature-embedding kernels (csrc/dgn_graph_cls.hip: dgn_feat_embed_*) on the GPU through ``ops.feature_embedding`` against fp64.

Forward: an output is ``b + sum_k W[f, k] x[r, k]``, at most 8 fused multiply-adds from the bias on; each of the K roundings is at most
2^-24 of a partial sum that the sum of the terms' magnitudes bounds, so K 2^-24 (|b| + sum_k |x_k W_k|) bounds the error of ANY order of
the K terms; the test asserts the bound with 16 in place of K <= 8.  Weight and bias gradient: the tolerance tests/test_linear_hip.py
applies to the streaming weight gradient at these row counts (``_close``: largest error <= 1e-5 of the largest reference magnitude)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EMB_ROWS = 128            # kEmbRows: rows per forward workgroup
SLOT_ROWS = 64            # kEmbMinRows (= kEmbTile): rows of one partial slot while there are fewer than SLOT_CAP slots
SLOT_CAP = 256            # kEmbMaxGroups: from SLOT_ROWS * SLOT_CAP rows on a slot's range grows past one staged tile
KS = [1, 2, 3, 5, 8]
FS = [1, 4, 13, 65, 75, 160]
ROWS = [0, 1, 3, 63, 64, 65, 1000, EMB_ROWS + 1, SLOT_ROWS + 1, SLOT_ROWS * SLOT_CAP + 1]


def _close(a, r, tol=1e-5):
    scale = float(r.abs().max()) + 1e-30
    assert float((a.double() - r).abs().max()) <= tol * scale, float((a.double() - r).abs().max()) / scale


def _case(R, K, F, seed=0, ld=None):
    gen = torch.Generator().manual_seed(seed + 1000 * K + F)
    xs = torch.rand(R, ld or K, generator=gen) * 2 - 0.5
    w = torch.randn(F, K, generator=gen) / K ** 0.5
    b = torch.randn(F, generator=gen)
    gy = torch.randn(R, F, generator=gen)
    return xs, w, b, gy


def _run(x, w, b, gy):
    """forward + backward through the op on the device; y, dW, db as CPU tensors."""
    from dgn_amd import ops
    dev = torch.device("cuda")
    xd = x.to(dev)
    wd = w.to(dev).requires_grad_(True)
    bd = b.to(dev).requires_grad_(True) if b is not None else None
    assert ops.feature_embedding_supported(xd, wd)
    y = ops.feature_embedding(xd, wd, bd)
    assert tuple(y.shape) == (x.shape[0], w.shape[0]) and y.is_contiguous()
    y.backward(gy.to(dev))
    torch.cuda.synchronize()
    return y.detach().cpu(), wd.grad.cpu(), bd.grad.cpu() if b is not None else None


def _check(x, w, b, gy, y, dw, db):
    x64, w64 = x.double(), w.double()
    b64 = b.double() if b is not None else torch.zeros(w.shape[0], dtype=torch.float64)
    y64 = x64 @ w64.t() + b64
    bound = 16 * 2.0 ** -24 * (x64.abs() @ w64.abs().t() + b64.abs())
    assert bool(((y.double() - y64).abs() <= bound).all()), float(((y.double() - y64).abs() - bound).max())
    if x.shape[0] == 0:
        assert bool((dw == 0).all()) and (db is None or bool((db == 0).all()))
        return
    _close(dw, gy.double().t() @ x64)
    if db is not None:
        _close(db, gy.double().sum(0))


@pytest.mark.parametrize("K,F", [(K, F) for K in KS for F in FS])
def test_forward_and_gradients_vs_fp64(K, F):
    for R in ROWS:
        x, w, b, gy = _case(R, K, F)
        _check(x, w, b, gy, *_run(x, w, b, gy))


@pytest.mark.parametrize("K,F,R", [(5, 65, 15000), (3, 75, 1000), (1, 6, SLOT_ROWS * SLOT_CAP + 1), (8, 160, 1000)])
def test_gradients_are_bit_equal_across_two_runs(K, F, R):
    x, w, b, gy = _case(R, K, F, seed=3)
    a, c = _run(x, w, b, gy), _run(x, w, b, gy)
    for p, q in zip(a, c):
        assert p.numpy().tobytes() == q.numpy().tobytes()


@pytest.mark.parametrize("K,F,R", [(3, 65, 130), (5, 75, 1000), (1, 13, 65), (8, 4, 129)])
def test_strided_input_and_no_bias(K, F, R):
    """x as a column slice of a wider tensor (ld > K): only its own K columns are read (the others hold NaN); without bias the outputs
    start at zero and no bias gradient exists."""
    x_wide, w, b, gy = _case(R, K, F, seed=5, ld=K + 3)
    x_wide[:, K:] = float("nan")
    xv = x_wide.cuda()[:, :K]
    assert xv.stride(0) == K + 3 and not xv.is_contiguous()
    from dgn_amd import ops
    wd, bd = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = ops.feature_embedding(xv, wd, bd)
    y.backward(gy.cuda())
    _check(x_wide[:, :K], w, b, gy, y.detach().cpu(), wd.grad.cpu(), bd.grad.cpu())
    y0, dw0, db0 = _run(x_wide[:, :K].contiguous(), w, b, gy)
    assert torch.equal(y.detach().cpu(), y0) and torch.equal(wd.grad.cpu(), dw0) and torch.equal(bd.grad.cpu(), db0)
    y1, dw1, db1 = _run(x_wide[:, :K].contiguous(), w, None, gy)
    assert db1 is None and torch.equal(dw1, dw0)
    _check(x_wide[:, :K], w, None, gy, y1, dw1, None)


def test_output_rows_at_an_unaligned_base_and_a_gradient_slice():
    """The C entry point on an output whose rows are dense but start 4 bytes past a 16-byte boundary, and on a strided output (ld_y > F):
    the element-wise route writes the same numbers as the flat chunks and nothing outside the rows; g as a column slice (ld_g > F)."""
    from dgn_amd import _lib
    lib, dev = _lib.load(), torch.device("cuda")
    R, K, F = 131, 5, 65
    x, w, b, gy = _case(R, K, F, seed=7)
    y_ref, dw_ref, db_ref = _run(x, w, b, gy)
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    flat = torch.full((R * F + 8,), 55.0, device=dev)
    rc = lib.dgn_feat_embed_forward(R, K, F, xd.data_ptr(), K, wd.data_ptr(), bd.data_ptr(), flat.data_ptr() + 4, F, _lib.stream_ptr(dev))
    _lib.check(rc, "dgn_feat_embed_forward")
    wide = torch.full((R, F + 3), 55.0, device=dev)
    rc = lib.dgn_feat_embed_forward(R, K, F, xd.data_ptr(), K, wd.data_ptr(), bd.data_ptr(), wide.data_ptr(), F + 3, _lib.stream_ptr(dev))
    _lib.check(rc, "dgn_feat_embed_forward")
    torch.cuda.synchronize()
    assert torch.equal(flat[1:1 + R * F].reshape(R, F).cpu(), y_ref) and float(flat[0]) == 55.0 and bool((flat[1 + R * F:] == 55.0).all())
    assert torch.equal(wide[:, :F].cpu(), y_ref) and bool((wide[:, F:] == 55.0).all())
    g_wide = torch.full((R, F + 2), float("nan"), device=dev)
    g_wide[:, :F] = gy.to(dev)
    dw, db = torch.empty(F, K, device=dev), torch.empty(F, device=dev)
    need = lib.dgn_feat_embed_backward_workspace_bytes(R, K, F)
    ws = torch.empty(need // 4, device=dev)
    rc = lib.dgn_feat_embed_backward(R, K, F, xd.data_ptr(), K, g_wide.data_ptr(), F + 2, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), need,
                                     _lib.stream_ptr(dev))
    _lib.check(rc, "dgn_feat_embed_backward")
    torch.cuda.synchronize()
    assert torch.equal(dw.cpu(), dw_ref) and torch.equal(db.cpu(), db_ref)


def test_input_that_asks_for_a_gradient_takes_the_linear_route():
    """``x.requires_grad``: not supported by the kernels (they have no input gradient), and the net's embedding still gives the right one
    through ``F.linear``."""
    from dgn_amd import nets, ops
    dev = torch.device("cuda")
    x, w, b, gy = _case(200, 5, 65, seed=9)
    fc = torch.nn.Linear(5, 65).to(dev)
    with torch.no_grad():
        fc.weight.copy_(w)
        fc.bias.copy_(b)
    xd = x.to(dev).requires_grad_(True)
    assert not ops.feature_embedding_supported(xd, fc.weight) and ops.feature_embedding_supported(xd.detach(), fc.weight)
    with pytest.raises(ValueError):
        ops.feature_embedding(xd, fc.weight, fc.bias)
    y = nets._feature_linear(fc, xd)
    y.backward(gy.to(dev))
    _close(xd.grad.cpu(), gy.double() @ w.double())
    _close(fc.weight.grad.cpu(), gy.double().t() @ x.double())
    y_k = nets._feature_linear(fc, xd.detach())                     # the same module on data: the kernel
    np.testing.assert_allclose(y_k.detach().cpu().numpy(), y.detach().cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert not ops.feature_embedding_supported(torch.zeros(4, 9, device=dev), torch.zeros(65, 9, device=dev))      # K > 8
    assert not ops.feature_embedding_supported(torch.zeros(4, 5, device=dev), torch.zeros(161, 5, device=dev))     # F > 160
    assert not ops.feature_embedding_supported(torch.zeros(4, 5, device=dev).double(), torch.zeros(65, 5, device=dev))
