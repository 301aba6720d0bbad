"""tests/combine_tail_ref.py -- the fp64 statements the direct GPU tests of the scale-combine and BatchNorm-tail kernels are judged
against -- tied to torch's own autograd in fp64 (``torch.nn.functional.batch_norm``, ``relu``, a residual add,
``oracle_backend.oracle_scale_combine``): outputs, every gradient, running statistics, the padded case written as BatchNorm over the
first n_valid rows with the rest masked.  Agreement at 1e-12 of the tensor's scale (its magnitude's largest entry: the bias gradient in
front of a BatchNorm is a sum that cancels to zero).  Also: every problem the GPU tests draw satisfies the conditions their bounds rest
on (ReLU margin, E[x^2] / var cap), and the magnitudes are positive wherever the value is not zero.  No GPU."""
import pytest
import torch

import combine_tail_ref as ref
from oracle_backend import oracle_scale_combine

RTOL = 1e-12
EPS = ref.EPS


def close(a, b, mag=None, what=""):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(float(b.abs().max()), float(mag.abs().max()) if mag is not None else 0.0, 1e-300)
    err = float((a - b).abs().max())
    assert err <= RTOL * scale, f"{what}: {err:.3e} > 1e-12 x {scale:.3e}"
    if mag is not None:
        assert bool((mag[a != 0] > 0).all()), f"{what}: a magnitude that is not positive under a non-zero value"
        assert bool((mag >= a.abs() * (1 - 1e-12)).all()), f"{what}: a magnitude below its value"


def leaf(t):
    return None if t is None else t.double().clone().requires_grad_(True)


@pytest.mark.parametrize("T,fo,S,table,N,bias,rows", [(3, 7, 1, False, 33, True, True), (3, 7, 1, True, 33, True, True), (5, 14, 3, True, 17, True, True),
                                                      (2, 5, 4, True, 9, False, True), (1, 9, 2, True, 1, True, False)])
def test_scale_combine_against_autograd(T, fo, S, table, N, bias, rows):
    z = ref.values((T, N, S * fo), 1)
    scale = ref.uniform((N, S), 2) if table else None
    b = ref.values((T * fo,), 3) if bias else None
    rs = ref.uniform((N,), 4) if rows else None
    ct = ref.values((N, T * fo), 5)
    zl, bl = leaf(z), leaf(b)
    y = oracle_scale_combine(zl, None if scale is None else scale.double(), bl, None if rs is None else rs.double())
    y.backward(ct.double())
    mine, mag = ref.scale_combine_forward(z, scale, b, rs)
    close(mine, y, mag, "y")
    back = ref.scale_combine_backward(ct, scale, rs, T, S, fo)
    close(back["g_z"], zl.grad, back["g_z_mag"], "g_z")
    if bias:
        close(back["g_bias"], bl.grad, back["g_bias_mag"], "g_bias")


def torch_tail(x, gamma, beta, rm, rv, momentum, training, relu, residual, nv):
    """F.batch_norm over the first nv rows (+ ReLU + residual); the padding rows normalised with the same (detached) statistics."""
    N = x.shape[0]
    y = torch.nn.functional.batch_norm(x[:nv], rm, rv, gamma, beta, training, momentum, EPS)
    if nv < N:
        mean, var = x[:nv].mean(0).detach(), x[:nv].var(0, unbiased=False).detach()
        pad = (x[nv:] - mean) / torch.sqrt(var + EPS)
        pad = pad * gamma if gamma is not None else pad
        pad = pad + beta if beta is not None else pad
        y = torch.cat([y, pad.detach()])
    y = torch.relu(y) if relu else y
    return y + residual if residual is not None else y


@pytest.mark.parametrize("N,F,nv", [(257, 7, None), (33, 70, None), (2, 3, None), (40, 5, 37), (40, 6, 2), (257, 75, 100)])
@pytest.mark.parametrize("relu,residual,affine", [(True, True, True), (False, False, True), (True, False, False)])
def test_bn_tail_against_autograd(N, F, nv, relu, residual, affine):
    d = ref.tail_data(N, F, seed=11, n_valid=nv)
    n = N if nv is None else nv
    gamma, beta = (d.gamma, d.beta) if affine else (None, None)
    res = d.residual if residual else None
    momentum = 0.1
    xl, gl, bl = leaf(d.x), leaf(gamma), leaf(beta)
    rm, rv = d.running_mean.double().clone(), d.running_var.double().clone()
    y = torch_tail(xl, gl, bl, rm, rv, momentum, True, relu, None if res is None else res.double(), n)
    ct = d.g.double().clone()
    ct[n:] = 0.0                                                     # the padding rows are masked out of the loss
    y.backward(ct)
    st = ref.bn_statistics(d.x, EPS, nv)
    fwd = ref.bn_tail_forward(d.x, gamma, beta, d.running_mean, d.running_var, momentum, EPS, True, relu, res, nv)
    close(fwd["y"], y, fwd["y_mag"], "y")
    close(fwd["running_mean"], rm, fwd["running_mean_mag"], "running_mean")
    close(fwd["running_var"], rv, fwd["running_var_mag"], "running_var")
    close(st["mean"], xl.detach()[:n].mean(0), None, "mean")
    close(st["invstd"], 1.0 / torch.sqrt(xl.detach()[:n].var(0, unbiased=False) + EPS), None, "invstd")
    bwd = ref.bn_tail_backward(d.g, d.x, gamma, beta, st["mean"], st["invstd"], relu, nv)
    close(bwd["g_x"], xl.grad, bwd["g_x_mag"], "g_x")
    assert bool((bwd["g_x"][n:] == 0).all())
    if affine:
        close(bwd["g_gamma"], gl.grad, bwd["sums_mag"][F:], "g_gamma")
        close(bwd["g_beta"], bl.grad, bwd["sums_mag"][:F], "g_beta")
    # eval mode: the running statistics
    ye = torch_tail(d.x.double(), None if gamma is None else gamma.double(), None if beta is None else beta.double(), d.running_mean.double(),
                    d.running_var.double(), momentum, False, relu, None if res is None else res.double(), N)
    ev = ref.bn_tail_forward(d.x, gamma, beta, d.running_mean, d.running_var, momentum, EPS, False, relu, res)
    close(ev["y"], ye, ev["y_mag"], "eval y")


def test_bn_tail_on_one_row():
    """torch refuses one row in training mode; the header's statement: mean = the row, biased variance 0, running_var takes the biased one."""
    d = ref.tail_data(1, 5, seed=3)
    fwd = ref.bn_tail_forward(d.x, d.gamma, d.beta, d.running_mean, d.running_var, 0.1, EPS, True, False, None)
    assert torch.equal(fwd["mean"], d.x.double()[0]) and bool((fwd["stats"]["var"] == 0).all())
    close(fwd["invstd"], torch.full((5,), EPS ** -0.5, dtype=torch.float64), None, "invstd")
    close(fwd["running_var"], 0.9 * d.running_var.double(), fwd["running_var_mag"], "running_var")
    close(fwd["running_mean"], 0.9 * d.running_mean.double() + 0.1 * d.x.double()[0], fwd["running_mean_mag"], "running_mean")
    close(fwd["y"], d.beta.double().reshape(1, 5), fwd["y_mag"], "y")


@pytest.mark.parametrize("T,fo,S,table,N,nv", [(1, 7, 1, False, 33, None), (1, 6, 1, True, 33, None), (5, 14, 3, True, 40, None), (1, 75, 1, False, 40, 37),
                                               (3, 2, 2, True, 40, 3)])
@pytest.mark.parametrize("relu", [True, False])
def test_combine_backward_behind_batchnorm_against_autograd(T, fo, S, table, N, nv, relu):
    """DgnBnGrad: z -> scale-combine -> BatchNorm (+ ReLU); d z, d bias, d gamma, d beta."""
    wy = T * fo
    n = N if nv is None else nv
    z = ref.values((T, N, S * fo), 21)
    scale = ref.uniform((N, S), 22) if table else None
    b, rs = ref.values((wy,), 23), ref.uniform((N,), 24)
    d = ref.tail_data(N, wy, seed=25)
    zl, bl, gl, bel = leaf(z), leaf(b), leaf(d.gamma), leaf(d.beta)
    y0 = oracle_scale_combine(zl, None if scale is None else scale.double(), bl, rs.double())
    out = torch_tail(y0, gl, bel, None, None, 0.1, True, relu, None, n)
    ct = d.g.double().clone()
    ct[n:] = 0.0
    out.backward(ct)
    y0d = y0.detach()
    st = ref.bn_statistics(y0d, EPS, nv)
    tail = ref.bn_tail_backward(d.g, y0d, d.gamma, d.beta, st["mean"], st["invstd"], relu, nv)
    close(tail["g_gamma"], gl.grad, tail["sums_mag"][wy:], "g_gamma")
    close(tail["g_beta"], bel.grad, tail["sums_mag"][:wy], "g_beta")
    back = ref.scale_combine_backward(None, scale, rs, T, S, fo, bn=dict(g_out=d.g, y=y0d, gamma=d.gamma, beta=d.beta, mean=st["mean"], invstd=st["invstd"],
                                                                       sums=tail["sums"], relu=relu, n_valid=nv))
    close(back["g_z"], zl.grad, back["g_z_mag"], "g_z")
    close(back["g_bias"], bl.grad, back["g_bias_mag"], "g_bias")
    assert bool((back["g_z"][:, n:] == 0).all())


# ---- the problems of tests/test_combine_tail_gpu.py ---------------------------------------------------------------------------------
def gpu_problems():
    """(N, F, n_valid) of every TailData the GPU tests draw, small ones first."""
    import test_combine_tail_gpu as g
    keys = {(N, W, None) for W in g.FLAT_WIDTHS for N in g.FLAT_ROWS}
    keys |= {(c[4], c[0] * c[1], None) for c in g.OFF_FLAT.values()}
    keys |= {(N, F, None) for F in g.TAIL_WIDTHS for N in g.TAIL_ROWS}
    keys |= {(N, F, kw.get("nv")) for N, F, kw in g.FWD_LAYOUT.values()}
    keys |= {(N, F, None) for table in (g.BWD_LAYOUT, g.BWD_FLAT) for N, F, kw in table.values()}
    keys |= {g.TOO_WIDE + (None,)}
    return sorted(keys, key=lambda k: (k[0] * k[1], k[0], k[1], k[2] or 0))


@pytest.mark.parametrize("N,F,nv", gpu_problems(), ids=lambda v: str(v))
def test_the_gpu_tests_problems_satisfy_the_conditions_of_the_bounds(N, F, nv):
    """No fp64 pre-activation within 1e-3 of zero except the planted exact zeros (offenders were MOVED, none excluded), E[x^2] / var <= 4 in
    every unplanted column, a column with gamma < 0, a column at a scale of 1e-4, the fp32 mean / invstd the fp64 statistics rounded."""
    d = ref.tail_data(N, F, n_valid=nv)
    assert d.conditions()
    assert d.x.dtype == d.g.dtype == d.mean.dtype == d.invstd.dtype == torch.float32 and tuple(d.x.shape) == (N, F)
    assert bool(torch.isfinite(d.x).all())
    if d.tiny_col is not None and N >= 16:
        assert 0 < float(d.x[:, d.tiny_col].abs().max()) < 20 * ref.TINY_SCALE
    if N >= 3:
        pre = ref.relu_preactivation(d.x, d.gamma, d.beta, d.mean, d.invstd)
        assert int((pre[:, d.zero_col] == 0).sum()) >= len(d.zero_rows)
