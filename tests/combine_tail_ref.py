"""fp64 statements of the scale-combine and BatchNorm-tail entry points of the C ABI (include/dgn_hip.h: dgn_scale_combine_forward /
_backward with and without DgnBnGrad, dgn_bn_tail_forward / _backward), written from the header's formulas in plain torch on CPU tensors,
and the seeded data the direct tests of those entry points run on (tests/test_combine_tail_gpu.py; tied to torch's autograd and checked
against the conditions of the bounds by tests/test_combine_tail_ref_cpu.py).

Every function returns its value AND A MAGNITUDE: the same expression with every term replaced by its absolute value.  The GPU tests'
bounds are ``k u magnitude`` with u = 2^-24 and k the fp32 roundings on the longest path from an input to the output.

``n_valid`` (None: every row): statistics and counts run over the first ``n_valid`` rows only, ``inv_n = 1 / n_valid``, the gradients
of rows >= n_valid are exactly zero and the bias gradient excludes them.

Nothing here rounds to fp32: a caller that wants the kernels' inputs (``mean``, ``invstd``, ``sums`` as fp32 values) passes them in."""
import numpy as np
import torch

U = 2.0 ** -24
F64 = torch.float64


def _d(t):
    return None if t is None else t.detach().to("cpu", F64)


def _nv(n_valid, N):
    return N if n_valid is None else min(int(n_valid), N)


# ---- dgn_scale_combine_forward ----------------------------------------------------------------------------------------------------
def scale_combine_forward(z, scale, bias, row_scale):
    """y[n, t fo + o] = row_scale[n] (bias[t fo + o] + sum_s scale[n, s] z[t][n][s fo + o]);  z [T, N, S fo] -> (y, magnitude) [N, T fo]."""
    z, scale, bias, row_scale = _d(z), _d(scale), _d(bias), _d(row_scale)
    T, N, W = z.shape
    S = 1 if scale is None else scale.shape[1]
    fo = W // S
    y, mag = torch.zeros(N, T * fo, dtype=F64), torch.zeros(N, T * fo, dtype=F64)
    for t in range(T):
        for s in range(S):
            term = z[t][:, s * fo:(s + 1) * fo] * (scale[:, s:s + 1] if scale is not None else 1.0)
            y[:, t * fo:(t + 1) * fo] += term
            mag[:, t * fo:(t + 1) * fo] += term.abs()
    if bias is not None:
        y, mag = y + bias.reshape(1, -1), mag + bias.abs().reshape(1, -1)
    if row_scale is not None:
        y, mag = y * row_scale.reshape(-1, 1), mag * row_scale.abs().reshape(-1, 1)
    return y, mag


# ---- BatchNorm backward, element by element (DgnBnGrad's formula = dgn_bn_tail_backward's g_x) ---------------------------------------
def relu_preactivation(x, gamma, beta, mean, invstd):
    """(x - mean) invstd gamma + beta: what the ReLU of the tail sees."""
    x, gamma, beta, mean, invstd = _d(x), _d(gamma), _d(beta), _d(mean), _d(invstd)
    e = (x - mean) * invstd
    if gamma is not None:
        e = e * gamma
    return e + beta if beta is not None else e


def bn_input_grad(g_out, x, gamma, beta, mean, invstd, sums, relu, n_valid=None):
    """g_x = gamma invstd (g' - sums[c] / n - xhat sums[F + c] / n), g' = g_out masked by the ReLU, xhat = (x - mean) invstd, n = n_valid;
    rows >= n_valid exactly 0.  -> (g_x, magnitude)."""
    g_out, x, gamma, mean, invstd, sums = _d(g_out), _d(x), _d(gamma), _d(mean), _d(invstd), _d(sums)
    N, F = x.shape
    nv = _nv(n_valid, N)
    ga = gamma if gamma is not None else torch.ones(F, dtype=F64)
    xh = (x - mean) * invstd
    gp = g_out.clone()
    if relu:
        gp = gp * (relu_preactivation(x, gamma, beta, mean, invstd) > 0)
    m1, m2 = sums[:F] / nv, sums[F:] / nv
    g = ga * invstd * (gp - m1 - xh * m2)
    mag = (ga * invstd).abs() * (gp.abs() + m1.abs() + (xh * m2).abs())
    g[nv:], mag[nv:] = 0.0, 0.0
    return g, mag


# ---- dgn_scale_combine_backward ---------------------------------------------------------------------------------------------------
def scale_combine_backward(g_y, scale, row_scale, T, S, fo, bn=None):
    """g_z[t][n][s fo + o] = row_scale[n] scale[n, s] g_y[n, t fo + o] and g_bias[c] = sum_n row_scale[n] g_y[n, c] (the amount ADDED to
    the caller's vector).  ``bn`` (the fields of a DgnBnGrad as a dict: g_out, y, gamma, beta, mean, invstd, sums, relu, n_valid): g_y is
    bn_input_grad of them.  -> dict(g_z, g_z_mag [T, N, S fo]; g_bias, g_bias_mag [T fo]; g_y, g_y_mag)."""
    if bn is not None:
        g_y, gy_mag = bn_input_grad(bn["g_out"], bn["y"], bn.get("gamma"), bn.get("beta"), bn["mean"], bn["invstd"], bn["sums"], bn.get("relu", 0),
                                    bn.get("n_valid"))
    else:
        g_y = _d(g_y)
        gy_mag = g_y.abs()
    scale, row_scale = _d(scale), _d(row_scale)
    N = g_y.shape[0]
    if row_scale is not None:
        g_y, gy_mag = g_y * row_scale.reshape(-1, 1), gy_mag * row_scale.abs().reshape(-1, 1)
    g_z, mag = torch.zeros(T, N, S * fo, dtype=F64), torch.zeros(T, N, S * fo, dtype=F64)
    for t in range(T):
        for s in range(S):
            f = scale[:, s:s + 1] if scale is not None else 1.0
            g_z[t][:, s * fo:(s + 1) * fo] = g_y[:, t * fo:(t + 1) * fo] * f
            mag[t][:, s * fo:(s + 1) * fo] = gy_mag[:, t * fo:(t + 1) * fo] * (f.abs() if scale is not None else 1.0)
    return dict(g_z=g_z, g_z_mag=mag, g_bias=g_y.sum(0), g_bias_mag=gy_mag.sum(0), g_y=g_y, g_y_mag=gy_mag)


# ---- dgn_bn_tail_forward ----------------------------------------------------------------------------------------------------------
def bn_statistics(x, eps, n_valid=None):
    """Batch statistics of the first n_valid rows -> dict(mean, var (biased), unbiased (n == 1: the biased one), invstd, ex2 = E[x^2],
    abs_mean = E|x|)."""
    x = _d(x)
    nv = _nv(n_valid, x.shape[0])
    xv = x[:nv]
    mean = xv.mean(0)
    var = ((xv - mean) ** 2).mean(0)
    unbiased = var * nv / (nv - 1) if nv > 1 else var
    return dict(mean=mean, var=var, unbiased=unbiased, invstd=1.0 / torch.sqrt(var + eps), ex2=(xv * xv).mean(0), abs_mean=xv.abs().mean(0), n=nv)


def bn_apply(x, gamma, beta, mean, invstd, relu, residual):
    """y = [relu]((x - mean) invstd gamma + beta) [+ residual] -> (y, magnitude)."""
    x, gamma, beta, mean, invstd, residual = _d(x), _d(gamma), _d(beta), _d(mean), _d(invstd), _d(residual)
    e = (x - mean) * invstd
    if gamma is not None:
        e = e * gamma
    mag = e.abs()
    if beta is not None:
        e, mag = e + beta, mag + beta.abs()
    if relu:
        e = torch.clamp_min(e, 0.0)
    if residual is not None:
        e, mag = e + residual, mag + residual.abs()
    return e, mag


def bn_tail_forward(x, gamma, beta, running_mean, running_var, momentum, eps, training, relu, residual, n_valid=None, stats=None):
    """Training: batch statistics (biased variance) of the first n_valid rows, running statistics updated with ``momentum`` (running_var
    with the unbiased variance; one row: the biased one), y by bn_apply on EVERY row.  ``stats = (mean, invstd)`` replaces the statistics
    of the apply step (the kernels' returned fp32 values).  Eval: the running statistics, invstd = 1 / sqrt(running_var + eps).
    -> dict(y, y_mag, and in training mean, invstd, running_mean, running_mean_mag, running_var, running_var_mag, stats)."""
    out = {}
    if training:
        st = bn_statistics(x, eps, n_valid)
        mean, invstd = (st["mean"], st["invstd"]) if stats is None else (_d(stats[0]), _d(stats[1]))
        out.update(mean=st["mean"], invstd=st["invstd"], stats=st)
        if running_mean is not None:
            rm, rv = _d(running_mean), _d(running_var)
            out["running_mean"] = (1.0 - momentum) * rm + momentum * st["mean"]
            out["running_mean_mag"] = ((1.0 - momentum) * rm).abs() + (momentum * st["mean"]).abs()
            out["running_var"] = (1.0 - momentum) * rv + momentum * st["unbiased"]
            out["running_var_mag"] = ((1.0 - momentum) * rv).abs() + (momentum * st["unbiased"]).abs()
    else:
        mean, invstd = _d(running_mean), 1.0 / torch.sqrt(_d(running_var) + eps)
    out["y"], out["y_mag"] = bn_apply(x, gamma, beta, mean, invstd, relu, residual)
    return out


# ---- dgn_bn_tail_backward ---------------------------------------------------------------------------------------------------------
def bn_tail_backward(g_y, x, gamma, beta, mean, invstd, relu, n_valid=None, sums=None):
    """sums[c] = sum_n g'[n, c] (= g_beta), sums[F + c] = sum_n g'[n, c] xhat[n, c] (= g_gamma) over the first n_valid rows, g_x by
    bn_input_grad from them (``sums``: other column sums for that step -- the kernels' returned fp32 values).
    -> dict(sums, sums_mag [2F] (sum |g'|, sum |g' xhat|), g_gamma, g_beta, g_x, g_x_mag)."""
    g_y, x = _d(g_y), _d(x)
    N, F = x.shape
    nv = _nv(n_valid, N)
    xh = (x - _d(mean)) * _d(invstd)
    gp = g_y.clone()
    if relu:
        gp = gp * (relu_preactivation(x, gamma, beta, mean, invstd) > 0)
    t0, t1 = gp[:nv], gp[:nv] * xh[:nv]
    s = torch.cat([t0.sum(0), t1.sum(0)])
    s_mag = torch.cat([t0.abs().sum(0), t1.abs().sum(0)])
    g_x, g_x_mag = bn_input_grad(g_y, x, gamma, beta, mean, invstd, s if sums is None else sums, relu, n_valid)
    return dict(sums=s, sums_mag=s_mag, g_beta=s[:F], g_gamma=s[F:], g_x=g_x, g_x_mag=g_x_mag)


# ---- data -------------------------------------------------------------------------------------------------------------------------
RELU_MARGIN = 1e-3      # no fp64 pre-activation of the ReLU within this of zero, except the planted exact zeros
MOMENT_CAP = 4.0        # E[x^2] / var of every unplanted column
TINY_SCALE = 1e-4
EPS = float(np.float32(1e-5))      # (the fp32 value the C ABI receives)


def f32(t):
    """fp64 -> the nearest fp32 (what the test hands to a kernel)."""
    return t.to(torch.float32)


def values(shape, seed):
    """N(0, 1) 2 + 0.7 in fp32, seeded on the CPU."""
    g = torch.Generator().manual_seed(int(seed))
    return (torch.randn(*shape, generator=g, dtype=torch.float32) * 2 + 0.7)


def uniform(shape, seed):
    """U(0.5, 1.5) in fp32: scales and row scales."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.rand(*shape, generator=g, dtype=torch.float32) + 0.5


class TailData:
    """One [N, F] BatchNorm-tail problem in fp32: x, the upstream gradient g, a residual, gamma / beta, running statistics and the fp32
    ``mean`` / ``invstd`` the backward entry points receive (the fp64 statistics of the first n_valid rows of the drawn x, rounded).

    Planted columns (the last ones the width has room for): ``zero_col`` -- beta = 0 and every third row of x equal to the fp32 mean, so
    the pre-activation is exactly 0 there and the ReLU mask must drop the gradient; ``neg_col`` -- gamma < 0; ``tiny_col`` -- values at
    a scale of 1e-4 (its variance is far below eps).  F == 1: the zero plant alone; F == 2: zero and negative gamma.
    Entries whose fp64 pre-activation lies within RELU_MARGIN of zero are moved to +-2 RELU_MARGIN (x changes, nothing is excluded);
    columns of fewer than 16 rows are centred where their E[x^2] / var exceeds MOMENT_CAP (one row: var = 0, no cap exists)."""

    def __init__(self, N, F, seed=0, n_valid=None):
        self.N, self.F, self.n_valid = N, F, n_valid
        nv = _nv(n_valid, N)
        base = 7919 * N + 31 * F + seed
        x = values((N, F), base)
        self.g = values((N, F), base + 1)
        self._base = base
        self.gamma, self.beta = uniform((F,), base + 3), values((F,), base + 4) * 0.25
        self.running_mean, self.running_var = values((F,), base + 5) * 0.1, uniform((F,), base + 6)
        self.zero_col, self.neg_col, self.tiny_col = F - 1, (F - 2 if F >= 2 else None), (F - 3 if F >= 3 else None)
        self.planted_cols = [c for c in (self.zero_col, self.neg_col, self.tiny_col) if c is not None]
        if self.neg_col is not None:
            self.gamma[self.neg_col] = -self.gamma[self.neg_col]
        if self.tiny_col is not None:
            x[:, self.tiny_col] *= TINY_SCALE
        self.beta[self.zero_col] = 0.0
        if 1 < nv < 16:      # a handful of rows: centre the columns whose mean dominates their spread
            st = bn_statistics(x, EPS, n_valid)
            bad = st["ex2"] > 0.9 * MOMENT_CAP * st["var"]
            x[:, bad] = f32(x.double()[:, bad] - st["mean"][bad])
        st = bn_statistics(x, EPS, n_valid)
        self.mean, self.invstd = f32(st["mean"]), f32(st["invstd"])
        self.zero_rows = torch.arange(0, N, 3)
        x[self.zero_rows, self.zero_col] = self.mean[self.zero_col]
        # ReLU margin: move the offenders (x is fp32, so the moved entries are re-checked by conditions())
        ga, is_, mu, be = self.gamma.double(), self.invstd.double(), self.mean.double(), self.beta.double()
        pre = relu_preactivation(x, self.gamma, self.beta, self.mean, self.invstd)
        near = pre.abs() < RELU_MARGIN
        near[self.zero_rows, self.zero_col] = False
        target = torch.where(pre >= 0, 2 * RELU_MARGIN, -2 * RELU_MARGIN)
        moved = mu + (target - be) / (ga * is_)
        x = torch.where(near, f32(moved.expand(N, F)), x)
        self.n_moved = int(near.sum())
        self.x = x

    @property
    def residual(self):
        return values((self.N, self.F), self._base + 2)

    def sums(self, relu, n_valid=None, gamma=True, beta=True):
        """The fp32 column sums a DgnBnGrad carries: fp64 over the first n_valid rows, rounded."""
        return f32(bn_tail_backward(self.g, self.x, self.gamma if gamma else None, self.beta if beta else None, self.mean, self.invstd, relu,
                                    n_valid)["sums"])

    def conditions(self):
        """The conditions the bounds rest on; raises AssertionError with the offending figure."""
        pre = relu_preactivation(self.x, self.gamma, self.beta, self.mean, self.invstd)
        planted = torch.zeros(self.N, self.F, dtype=torch.bool)
        planted[self.zero_rows, self.zero_col] = True
        assert bool((pre[planted] == 0).all()), "a planted pre-activation is not exactly 0"
        assert float(pre[~planted].abs().min()) >= RELU_MARGIN if bool((~planted).any()) else True, float(pre[~planted].abs().min())
        nv = _nv(self.n_valid, self.N)
        if nv > 1:
            st = bn_statistics(self.x, EPS, self.n_valid)
            keep = torch.ones(self.F, dtype=torch.bool)
            keep[self.planted_cols] = False
            if bool(keep.any()):
                ratio = float((st["ex2"][keep] / st["var"][keep]).max())
                assert ratio <= MOMENT_CAP, ratio
        assert float(self.gamma[self.neg_col]) < 0 if self.neg_col is not None else True
        return True


_TAIL = {}


def tail_data(N, F, seed=0, n_valid=None):
    """TailData, built once per key and shared unchanged."""
    key = (N, F, seed, n_valid)
    if N * F > (1 << 21):      # (the few large problems are used once)
        return TailData(N, F, seed, n_valid)
    if key not in _TAIL:
        _TAIL[key] = TailData(N, F, seed, n_valid)
    return _TAIL[key]
