"""The directional-aggregation sweep (csrc/dgn_agg_kernels.hpp behind ``dgn_agg_forward`` / ``dgn_agg_backward``) stated in plain fp64
numpy: no GPU, no library, no autograd.  tests/test_agg_ref_cpu.py ties it to ``oracle.dgn_oracle.aggregate_graph`` (values and autograd
gradients in fp64) and to the fixtures G1 / G5; tests/test_agg_grid_gpu.py judges the kernels against it.

    m_j = x_src[src_j] + x_dst[i] + m_edge[j]          (m_edge[edge_type[j]] in table mode), slot j of row i, CSR order
    out[i] columns [T][S][A][F / T]                     (include/dgn_hip.h: DgnAggSpec); zero in-degree rows are zeros apart from __x_in__

Backward, in closed form.  With g_a = sum_s factor_s(i) g_out[i, s, a] the upstream gradient of aggregator a of row i, d = in-degree:

    dm_j = c0 + cv m_j + sum_c (w_jc cs_c + |w_jc| ca_c) + [j == argmax] gmax + [j == argmin] gmin
        mean: c0 += g / d        sum: c0 += g        max / min: gmax / gmin += g, at the FIRST slot of the row (CSR order) holding the extreme
        var (where E[m^2] - mean^2 > 0): cv += 2 g / d, c0 -= (2 g / d) mean          std: the same with g / (2 std) for g
        dirC-av: ca_c += g       dirC-wsum: cs_c += g
        dirC-dx-no-abs: cs_c += g, d x_in -= (sum_j w_jc) g          dirC-dx: the same with sign(r_c) g, sign(0) = 0
        __x_in__: d x_in += g
    d x_src[u] = sum of dm_j over the slots with src_j = u;  d x_dst[i] = sum_j dm_j;  d m_edge[j] = dm_j (table: summed by type).

``sweep`` also returns, per (row, feature), the CONDITIONING facts the GPU grid builds its inputs and its comparison masks on:
``dx_ok`` -- every residual r_c of an abs-valued dx aggregator keeps |r_c| >= 1e-3 (sum_j |w_jc m_j| + |(sum_j w_jc) x_in|), so its sign is
the same in fp32 -- and ``var_ok`` -- E[m^2] - mean^2 is either exactly zero with every message of the row equal, or at least 1e-3
(E[m^2] + mean^2), so std / var and the relu' of their gradient do not hang on the cancellation."""
import numpy as np

MEAN, SUM, MAX, MIN, STD, VAR, DIR_AV, DIR_WSUM, DIR_DX, DIR_DX_NO_ABS, X_IN = range(11)      # include/dgn_hip.h: DGN_AGG_*
IDENTITY, AMPLIFICATION, ATTENUATION = range(3)                                                # DGN_SCALE_*
COND = 1e-3


def _cast(a, dtype=np.float64):
    return None if a is None else np.asarray(a, dtype=dtype)


def _seg(ufunc, a, indptr):
    """ufunc-reduce the rows of ``a [E, ...]`` over every CSR row; [N, ...], rows without slots keep the ufunc's identity-free 0."""
    deg = np.diff(indptr)
    out = np.zeros((len(deg),) + a.shape[1:], dtype=a.dtype)
    nz = deg > 0
    if nz.any():
        out[nz] = ufunc.reduceat(a, indptr[:-1][nz], axis=0)
    return out


def scaler_factors(scalers, log_deg, avg_log, n, dtype=np.float64):
    """[S, n] factors of scalers.py:7-18 from the per-row log_deg the caller hands the kernel."""
    fac = np.ones((len(scalers), n), dtype=dtype)
    for s, kind in enumerate(scalers):
        if kind == AMPLIFICATION:
            fac[s] = _cast(log_deg, dtype) / dtype(avg_log)
        elif kind == ATTENUATION:
            with np.errstate(divide="ignore"):
                fac[s] = dtype(avg_log) / _cast(log_deg, dtype)
    return fac


def messages(indptr, src, x_src=None, x_dst=None, m_edge=None, edge_type=None, dtype=np.float64):
    indptr, src = np.asarray(indptr, dtype=np.int64), np.asarray(src, dtype=np.int64)
    dst = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    m = dtype(0.0)
    if x_dst is not None:
        m = m + _cast(x_dst, dtype)[dst]
    if x_src is not None:
        m = m + _cast(x_src, dtype)[src]
    if m_edge is not None:
        m = m + (_cast(m_edge, dtype)[np.asarray(edge_type, dtype=np.int64)] if edge_type is not None else _cast(m_edge, dtype))
    return m, dst


def sweep(indptr, src, n_src, ops, chs, scalers, avg_log=1.0, eps=1e-8, n_towers=1, x_src=None, x_dst=None, m_edge=None,
          edge_type=None, x_in=None, w=None, log_deg=None, g_out=None, facts_only=False, dtype=np.float64):
    """Forward (and, given ``g_out [N, T*S*A*F/T]``, backward) of one launch.  ``w [n_ch, E]``; ``ops`` / ``chs``: the aggregator list.
    ``facts_only``: just the two conditioning facts.  ``dtype``: np.float32 evaluates the same formulas in fp32 (the yardstick of the
    GPU grid's error ratios).  Returns a dict: ``out`` [N, T*S*A*F/T], ``dx_ok`` / ``var_ok`` [N, F] bool, and with g_out ``g_src`` [n_src, F] (None without x_src),
    ``g_dst``, ``g_edge`` ([E, F], or the table's [K, F]; None without m_edge), ``g_in`` (None without x_in)."""
    indptr, src = np.asarray(indptr, dtype=np.int64), np.asarray(src, dtype=np.int64)
    N, E = len(indptr) - 1, len(src)
    m, dst = messages(indptr, src, x_src, x_dst, m_edge, edge_type, dtype)
    zeros = lambda *shape: np.zeros(shape, dtype=dtype)
    avg_log, eps = dtype(avg_log), dtype(eps)
    F = m.shape[1]
    assert m.shape == (E, F) and F % n_towers == 0
    deg = np.diff(indptr)
    d = np.maximum(deg, 1).astype(dtype)[:, None]
    has = (deg > 0)[:, None]
    xin = _cast(x_in, dtype) if x_in is not None else zeros(N, F)
    w = _cast(w, dtype) if w is not None else zeros(0, E)
    S_, A_, Ft = len(scalers), len(ops), F // n_towers

    tot = _seg(np.add, m, indptr)
    mean = tot / d
    msq = _seg(np.add, m * m, indptr) / d
    rawvar = msq - mean * mean
    var = np.maximum(rawvar, dtype(0.0))
    std = np.sqrt(var + eps)
    big = np.where(has, _seg(np.maximum, m, indptr), dtype(0.0))
    small = np.where(has, _seg(np.minimum, m, indptr), dtype(0.0))
    used = sorted({c for o, c in zip(ops, chs) if DIR_AV <= o <= DIR_DX_NO_ABS})
    ws = {c: _seg(np.add, w[c][:, None] * m, indptr) for c in used}
    wa = {c: _seg(np.add, np.abs(w[c])[:, None] * m, indptr) for c in used}
    sw = {c: _seg(np.add, w[c][:, None], indptr) for c in used}
    res = {c: ws[c] - sw[c] * xin for c in used}

    dx_ok = np.ones((N, F), dtype=bool)
    for c in sorted({c for o, c in zip(ops, chs) if o == DIR_DX}):
        mag = _seg(np.add, np.abs(w[c][:, None] * m), indptr) + np.abs(sw[c] * xin)
        dx_ok &= ~has | (np.abs(res[c]) >= COND * mag)
    all_equal = big == small
    var_ok = ~has | (deg[:, None] == 1) | ((rawvar == 0.0) & all_equal) | (rawvar >= COND * (msq + mean * mean))

    if facts_only:
        return dict(dx_ok=dx_ok, var_ok=var_ok)

    def value(o, c):
        return {MEAN: mean, SUM: tot, MAX: big, MIN: small, STD: std, VAR: var, X_IN: xin}[o] if o < DIR_AV or o == X_IN else \
               wa[c] if o == DIR_AV else ws[c] if o == DIR_WSUM else np.abs(res[c]) if o == DIR_DX else res[c]

    fac = scaler_factors(scalers, log_deg, avg_log, N, dtype)
    out = zeros(N, n_towers, S_, A_, Ft)
    for s in range(S_):
        for a, (o, c) in enumerate(zip(ops, chs)):
            with np.errstate(invalid="ignore"):             # (rows without slots: 0 x the attenuation's inf, masked below)
                v = value(o, c) * fac[s][:, None]
            if o == X_IN:
                v = xin if scalers[s] == IDENTITY else np.where(has, v, 0.0)
            else:
                v = np.where(has, v, 0.0)
            out[:, :, s, a, :] = v.reshape(N, n_towers, Ft)
    r = dict(out=out.reshape(N, -1), dx_ok=dx_ok, var_ok=var_ok)
    if g_out is None:
        return r

    go = _cast(g_out, dtype).reshape(N, n_towers, S_, A_, Ft)
    slot = np.broadcast_to(np.arange(E)[:, None], (E, F))
    amax = _seg(np.minimum, np.where(m == big[dst], slot, E), indptr)        # the FIRST slot that holds the extreme
    amin = _seg(np.minimum, np.where(m == small[dst], slot, E), indptr)
    c0, cv, gmax, gmin, gxin = (zeros(N, F) for _ in range(5))
    cs, ca = {c: zeros(N, F) for c in used}, {c: zeros(N, F) for c in used}
    for a, (o, c) in enumerate(zip(ops, chs)):
        if o == X_IN:                                  # (validate(): the single identity scaler) -- rows without slots included
            gxin += go[:, :, 0, a, :].reshape(N, F)
            continue
        g = zeros(N, F)
        for s in range(S_):
            g += np.where(has, fac[s][:, None], dtype(0.0)) * go[:, :, s, a, :].reshape(N, F)
        g = np.where(has, g, dtype(0.0))
        if o == MEAN:
            c0 += g / d
        elif o == SUM:
            c0 += g
        elif o == MAX:
            gmax += g
        elif o == MIN:
            gmin += g
        elif o in (STD, VAR):
            gg = np.where(rawvar > 0.0, g / (dtype(2.0) * std) if o == STD else g, dtype(0.0))
            t = dtype(2.0) * gg / d
            cv += t
            c0 -= t * mean
        elif o == DIR_AV:
            ca[c] += g
        elif o == DIR_WSUM:
            cs[c] += g
        else:
            sg = np.sign(res[c]) if o == DIR_DX else dtype(1.0)
            cs[c] += sg * g
            gxin -= sg * sw[c] * g
    dm = c0[dst] + cv[dst] * m
    for c in used:
        dm += w[c][:, None] * cs[c][dst] + np.abs(w[c])[:, None] * ca[c][dst]
    dm += np.where(slot == amax[dst], gmax[dst], dtype(0.0)) + np.where(slot == amin[dst], gmin[dst], dtype(0.0))
    r["dm"] = dm
    r["g_dst"] = _seg(np.add, dm, indptr)
    r["g_src"] = None
    if x_src is not None:
        r["g_src"] = zeros(n_src, F)
        np.add.at(r["g_src"], src, dm)
    r["g_edge"] = None
    if m_edge is not None and edge_type is None:
        r["g_edge"] = dm
    elif m_edge is not None:
        r["g_edge"] = zeros(np.asarray(m_edge).shape[0], F)
        np.add.at(r["g_edge"], np.asarray(edge_type, dtype=np.int64), dm)
    r["g_in"] = gxin if x_in is not None else None
    return r
