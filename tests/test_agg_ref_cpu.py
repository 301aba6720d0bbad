"""tests/agg_ref.py -- the fp64 statement tests/test_agg_grid_gpu.py judges the sweep kernels against -- tied to the oracle: values and
autograd gradients of ``oracle.dgn_oracle.aggregate_graph`` in fp64 for all ten ops and the three scalers, with the weights of
``edge_weights_ref``; the mailbox fixtures G1 / G5 (computed by the reference itself, fp32); the tower layout, the edge-type table, the
first-slot rule of max / min on exact ties, and the conditioning facts.  No GPU."""
import numpy as np
import pytest
import torch

import agg_ref as ref
from oracle import dgn_oracle as orc

RT = 1e-12      # a few fp64 roundings of sums of at most a dozen O(1) terms

# a small multigraph: a row without slots, a duplicated source (row 1), a self loop (row 2), in-degrees 0..5; source 7 has no out-edge
DEGS = [0, 3, 2, 1, 5, 4, 2, 0]
SRC = [4, 4, 0,  2, 5,  6,  0, 1, 2, 3, 5,  1, 3, 3, 6,  0, 2]
N, F_ = len(DEGS), 6
INDPTR = np.concatenate([[0], np.cumsum(DEGS)])
CHANNELS = ((orc.W_ABSNORM, 1, 0.0), (orc.W_SOFTMAX, 2, 0.1), (orc.W_ABSNORM, 3, 0.0))
NAMES = "mean sum max min std var dir1-av dir2-0.1 dir1-dx dir1-dx-no-abs dir3-dx x_in".split()
OPS = [ref.MEAN, ref.SUM, ref.MAX, ref.MIN, ref.STD, ref.VAR, ref.DIR_AV, ref.DIR_WSUM, ref.DIR_DX, ref.DIR_DX_NO_ABS, ref.DIR_DX, ref.X_IN]
CHS = [0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 2, 0]
SCALERS = {"identity": ref.IDENTITY, "amplification": ref.AMPLIFICATION, "attenuation": ref.ATTENUATION}
AVG = 1.3


def close(a, b, what, rt=RT):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, scale = float(np.abs(a - b).max()), max(1.0, float(np.abs(b).max()))
    assert err <= rt * scale, f"{what}: {err:.3e} > {rt:g} x {scale:.3e}"


def problem(seed=0):
    rng = np.random.default_rng(seed)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s))
    return dict(x_src=t(N, F_), x_dst=t(N, F_), m_edge=t(len(SRC), F_), x_in=t(N, F_), eig=t(N, 4).float())


def oracle(p, names, scalers, terms, ct, table=None):
    """aggregate_graph in fp64 with autograd: out [N, S*A*F] and the gradients of the given terms"""
    src, dst = torch.tensor(SRC), torch.repeat_interleave(torch.arange(N), torch.tensor(DEGS))
    leaves = {k: p[k].clone().requires_grad_(True) for k in terms}
    msg = 0.0
    if "x_dst" in leaves:
        msg = msg + leaves["x_dst"][dst]
    if "x_src" in leaves:
        msg = msg + leaves["x_src"][src]
    if "m_edge" in leaves:
        msg = msg + (leaves["m_edge"] if table is None else leaves["m_edge"][table])
    x_in = leaves["x_in"]
    cols = []
    for s in scalers:                                   # (the oracle applies the scaler concat only to lists of several: one at a time here)
        y = orc.aggregate_graph(src, dst, N, msg, p["eig"].double(), x_in, [n for n in names if n != "x_in"], ["identity"], AVG)
        y = y.reshape(N, -1, F_)
        if "x_in" in names:
            y = torch.cat([y, x_in.unsqueeze(1)], dim=1)
        deg = torch.tensor(DEGS)
        f = torch.ones(N, dtype=torch.float64)
        if s == "amplification":
            f = torch.log(deg.double() + 1.0) / AVG
        elif s == "attenuation":
            f = torch.where(deg > 0, AVG / torch.log(deg.double() + 1.0), torch.zeros(N, dtype=torch.float64))
        cols.append(y * f[:, None, None])
    out = torch.stack(cols, dim=1).reshape(N, -1)
    grads = torch.autograd.grad(out, list(leaves.values()), ct, allow_unused=True)
    return out.detach().numpy(), {k: (g.numpy() if g is not None else np.zeros_like(p[k].numpy())) for k, g in zip(leaves, grads)}


def mine(p, ops, chs, scalers, terms, ct=None, table=None, n_towers=1):
    w = orc.edge_weights_ref(INDPTR, SRC, p["eig"], CHANNELS).numpy()
    kw = {k: p[k].numpy() for k in terms}
    return ref.sweep(INDPTR, SRC, N, ops, chs, [SCALERS[s] for s in scalers], AVG, orc.EPS, n_towers, w=w, edge_type=table,
                     log_deg=np.log(np.asarray(DEGS) + 1.0), g_out=ct, **kw)


@pytest.mark.parametrize("terms", [("x_src", "x_in"), ("x_src", "x_dst", "x_in"), ("m_edge", "x_in"), ("x_src", "x_dst", "m_edge", "x_in")])
@pytest.mark.parametrize("scalers", [("identity",), ("identity", "amplification", "attenuation"), ("attenuation", "identity")])
def test_every_op_and_scaler_against_the_oracle_in_fp64(terms, scalers):
    p = problem(1)
    with_xin = scalers == ("identity",)                 # (the pass-through takes the single identity scaler)
    k = len(NAMES) if with_xin else len(NAMES) - 1
    names, ops, chs = NAMES[:k], OPS[:k], CHS[:k]
    ct = np.random.default_rng(2).standard_normal((N, len(scalers) * k * F_))
    out, grads = oracle(p, names, scalers, terms, torch.from_numpy(ct))
    r = mine(p, ops, chs, scalers, terms, ct)
    close(r["out"], out, "out")
    assert (r["out"][[0, 7], :(k - 1) * F_] == 0).all()                      # rows without slots: zeros ...
    if with_xin:
        assert (r["out"][[0, 7], (k - 1) * F_:] == p["x_in"].numpy()[[0, 7]]).all()      # ... apart from the x_in block
    for key, name in (("x_src", "g_src"), ("x_dst", "g_dst"), ("m_edge", "g_edge"), ("x_in", "g_in")):
        if key in terms:
            close(r[name], grads[key], name)
        elif key != "x_dst":
            assert r[name] is None


def test_edge_type_table_and_bipartite_sources():
    p = problem(3)
    table = np.array([k % 3 for k in range(len(SRC))])
    p["m_edge"] = p["m_edge"][:3]
    terms = ("x_src", "m_edge", "x_in")
    ct = np.random.default_rng(4).standard_normal((N, len(NAMES) * F_))
    out, grads = oracle(p, NAMES, ("identity",), terms, torch.from_numpy(ct), table=torch.from_numpy(table))
    r = mine(p, OPS, CHS, ("identity",), terms, ct, table=table)
    close(r["out"], out, "out")
    close(r["g_edge"], grads["m_edge"], "the table's gradient")
    close(r["g_src"], grads["x_src"], "g_src")
    # more source rows than destinations: the rows beyond get no gradient, the rest is unchanged
    w = orc.edge_weights_ref(INDPTR, SRC, p["eig"], CHANNELS).numpy()
    xs = np.concatenate([p["x_src"].numpy(), np.ones((3, F_))])
    r2 = ref.sweep(INDPTR, SRC, N + 3, OPS, CHS, [ref.IDENTITY], AVG, orc.EPS, x_src=xs, m_edge=p["m_edge"].numpy(), edge_type=table,
                   x_in=p["x_in"].numpy(), w=w, g_out=ct)
    assert r2["g_src"].shape == (N + 3, F_) and (r2["g_src"][N:] == 0).all() and np.array_equal(r2["g_src"][:N], r["g_src"])


def test_tower_layout_is_a_permutation_of_the_reference_order():
    """[T][S][A][F/T]: column block (t, s, a) holds features t F/T .. of (s, a) -- values and the upstream gradient alike"""
    p = problem(5)
    terms, scalers, T = ("x_src", "x_in"), ("identity", "amplification"), 3
    k = len(NAMES) - 1
    S_, Ft = len(scalers), F_ // T
    ct = np.random.default_rng(6).standard_normal((N, S_ * k * F_))
    one = mine(p, OPS[:k], CHS[:k], scalers, terms, ct)
    perm = lambda a: a.reshape(N, S_, k, T, Ft).transpose(0, 3, 1, 2, 4).reshape(N, -1)
    tw = mine(p, OPS[:k], CHS[:k], scalers, terms, perm(ct), n_towers=T)
    assert np.array_equal(tw["out"], perm(one["out"]))
    for name in ("g_src", "g_dst", "g_in"):
        assert np.array_equal(tw[name], one[name]), name


def test_max_min_gradient_goes_to_the_first_slot_on_exact_ties():
    """Acc::add compares strictly: the first slot of the row, in CSR order, that holds the extreme takes the whole gradient"""
    indptr, src = [0, 4, 4, 6], [0, 1, 2, 1, 2, 2]
    x = np.array([[1.0, -2.0], [3.0, -2.0], [3.0, 5.0]])
    ct = np.arange(1.0, 13.0).reshape(3, 4)
    r = ref.sweep(indptr, src, 3, [ref.MAX, ref.MIN], [0, 0], [ref.IDENTITY], x_src=x, m_edge=np.zeros((6, 2)), g_out=ct)
    assert np.array_equal(r["out"], [[3, 5, 1, -2], [0, 0, 0, 0], [3, 5, 3, 5]])
    want = np.zeros((6, 2))
    want[1, 0], want[2, 1] = ct[0, 0], ct[0, 1]          # row 0, max: slot 1 (node 1, before its repeat in slot 3) / slot 2
    want[0, 0], want[0, 1] = ct[0, 2], ct[0, 3]          # row 0, min: slot 0 in both columns (-2 again in slots 1 and 3)
    want[4] = ct[2, :2] + ct[2, 2:]                      # row 2: two equal messages, the first takes max and min
    assert np.array_equal(r["g_edge"], want)
    assert np.array_equal(r["g_src"], [want[0], want[1] + want[3], want[2] + want[4] + want[5]])


def test_conditioning_facts():
    indptr, src = [0, 2, 4, 6], [0, 1, 0, 1, 2, 2]
    x = np.array([[1.0], [1.0 + 2.0 ** -10], [2.0]])
    w = np.array([[0.5, -0.5, 0.5, 0.5, 1.0, -1.0]])
    x_in = np.array([[1.0], [0.25], [7.0]])
    r = ref.sweep(indptr, src, 3, [ref.DIR_DX, ref.STD], [0, 0], [ref.IDENTITY], x_src=x, x_in=x_in, w=w)
    # row 0: r = -2^-11 against sum |w m| ~ 1: unconditioned.  row 1: r ~ 1 - 0.25.  row 2: weights cancel, r = 0 exactly: unconditioned
    assert r["dx_ok"].ravel().tolist() == [False, True, False]
    # rows 0 / 1: var = 2^-22 against E[m^2] ~ 1: unconditioned; row 2: two equal messages, exactly zero: fine
    assert r["var_ok"].ravel().tolist() == [False, False, True]
    r = ref.sweep(indptr, src, 3, [ref.DIR_DX_NO_ABS, ref.MEAN], [0, 0], [ref.IDENTITY], x_src=x, x_in=x_in, w=w)
    assert r["dx_ok"].all()                              # (no sign to lose without the absolute value)


NAME_OPS = {"mean": ref.MEAN, "sum": ref.SUM, "max": ref.MAX, "min": ref.MIN, "std": ref.STD, "var": ref.VAR}
KINDS = {"av": (ref.DIR_AV, orc.W_ABSNORM, 0.0), "dx": (ref.DIR_DX, orc.W_ABSNORM, 0.0), "dx-no-abs": (ref.DIR_DX_NO_ABS, orc.W_ABSNORM, 0.0),
         "dx-balanced": (ref.DIR_DX, orc.W_BALANCED, 0.0), "0.1": (ref.DIR_WSUM, orc.W_SOFTMAX, 0.1), "neg-0.1": (ref.DIR_WSUM, orc.W_SOFTMAX, -0.1)}


@pytest.mark.parametrize("fixture", ["g1_aggregators", "g5_edge_cases"])
def test_mailbox_fixtures_of_the_reference(golden, fixture):
    """G1 / G5: mailboxes [n, D, F] the reference's own aggregators were run on (fp32): every name, value and both gradients.  The
    mailbox is a CSR of n rows of D slots whose messages are the dense edge term; the weights come from the slots' eig pairs."""
    g = golden(fixture)
    cases = [f"c{i}" for i in range(int(g["n_cases"]))] if fixture == "g1_aggregators" else g["cases"].tolist()
    for c in cases:
        h, es, ed, x, ct = (g[f"{c}/{k}"] for k in ("h", "eig_s", "eig_d", "h_in", "cot"))
        n, D, F = h.shape
        indptr, src = np.arange(n + 1) * D, np.zeros(n * D, dtype=np.int64)
        for name in g["names"].tolist():
            if name in NAME_OPS:
                op, w = NAME_OPS[name], None
            else:
                k, kind = int(name[3]), name[5:]
                op, wk, alpha = KINDS[kind]
                w = orc.edge_weights_ref(indptr, src, None, ((wk, k, alpha),), eig_s_edge=es.reshape(n * D, -1), eig_d_edge=ed.reshape(n * D, -1)).numpy()
            r = ref.sweep(indptr, src, 1, [op], [0], [ref.IDENTITY], 1.0, orc.EPS, m_edge=h.reshape(n * D, F), x_in=x, w=w, g_out=ct)
            # (fp32 fixtures; the reference's own fp32 std / var gradient carries the cancellation of E[m^2] - mean^2: 2.3e-4 on c7)
            tol = dict(rtol=1e-3 if name in ("std", "var") else 2e-5, atol=2e-6)
            np.testing.assert_allclose(r["out"], g[f"{c}/{name}/y"], err_msg=f"{c} {name} y", **tol)
            np.testing.assert_allclose(r["g_edge"].reshape(n, D, F), g[f"{c}/{name}/gh"], err_msg=f"{c} {name} gh", **tol)
            np.testing.assert_allclose(r["g_in"], g[f"{c}/{name}/gx"], err_msg=f"{c} {name} gx", **tol)
