"""``oracle.dgn_oracle.edge_weights_ref`` -- the fp64 statement of the per-edge directional weights that tests/test_edge_weights_gpu.py holds
the HIP kernels to -- against the oracle's own aggregators, which the golden fixtures pin (tests/test_oracle_vs_golden.py).

With identity messages (the mailbox of every node is ``eye(D)``) and ``x = 0`` an aggregator returns the weights it multiplies by:
``agg_dir_dx_no_abs`` the ABSNORM weights, ``agg_dir_av`` their absolute values, ``agg_dir_dx_balanced`` the BALANCED weights (non-negative:
its ``abs`` changes nothing), ``agg_dir_softmax`` the SOFTMAX weights.  Both sides are fp64 evaluations of the same formulas, so they agree
to a few fp64 roundings (``4 * 2^-53`` relative; exact zeros stay exact)."""
import numpy as np
import pytest
import torch

from oracle import dgn_oracle as orc

U64 = 2.0 ** -53
ABSNORM, BALANCED, SOFTMAX = orc.W_ABSNORM, orc.W_BALANCED, orc.W_SOFTMAX
K = 4
CHANNELS = ((ABSNORM, 1, 0.0), (BALANCED, 2, 0.0), (SOFTMAX, 3, 0.1), (SOFTMAX, 2, -0.1), (ABSNORM, 0, 0.0))


def _close(a, b, what):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, what
    assert bool(((a - b).abs() <= 4 * U64 * b.abs()).all()), f"{what}: max |diff| {float((a - b).abs().max()):.3e}"
    assert bool((a[b == 0] == 0).all()), what


def _bucket(D, seed):
    """7 rows of in-degree D over 40 nodes: random sources with a duplicate and a self loop; row 1 sees only nodes whose eig equals its own
    (every delta exactly 0), row 2 only larger values (one-signed deltas), row 3 only smaller ones."""
    rng = np.random.default_rng(seed)
    n, N = 7, 40
    eig = rng.standard_normal((N, K)).astype(np.float32)
    src = rng.integers(n, N, size=(n, D))
    src[0, 0] = 0                                   # self loop
    if D >= 3:
        src[0, -1] = src[0, 1]                      # duplicate source
    eig[30:33] = eig[1]                             # three copies of row 1's node
    src[1] = rng.integers(30, 33, size=D)
    src[1, 0] = 1
    eig[33:36] = eig[2] + np.abs(rng.standard_normal((3, K))).astype(np.float32) + 0.5
    src[2] = rng.integers(33, 36, size=D)
    eig[36:39] = eig[3] - np.abs(rng.standard_normal((3, K))).astype(np.float32) - 0.5
    src[3] = rng.integers(36, 39, size=D)
    indptr = np.arange(n + 1) * D
    return indptr, src.reshape(-1), torch.from_numpy(eig), n


@pytest.mark.parametrize("D", [1, 2, 5, 17])
def test_edge_weights_ref_is_what_the_aggregators_multiply_by(D):
    indptr, src, eig, n = _bucket(D, 100 + D)
    w = orc.edge_weights_ref(indptr, src, eig, CHANNELS)
    assert w.dtype == torch.float64 and tuple(w.shape) == (len(CHANNELS), n * D)
    e64 = eig.double()
    es = e64[torch.from_numpy(src)].reshape(n, D, K)
    ed = e64[:n].unsqueeze(1).expand(n, D, K)
    m = torch.eye(D, dtype=torch.float64).expand(n, D, D)
    x = torch.zeros(n, D, dtype=torch.float64)
    for c, (kind, k, alpha) in enumerate(CHANNELS):
        wc = w[c].reshape(n, D)
        if kind == ABSNORM:
            _close(wc, orc.agg_dir_dx_no_abs(m, es, ed, x, k), f"D={D} ABSNORM col {k}")
            _close(wc.abs(), orc.agg_dir_av(m, es, ed, x, k), f"D={D} |ABSNORM| col {k}")
            _close(wc.abs(), orc.agg_dir_dx(m, es, ed, x, k), f"D={D} dx col {k}")
        elif kind == BALANCED:
            assert bool((wc >= 0).all())
            _close(wc, orc.agg_dir_dx_balanced(m, es, ed, x, k), f"D={D} BALANCED col {k}")
        else:
            _close(wc, orc.agg_dir_softmax(m, es, ed, x, k, alpha), f"D={D} SOFTMAX col {k} alpha {alpha}")
    # the planted rows say what they were planted for
    r = lambda c, i: w[c].reshape(n, D)[i]
    assert bool((r(0, 1) == 0).all()) and bool((r(1, 1) == 0).all()) and bool((r(4, 1) == 0).all())      # all-zero deltas
    _close(r(2, 1), torch.full((D,), 1.0 / D, dtype=torch.float64), "softmax of equal scores")
    assert bool((r(0, 2) > 0).all()) and bool((r(0, 3) < 0).all())                                         # one-signed deltas
    a2 = orc.edge_weights_ref(indptr, src, eig, ((ABSNORM, 2, 0.0),))[0].reshape(n, D)                    # BALANCED's column
    _close(r(1, 2), a2[2] / 2, "BALANCED, no backward field")                                              # sneg = 0: half the forward field
    _close(r(1, 3), -a2[3] / 2, "BALANCED, no forward field")
    if D > 1:
        assert float(r(0, 0)[0]) == 0.0 and float(r(0, 0).abs().sum()) > 0.5                                 # the self loop's slot only


def test_edge_weights_ref_on_a_mixed_graph_through_aggregate_graph():
    """Rows of in-degree 0, 1, 2, 5 and 17 in one CSR, through the oracle's own bucketing (``aggregate_graph``): the message of slot j of a
    row is the unit vector e_j, so columns [0, D) of a row's aggregate are its weights in slot order.  Also the two other addressings of the
    same weights: a destination-range shard (``row_base``) and slot mode."""
    rng = np.random.default_rng(7)
    degs = np.array([0, 1, 2, 5, 17, 5, 0, 2, 17, 1, 5])
    n, F = len(degs), 17
    indptr = np.concatenate([[0], np.cumsum(degs)])
    E = int(indptr[-1])
    src = rng.integers(0, n, E)
    dst = np.repeat(np.arange(n), degs)
    eig = torch.from_numpy(rng.standard_normal((n, K)).astype(np.float32))
    w = orc.edge_weights_ref(indptr, src, eig, CHANNELS)
    msg = torch.zeros(E, F, dtype=torch.float64)
    msg[torch.arange(E), torch.from_numpy(np.arange(E) - indptr[dst])] = 1.0
    aggs = ["dir1-dx-no-abs", "dir2-dx-balanced", "dir3-0.1", "dir2-neg-0.1", "dir1-av"]
    out = orc.aggregate_graph(torch.from_numpy(src), torch.from_numpy(dst), n, msg, eig.double(), torch.zeros(n, F, dtype=torch.float64),
                              aggs, ["identity"], 1.0).reshape(n, len(aggs), F)
    for i in range(n):
        sl = slice(int(indptr[i]), int(indptr[i + 1]))
        for c in range(4):
            _close(w[c, sl], out[i, c, :degs[i]], f"row {i} channel {c}")
        _close(w[0, sl].abs(), out[i, 4, :degs[i]], f"row {i} dir1-av")
    # rows [3, 9) as a shard: same slots
    e0, e1 = int(indptr[3]), int(indptr[9])
    w_sh = orc.edge_weights_ref(indptr[3:10] - e0, src[e0:e1], eig, CHANNELS, row_base=3)
    assert torch.equal(w_sh, w[:, e0:e1])
    # slot mode: both endpoints per slot, no node table
    w_slot = orc.edge_weights_ref(indptr, src, None, CHANNELS, eig_s_edge=eig[torch.from_numpy(src)], eig_d_edge=eig[torch.from_numpy(dst)])
    assert torch.equal(w_slot, w)
