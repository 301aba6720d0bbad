"""The numpy restatement of the input stage and of the masked L1 (tests/input_stage_oracle.py) against fixture G18 -- the reference's own
nets with ``pos_enc_dim = 3`` -- and the CPU-side facts of the feature: ``state_dict`` keys, the captured steps' refusals, the header.

The fp32 restatement keeps torch's CPU order where torch has one that numpy can state: the embedding gradient (rows added one by one in
row order) is asserted bit-equal.  ``h0``, the Linear's two gradients and the loss go through torch's GEMM / vectorised reductions, whose
order is the BLAS library's: they are judged by ``parity_util.check_reduced`` at its defaults against the fp64 restatement, the allowance
being the reference's own fp32 error."""
import numpy as np
import pytest
import torch

import input_stage_oracle as iso
from parity_util import check_reduced

CASES = ["zinc_towers", "zinc_simple", "sbm_complex"]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def pos_enc_net(g, case, device):
    """The package's net for a G18 case, with the fixture's weights."""
    from dgn_amd.nets import DGNNet, DGNNodeNet
    kind, type_net, mode, aggs, scalers = [str(x) for x in g[f"{case}/cfg"]]
    common = dict(hidden_dim=20, out_dim=20, in_feat_dropout=0.0, dropout=0.0, L=2, pos_enc_dim=int(g["pos_enc_dim"]), graph_norm=True,
                  batch_norm=True, avg_d={"log": torch.tensor(1.1)}, residual=True, edge_feat=False, edge_dim=0, pretrans_layers=1,
                  posttrans_layers=1, device=device, type_net=type_net, readout=mode, aggregators=aggs, scalers=scalers)
    net = DGNNet(dict(common, num_atom_type=6, num_bond_type=4)) if kind == "mol" else DGNNodeNet(dict(common, in_dim=3, n_classes=2))
    sd = {k.split("sd::", 1)[1]: _t(v) for k, v in g.items() if k.startswith(f"{case}/sd::")}
    return net, sd, kind


def _inputs(g, case):
    kind = str(g[f"{case}/cfg"][0])
    idx = g["atoms"] if kind == "mol" else g["feats"]
    K = int(g["pos_enc_dim"])
    return idx, g["eig"][:, 1:K + 1], g[f"{case}/sd::embedding_h.weight"], g[f"{case}/sd::embedding_pos_enc.weight"], \
        g[f"{case}/sd::embedding_pos_enc.bias"]


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_fixture(golden, case):
    g = golden("g18_pos_enc_nets")
    idx, pe, table, w, b = _inputs(g, case)
    h32, h64 = iso.input_stage(idx, [table], pe, w, b, np.float32), iso.input_stage(idx, [table], pe, w, b, np.float64)
    assert h32.dtype == np.float32
    check_reduced(_t(h32), _t(g[f"{case}/h0"]), _t(h64), f"G18 {case} h0")
    up = g[f"{case}/g_h0"]
    (t32,), w32, b32 = iso.input_stage_grads(idx, [table.shape[0]], pe, up, np.float32)
    (t64,), w64, b64 = iso.input_stage_grads(idx, [table.shape[0]], pe, up, np.float64)
    assert t32.tobytes() == g[f"{case}/gp::embedding_h.weight"].tobytes()           # torch's row order, kept
    np.testing.assert_allclose(t64, g[f"{case}/gp::embedding_h.weight"], rtol=1e-5, atol=1e-6)
    scale = float(np.abs(up).max())
    check_reduced(_t(w32), _t(g[f"{case}/gp::embedding_pos_enc.weight"]), _t(w64), f"G18 {case} dW", upstream_scale=scale)
    check_reduced(_t(b32), _t(g[f"{case}/gp::embedding_pos_enc.bias"]), _t(b64), f"G18 {case} db", upstream_scale=scale)


@pytest.mark.parametrize("case", ["zinc_towers", "zinc_simple"])
def test_masked_l1_restatement_reproduces_the_fixture(golden, case):
    g = golden("g18_pos_enc_nets")
    scores, targets = g[f"{case}/scores"], g["targets"]
    l32, g32 = iso.masked_l1(scores, targets, np.float32)
    l64, g64 = iso.masked_l1(scores, targets, np.float64)
    check_reduced(_t(np.array([l32])), _t(g[f"{case}/loss"].reshape(1)), _t(np.array([l64])), f"G18 {case} loss")
    ref = torch.from_numpy(scores.copy()).requires_grad_(True)
    torch.nn.L1Loss()(ref, _t(targets)).backward()
    assert g32.tobytes() == ref.grad.numpy().tobytes()                               # sign / count: no order to keep
    # NaN targets: the mean over the others, zero gradient at the masked entries
    t_nan = targets.copy()
    t_nan[::3] = np.nan
    keep = ~np.isnan(t_nan[:, 0])
    lm, gm = iso.masked_l1(scores, t_nan, np.float64)
    assert abs(lm - np.abs(scores[keep].astype(np.float64) - t_nan[keep]).mean()) <= 1e-12 and bool((gm[~keep] == 0).all())
    ln, gn = iso.masked_l1(scores, np.full_like(targets, np.nan), np.float32)
    assert np.isnan(ln) and bool((gn == 0).all())


@pytest.mark.parametrize("case", CASES)
def test_state_dict_keys_with_pos_enc(golden, case):
    g = golden("g18_pos_enc_nets")
    net, sd, _ = pos_enc_net(g, case, "cpu")
    assert set(sd) == set(net.state_dict()), set(sd) ^ set(net.state_dict())
    assert "embedding_pos_enc.weight" in sd and tuple(sd["embedding_pos_enc.weight"].shape) == (20, 3)
    net.load_state_dict(sd, strict=True)


def test_captured_steps_refusals():
    from dgn_amd import hipgraph
    names_pos_enc = lambda cls: any("pos_enc_dim" in why for _, why in cls._REFUSED)
    assert not names_pos_enc(hipgraph.CapturedNetStep) and not names_pos_enc(hipgraph.CapturedNodeStep)
    assert not names_pos_enc(hipgraph.CapturedSuperpixelStep)
    assert names_pos_enc(hipgraph.CapturedMolStep)


def test_header_declares_the_new_entry_points():
    from dgn_amd import _lib
    assert _lib._abi.constants["DGN_NODE_INPUT_MAX_K"] == 40 and _lib.ABI_VERSION >= 36
    protos = _lib._abi.prototypes
    for name, n_args in (("dgn_node_input_supported", 4), ("dgn_node_input_forward", 15), ("dgn_node_input_backward_workspace_bytes", 5),
                         ("dgn_node_input_backward", 17), ("dgn_masked_mae_workspace_bytes", 2), ("dgn_masked_mae_forward", 12),
                         ("dgn_masked_mae_backward", 8)):
        assert name in protos and len(protos[name][1]) == n_args, name
    from dgn_amd import ops
    assert ops.NODE_INPUT_MAX_K == 40 and callable(ops.node_input) and callable(ops.masked_l1_loss) and callable(ops.node_input_supported)
