"""The CPU restatement of the node-classification tail (tests/node_ce_oracle.py) against fixture G12 -- the reference's own
``DGNNet.loss`` (nets/SBMs_node_classification/dgn_net.py:67-81) and ``accuracy_SBM`` (train/metrics.py:37-54) -- and the host-side
argument checks of the ``dgn_node_ce_*`` entry points.  No GPU.

Tolerances: loss and gradient at rtol 1e-5 / atol 1e-6, what tests/test_readout_oracle_vs_golden.py uses where a restatement in another
op order meets a float32 fixture; the accuracy within 1e-4 percent points (the reference rounds each class ratio to float32 once, 6e-8
relative of at most 100; one node's worth is 100 / count >= 0.03 at these sizes)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import node_ce_oracle as nco


def _cases(g):
    return [str(c) for c in g["cases"]]


def _case(g, name, dtype):
    return (torch.from_numpy(g[f"{name}/scores"]).to(dtype), torch.from_numpy(g[f"{name}/labels"]), int(g[f"{name}/C"]))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_restatement_vs_reference_fixture(golden, dtype):
    g = golden("g12_node_ce")
    names = _cases(g)
    assert len(names) == 8
    n_finite = 0
    for name in names:
        scores, labels, n_classes = _case(g, name, dtype)
        loss, grad = nco.loss_and_grad(scores, labels, n_classes)
        assert loss.dtype == dtype and grad.dtype == dtype
        ref_loss = float(g[f"{name}/loss"])
        if np.isnan(ref_loss):                                    # one class only: 0 / 0 in the reference and here
            assert name.startswith("single") and bool(torch.isnan(loss)) and bool(torch.isnan(grad).all())
            assert f"{name}/acc" not in g.files
            continue
        n_finite += 1
        np.testing.assert_allclose(float(loss), ref_loss, rtol=1e-5, atol=1e-6, err_msg=name)
        np.testing.assert_allclose(grad.numpy(), g[f"{name}/grad"], rtol=1e-5, atol=1e-6, err_msg=name)
        assert nco.prediction_gap(scores, labels) >= 1e-4, name       # (the fixture's condition: both precisions see the same predictions)
        cm = nco.confusion_matrix(scores, labels, n_classes)
        assert int(cm.sum()) == labels.numel() and torch.equal(cm.sum(1), nco.class_counts(labels, n_classes))
        assert abs(nco.accuracy(cm) - float(g[f"{name}/acc"])) <= 1e-4, (name, nco.accuracy(cm), float(g[f"{name}/acc"]))
    assert n_finite == 7


def test_missing_classes_have_zero_weight(golden):
    g = golden("g12_node_ce")
    scores, labels, n_classes = _case(g, "missing_n500_c6", torch.float64)
    w = nco.class_weights(labels, n_classes)
    assert w[1] == 0 and w[4] == 0 and bool((w[[0, 2, 3, 5]] > 0).all())
    _, grad = nco.loss_and_grad(scores, labels, n_classes)
    assert bool(torch.isfinite(grad).all())


def test_padding_rows_change_nothing_bit_for_bit(golden):
    g = golden("g12_node_ce")
    gen = torch.Generator().manual_seed(0)
    for name in _cases(g):
        scores, labels, n_classes = _case(g, name, torch.float64)
        N = labels.numel()
        pad = 7
        # padding rows in front, in the middle and behind, with arbitrary scores
        keep = torch.cat([torch.arange(pad, pad + N // 2), torch.arange(2 * pad + N // 2, 2 * pad + N)])
        scores_p = 5.0 * torch.randn(N + 3 * pad, n_classes, generator=gen, dtype=torch.float64)
        labels_p = torch.full((N + 3 * pad,), -1, dtype=torch.int64)
        scores_p[keep], labels_p[keep] = scores, labels
        loss, grad = nco.loss_and_grad(scores, labels, n_classes)
        loss_p, grad_p = nco.loss_and_grad(scores_p, labels_p, n_classes)
        assert loss.numpy().tobytes() == loss_p.numpy().tobytes(), name
        assert grad.numpy().tobytes() == grad_p[keep].numpy().tobytes(), name
        mask = torch.ones(N + 3 * pad, dtype=torch.bool)
        mask[keep] = False
        assert bool((grad_p[mask] == 0).all()), name
        assert torch.equal(nco.confusion_matrix(scores, labels, n_classes), nco.confusion_matrix(scores_p, labels_p, n_classes)), name
    loss, grad = nco.loss_and_grad(torch.randn(4, 3, dtype=torch.float64), torch.full((4,), -1), 3)       # no valid row at all
    assert float(loss) == 0.0 and bool((grad == 0).all())


def test_accuracy_without_a_hit_is_zero():
    assert nco.accuracy(torch.tensor([[0, 3], [2, 0]])) == 0.0
    assert nco.accuracy(torch.tensor([[2, 2], [0, 0]])) == 100.0 * 0.5 / 1          # class 1 absent from the labels


@pytest.fixture(scope="module")
def lib():
    from dgn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_node_ce_entry_points_validate_before_any_device_work(lib):
    """dgn_node_ce_*: class-count range, nulls, the int32 row range, row strides and the workspace size are host-side checks: an error
    code and a message, no kernel launched (runs without a GPU)."""
    err = lambda: lib.dgn_last_error().decode()
    a = 1 << 12                                                  # dummy aligned pointer, never dereferenced
    need = lib.dgn_node_ce_workspace_bytes(1000, 6)
    assert need > 0 and lib.dgn_node_ce_workspace_bytes(1000, 33) == 0 and lib.dgn_node_ce_workspace_bytes(2 ** 31, 6) == 0
    assert lib.dgn_node_ce_workspace_bytes(300001, 32) >= lib.dgn_node_ce_workspace_bytes(300001, 2) > 0
    fwd = lib.dgn_node_ce_forward
    assert fwd(1000, 33, a, 33, a, a, None, None, 0, None, a, 1 << 30, None) == -1 and "n_classes" in err()
    assert fwd(1000, 0, a, 1, a, a, None, None, 0, None, a, 1 << 30, None) == -1 and "n_classes" in err()
    assert fwd(1000, 6, None, 6, a, a, None, None, 0, None, a, need, None) == -1 and "null" in err()
    assert fwd(1000, 6, a, 6, None, a, None, None, 0, None, a, need, None) == -1 and "null" in err()
    assert fwd(1000, 6, a, 6, a, None, None, None, 0, None, a, need, None) == -1 and "null" in err()
    assert fwd(2 ** 31, 6, a, 6, a, a, None, None, 0, None, a, 1 << 40, None) == -1 and "int32" in err()
    assert fwd(1000, 6, a, 5, a, a, None, None, 0, None, a, need, None) == -1 and "stride" in err()
    assert fwd(1000, 6, a, 6, a, a, None, a, 4, None, a, need, None) == -1 and "stride" in err()
    assert fwd(1000, 6, a, 6, a, a, None, None, 0, None, a, need - 1, None) == -1 and "workspace" in err()
    assert fwd(1000, 6, a, 6, a, a, None, None, 0, None, None, need, None) == -1 and "workspace" in err()
    assert fwd(1000, 6, a, 6, a, a, None, None, 0, None, a + 4, need, None) == -1 and "workspace" in err()
    bwd = lib.dgn_node_ce_backward
    assert bwd(1000, 33, a, 33, a, a, 33, None) == -1 and "n_classes" in err()
    assert bwd(1000, 6, None, 6, a, a, 6, None) == -1 and "null" in err()
    assert bwd(1000, 6, a, 6, a, a, 5, None) == -1 and "stride" in err()
    assert bwd(0, 6, None, 6, None, None, 6, None) == 0                                 # no rows: nothing to do


def test_public_names():
    import dgn_amd
    from dgn_amd import hipgraph, nets, ops
    assert dgn_amd.DGNNodeNet is nets.DGNNodeNet and dgn_amd.balanced_cross_entropy is ops.balanced_cross_entropy
    assert dgn_amd.accuracy_sbm is nets.accuracy_sbm and hasattr(hipgraph, "CapturedNodeStep")
    cm = torch.tensor([[5, 1, 0], [2, 0, 2], [0, 0, 0]])
    acc = nets.accuracy_sbm(cm)
    assert acc.dim() == 0 and abs(float(acc) - nco.accuracy(cm)) < 1e-12 and abs(float(acc) - 100.0 * (5 / 6) / 1) < 1e-9
    assert float(nets.accuracy_sbm(torch.zeros(3, 3, dtype=torch.int64))) == 0.0
    with pytest.raises(dgn_amd._lib.DgnError):                     # no CPU path
        ops.balanced_cross_entropy(torch.zeros(4, 2), torch.zeros(4, dtype=torch.int64), 2)


def test_node_net_state_dict_layout_matches_reference(golden):
    from dgn_amd.nets import DGNNodeNet
    g = golden("g11_node_net")
    for case in [str(c) for c in g["cases"]]:
        type_net, hidden, aggs, scalers, n_classes = [str(x) for x in g[f"{case}/cfg"]]
        net = DGNNodeNet(node_net_params(type_net, int(hidden), aggs, scalers, int(n_classes), "cpu"))
        ref = {k.split("sd::", 1)[1]: tuple(g[k].shape) for k in g.files if k.startswith(f"{case}/sd::")}
        assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == ref, case


def node_net_params(type_net, hidden, aggs, scalers, n_classes, device, L=3):
    return dict(in_dim=3, hidden_dim=hidden, out_dim=hidden, n_classes=n_classes, in_feat_dropout=0.0, dropout=0.0, L=L, type_net=type_net,
                pos_enc_dim=0, readout="mean", graph_norm=True, batch_norm=True, aggregators=aggs, scalers=scalers,
                avg_d={"log": torch.tensor(1.1)}, residual=True, edge_feat=False, edge_dim=0, pretrans_layers=1, posttrans_layers=1, device=device)
