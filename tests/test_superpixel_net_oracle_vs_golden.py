"""The CPU restatement of the superpixel net's loss tail (tests/superpixel_net_oracle.py) against fixture G17 -- the reference's own
``DGNNet.loss`` (nets/superpixels_graph_classification/dgn_net.py:75-78) and ``accuracy_MNIST_CIFAR`` (train/metrics.py:25-28) --, the
``state_dict`` layout of ``dgn_amd.nets.DGNSuperpixelNet`` against fixture G16, and the host-side argument checks of the
``dgn_feat_embed_*`` / ``dgn_class_ce_*`` entry points.  No GPU.

Tolerances: loss and gradient at rtol 1e-5 / atol 1e-6, as tests/test_node_ce_oracle_vs_golden.py uses where a restatement in another op
order meets a float32 fixture; the hit count is exact (outside the tie case the fixture's top-two gaps are >= 1e-4 in both precisions;
the tie case's equal scores are equal in both)."""
import os

import numpy as np
import pytest
import torch

import superpixel_net_oracle as spo


def _cases(g):
    return [str(c) for c in g["cases"]]


def superpixel_net_params(type_net, hidden, in_dim, aggs, scalers, readout, edge_feat, L=3, n_classes=10, dropout=0.0):
    return dict(in_dim=in_dim, in_dim_edge=1, hidden_dim=hidden, out_dim=hidden, n_classes=n_classes, in_feat_dropout=0.0, dropout=dropout, L=L,
                type_net=type_net, readout=readout, graph_norm=True, batch_norm=True, residual=True, aggregators=aggs, scalers=scalers,
                avg_d={"log": torch.tensor(1.1)}, edge_feat=edge_feat, edge_dim=6 if edge_feat else 0, pretrans_layers=1, posttrans_layers=1)


def fixture_net_params(g, case):
    type_net, hidden, in_dim, aggs, scalers, readout, edge_feat = [str(x) for x in g[f"{case}/cfg"]]
    return superpixel_net_params(type_net, int(hidden), int(in_dim), aggs, scalers, readout, bool(int(edge_feat)))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_restatement_vs_reference_fixture(golden, dtype):
    g = golden("g17_class_ce")
    names = _cases(g)
    assert len(names) == 10 and "ties" in names and "big_g64_c10" in names
    for name in names:
        scores, labels = torch.from_numpy(g[f"{name}/scores"]).to(dtype), torch.from_numpy(g[f"{name}/labels"])
        loss, grad = spo.loss_and_grad(scores, labels)
        assert loss.dtype == dtype and grad.dtype == dtype
        np.testing.assert_allclose(float(loss), float(g[f"{name}/loss"]), rtol=1e-5, atol=1e-6, err_msg=name)
        np.testing.assert_allclose(grad.numpy(), g[f"{name}/grad"], rtol=1e-5, atol=1e-6, err_msg=name)
        assert spo.hits(scores, labels) == int(g[f"{name}/hits"]), name
        assert name == "ties" or spo.top_gap(scores, labels) >= 1e-4, name      # (the fixture's condition: both precisions see the same predictions)
    assert float(np.abs(g["big_g64_c10/scores"]).min()) > 70.0


def test_tie_case_follows_the_first_maximum_rule(golden):
    g = golden("g17_class_ce")
    scores, labels = torch.from_numpy(g["ties/scores"]), torch.from_numpy(g["ties/labels"])
    top = scores.max(dim=1, keepdim=True).values
    assert bool(((scores == top).sum(1) == 2).all())                       # every row has an exact two-way tie at the top
    tied_label = scores.gather(1, labels[:, None])[:, 0] == top[:, 0]
    assert tied_label.tolist() == [False] * 4 + [True] * 8                  # rows 0-3: the tie does not involve the label
    pred = spo.predictions(scores)
    assert (pred == labels).tolist() == [False] * 4 + [True] * 4 + [False] * 4      # label first: hit; label second: miss
    assert torch.equal(pred, scores.argmax(dim=1)) and int(g["ties/hits"]) == 4


def test_padding_rows_change_nothing_bit_for_bit(golden):
    g = golden("g17_class_ce")
    gen = torch.Generator().manual_seed(0)
    for name in _cases(g):
        scores, labels = torch.from_numpy(g[f"{name}/scores"]).double(), torch.from_numpy(g[f"{name}/labels"])
        G, C, pad = labels.numel(), scores.shape[1], 5
        keep = torch.cat([torch.arange(pad, pad + G // 2), torch.arange(2 * pad + G // 2, 2 * pad + G)])
        scores_p = 5.0 * torch.randn(G + 3 * pad, C, generator=gen, dtype=torch.float64)
        labels_p = torch.full((G + 3 * pad,), -1, dtype=torch.int64)
        scores_p[keep], labels_p[keep] = scores, labels
        loss, grad = spo.loss_and_grad(scores, labels)
        loss_p, grad_p = spo.loss_and_grad(scores_p, labels_p)
        assert loss.numpy().tobytes() == loss_p.numpy().tobytes(), name
        assert grad.numpy().tobytes() == grad_p[keep].numpy().tobytes(), name
        mask = torch.ones(G + 3 * pad, dtype=torch.bool)
        mask[keep] = False
        assert bool((grad_p[mask] == 0).all()) and spo.hits(scores_p, labels_p) == spo.hits(scores, labels), name
    loss, grad = spo.loss_and_grad(torch.randn(4, 3, dtype=torch.float64), torch.full((4,), -1))       # no valid row at all
    assert bool(torch.isnan(loss)) and bool((grad == 0).all()) and spo.hits(torch.randn(4, 3), torch.full((4,), -1)) == 0


def test_superpixel_net_state_dict_layout_matches_reference(golden):
    from dgn_amd.nets import DGNSuperpixelNet
    g = golden("g16_superpixel_net")
    cases = _cases(g)
    assert cases == ["simple", "towers", "complex"]
    for case in cases:
        net = DGNSuperpixelNet(fixture_net_params(g, case))
        sd = {k.split("sd::", 1)[1]: torch.from_numpy(np.asarray(g[k])) for k in g.files if k.startswith(f"{case}/sd::")}
        assert set(sd) == set(net.state_dict()), (case, set(sd) ^ set(net.state_dict()))
        net.load_state_dict(sd, strict=True)
        assert ("embedding_e.weight" in sd) == (case == "complex")
        assert isinstance(net.embedding_h, torch.nn.Linear) and net.embedding_h.in_features == int(g[f"{case}/cfg"][2])


def test_cpu_loss_is_the_reference_call(golden):
    """``loss`` on CPU tensors is ``F.cross_entropy``: the fixture's own numbers; ``accuracy_mnist_cifar`` is the reference's count."""
    from dgn_amd.nets import DGNSuperpixelNet, accuracy_mnist_cifar
    g16, g17 = golden("g16_superpixel_net"), golden("g17_class_ce")
    net = DGNSuperpixelNet(fixture_net_params(g16, "simple"))
    for name in _cases(g17):
        scores, labels = torch.from_numpy(g17[f"{name}/scores"]), torch.from_numpy(g17[f"{name}/labels"])
        loss, hits = net.loss(scores, labels, hits=True)
        np.testing.assert_allclose(float(loss), float(g17[f"{name}/loss"]), rtol=1e-6, err_msg=name)      # (the same op; the thread count may differ)
        assert net.loss(scores, labels).item() == loss.item()
        assert hits.dim() == 0 and hits.dtype == torch.int64 and int(hits) == int(g17[f"{name}/hits"]) == int(accuracy_mnist_cifar(scores, labels))


@pytest.fixture(scope="module")
def lib():
    from dgn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_graph_cls_entry_points_validate_before_any_device_work(lib):
    """dgn_feat_embed_* / dgn_class_ce_*: width and class-count ranges, nulls, the int32 row range, row strides and the workspace size are
    host-side checks: an error code and a message, no kernel launched (runs without a GPU); no row: success, nothing launched."""
    err = lambda: lib.dgn_last_error().decode()
    a = 1 << 12                                                  # dummy aligned pointer, never dereferenced
    assert lib.dgn_feat_embed_supported(5, 65) == 1 and lib.dgn_feat_embed_supported(1, 1) == 1 and lib.dgn_feat_embed_supported(8, 160) == 1
    assert lib.dgn_feat_embed_supported(9, 65) == 0 and lib.dgn_feat_embed_supported(5, 161) == 0 and lib.dgn_feat_embed_supported(0, 65) == 0
    need = lib.dgn_feat_embed_backward_workspace_bytes(1000, 5, 65)
    assert need >= (1000 // 64) * 6 * 65 * 4 and lib.dgn_feat_embed_backward_workspace_bytes(1000, 9, 65) == 0
    assert lib.dgn_feat_embed_backward_workspace_bytes(2 ** 31, 5, 65) == 0
    fwd = lib.dgn_feat_embed_forward
    assert fwd(10, 9, 65, a, 9, a, a, a, 65, None) == -1 and "k <= 8" in err()
    assert fwd(10, 5, 161, a, 5, a, a, a, 161, None) == -1 and "f_out <= 160" in err()
    assert fwd(10, 5, 65, None, 5, a, a, a, 65, None) == -1 and "null" in err()
    assert fwd(10, 5, 65, a, 4, a, a, a, 65, None) == -1 and "stride" in err()
    assert fwd(10, 5, 65, a, 5, a, a, a, 64, None) == -1 and "stride" in err()
    assert fwd(2 ** 31, 5, 65, a, 5, a, a, a, 65, None) == -1 and "int32" in err()
    assert fwd(0, 5, 65, None, 5, None, None, None, 65, None) == 0                       # no rows: nothing to do
    bwd = lib.dgn_feat_embed_backward
    assert bwd(1000, 5, 65, a, 5, a, 65, a, a, a, need - 1, None) == -1 and "workspace" in err()
    assert bwd(1000, 5, 65, a, 5, a, 65, a, a, None, need, None) == -1 and "workspace" in err()
    assert bwd(1000, 5, 65, a, 5, a, 64, a, a, a, need, None) == -1 and "stride" in err()
    assert bwd(1000, 5, 65, a, 5, a, 65, None, a, a, need, None) == -1 and "null" in err()
    assert bwd(0, 5, 65, None, 5, None, 65, None, None, None, 0, None) == 0
    assert lib.dgn_class_ce_supported(2) == 1 and lib.dgn_class_ce_supported(64) == 1
    assert lib.dgn_class_ce_supported(1) == 0 and lib.dgn_class_ce_supported(65) == 0
    need = lib.dgn_class_ce_workspace_bytes(128, 10)
    assert need > 0 and lib.dgn_class_ce_workspace_bytes(0, 10) > 0 and lib.dgn_class_ce_workspace_bytes(128, 65) == 0
    fwd = lib.dgn_class_ce_forward
    assert fwd(128, 65, a, 65, a, a, None, None, 0, a, 1 << 20, None) == -1 and "n_classes" in err()
    assert fwd(128, 1, a, 1, a, a, None, None, 0, a, 1 << 20, None) == -1 and "n_classes" in err()
    assert fwd(128, 10, None, 10, a, a, None, None, 0, a, need, None) == -1 and "null" in err()
    assert fwd(128, 10, a, 10, None, a, None, None, 0, a, need, None) == -1 and "null" in err()
    assert fwd(128, 10, a, 10, a, None, None, None, 0, a, need, None) == -1 and "null" in err()
    assert fwd(2 ** 31, 10, a, 10, a, a, None, None, 0, a, 1 << 40, None) == -1 and "int32" in err()
    assert fwd(128, 10, a, 9, a, a, None, None, 0, a, need, None) == -1 and "stride" in err()
    assert fwd(128, 10, a, 10, a, a, None, a, 9, a, need, None) == -1 and "stride" in err()
    assert fwd(128, 10, a, 10, a, a, None, None, 0, a, need - 1, None) == -1 and "workspace" in err()
    assert fwd(128, 10, a, 10, a, a, None, None, 0, a + 4, need, None) == -1 and "workspace" in err()
    bwd = lib.dgn_class_ce_backward
    assert bwd(128, 65, a, 65, a, a, 65, None) == -1 and "n_classes" in err()
    assert bwd(128, 10, None, 10, a, a, 10, None) == -1 and "null" in err()
    assert bwd(128, 10, a, 10, a, a, 9, None) == -1 and "stride" in err()
    assert bwd(0, 10, None, 10, None, None, 10, None) == 0                               # no rows: nothing to do


def test_public_names():
    import dgn_amd
    from dgn_amd import hipgraph, nets, ops
    assert dgn_amd.DGNSuperpixelNet is nets.DGNSuperpixelNet and dgn_amd.accuracy_mnist_cifar is nets.accuracy_mnist_cifar
    assert dgn_amd.feature_embedding is ops.feature_embedding and dgn_amd.class_cross_entropy is ops.class_cross_entropy
    assert issubclass(hipgraph.CapturedSuperpixelStep, hipgraph.CapturedNetStep)
    with pytest.raises(dgn_amd._lib.DgnError):                     # no CPU path
        ops.class_cross_entropy(torch.zeros(4, 10), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(dgn_amd._lib.DgnError):
        ops.feature_embedding(torch.zeros(4, 3), torch.zeros(20, 3), None)
    assert not ops.feature_embedding_supported(torch.zeros(4, 3), torch.zeros(20, 3))
