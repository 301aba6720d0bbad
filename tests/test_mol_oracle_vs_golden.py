"""The CPU restatement of the OGB molecule nets' encoders, loss and metrics (tests/mol_oracle.py) against fixtures G13 / G14 -- the
reference's own nets, the reference loop's masking lines in front of ``BCEWithLogitsLoss`` in fp32 and fp64, scikit-learn's metrics under
ogb's evaluator rule -- plus what needs no GPU of the new code: the ``state_dict`` layout of ``DGNHIVNet`` / ``DGNPCBANet``, the device-op
metrics (they run on CPU tensors too), the bond encoder's combined table, and the host-side argument checks of the entry points.

Tolerances: the encoder is a fixed sequence of fp32 adds: bit-equal.  Loss and gradient at rtol 1e-5 / atol 1e-6 against the fp32 results
(what tests/test_node_ce_oracle_vs_golden.py uses where a restatement in another op order meets a float32 fixture) and at rtol 1e-12 /
atol 1e-14 against the fp64 ones.  The metrics are rank statistics, exact up to the fp64 rounding of a mean: 1e-9."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mol_oracle as mo


def _cases(g):
    return [str(c) for c in g["cases"]]


def mol_net_params(cfg, device, L=3):
    """The constructor dictionary of a G13 case from its ``cfg`` strings."""
    which, type_net, hidden, aggs, scalers, edge_feat, edge_dim, pos_enc_dim, virtual_node = [str(x) for x in cfg]
    p = dict(hidden_dim=int(hidden), out_dim=int(hidden), in_feat_dropout=0.0, dropout=0.0, L=L, type_net=type_net, readout="mean", graph_norm=True,
             batch_norm=True, aggregators=aggs, scalers=scalers, avg_d={"log": torch.tensor(1.1)}, residual=True, pretrans_layers=1,
             posttrans_layers=1, device=device, edge_feat=bool(int(edge_feat)), edge_dim=int(edge_dim))
    if which == "hiv":
        p["pos_enc_dim"] = int(pos_enc_dim)
    else:
        p.update(towers=5, virtual_node=virtual_node, decreasing_dim=True)
    return which, p


def mol_state_dict(g, case):
    return {k.split("sd::", 1)[1]: torch.from_numpy(np.asarray(g[k])) for k in g.files if k.startswith(f"{case}/sd::")}


def test_fixture_shapes_and_versions(golden):
    g13, g14 = golden("g13_mol_nets"), golden("g14_mol_loss_metrics")
    assert _cases(g13) == ["hiv_simple", "pcba_towers_vn", "hiv_complex_edge"]
    assert str(g14["sklearn_version"]) == "1.7.2" and len(_cases(g14)) == 10
    lab = g13["pcba_towers_vn/labels"]
    assert lab.shape == (3, 128) and 0.5 < np.isnan(lab).mean() < 0.7 and bool(np.isnan(lab).all(0).any())
    atoms, dims = g13["atoms"], g13["atom_dims"]
    assert atoms.shape[1] == 9 and bool((atoms >= 0).all()) and bool((atoms < dims).all())
    for c in range(9):                                          # skewed: one value carries most of every column
        assert np.bincount(atoms[:, c]).max() >= 0.6 * len(atoms)
    shapes = {tuple(g14[f"{n}/scores"].shape) for n in _cases(g14)}
    assert shapes == {(1, 1), (63, 1), (64, 1), (65, 128), (300, 128)}


def test_encoder_restatement_is_bit_equal_to_the_reference(golden):
    g = golden("g13_mol_nets")
    atoms, bonds = torch.from_numpy(g["atoms"]), torch.from_numpy(g["bonds"])
    for case in _cases(g):
        sd = mol_state_dict(g, case)
        w = [sd[f"embedding_h.atom_embedding_list.{i}.weight"] for i in range(9)]
        assert mo.encoder_sum(w, atoms).numpy().tobytes() == g[f"{case}/h0"].tobytes(), case
        if f"{case}/e0" in g.files:
            w = [sd[f"embedding_e.bond_embedding_list.{i}.weight"] for i in range(3)]
            assert mo.encoder_sum(w, bonds).numpy().tobytes() == g[f"{case}/e0"].tobytes(), case


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_loss_restatement_vs_reference_fixture(golden, dtype):
    g = golden("g14_mol_loss_metrics")
    tag, rtol, atol = ("32", 1e-5, 1e-6) if dtype == torch.float32 else ("64", 1e-12, 1e-14)
    for name in _cases(g):
        scores, labels = torch.from_numpy(g[f"{name}/scores"]).to(dtype), torch.from_numpy(g[f"{name}/labels"])
        loss, grad = mo.masked_bce(scores, labels)
        assert loss.dtype == dtype and grad.dtype == dtype
        ref = float(g[f"{name}/loss{tag}"])
        if np.isnan(ref):
            assert name.startswith("allnan") and bool(torch.isnan(loss)) and bool((grad == 0).all())
            continue
        np.testing.assert_allclose(float(loss), ref, rtol=rtol, atol=atol, err_msg=name)
        assert bool(torch.isfinite(grad).all()) and bool((grad[torch.isnan(labels)] == 0).all()), name
        if f"{name}/grad{tag}" in g.files:
            np.testing.assert_allclose(grad.numpy(), g[f"{name}/grad{tag}"], rtol=rtol, atol=atol, err_msg=name)


def test_metric_restatements_and_device_op_metrics_vs_scikit_learn(golden):
    from dgn_amd.nets import ap_ogb, rocauc_ogb
    g = golden("g14_mol_loss_metrics")
    n_scored = 0
    for name in _cases(g):
        scores, labels = g[f"{name}/scores"], g[f"{name}/labels"]
        ts, tl = torch.from_numpy(scores), torch.from_numpy(labels)
        for key, restated, op in (("rocauc", mo.rocauc, rocauc_ogb), ("ap", mo.average_precision, ap_ogb)):
            ref, mine = float(g[f"{name}/{key}"]), op(ts, tl)
            assert mine.dim() == 0 and mine.dtype == torch.float64
            if np.isnan(ref):                                     # no task with a positive and a negative: ogb raises, nan here
                assert np.isnan(restated(scores, labels)) and bool(torch.isnan(mine)), (name, key)
                continue
            n_scored += 1
            assert abs(restated(scores, labels) - ref) <= 1e-9, (name, key)
            assert abs(float(mine) - ref) <= 1e-9, (name, key, float(mine), ref)
    assert n_scored == 16
    # 1-D scores / labels are one task
    s, y = torch.from_numpy(g["ties_g63_t1/scores"]), torch.from_numpy(g["ties_g63_t1/labels"])
    assert float(rocauc_ogb(s[:, 0], y[:, 0])) == float(rocauc_ogb(s, y)) and float(ap_ogb(s[:, 0], y[:, 0])) == float(ap_ogb(s, y))
    assert bool(torch.isnan(rocauc_ogb(torch.zeros(0, 3), torch.zeros(0, 3))))


def test_mol_net_state_dict_layout_matches_reference(golden):
    from dgn_amd.nets import DGNHIVNet, DGNPCBANet
    g = golden("g13_mol_nets")
    for case in _cases(g):
        which, params = mol_net_params(g[f"{case}/cfg"], "cpu")
        net = (DGNHIVNet if which == "hiv" else DGNPCBANet)(params)
        sd = mol_state_dict(g, case)
        assert set(sd) == set(net.state_dict()), (case, set(sd) ^ set(net.state_dict()))
        assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}, case
        net.load_state_dict(sd, strict=True)
    assert any(k.startswith("virtual_node_layers.") for k in mol_state_dict(g, "pcba_towers_vn"))
    assert "embedding_pos_enc.weight" in mol_state_dict(g, "hiv_simple")


def test_encoders_init_dims_and_combined_bond_table(golden):
    from dgn_amd.nets import OGB_ATOM_DIMS, OGB_BOND_DIMS, AtomEncoder, BondEncoder
    g = golden("g13_mol_nets")
    assert OGB_ATOM_DIMS == g["atom_dims"].tolist() and OGB_BOND_DIMS == g["bond_dims"].tolist()
    torch.manual_seed(0)
    enc = AtomEncoder(16)
    assert list(enc.state_dict()) == [f"atom_embedding_list.{i}.weight" for i in range(9)]
    for w, d in zip(enc.weights, OGB_ATOM_DIMS):
        bound = (6.0 / (d + 16)) ** 0.5                           # xavier-uniform
        assert tuple(w.shape) == (d, 16) and float(w.detach().abs().max()) <= bound and float(w.detach().abs().max()) > 0.5 * bound
    other = AtomEncoder(16, dims=[119, 5, 12, 12, 10, 6, 6, 2, 2])         # a release with five chirality values
    assert tuple(other.atom_embedding_list[1].weight.shape) == (5, 16)
    bond = BondEncoder(6)
    assert list(bond.state_dict()) == [f"bond_embedding_list.{i}.weight" for i in range(3)]
    e = torch.from_numpy(g["bonds"])
    table, types = bond.combined_table(), bond.combined_types(e)
    assert tuple(table.shape) == (60, 6) and int(types.min()) >= 0 and int(types.max()) < 60
    assert torch.equal(table[types], mo.encoder_sum(bond.weights, e))        # the same adds in the same order
    (table[types] * torch.arange(6.0)).sum().backward()
    for w, gw in zip(bond.weights, mo.encoder_grads([w.detach() for w in bond.weights], e, torch.arange(6.0).expand(len(e), 6))):
        np.testing.assert_allclose(w.grad.numpy(), gw.numpy(), rtol=1e-5, atol=1e-5)
    bad = e.clone()
    bad[0, 1], bad[1, 0] = 99, -3                                 # out of range: clamped into the table, and validate() raises
    t_bad = bond.combined_types(bad)
    assert int(t_bad.min()) >= 0 and int(t_bad.max()) < 60 and torch.equal(t_bad[2:], types[2:])
    with pytest.raises(IndexError):
        bond.validate(bad)
    bond.validate(e)


@pytest.fixture(scope="module")
def lib():
    from dgn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_mol_io_entry_points_validate_before_any_device_work(lib):
    """dgn_multi_embedding_* / dgn_masked_bce_*: column count, table rows, nulls, the int32 row range, row strides, the LDS budget and the
    workspace size are host-side checks: an error code and a message, no kernel launched (runs without a GPU)."""
    err = lambda: lib.dgn_last_error().decode()
    a = 1 << 12                                                  # dummy aligned pointer, never dereferenced
    i32 = lambda v: (C.c_int32 * len(v))(*v)
    ptrs = lambda n, v=a: (C.c_void_p * n)(*([v] * n))
    atom = [119, 4, 12, 12, 10, 6, 6, 2, 2]
    sup = lib.dgn_multi_embedding_supported
    assert sup(9, i32(atom), 70) == 1 and sup(9, i32(atom), 128) == 1 and sup(9, i32(atom), 236) == 1 and sup(9, i32(atom), 237) == 0
    assert sup(17, i32([2] * 17), 8) == 0 and sup(0, i32([1]), 8) == 0 and sup(1, i32([0]), 8) == 0 and sup(1, i32([40960]), 1) == 1
    need = lib.dgn_multi_embedding_backward_workspace_bytes(3000, 9, i32(atom), 70)
    assert need == 47 * 173 * 70 * 4 and lib.dgn_multi_embedding_backward_workspace_bytes(3000, 9, i32(atom), 237) == 0
    assert lib.dgn_multi_embedding_backward_workspace_bytes(10 ** 6, 9, i32(atom), 70) == 256 * 173 * 70 * 4
    fwd = lib.dgn_multi_embedding_forward
    assert fwd(10, 17, 8, a, 17, ptrs(17), i32([2] * 17), a, 8, None) == -1 and "n_cols" in err()
    assert fwd(10, 3, 8, None, 3, ptrs(3), i32([5, 6, 2]), a, 8, None) == -1 and "null" in err()
    assert fwd(10, 3, 8, a, 3, ptrs(3, None), i32([5, 6, 2]), a, 8, None) == -1 and "null table" in err()
    assert fwd(10, 3, 8, a, 2, ptrs(3), i32([5, 6, 2]), a, 8, None) == -1 and "stride" in err()
    assert fwd(10, 3, 8, a, 3, ptrs(3), i32([5, 6, 2]), a, 7, None) == -1 and "stride" in err()
    assert fwd(2 ** 31, 3, 8, a, 3, ptrs(3), i32([5, 6, 2]), a, 8, None) == -1 and "int32" in err()
    assert fwd(0, 3, 8, None, 3, ptrs(3), i32([5, 6, 2]), None, 8, None) == 0                     # no rows: nothing to do
    bwd = lib.dgn_multi_embedding_backward
    assert bwd(3000, 9, 237, a, 9, i32(atom), a, 237, ptrs(9), a, 1 << 30, None) == -1 and "LDS" in err()
    assert bwd(3000, 9, 70, a, 9, i32(atom), a, 70, ptrs(9), a, need - 1, None) == -1 and "workspace" in err()
    assert bwd(3000, 9, 70, a, 9, i32(atom), a, 70, ptrs(9), None, need, None) == -1 and "workspace" in err()
    assert bwd(3000, 9, 70, a, 9, i32(atom), None, 70, ptrs(9), a, need, None) == -1 and "null" in err()
    assert bwd(3000, 9, 70, a, 9, i32(atom), a, 69, ptrs(9), a, need, None) == -1 and "stride" in err()
    assert bwd(3000, 9, 70, a, 9, i32(atom), a, 70, ptrs(9, None), a, need, None) == -1 and "null gradient table" in err()
    need = lib.dgn_masked_bce_workspace_bytes(300, 128)
    assert need > 0 and lib.dgn_masked_bce_workspace_bytes(300, 0) == 0 and lib.dgn_masked_bce_workspace_bytes(2 ** 31, 1) == 0
    f = lib.dgn_masked_bce_forward
    assert f(300, 0, a, 0, a, 0, a, None, 0, a, need, None) == -1 and "n_tasks" in err()
    assert f(300, 128, None, 128, a, 128, a, None, 0, a, need, None) == -1 and "null" in err()
    assert f(300, 128, a, 128, a, 128, None, None, 0, a, need, None) == -1 and "null loss" in err()
    assert f(300, 128, a, 127, a, 128, a, None, 0, a, need, None) == -1 and "stride" in err()
    assert f(300, 128, a, 128, a, 128, a, a, 100, a, need, None) == -1 and "stride" in err()
    assert f(300, 128, a, 128, a, 128, a, None, 0, a, need - 1, None) == -1 and "workspace" in err()
    assert f(300, 128, a, 128, a, 128, a, None, 0, a + 4, need, None) == -1 and "workspace" in err()
    b = lib.dgn_masked_bce_backward
    assert b(300, 128, None, 128, a, a, 128, None) == -1 and "null" in err()
    assert b(300, 128, a, 128, a, a, 127, None) == -1 and "stride" in err()
    assert b(0, 128, None, 128, None, None, 128, None) == 0


def test_public_names_and_no_cpu_path():
    import dgn_amd
    from dgn_amd import hipgraph, nets, ops
    for name in ("multi_embedding", "masked_bce_with_logits"):
        assert getattr(dgn_amd, name) is getattr(ops, name)
    for name in ("AtomEncoder", "BondEncoder", "DGNHIVNet", "DGNPCBANet", "rocauc_ogb", "ap_ogb"):
        assert getattr(dgn_amd, name) is getattr(nets, name)
    assert issubclass(hipgraph.CapturedMolStep, hipgraph.CapturedNetStep)
    with pytest.raises(dgn_amd._lib.DgnError):
        ops.masked_bce_with_logits(torch.zeros(4, 2), torch.zeros(4, 2))
    with pytest.raises(dgn_amd._lib.DgnError):
        ops.multi_embedding([torch.zeros(3, 4)], torch.zeros(5, 1, dtype=torch.int64))
