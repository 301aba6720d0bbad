"""The reference's SHIPPED layer configurations, each exactly as its json names it, in front of the oracle on the GPU
(no BASELINE config and no json config may stay without a layer-level oracle test).

* C4 / ogbg-molhiv (configs/molecules_graph_classification_DGN_HIV.json:23-34, PCBA json the same): ``simple``, hidden 70,
  ``mean max min dir1-dx dir1-av``, ``graph_norm = False``, BatchNorm, residual -- with the json's ``identity`` scaler and with
  BASELINE's three PNA scalers (the form bench.py times);
* ZINC json (configs/molecules_graph_regression_DGN_ZINC.json:21-41): ``complex``, hidden **45** (odd), ``mean dir1-dx dir1-av``
  x three scalers, graph norm;
* PATTERN json (configs/SBMs_node_clustering_DGN_PATTERN.json:22-42): ``complex``, hidden **47** (odd), ``mean dir1-dx dir2-dx``
  x three scalers, on SBM-like graphs (dense rows: ~25 in-edges);
both routes of the dense products (this library's kernels / the library GEMM small batches take).
Checked: output, d h, every parameter gradient, BatchNorm running statistics.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _check_grad(a, r32, r64, name, strict=True):
    """the headline test's criterion: within tolerance of the fp32 oracle, or as close to the fp64 oracle as the fp32 oracle is -- counted,
    reported and bounded by parity_util.check; and never far from the fp64 evaluation.  ``strict`` (the BASELINE / shipped-json lists:
    every config test of this module and of test_block_layer_gpu.py): NO entry may need the tensor-wide fp64 clause (DESIGN section 3's
    claim, asserted); lists with ``std`` / ``var`` -- ill-conditioned in the reference's own fp32 arithmetic -- name looser caps."""
    from parity_util import check
    if strict:
        check(a, r32, r64, name, rtol=1e-4, atol=2e-5, max_escape_fraction=0.0)
    else:
        check(a, r32, r64, name, rtol=1e-4, atol=2e-5)
    a, r32 = a.cpu().double(), r32.double()
    scale = max(1.0, float(r64.abs().max()))
    # (a max / min / |.| routing that flips between fp32 and fp64 moves a gradient entry by O(weight): with O(1) weights the fp32
    #  REFERENCE itself is that far from fp64 on a few entries, so the bound carries the reference's own worst error)
    assert float((a - r64).abs().max()) <= 10 * 2e-5 * scale + 4 * float((r32 - r64).abs().max()), f"{name}: not close to the fp64 evaluation"


def _o1_layer(type_net, hidden, aggs, scalers, graph_norm, towers, b):
    """The layer on the CPU with O(1) weights -- the reference's init (gain 1/in_size) makes layer outputs ~1e-3 and hides errors (SURVEY
    appendix B #5) -- and h, cotangent ~ N(0, 1) from a CPU generator: (layer, avg_log, h, cotangent)."""
    import dgn_amd
    N = int(b["num_nodes"])
    avg = float(torch.log(torch.bincount(b["dst"], minlength=N).float() + 1).mean())
    torch.manual_seed(0)
    kw = dict(towers=towers) if type_net == "towers" else {}
    layer = dgn_amd.DGNLayer(hidden, hidden, 0.0, graph_norm, True, aggs, scalers, {"log": torch.tensor(avg)}, type_net, True,
                             edge_features=False, edge_dim=0, **kw).model
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in layer.parameters():
            if p.dim() == 2 and type_net != "towers":
                p.copy_(torch.randn(p.shape, generator=gen) / p.shape[1] ** 0.5)
            else:          # (biases and BatchNorm's affine pair; towers: every parameter, the default init plus N(0, 0.1))
                p.add_(0.1 * torch.randn(p.shape, generator=gen))
    return layer, avg, torch.randn(N, hidden, generator=gen), torch.randn(N, hidden, generator=gen)


def _oracle_of(layer, type_net, aggs, scalers, avg, graph_norm, towers, b, h, ct):
    """``oracle(dtype, keep_graph=False)`` -> (y, [d h] + parameter gradients, parameter names, BatchNorm running statistics, again):
    the oracle's layer step on the layer's state.  With ``keep_graph`` the autograd graph is retained and ``again(cotangent)`` pulls
    another cotangent back through it (the gradient is linear in the cotangent); ``again`` is None otherwise."""
    from oracle import dgn_oracle as orc
    N = int(b["num_nodes"])

    def oracle(dtype, keep_graph=False):
        sd = {k: (v.detach().to(dtype).requires_grad_("running" not in k) if v.dtype.is_floating_point else v.clone())
              for k, v in layer.state_dict().items()}
        names = [k for k, v in sd.items() if v.dtype.is_floating_point and v.requires_grad]
        cfg = dict(aggregators=aggs, scalers=scalers, avg_log=torch.tensor(avg, dtype=dtype), graph_norm=graph_norm, batch_norm=True,
                   residual=True, towers=towers, divide_input=True, edge_features=False)
        hh = h.to(dtype).requires_grad_(True)
        y, stats = orc.layer_forward(type_net, sd, cfg, b["src"], b["dst"], N, b["eig"].to(dtype), hh, None, b["snorm_n"].to(dtype), training=True)
        wrt = [hh] + [sd[k] for k in names]
        again = (lambda c: torch.autograd.grad(y, wrt, c.to(dtype), retain_graph=True)) if keep_graph else None
        return y, torch.autograd.grad(y, wrt, ct.to(dtype), retain_graph=keep_graph), names, stats, again

    return oracle


def _check_running_stats(layer, stats):
    """BatchNorm running statistics of every BatchNorm module against the oracle's; one batch counted."""
    sd = layer.state_dict()
    assert stats and len(stats) == 2 * sum(isinstance(m, torch.nn.BatchNorm1d) for m in layer.modules()), sorted(stats)
    for k, v in stats.items():
        np.testing.assert_allclose(sd[k].cpu().numpy(), v.numpy(), rtol=1e-5, atol=1e-6, err_msg=k)
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1, k


def _layer_vs_oracle(monkeypatch, type_net, F_, aggs, scalers, graph_norm, batch, min_rows, strict=True):
    import dgn_amd
    if min_rows is not None:
        monkeypatch.setattr(dgn_amd.ops, "LINEAR_MIN_ROWS", min_rows)
        monkeypatch.setattr(dgn_amd.ops, "WIDE_MIN_ROWS", min_rows)
        monkeypatch.setattr(dgn_amd.ops, "WHOLE_LAYER_MIN_ROWS", min_rows)      # (1 << 40: the per-op route on the library's GEMMs)
    dev = torch.device("cuda")
    src, dst, N = batch["src"], batch["dst"], int(batch["num_nodes"])
    layer, avg, h, ct = _o1_layer(type_net, F_, aggs, scalers, graph_norm, 1, batch)
    oracle = _oracle_of(layer, type_net, aggs, scalers, avg, graph_norm, 1, batch, h, ct)
    y32, g32, names, stats, _ = oracle(torch.float32)
    y64, g64, _, _, _ = oracle(torch.float64)
    layer = layer.to(dev).train()
    graph = dgn_amd.DGNGraph(src.to(dev), dst.to(dev), N, eig=batch["eig"].to(dev))
    hd = h.to(dev).requires_grad_(True)
    y = layer(graph, hd, None, batch["snorm_n"].to(dev))
    params = dict(layer.named_parameters())
    gd = torch.autograd.grad(y, [hd] + [params[k] for k in names], ct.to(dev))
    from parity_util import check
    check(y, y32, y64, f"{type_net} F={F_} y", rtol=2e-5, atol=2e-5, abs_scale=1.0, max_escape_fraction=0.0)
    for a, r32, r64, k in zip(gd, g32, g64, ["h"] + names):
        _check_grad(a, r32, r64, k, strict=strict)
    _check_running_stats(layer, stats)


ROUTES = pytest.mark.parametrize("min_rows", [0, 1 << 40], ids=["own-kernels", "library-gemm"])


@ROUTES
@pytest.mark.parametrize("scalers", ["identity", "identity amplification attenuation"], ids=["json-identity", "baseline-3-scalers"])
def test_c4_molhiv_simple_layer_vs_oracle(monkeypatch, scalers, min_rows):
    from dgn_amd import synth
    b = synth.molecule_batch(256, seed=41, n_lo=10, n_hi=41, extra_bonds=4.3, eig_dim=4)      # bench.py's c4 generator, 256 graphs
    _layer_vs_oracle(monkeypatch, "simple", 70, "mean max min dir1-dx dir1-av", scalers, False, b, min_rows)


@ROUTES
def test_c1_zinc_simple_hidden75_vs_oracle(monkeypatch, min_rows):
    """BASELINE configs[0] at its OWN width: simple, hidden 75 (odd), mean dir1-dx-no-abs x the ZINC json's three
    scalers, graph norm, BatchNorm, residual (configs/molecules_graph_regression_DGN_ZINC.json:26-34)."""
    from dgn_amd import synth
    b = synth.molecule_batch(200, seed=41, extra_bonds=3.9, eig_dim=6)
    _layer_vs_oracle(monkeypatch, "simple", 75, "mean dir1-dx-no-abs", "identity amplification attenuation", True, b, min_rows)


@ROUTES
@pytest.mark.parametrize("type_net", ["simple", "complex"])
def test_c3_cifar10_hidden65_vs_oracle(monkeypatch, type_net, min_rows):
    """BASELINE configs[2] at its own width: hidden 65 (odd), mean dir1-dx dir2-dx, the json's identity scaler
    (configs/superpixels_graph_classification_DGN_CIFAR10.json:23,32-33), k-NN graphs with eig = [0, x, y]."""
    from dgn_amd import synth
    b = synth.knn_batch(8, seed=41)
    _layer_vs_oracle(monkeypatch, type_net, 65, "mean dir1-dx dir2-dx", "identity", True, b, min_rows)


@pytest.mark.parametrize("type_net,F_,aggs", [("simple", 70, "mean max min dir1-dx dir1-av"), ("complex", 70, "mean max min dir1-av dir1-dx"),
                                              ("towers", 70, "mean max min dir1-av dir1-dx")])
def test_every_layer_type_on_the_default_routes_vs_oracle(monkeypatch, type_net, F_, aggs):
    """tests/conftest.py lowers the thresholds of the degree-class posttrans and of the block backward so that the small oracle batches
    run those routes; here every layer type at the library's DEFAULTS: folded posttrans, staged backward, the
    Linears on whichever route the row count selects."""
    import dgn_amd
    from dgn_amd import synth
    monkeypatch.setattr(dgn_amd.ops, "DC_MIN_NODES", 16384)
    monkeypatch.setattr(dgn_amd.ops, "BLOCK_LAYER_MAX_NODES", 8192)       # (the default: this batch takes the graph-block route)
    monkeypatch.delenv("DGN_DC_MIN_NODES", raising=False)
    monkeypatch.setattr(dgn_amd._lib.options, "blk_min_nodes", 131072)
    b = synth.molecule_batch(150, seed=45, extra_bonds=3.9, eig_dim=6)
    if type_net == "towers":
        _towers_vs_oracle(monkeypatch, 70, 5, b)
    else:
        _layer_vs_oracle(monkeypatch, type_net, F_, aggs, "identity amplification attenuation", True, b, None)


@ROUTES
def test_zinc_json_complex_hidden45_vs_oracle(monkeypatch, min_rows):
    from dgn_amd import synth
    b = synth.molecule_batch(200, seed=41, extra_bonds=3.9, eig_dim=6)
    _layer_vs_oracle(monkeypatch, "complex", 45, "mean dir1-dx dir1-av", "identity amplification attenuation", True, b, min_rows)


@ROUTES
def test_pattern_json_complex_hidden47_vs_oracle(monkeypatch, min_rows):
    from dgn_amd import synth
    b = synth.sbm_batch(12, seed=41, n_lo=44, n_hi=90)
    _layer_vs_oracle(monkeypatch, "complex", 47, "mean dir1-dx dir2-dx", "identity amplification attenuation", True, b, min_rows)


@pytest.mark.parametrize("hidden,towers", [(45, 5), (35, 5)])
def test_towers_layer_odd_tower_width_vs_oracle(monkeypatch, hidden, towers):
    """towers with an ODD per-tower width (45 / 5 = 9, 35 / 5 = 7): the padded message path of the towers layer."""
    import dgn_amd
    from dgn_amd import synth
    monkeypatch.setattr(dgn_amd.ops, "LINEAR_MIN_ROWS", 0)
    _towers_vs_oracle(monkeypatch, hidden, towers, synth.molecule_batch(120, seed=7, extra_bonds=3.9, eig_dim=6))


def _towers_vs_oracle(monkeypatch, hidden, towers, b):
    import dgn_amd
    dev = torch.device("cuda")
    src, dst, N = b["src"], b["dst"], int(b["num_nodes"])
    aggs, scalers = "mean max min dir1-av dir1-dx", "identity amplification attenuation"
    layer, avg, h, ct = _o1_layer("towers", hidden, aggs, scalers, True, towers, b)
    oracle = _oracle_of(layer, "towers", aggs, scalers, avg, True, towers, b, h, ct)
    y32, g32, names, stats, _ = oracle(torch.float32)
    y64, g64, _, _, _ = oracle(torch.float64)
    layer = layer.to(dev).train()
    graph = dgn_amd.DGNGraph(src.to(dev), dst.to(dev), N, eig=b["eig"].to(dev))
    hd = h.to(dev).requires_grad_(True)
    y = layer(graph, hd, None, b["snorm_n"].to(dev))
    params = dict(layer.named_parameters())
    gd = torch.autograd.grad(y, [hd] + [params[k] for k in names], ct.to(dev))
    np.testing.assert_allclose(y.detach().cpu().numpy(), y32.detach().numpy(), rtol=2e-5, atol=2e-5)
    for a, r32, r64, k in zip(gd, g32, g64, ["h"] + names):
        _check_grad(a, r32, r64, k)
    _check_running_stats(layer, stats)          # (the five per-tower BatchNorms)


def test_c4_at_the_default_threshold_takes_the_degree_class_route_vs_oracle(monkeypatch):
    """The node count from which the simple / complex layers run posttrans per in-degree class is 16 384 by default (the other tests
    lower it, tests/conftest.py): here the default, on a batch above it -- the route must be taken and meet the oracle."""
    import dgn_amd
    from dgn_amd import synth
    monkeypatch.setattr(dgn_amd.ops, "DC_MIN_NODES", 16384)
    b = synth.molecule_batch(720, seed=43, n_lo=10, n_hi=41, extra_bonds=4.3, eig_dim=4)
    assert int(b["num_nodes"]) >= 16384
    taken = []
    real = dgn_amd.ops._degree_classes
    monkeypatch.setattr(dgn_amd.ops, "_degree_classes", lambda *a: taken.append(real(*a)) or taken[-1])
    _layer_vs_oracle(monkeypatch, "simple", 70, "mean max min dir1-dx dir1-av", "identity amplification attenuation", False, b, None)
    assert taken and taken[0] is not None
    small = synth.molecule_batch(450, seed=43, n_lo=10, n_hi=41, extra_bonds=4.3, eig_dim=4)      # ~11.5 k nodes
    assert 8192 <= int(small["num_nodes"]) < 16384
    taken.clear()
    _layer_vs_oracle(monkeypatch, "simple", 70, "mean max min dir1-dx dir1-av", "identity amplification attenuation", False, small, None)
    assert taken and taken[0] is None                      # below the threshold: the folded route


@pytest.mark.parametrize("n_graphs,expect_dc", [(450, False), (720, True)], ids=["11k-nodes-folded", "18k-nodes-degree-classes"])
def test_molecule_batches_between_the_dispatch_thresholds_at_the_library_defaults_vs_oracle(monkeypatch, n_graphs, expect_dc):
    """the gaps between the dispatch thresholds at the LIBRARY'S DEFAULTS (tests/conftest.py lowers three of them for
    the rest of the suite).  A molecule batch above the graph-block route (8 192 nodes) and below the block backward (131 072 nodes) runs
    the STAGED backward sweep (agg_bwd_short + seg_sum_rows); below 16 384 nodes posttrans is the folded product, above it one product per
    in-degree class.  BASELINE C4's layer on (a) 450 graphs, ~11.5 k nodes: folded posttrans + staged backward, (b) 720 graphs, ~18.4 k
    nodes: degree-class posttrans + staged backward (the routes of bench.py's c4 leg; C4's OWN batch, 2048 graphs / 52 754 nodes, is
    tests/test_bench_sizes_gpu.py) -- values and every gradient vs the oracle."""
    import dgn_amd
    from dgn_amd import _lib, synth
    monkeypatch.setattr(dgn_amd.ops, "DC_MIN_NODES", 16384)
    monkeypatch.setattr(dgn_amd.ops, "BLOCK_LAYER_MAX_NODES", 8192)
    monkeypatch.setattr(_lib.options, "blk_min_nodes", 131072)
    b = synth.molecule_batch(n_graphs, seed=43, n_lo=10, n_hi=41, extra_bonds=4.3, eig_dim=4)
    N = int(b["num_nodes"])
    assert 8192 < N < 131072 and (N >= 16384) == expect_dc
    taken, blocks = [], []
    real = dgn_amd.ops._degree_classes
    monkeypatch.setattr(dgn_amd.ops, "_degree_classes", lambda *a: taken.append(real(*a)) or taken[-1])
    real_blk = dgn_amd.ops.block_layer
    monkeypatch.setattr(dgn_amd.ops, "block_layer", lambda *a, **k: blocks.append(1) or real_blk(*a, **k))
    # (above 16 k nodes: the counted clause with its default caps, not the zero of the small config tests -- a few routings of the 1.3 M
    #  gradient entries behind max / min flip between any two fp32 evaluations, the oracle's own included)
    _layer_vs_oracle(monkeypatch, "simple", 70, "mean max min dir1-dx dir1-av", "identity amplification attenuation", False, b, None, strict=not expect_dc)
    assert not blocks, "the graph-block route took a batch above its node limit"
    assert taken and (taken[0] is not None) == expect_dc


@pytest.mark.parametrize("type_net", ["simple", "complex"])
def test_isolated_nodes_through_the_degree_class_route_vs_oracle(monkeypatch, type_net):
    """Zero in-degree nodes are a class of their own (class 0: amplification and attenuation factors 0, the complex layer's h block
    still contributes): a molecule batch with every in-edge of ~6 % of the nodes removed, three scalers, against the oracle."""
    import dgn_amd
    from dgn_amd import synth
    b = dict(synth.molecule_batch(220, seed=47, extra_bonds=3.9, eig_dim=6))
    N = int(b["num_nodes"])
    cut = torch.rand(N, generator=torch.Generator().manual_seed(48)) < 0.06
    keep = ~cut[b["dst"]]
    b["src"], b["dst"] = b["src"][keep], b["dst"][keep]
    assert int((torch.bincount(b["dst"], minlength=N) == 0).sum()) > 50
    taken = []
    real = dgn_amd.ops._degree_classes
    monkeypatch.setattr(dgn_amd.ops, "_degree_classes", lambda *a: taken.append(real(*a)) or taken[-1])
    _layer_vs_oracle(monkeypatch, type_net, 70, "mean max min dir1-dx dir1-av", "identity amplification attenuation", True, b, 0)
    assert taken and taken[0] is not None and int(taken[0][0]["present"][0]) > 50


@pytest.mark.parametrize("hidden,aggs,gen", [(75, "mean dir1-dx-no-abs", "molecules"), (65, "mean dir1-dx dir2-dx", "knn"), (65, "mean dir1-dx dir2-dx", "molecules")])
def test_odd_hidden_size_without_the_padded_copy_is_bitwise_the_padded_layer(monkeypatch, hidden, aggs, gen):
    """Simple layers at odd hidden sizes (ZINC simple 75, CIFAR10 65): the sweep reads the un-padded rows itself (DgnMsg.f_valid, kernels
    with Cfg::ODD: the last lane of a row shifts its pair and hands on a zero) -- output, d h and every parameter gradient carry the bits
    of the layer run on a zero-padded copy (library option odd_direct = 0), molecule batches (four rows per wave, block backward lowered
    to this size by the conftest) and k-NN batches (row kernels, graph backward)."""
    import copy
    import dgn_amd
    from dgn_amd import _lib, synth
    dev = torch.device("cuda")
    b = synth.molecule_batch(90, seed=12, extra_bonds=3.9, eig_dim=6) if gen == "molecules" else synth.knn_batch(9, seed=12)
    N = int(b["num_nodes"])
    avg = float(torch.log(torch.bincount(b["dst"], minlength=N).float() + 1).mean())
    torch.manual_seed(0)
    scalers = "identity amplification attenuation" if hidden == 75 else "identity"
    layer = dgn_amd.DGNLayer(hidden, hidden, 0.0, True, True, aggs, scalers, {"log": torch.tensor(avg)}, "simple", True, edge_features=False, edge_dim=0).model.to(dev).train()
    gen_ = torch.Generator().manual_seed(3)
    h, ct = torch.randn(N, hidden, generator=gen_).to(dev), torch.randn(N, hidden, generator=gen_).to(dev)
    snorm = b["snorm_n"].to(dev)
    sd0 = copy.deepcopy(layer.state_dict())
    outs = []
    for direct in (1, 0):
        monkeypatch.setattr(_lib.options, "odd_direct", direct)
        layer.load_state_dict(sd0)
        graph = dgn_amd.DGNGraph(b["src"].to(dev), b["dst"].to(dev), N, eig=b["eig"].to(dev))
        hh = h.clone().requires_grad_(True)
        y = layer(graph, hh, None, snorm)
        g = torch.autograd.grad(y, [hh] + list(layer.parameters()), ct)
        outs.append([y.detach()] + list(g))
    for a, c in zip(*outs):
        assert torch.equal(a, c)
