"""Which kernel an aggregator list gets: the lists of csrc/dgn_agg_hot.hpp run kernels with the list baked in (`StaticOps` in the
kernel's name), any other list the generic ones (`DynOps`) -- on the streaming sweep forward and backward (short-row and row-per-wave
kernels), the block backward, the graph-block layer and the fused no-grad towers forward.  Kernel names come from the profiler; no
values are compared here (the parity tests do that)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

F_ = 16
HOT = ["mean max min dir1-av dir1-dx", "mean dir1-dx dir2-dx"]
NOT_HOT = "max mean min dir1-av dir1-dx"                      # the first list with its first two aggregators swapped
BLK_HOT, BLK_NOT_HOT = "mean max min dir1-dx dir1-av", "max mean min dir1-dx dir1-av"      # the HIV json list / its permutation


def _device_events(step):
    """Names of the device activities of one step, one entry per launch (the pattern of tests/test_mol_io_gpu.py)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    evs = prof.profiler.kineto_results.events()
    return [e.name() for e in evs if str(e.device_type()).endswith("CUDA")]


def _rings():
    """64 ring graphs of 12 nodes: in-degree 2, the short-row kernels."""
    n, k = 64, 12
    i = torch.arange(n * k)
    nxt = (i // k) * k + (i % k + 1) % k
    return torch.cat([i, nxt]), torch.cat([nxt, i]), n * k


def _dense():
    """One graph of 256 nodes, in-degree 10: the row-per-wave kernels."""
    N = 256
    i = torch.arange(N).repeat_interleave(10)
    return (i + torch.arange(1, 11).repeat(N)) % N, i, N


@functools.lru_cache(maxsize=None)
def _batch(kind):
    import dgn_amd
    dev = torch.device("cuda")
    src, dst, N = _rings() if kind == "rings" else _dense()
    gen = torch.Generator().manual_seed(3)
    eig = torch.randn(N, 4, generator=gen).to(dev)
    return dgn_amd.DGNGraph(src.to(dev), dst.to(dev), N, eig=eig), torch.randn(N, F_, generator=gen).to(dev)


def _sweep_names(graph, x, aggs):
    """agg_* kernels of one directional_aggregate forward and of its backward"""
    import dgn_amd
    from dgn_amd.ops import directional_aggregate
    plan = dgn_amd.make_plan(aggs.split(), ["identity"])
    xr = x.clone().requires_grad_(True)
    out = []
    fwd = _device_events(lambda: out.append(directional_aggregate(graph, plan, 1.1, x_src=xr, x_in=xr)))
    ct = torch.ones_like(out[0])
    bwd = _device_events(lambda: torch.autograd.grad(out[0], xr, ct))
    fwd, bwd = [n for n in fwd if "agg_" in n], [n for n in bwd if "agg_" in n]
    assert fwd and bwd, (fwd, bwd)
    return fwd, bwd


@pytest.fixture
def staged_backward(monkeypatch):
    """The block backward at the library's default threshold (tests/conftest.py lowers it to 0): these batches run the staged kernels."""
    import dgn_amd
    monkeypatch.setattr(dgn_amd._lib.options, "blk_min_nodes", 131072)


@pytest.mark.parametrize("kind", ["rings", "dense"])
@pytest.mark.parametrize("aggs", HOT)
def test_sweep_of_a_hot_list_runs_baked_kernels(staged_backward, kind, aggs):
    graph, x = _batch(kind)
    fwd, bwd = _sweep_names(graph, x, aggs)
    assert all("StaticOps" in n and "DynOps" not in n for n in fwd + bwd), (kind, fwd, bwd)
    assert any(("agg_fwd_short" if kind == "rings" else "agg_fwd_rows") in n for n in fwd), (kind, fwd)
    assert not any("agg_bwd_block" in n for n in bwd), (kind, bwd)


@pytest.mark.parametrize("kind", ["rings", "dense"])
def test_sweep_of_another_list_runs_generic_kernels(staged_backward, kind):
    graph, x = _batch(kind)
    fwd, bwd = _sweep_names(graph, x, NOT_HOT)
    assert all("DynOps" in n and "StaticOps" not in n for n in fwd + bwd), (kind, fwd, bwd)


def test_block_backward_takes_hot_lists_only(monkeypatch):
    """(blk_min_nodes lowered through dgn_set_option for the test: the block backward otherwise starts at 131 072 nodes)"""
    import dgn_amd
    graph, x = _batch("rings")
    monkeypatch.setattr(dgn_amd._lib.options, "blk_min_nodes", 0)
    for aggs in HOT:
        _, bwd = _sweep_names(graph, x, aggs)
        assert any("agg_bwd_block" in n for n in bwd) and all("StaticOps" in n for n in bwd), (aggs, bwd)
    _, bwd = _sweep_names(graph, x, NOT_HOT)
    assert not any("agg_bwd_block" in n for n in bwd) and all("DynOps" in n for n in bwd), bwd


def _layer(type_net, aggs, towers=2):
    import dgn_amd
    torch.manual_seed(0)
    return dgn_amd.DGNLayer(F_, F_, 0.0, False, True, aggs, "identity", {"log": torch.tensor(1.1)}, type_net, True, towers=towers,
                            edge_features=False, edge_dim=0).model.to(torch.device("cuda"))


@pytest.mark.parametrize("aggs,ops", [(BLK_HOT, "StaticOps"), (BLK_NOT_HOT, "DynOps")])
def test_graph_block_layer_picks_by_list(monkeypatch, aggs, ops):
    import dgn_amd
    monkeypatch.setattr(dgn_amd.ops, "BLOCK_LAYER_MAX_NODES", 8192)      # (the library's default: tests/conftest.py switches the route off)
    dev = torch.device("cuda")
    src, dst, N = _rings()
    gen = torch.Generator().manual_seed(5)
    graph = dgn_amd.DGNGraph(src.to(dev), dst.to(dev), N, eig=torch.randn(N, 4, generator=gen).to(dev))
    layer = _layer("simple", aggs).train()
    h = torch.randn(N, F_, generator=gen).to(dev).requires_grad_(True)
    snorm = torch.full((N, 1), 12 ** -0.5, device=dev)
    out = []
    fwd = _device_events(lambda: out.append(layer(graph, h, None, snorm)))
    bwd = _device_events(lambda: out[0].sum().backward())
    for names, kernel in ((fwd, "blk_forward"), (bwd, "blk_backward")):
        mine = [n for n in names if kernel in n]
        assert len(mine) == 1 and ops in mine[0] and ("DynOps" if ops == "StaticOps" else "StaticOps") not in mine[0], (kernel, names)


def test_fused_towers_forward_exists_for_hot_lists_only(monkeypatch):
    import dgn_amd
    from dgn_amd.dgn_layer import X_IN_NAME
    dev = torch.device("cuda")
    assert dgn_amd.ops.BLOCK_LAYER_MAX_NODES == 0              # (tests/conftest.py: the streaming route's no-grad forward, not the graph-block one)
    src, dst, N = _rings()
    gen = torch.Generator().manual_seed(7)
    graph = dgn_amd.DGNGraph(src.to(dev), dst.to(dev), N, eig=torch.randn(N, 4, generator=gen).to(dev))
    h = torch.randn(N, F_, generator=gen).to(dev)
    snorm = torch.full((N, 1), 12 ** -0.5, device=dev)
    for aggs, hot in ((HOT[0], True), (NOT_HOT, False)):
        plan_x = dgn_amd.make_plan(aggs.split() + [X_IN_NAME], ["identity"])
        assert dgn_amd.ops.fused_sweep_posttrans_supported(graph, plan_x, 2, F_, 1, F_ // 2) == hot, aggs
        layer = _layer("towers", aggs).eval()
        with torch.no_grad():
            names = _device_events(lambda: layer(graph, h, None, snorm))
        fused, sweep = [n for n in names if "layer_fwd_fused" in n], [n for n in names if "agg_" in n]
        if hot:
            assert len(fused) == 1 and "StaticOps" in fused[0] and not sweep, names
        else:
            assert not fused and sweep and all("DynOps" in n for n in sweep), names
