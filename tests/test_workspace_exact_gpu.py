"""The entry points with a multi-part workspace, run in a workspace of EXACTLY the queried size.

A carve that disagrees with the exported ``*_workspace_bytes()`` query writes past the buffer, and no other test sees that unless the
bytes behind it happen to matter.  Every case here runs its entry points twice: first each gets a workspace of exactly the size its
caller asked the library for, at the front of a larger allocation of the test's own whose tail -- like the workspace itself -- holds
a byte pattern; then a roomy one.  The outputs of the two runs are bit-identical and the tails keep their pattern: a wrong carve shows
up as a changed byte inside the test's allocation, not as a fault.

The calls are made by the package's own Python side (which sizes every workspace with the query); the test swaps the workspace
argument -- or the whole-layer struct's ``ws`` / ``ws_bytes`` -- on the way into the library."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 1 << 20
PATTERN = 0xA5

# entry point -> position of `ws` in its arguments (`ws_bytes` follows it); None: DgnXxxLayer.ws / .ws_bytes of the first argument
WS_AT = {"dgn_agg_forward_aux": 9, "dgn_agg_backward_aux": 10, "dgn_edge_weights": 9, "dgn_graph_build": 12, "dgn_graph_build_cuts": 6,
         "dgn_graph_build_csc": 6, "dgn_bn_tail_backward": 14, "dgn_dc_wgrad": 11,
         "dgn_towers_layer_forward": None, "dgn_towers_layer_backward": None, "dgn_dense_layer_forward": None, "dgn_dense_layer_backward": None,
         "dgn_block_layer_forward": None, "dgn_block_layer_backward": None}


class Swap:
    """Every entry point of WS_AT, wrapped on the loaded library: the call goes through with a workspace of this test's."""

    def __init__(self, monkeypatch):
        from dgn_amd import _lib
        self.exact, self.guarded, self.seen = True, [], {}
        self.dense_dc = []      # per dense-layer call of the test (NOT reset per run by twice()): whether the struct carried degree classes
        lib = _lib.load()
        for name, at in WS_AT.items():
            monkeypatch.setattr(lib, name, self._wrap(getattr(lib, name), name, at))

    def _wrap(self, real, name, at):
        def call(*args):
            layer = args[0]._obj if at is None else None
            nbytes = int(layer.ws_bytes if at is None else args[at + 1])
            if nbytes == 0:                                   # (no workspace asked for: nothing to swap)
                return real(*args)
            buf = torch.full((nbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
            given = nbytes if self.exact else nbytes + GUARD
            if self.exact:
                self.guarded.append((name, buf, nbytes))
            else:
                self.guarded.append((name, buf, None))        # (kept alive until the run has finished)
            self.seen[name] = self.seen.get(name, 0) + 1
            if at is None:
                if name.startswith("dgn_dense_layer"):
                    self.dense_dc.append(bool(layer.dc))
                layer.ws, layer.ws_bytes = buf.data_ptr(), given
                return real(*args)
            return real(*args[:at], buf.data_ptr(), given, *args[at + 2:])
        return call

    def twice(self, run, reached):
        """run() with exact workspaces, then with roomy ones: the same bits, the guards intact, every entry point of `reached` swapped"""
        results = []
        for exact in (True, False):
            self.exact, self.guarded, self.seen = exact, [], {}
            results.append([t.detach().clone() for t in run()])
            torch.cuda.synchronize()
            assert set(reached) <= set(self.seen), f"not reached with a workspace: {set(reached) - set(self.seen)}"
            for name, buf, nbytes in self.guarded:
                if nbytes is not None:
                    assert bool((buf[nbytes:] == PATTERN).all()), f"{name}: bytes behind its workspace of {nbytes} bytes were written"
        a, b = results
        assert len(a) == len(b) and len(a) > 0
        for i, (x, y) in enumerate(zip(a, b)):
            assert x.shape == y.shape and x.dtype == y.dtype
            same = torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
            assert same, f"output {i}: the exact and the roomy workspace gave different bits"


@pytest.fixture
def swap(monkeypatch):
    return Swap(monkeypatch)


def _hub_graph(seed=5, N=300):
    """a few hundred nodes, in-degree about 2, and two hub rows (40 and 45 in-edges) that hub_threshold 16 / hub_chunk 8 cut in 5 + 6 chunks"""
    rng = np.random.default_rng(seed)
    dst = np.concatenate([2 + (np.arange(600) % (N - 3)), np.zeros(40, np.int64), np.ones(45, np.int64)])      # (node N - 1: no in-edge)
    src = rng.integers(0, N, dst.size)
    perm = rng.permutation(dst.size)
    return torch.from_numpy(src[perm]), torch.from_numpy(dst[perm]), N


def _graph_outputs(g):
    g.ensure_csc()
    cut, gap = g._closed_cuts()
    return [g.indptr, g.src, g.dst_csr, g.log_deg, g.csc_ptr, g.csc_pos, g.csc_order, cut, torch.tensor([gap])]


@pytest.mark.parametrize("which", ["hub", "few_edges"])
def test_graph_build(swap, which):
    import dgn_amd
    if which == "hub":
        src, dst, N = _hub_graph()
    else:                                                     # n_edges < n_nodes: the node-sized blocks are the larger ones
        N = 300
        src, dst = torch.arange(0, 90) * 3, torch.arange(0, 90) * 3 + 1
    run = lambda: _graph_outputs(dgn_amd.DGNGraph(src.cuda(), dst.cuda(), N, hub_threshold=16, hub_chunk=8))
    swap.twice(run, ["dgn_graph_build", "dgn_graph_build_csc", "dgn_graph_build_cuts"])


def test_sweep_and_edge_weights_on_hub_rows(swap):
    """dgn_edge_weights, dgn_agg_forward and the deterministic dgn_agg_backward with a four-type edge table at an even F: the hub parts, the
    staging buffer and the table's partials, all three spans of the backward layout.  d x_src and the table's gradient are summed by the
    two-phase scatter in a fixed order and compared whole; d x_dst and d x_in of a HUB row are added over its slices with atomics, whose
    order -- and with it the last bit -- varies from run to run whatever the workspace, so those two are compared on every other row."""
    import dgn_amd
    from dgn_amd.ops import directional_aggregate
    src, dst, N = _hub_graph()
    gen = torch.Generator().manual_seed(3)
    F_, K = 12, 4
    eig = torch.randn(N, 3, generator=gen).cuda()
    P, Q, x = (torch.randn(N, F_, generator=gen).cuda() for _ in range(3))
    table = torch.randn(K, F_, generator=gen).cuda()
    types = torch.randint(0, K, (src.numel(),), generator=gen)
    plan = dgn_amd.make_plan(["mean", "max", "std", "dir1-dx", "dir1-av"], ["identity", "amplification"])
    assert len(plan.launches) == 1
    ct = torch.randn(N, plan.out_width(F_), generator=gen).cuda()

    def run():
        graph = dgn_amd.DGNGraph(src.cuda(), dst.cuda(), N, eig=eig, hub_threshold=16, hub_chunk=8)
        assert graph.n_hub >= 2 and graph.c_graph.n_chunks >= 2 * 3
        types_slot = graph.to_slot_order(types.cuda()).to(torch.int32).contiguous()
        leaves = [t.clone().requires_grad_(True) for t in (P, table, Q, x)]
        w = graph.edge_weights(plan)
        y = directional_aggregate(graph, plan, 1.2, x_src=leaves[0], x_dst=leaves[2], m_edge=leaves[1], x_in=leaves[3], weights=w, edge_type=types_slot)
        g_src, g_table, g_dst, g_in = torch.autograd.grad(y, leaves, ct)
        hub_rows = torch.nonzero(torch.bincount(dst.cuda(), minlength=N) > 16).flatten()
        assert hub_rows.tolist() == [0, 1]
        g_dst[hub_rows] = 0
        g_in[hub_rows] = 0
        return [w, y, g_src, g_table, g_dst, g_in]

    swap.twice(run, ["dgn_edge_weights", "dgn_agg_forward_aux", "dgn_agg_backward_aux"])


@pytest.mark.parametrize("F_", [70, 75])
def test_bn_tail_backward_with_its_own_sums(swap, F_):
    """sums_out == NULL: the two column sums live behind the partials, in the workspace"""
    from dgn_amd import _lib
    lib = _lib.load()
    N = 300
    gen = torch.Generator().manual_seed(F_)
    g_y, x = (torch.randn(N, F_, generator=gen).cuda() for _ in range(2))
    gamma, beta, mean = (torch.randn(F_, generator=gen).cuda() for _ in range(3))
    invstd = (torch.rand(F_, generator=gen) + 0.5).cuda()
    nbytes = lib.dgn_bn_tail_workspace_bytes(N, F_)

    def run():
        g_x, g_gamma, g_beta = torch.empty(N, F_, device="cuda"), torch.empty(F_, device="cuda"), torch.empty(F_, device="cuda")
        _lib.check(lib.dgn_bn_tail_backward(N, F_, g_y.data_ptr(), x.data_ptr(), F_, gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), invstd.data_ptr(), 1,
                                            g_x.data_ptr(), g_gamma.data_ptr(), g_beta.data_ptr(), None, None, nbytes, None,
                                            _lib.stream_ptr(g_y.device)), "dgn_bn_tail_backward")
        return [g_x, g_gamma, g_beta]

    swap.twice(run, ["dgn_bn_tail_backward"])


def test_dc_wgrad_on_the_small_table(swap):
    from dgn_amd import _lib
    from test_dc_grid_gpu import SMALL_SIZES, Table
    lib = _lib.load()
    tab = Table(SMALL_SIZES, seed=7)
    assert tab.n_units == 15
    S, k, n = 3, 280, 70
    gen = torch.Generator().manual_seed(1)
    g, x = torch.randn(tab.N, n, generator=gen).cuda(), torch.randn(tab.N, k, generator=gen).cuda()
    scale = (torch.rand(32, S, generator=gen) + 0.5).cuda()
    s = tab.struct(scale)
    nbytes = lib.dgn_dc_wgrad_workspace_bytes(tab.n_units, k, n)

    def run():
        out = torch.empty(S * n, k, device="cuda")
        _lib.check(lib.dgn_dc_wgrad(C.byref(s), S, k, n, g.data_ptr(), n, x.data_ptr(), k, out.data_ptr(), k, None, None, nbytes,
                                    _lib.stream_ptr(g.device)), "dgn_dc_wgrad")
        return [out]

    swap.twice(run, ["dgn_dc_wgrad"])


# the whole-layer steps on a six-molecule batch: (layer type, towers, hidden size, scalers, degree-class posttrans, graph-block route)
LAYERS = {"towers": ("towers", 5, 70, "identity amplification attenuation", False, False),
          "simple": ("simple", 1, 75, "identity amplification attenuation", False, False),
          "complex": ("complex", 1, 70, "identity amplification attenuation", False, False),
          "dc": ("simple", 1, 70, "identity amplification attenuation", True, False),
          "block_towers": ("towers", 5, 70, "identity amplification attenuation", False, True),
          "block_simple": ("simple", 1, 75, "identity", False, True)}
REACHED = {"towers": ["dgn_towers_layer_forward", "dgn_towers_layer_backward"], "block": ["dgn_block_layer_forward", "dgn_block_layer_backward"],
           "dense": ["dgn_dense_layer_forward", "dgn_dense_layer_backward"]}


@pytest.mark.parametrize("name", sorted(LAYERS))
def test_layer_step(swap, monkeypatch, name):
    import dgn_amd
    from dgn_amd import _lib, synth
    type_net, T, F_, scalers, dc, block = LAYERS[name]
    b = synth.molecule_batch(6, seed=11, eig_dim=4)
    N = int(b["num_nodes"])
    avg = float(torch.log(torch.bincount(b["dst"], minlength=N).float() + 1).mean())
    torch.manual_seed(2)
    layer = dgn_amd.DGNLayer(F_, F_, 0.0, True, True, "mean max min dir1-av dir1-dx", scalers, {"log": torch.tensor(avg)}, type_net, True,
                             towers=T, edge_features=False, edge_dim=0).model.cuda().train()
    sd0 = {k: v.clone() for k, v in layer.state_dict().items()}
    gen = torch.Generator().manual_seed(4)
    h, ct, snorm = torch.randn(N, F_, generator=gen).cuda(), torch.randn(N, F_, generator=gen).cuda(), b["snorm_n"].cuda()
    monkeypatch.setattr(dgn_amd.ops, "BLOCK_LAYER_MAX_NODES", (1 << 20) if block else 0)
    monkeypatch.setattr(dgn_amd.ops, "BLOCK_LAYER_MAX_POST", 1 << 30)
    monkeypatch.setattr(dgn_amd.ops, "DC_POSTTRANS", bool(dc))
    monkeypatch.setattr(dgn_amd.ops, "DC_MIN_NODES", 0)

    def run():
        graph = dgn_amd.DGNGraph(b["src"].cuda(), b["dst"].cuda(), N, eig=b["eig"].cuda())
        layer.load_state_dict(sd0)
        hh = h.clone().requires_grad_(True)
        y = layer(graph, hh, None, snorm)
        grads = torch.autograd.grad(y, [hh] + list(layer.parameters()), ct)
        return [y] + list(grads) + [v for k, v in layer.state_dict().items() if "running" in k]

    swap.twice(run, REACHED["block" if block else ("towers" if type_net == "towers" else "dense")])
    if not block and type_net != "towers":
        # the degree-class route is taken exactly where the case says so: the struct carries the classes, and the widths are the route's
        lib, K = _lib.load(), (5 + (type_net == "complex")) * (F_ + (F_ & 1))
        # (a forward and a backward call in each of the two runs)
        assert len(swap.dense_dc) == 4 and all(v == bool(dc) for v in swap.dense_dc)
        assert not dc or (lib.dgn_dc_supported(K, F_) and lib.dgn_dc_supported(F_, K) and lib.dgn_dc_wgrad_supported(K, F_))
