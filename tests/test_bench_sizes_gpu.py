"""The three batches every published number comes from -- bench.py's ``c2`` (ZINC-12k as one batch, towers x5, hidden 70), ``c1`` (the same
graph, simple, hidden 75) and ``c4`` (2 048 molhiv-like graphs, simple, hidden 70, three scalers) -- AT THEIR OWN SIZE and at the LIBRARY'S
DEFAULTS, one training step against the oracle's arithmetic.

tests/conftest.py lowers the dispatch thresholds so that batches of a few thousand nodes run the big-batch kernels with one or two
workgroups' worth of rows; what exists only at full size is checked here: ``agg_bwd_block`` over real ``blk_cut`` bins, the per-workgroup
BatchNorm slots whose number depends on the batch size, the partial slots of ``ts_wgrad`` / ``dc_wgrad`` / ``bd_backward_both`` and
their finalize kernels, ``dc_gemm<5>`` on 275 k rows, ``dc_gemm_small`` on 52 k rows, the flat 16-byte-chunk BatchNorm kernels, 64-bit
offsets (N x 84 x 5 floats) and the ragged last rows (275 167 is odd).

* the batch is bench.py's (generator and arguments read from ``bench.WORKLOADS``, seed 41; N and E pinned); weights, h and the cotangent
  are the suite's (O(1) weights, N(0, 1) from a CPU generator: tests/test_shipped_configs_gpu.py's helpers);
* y and d h with ``parity_util.check``; every parameter gradient -- a sum over the batch's rows, on which the fp32 oracle itself is
  ~1e-3 (relative) off its fp64 evaluation at this size -- with ``parity_util.check_reduced``: against the fp64 oracle, allowance = the
  reference's own fp32 error on that tensor, x1; BatchNorm running statistics of every BatchNorm module;
* the comparator's teeth are shown in the test: the fp64 oracle's gradient for the cotangent with its LAST 64 ROWS zeroed (one wave's
  share of an epilogue reduction, in the ragged tail) is what a kernel losing one such slab would return, and ``check_reduced`` must
  reject it on every parameter gradient that is not numerically zero;
* the routes are proved: one more step under torch.profiler, kernel names against the committed tables profiles/r06_{c2,c1,c4}_kernel_stats.txt
  (the profiler must see device kernels: an empty list fails), next to spies on the Python dispatch and a read of the library's option;
* the compared step runs twice from the same state: output, every gradient and the running statistics are bit-equal.

``c2c`` (the same graph, complex, hidden 70) is NOT a case, on purpose: measured once through this test, its y, d h, running statistics,
routes and the dropped-slab rejection all hold, but ``check_reduced``'s premise -- the allowance is a SUMMATION error -- does not: node
161 755, feature 28 of BatchNorm's output is +1.8e-7 in fp64, 50 x closer to zero than any fp32 evaluation of y is accurate, the ReLU
behind it has derivative 1 in fp64 and 0 in the fp32 oracle and in the library alike, and that single row is the worst entry of three
parameter gradients in both (E_ours / E_ref = 1.001, 1.000, 0.975: a coin that another thread count of the CPU oracle tosses again).
DESIGN section 3 has the figures.

The time limits are hang guards (x3 over the measured wall times on an MI355X host with 16 CPU threads -- c2 33.6 s, c1 17.2 s,
c4 2.3 s inside the whole suite: WALL_S below), not performance criteria."""
import copy
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

# bench.py's batches at seed 41 (BENCH_r06.json: num_nodes / num_edges of c2 and c1): a generator change cannot silently shrink the test
SIZES = {"c2": (275167, 586426), "c1": (275167, 586426), "c4": (52754, 112702)}
GENERATORS = {"molecules": "molecule_batch", "knn": "knn_batch", "sbm": "sbm_batch"}
# kernel-name substrings of one training step, from the committed rocprofv3 tables of bench.py's legs
EXPECT = {
    "c2": ["agg_bwd_block", "agg_fwd_short", "bd_backward_both", "ts_wgrad"],
    "c1": ["dc_gemm<5", "dc_wgrad", "agg_bwd_block", "combine_bwd_flat4", "bn_apply_flat4"],
    "c4": ["dc_gemm_small", "dc_wgrad", "agg_bwd_short", "seg_sum_rows", "combine_bwd_flat4", "bn_apply_flat4"],
}
FORBID = {"c2": [], "c1": [], "c4": ["agg_bwd_block"]}          # (52 k nodes < 131 072: the staged backward)
BLOCK_ROUTE = ["blk_forward", "blk_tail_fwd", "blk_tail_bwd", "blk_backward", "blk_reduce"]
# measured wall time of each test in seconds (an MI355X host, 16 CPU threads; the oracle's fp32 + fp64 passes and the dropped-slab
# backward dominate, the GPU steps are milliseconds): inside the whole GPU suite -- 22.5 / 10.6 / 2.3 s when the module runs alone --
# and the hang guards: x3 over it, none below 60 s (whichever case runs first pays the start-up of the HIP runtime and of the
# profiler, seconds that do not scale with the batch)
WALL_S = {"c2": 33.6, "c1": 17.2, "c4": 2.3}
TIMEOUT_S = {k: max(60, int(3 * v + 0.999)) for k, v in WALL_S.items()}


def _base_name(kernel):
    """'void dgn::lin::ts_wgrad<3, 6, true, false>(dgn::lin::Args)' -> 'dgn::lin::ts_wgrad'; 'dgn::(anonymous namespace)::bn_finalize(...)'
    -> 'dgn::bn_finalize'"""
    k = kernel.strip().replace("(anonymous namespace)::", "")
    if k.startswith("void "):
        k = k[5:]
    for stop in "<(":
        k = k.split(stop, 1)[0]
    return k.strip()


def _device_kernels(step):
    """Names of the device kernels of one step (torch.profiler, device activities: tools/step_small_launches.py's pattern)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    evs = prof.profiler.kineto_results.events()
    return sorted({e.name() for e in evs if str(e.device_type()).endswith("CUDA")})


@pytest.mark.parametrize("name", [pytest.param(k, marks=pytest.mark.timeout(TIMEOUT_S[k])) for k in ("c2", "c1", "c4")])
def test_bench_batch_at_its_own_size_and_the_library_defaults_vs_oracle(monkeypatch, name):
    """One training step of bench.py's ``name`` leg, as the module's docstring says.  Profiler: torch.profiler sees the device kernels on
    the MI355X hosts this was written on, so the kernel-name assertions are unconditional (an empty kernel list fails); the dispatch
    spies and the option read are asserted as well."""
    import bench
    import dgn_amd
    from dgn_amd import _lib, ops, synth
    from parity_util import check, check_reduced, note, numerically_zero
    from test_shipped_configs_gpu import _check_running_stats, _o1_layer, _oracle_of

    # the library's defaults, all of them (tests/conftest.py lowers these three for the rest of the suite)
    monkeypatch.setattr(ops, "DC_MIN_NODES", 16384)
    monkeypatch.setattr(ops, "BLOCK_LAYER_MAX_NODES", 8192)
    monkeypatch.setattr(_lib.options, "blk_min_nodes", 131072)
    assert _lib.options.blk_min_nodes == 131072

    wl = bench.WORKLOADS[name]
    kind, kw = wl["gen"]
    b = getattr(synth, GENERATORS[kind])(seed=41, **kw)
    N, E = int(b["num_nodes"]), int(b["src"].numel())
    assert (N, E) == SIZES[name], f"bench.py's {name} batch changed size: N {N} E {E}"
    type_net, F_, towers = wl["type_net"], wl["hidden"], wl["towers"]
    aggs, scalers, graph_norm = wl["aggregators"], wl["scalers"], wl.get("graph_norm", True)
    assert wl.get("dropout", 0.0) == 0.0 and not wl.get("edge_dim")
    layer, avg, h, ct = _o1_layer(type_net, F_, aggs, scalers, graph_norm, towers, b)
    oracle = _oracle_of(layer, type_net, aggs, scalers, avg, graph_norm, towers, b, h, ct)
    names = [k for k, _ in layer.named_parameters()]

    dev = torch.device("cuda")
    taken, blocks = [], []
    real_dc, real_blk = ops._degree_classes, ops.block_layer
    monkeypatch.setattr(ops, "_degree_classes", lambda *a: taken.append(real_dc(*a)) or taken[-1])
    monkeypatch.setattr(ops, "block_layer", lambda *a, **k: blocks.append(1) or real_blk(*a, **k))
    layer_dev = copy.deepcopy(layer).to(dev)
    graph = dgn_amd.DGNGraph(b["src"].to(dev), b["dst"].to(dev), N, eig=b["eig"].to(dev))
    h_dev, ct_dev, snorm = h.to(dev), ct.to(dev), b["snorm_n"].to(dev)

    def run():
        lay = copy.deepcopy(layer_dev).train()
        hd = h_dev.clone().requires_grad_(True)
        y = lay(graph, hd, None, snorm)
        params = dict(lay.named_parameters())
        gd = torch.autograd.grad(y, [hd] + [params[k] for k in names], ct_dev)
        torch.cuda.synchronize()
        return y.detach(), list(gd), lay

    failures = []
    try:
        # ---- the GPU steps: twice from the same state, then once more under the profiler
        y, gd, lay = run()
        y2, gd2, lay2 = run()
        assert torch.equal(y, y2), "y differs between two runs from the same state"
        for a, c, k in zip(gd, gd2, ["h"] + names):
            assert torch.equal(a, c), f"d {k} differs between two runs from the same state"
        for (k, a), (_, c) in zip(lay.named_buffers(), lay2.named_buffers()):
            assert torch.equal(a, c), f"{k} differs between two runs from the same state"
        del y2, gd2, lay2
        assert not blocks, "the graph-block route took a batch above its node limit"
        if type_net == "towers":
            assert not taken or all(t is None for t in taken)
        else:
            assert taken and taken[0] is not None, "the degree-class posttrans was not taken above 16 384 nodes"
        kernels = _device_kernels(lambda: run())
        dgn = [k for k in kernels if "dgn::" in k]
        note(f"KERNELS {name}: {len(kernels)} device kernel names, {len(dgn)} of the library: " + " | ".join(_base_name(k) for k in dgn))
        assert dgn, f"torch.profiler saw no device kernel of the library ({len(kernels)} device events' names in all)"
        for want in EXPECT[name]:
            assert any(want in k for k in dgn), f"{name}: no kernel '{want}' in the step: {dgn}"
        for bad in FORBID[name] + BLOCK_ROUTE:
            assert not any(bad in k for k in dgn), f"{name}: kernel '{bad}' in the step: {dgn}"
        assert not any(_base_name(k).rsplit("::", 1)[-1] == "bn_stats" for k in dgn), "BatchNorm's forward column sums ran as a pass of their own"
        y, gd = y.cpu(), [g.cpu() for g in gd]

        # ---- the oracle: fp32, fp64 (graph kept), and the fp64 gradient of the cotangent without its last 64 rows
        y32, g32, onames, stats, _ = oracle(torch.float32)
        assert onames == names
        y64, g64, _, _, again = oracle(torch.float64, keep_graph=True)
        ct_dropped = ct.clone()
        ct_dropped[-64:] = 0
        g64_dropped = again(ct_dropped)
        del again
        y32, y64 = y32.detach(), y64.detach()
        gc.collect()

        def collect(fn, *a, **k):
            try:
                return fn(*a, **k)
            except AssertionError as exc:
                failures.append(str(exc))
                return None

        collect(check, y, y32, y64, f"{name} y", rtol=2e-5, atol=2e-5, abs_scale=1.0, max_escape_fraction=0.0)
        # d h: the counted clause with its default caps (a few max / min / |.| routings of millions of entries flip between any two fp32
        # evaluations, the oracle's own included), and no more than x10 the oracle's own flips: they land on different entries in any
        # two fp32 evaluations and the library's tie-breaking differs from torch's
        counts = collect(check, gd[0], g32[0], g64[0], f"{name} d h", rtol=1e-4, atol=2e-5)
        if counts is not None:
            ours_flips, allowed = counts.local + counts.escaped, 10 * max(counts.oracle_fp32_flips, 1)
            note(f"PARITY {name} d h: local + escaped = {ours_flips}, oracle_fp32_flips = {counts.oracle_fp32_flips}, "
                 f"ratio {ours_flips / max(counts.oracle_fp32_flips, 1):.3f} (allowed 10)")
            if ours_flips > allowed:
                failures.append(f"{name} d h: {ours_flips} entries on the fp64 clauses, the oracle's own flips {counts.oracle_fp32_flips}")
        for a, r32, r64, r64d, k in zip(gd[1:], g32[1:], g64[1:], g64_dropped[1:], names):
            collect(check_reduced, a, r32, r64, f"{name} {k}")
            if numerically_zero(r64):
                continue          # (a bias in front of a BatchNorm: check's bound, no ratio, and nothing a dropped slab could change)
            gap = float((r64d - r64).abs().max())
            try:
                check_reduced(r64d, r32, r64, f"{name} {k} [fp64 oracle WITHOUT the cotangent's last 64 rows: to be rejected]")
            except AssertionError:
                continue
            failures.append(f"{name} {k}: check_reduced accepted a gradient that lost the last 64 rows (max|r64 - r64_dropped| = {gap:.3e})")
        collect(_check_running_stats, lay, stats)
        assert not failures, f"{len(failures)} failed:\n" + "\n".join(failures)
    finally:
        y = gd = lay = y32 = y64 = g32 = g64 = g64_dropped = layer_dev = graph = h_dev = ct_dev = snorm = oracle = None
        gc.collect()
        torch.cuda.empty_cache()
