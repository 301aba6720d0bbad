"""Host predicates over the baked-in aggregator lists (csrc/dgn_agg_hot.hpp), no GPU: the committed table is what its generator renders, and
dgn_agg_f_valid_supported / dgn_layer_fused_supported answer for every row of the table and for one-step perturbations of it.

A perturbation changes the DgnAggSpec, which is all the host sees of a list: the first two aggregators swapped; the last directional
aggregator moved to an eig column of its own (in the spec that is a new channel: index n_ch, n_ch + 1 -- renaming the only direction of a
list leaves the spec as it was); one more scaler; the list as a slice (agg_offset = 1 of agg_total = n_agg + 1)."""
import ctypes as C
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HOT_ON = "DGN_NO_HOT" not in os.environ                         # (the switch of the README: present = generic kernels everywhere)
ODD_WIDTH = ("mean dir1-dx-no-abs", "mean dir1-dx dir2-dx")      # the lists with kernels for rows of an odd width (Cfg::ODD)


@pytest.fixture(scope="module")
def lib():
    from dgn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_hot_lists", os.path.join(ROOT, "tools", "gen_hot_lists.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _spec_of(aggs, scalers):
    from dgn_amd import ops, spec
    plan = spec.make_plan(aggs.split(), scalers.split())
    assert len(plan.launches) == 1
    return ops._spec_structs(plan, 1, 1.0, 0)[0]


def _perturbed(s):
    from dgn_amd import _lib, spec
    out = {}
    if s.n_agg > 1:
        t = _lib.DgnAggSpec.from_buffer_copy(s)
        t.agg_op[0], t.agg_op[1], t.agg_ch[0], t.agg_ch[1] = s.agg_op[1], s.agg_op[0], s.agg_ch[1], s.agg_ch[0]
        out["swapped"] = t
    dirs = [a for a in range(s.n_agg) if spec.AGG_DIR_AV <= s.agg_op[a] <= spec.AGG_DIR_DX_NO_ABS]
    if dirs:
        t = _lib.DgnAggSpec.from_buffer_copy(s)
        t.agg_ch[dirs[-1]], t.n_ch = s.n_ch, s.n_ch + 1
        out["eig column"] = t
    t = _lib.DgnAggSpec.from_buffer_copy(s)
    t.scaler[s.n_scalers], t.n_scalers = spec.SCALE_AMPLIFICATION, s.n_scalers + 1
    out["scaler added"] = t
    t = _lib.DgnAggSpec.from_buffer_copy(s)
    t.agg_offset, t.agg_total = 1, s.n_agg + 1
    out["slice"] = t
    return out


def test_committed_table_is_what_the_generator_renders(gen):
    with open(os.path.join(ROOT, "dgn_amd", "csrc", "dgn_agg_hot.hpp")) as f:
        assert f.read() == gen.render()


def test_f_valid_supported_over_the_table_and_its_perturbations(lib, gen):
    assert [aggs for aggs, scalers, _ in gen.HOT if aggs in ODD_WIDTH and scalers == "identity"] == list(ODD_WIDTH)
    n = 0
    for aggs, scalers, _ in gen.HOT:
        s = _spec_of(aggs, scalers)
        assert lib.dgn_agg_f_valid_supported(C.byref(s)) == (1 if aggs in ODD_WIDTH and HOT_ON else 0), aggs
        for what, t in _perturbed(s).items():
            assert lib.dgn_agg_f_valid_supported(C.byref(t)) == 0, (aggs, what)
            n += 1
        s.n_towers = 2
        assert lib.dgn_agg_f_valid_supported(C.byref(s)) == 0, aggs
    assert n == 4 * len(gen.HOT) - 2                 # ("mean" has neither two aggregators nor a direction)
    assert lib.dgn_agg_f_valid_supported(None) == 0


def test_layer_fused_supported_over_the_table_and_its_perturbations(lib, gen):
    from dgn_amd import _lib
    g = _lib.DgnGraph()                              # hub-free, not bipartite, short rows: never dereferenced
    g.n_nodes, g.n_edges, g.max_in_degree = 8, 16, 2
    F = 8                                            # (even, and K = n_agg * F <= 96 for every row of the table)
    supported = lambda s: lib.dgn_layer_fused_supported(C.byref(g), C.byref(s), F, 1, 8)
    for aggs, scalers, _ in gen.HOT:
        s = _spec_of(aggs, scalers)
        assert supported(s) == (1 if s.n_scalers == 1 and HOT_ON else 0), aggs
        for what, t in _perturbed(s).items():
            assert supported(t) == 0, (aggs, what)
    assert sum(len(sc.split()) == 3 for _, sc, _ in gen.HOT) == 1
    s = _spec_of(gen.HOT[0][0], gen.HOT[0][1])
    assert lib.dgn_layer_fused_supported(C.byref(g), C.byref(s), F + 1, 1, 8) == 0      # odd width
    g.n_hub = 1
    assert supported(s) == 0                         # hub rows
