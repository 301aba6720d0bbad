"""tests/agg_blk_graphs.py -- the graphs and host-side restatements behind tests/test_agg_blk_grid_gpu.py -- and that grid's cells: every
claim of the generators, the corners of blk_plan and of the graph backward's tiling the cells reach, and the conditioning of the
reference on every cell's inputs (the grid's own lattice inputs and its std / var and abs-dx rules, unchanged).  No GPU."""
import numpy as np
import pytest

import agg_blk_graphs as BG
import test_agg_blk_grid_gpu as B
import test_agg_grid_gpu as G

BLK = [c for c in B.CELLS if c.route == "blk"]
GPH = [c for c in B.CELLS if c.route == "gph"]


@pytest.mark.parametrize("name", BG.ALL_GRAPHS)
def test_whole_graphs_with_closed_boundaries(name):
    g = BG.graph(name)
    assert g.src.min() >= 0 and g.src.max() < g.N <= g.n_src
    assert np.array_equal(g.graph_of(g.src), g.graph_of(g.dst)), "a source outside its row's graph"
    # the closed cuts are exactly the graph boundaries: blk_cut[i] = the start of i's graph (N for i == N), the gap the largest graph
    want = np.concatenate([g.bounds[g.graph_of(np.arange(g.N))], [g.N]])
    assert np.array_equal(g.blk_cut, want) and g.blk_gap == g.sizes.max() == g.gblk_rows
    for lo, hi, s0, s1 in g.gblk_desc:                                    # every gblk_desc block is closed, and they partition the rows
        assert ((g.src[s0:s1] >= lo) & (g.src[s0:s1] < hi)).all() and (s0, s1) == (g.indptr[lo], g.indptr[hi])
    assert np.array_equal(g.gblk_desc[1:, 0], g.gblk_desc[:-1, 1]) and g.gblk_desc[0, 0] == 0 and g.gblk_desc[-1, 1] == g.N
    # csc_order / csc_pos / csc_ptr / dst_csr as include/dgn_hip.h states them
    assert np.array_equal(g.csc_order[g.csc_pos], np.arange(g.E)) and np.array_equal(np.sort(g.csc_order), np.arange(g.E))
    keys = g.src[g.csc_order] * (g.E + 1) + g.csc_order
    assert (np.diff(keys) > 0).all(), "csc_order is not ascending in (source, slot)"
    assert np.array_equal(np.diff(g.csc_ptr), np.bincount(g.src, minlength=g.n_src)) and len(g.csc_ptr) == g.n_src + 1
    assert np.array_equal(g.dst, np.repeat(np.arange(g.N), np.diff(g.indptr)))
    # duplicated sources, self loops, a source without an out-edge
    assert any(len(set(r)) < len(r) for r in g.rows) and (g.src == g.dst).any() and (g.out_deg[:g.N] == 0).any()
    assert g.route == ("short" if name.startswith(("mol", "short")) else "rows4")
    assert (g.E <= 3 * g.N) == (g.route == "short")


def test_block_graphs():
    g = BG.graph("mol37")
    assert set(BG.MOL37_MUST) <= set(g.sizes.tolist()) and g.sizes.max() == 37 and 480 <= g.N <= 540 and g.N % 4 == 3
    assert g.degs[g.bounds[g.sizes.tolist().index(1)]] == 0                                   # the isolated node
    hist = np.bincount(g.degs)
    assert hist[1:5].sum() >= 0.9 * g.N and hist[0] >= 5 and hist[5:10].sum() == 1 and hist[70] == 1 and hist[10:70].sum() == 0
    long_row = int(np.argmax(g.degs))
    assert len(set(g.rows[long_row])) == 7
    bin_, rcap = BG.blk_plan(70, g.blk_gap)
    assert (bin_, rcap) == (11, 47)
    bins = BG.blk_bins(g.blk_cut, g.N, bin_)
    assert {lo & 3 for lo, hi in bins if lo < hi} == {0, 1, 2, 3}
    for name, big, rem in (("mol23", 23, 1), ("mol52", 52, 2)):
        h = BG.graph(name)
        assert h.sizes.max() == h.blk_gap == big and h.N % 4 == rem and np.bincount(h.degs)[70] == 1
    assert BG.graph("mol52").blk_gap == BG.BLOCK_MAX_GAP
    one = BG.graph("mol_one")
    assert one.N == 5 and len(one.sizes) == 1
    a, b = BG.graph("mol23"), BG.graph("mol_chain")
    assert b.E == a.E + 1 and b.N == a.N and len(b.sizes) == len(a.sizes) - 1 and a.blk_gap < b.blk_gap <= BG.BLOCK_MAX_GAP
    joint = int(np.setdiff1d(np.unique(a.blk_cut), np.unique(b.blk_cut))[0])                   # the boundary that is no closed cut any more
    assert (b.src[b.indptr[joint]:b.indptr[joint + 1]] == joint - 1).any()
    assert BG.graph("mol_bip").n_src == BG.graph("mol_bip").N + 3


def test_graph_route_graphs():
    g = BG.graph("knn")
    assert g.sizes.tolist() == [9, 40, 85, 150]
    hist = np.bincount(g.degs)
    assert hist[8] >= 0.9 * g.N and hist[0] >= 3 and hist[70] == 1 and hist[0] + hist[8] + hist[70] == g.N
    assert g.out_deg.max() > 64 and (g.out_deg == 0).sum() == 1
    big = BG.graph("knn_big")
    assert big.sizes.tolist() == [300] and big.E > 3 * big.N
    for nco_alias in (3, 4):                                              # every tiling of one coefficient vector more is refused too
        assert 300 * nco_alias * 128 * 4 > BG.GRAPH_LDS_MAX


def test_restatements_on_hand_made_cases():
    # two graphs of 3 and 2 rows and an isolated node: cuts 0 3 5 6
    src, dst = np.array([1, 0, 1, 4]), np.array([0, 1, 2, 3])
    cut, gap = BG.closed_cuts(src, dst, 6)
    assert cut.tolist() == [0, 0, 0, 3, 3, 5, 6] and gap == 3
    assert BG.blk_bins(cut, 6, 4) == [(0, 3), (3, 6)] and BG.blk_bins(cut, 6, 2) == [(0, 0), (0, 3), (3, 6)]
    assert BG.blk_plan(70, 37, 13) == (11, 47) and BG.blk_plan(70, 37, 11) == (4, 40) and BG.blk_plan(70, 37, 24) == (16, 52)
    assert BG.blk_plan(46, 52, 13) == (5, 56) and BG.blk_plan(70, 52, 13) is None and BG.blk_plan(70, 5, 13) == (16, 20)
    # CIFAR10's list (two channels, no |w|) at F = 66 on 128 graphs of at most 118 rows: 1 + 2 coefficient vectors, two tiles
    assert BG.graph_plan(66, 128, 118, 2, False, False, has_aux=True, need_signs=True) == (2, (118 * 3 * 17 * 2 + 118 * 2) * 4)
    assert BG.graph_plan(66, 128, 118, 2, False, False, need_signs=True) is None
    assert BG.graph_plan(70, 4, 150, 1, True, False, 3)[0] == 3 and BG.graph_plan(2, 4, 150, 1, True, False, 4)[0] == 1


def test_block_cells_reach_the_corners_of_blk_plan():
    taken = [c for c in BLK if c.taken]
    for c in taken:
        assert B.blk_plan_of(c) is not None, c.name
        assert BG.graph(c.graph).route == "short" and c.vec == 2 and c.F <= 128
    plans = {c.name: B.blk_plan_of(c) for c in taken}
    gap = lambda c: BG.graph(c.graph).blk_gap
    assert any(p[0] == 4 for p in plans.values())
    assert any(p[1] == BG.K_BLK_ROWS_MAX == 56 for p in plans.values())
    assert any(p[1] == gap(c) + 15 < 56 for c, p in zip(taken, plans.values()))
    assert any(p[1] == (c.lds_kb * 1024) // (4 * c.F) < min(56, gap(c) + 15) for c, p in zip(taken, plans.values()))
    refused = [c for c in BLK if B.blk_plan_of(c) is None]
    assert [c.name for c in refused] == ["blk-declined-plan"] and not refused[0].taken
    n_bins, empty = set(), 0
    for c in taken:
        g = BG.graph(c.graph)
        bins = BG.blk_bins(g.blk_cut, g.N, plans[c.name][0])
        n_bins.add(len(bins))
        empty += any(lo >= hi for lo, hi in bins)
        assert max(hi - lo for lo, hi in bins) <= plans[c.name][1], c.name          # (what the LDS rows are sized for)
        assert sum(hi - lo for lo, hi in bins if lo < hi) == g.N, c.name             # every row in exactly one bin
    assert empty >= 10 and 1 in n_bins and any(n % 8 for n in n_bins) and {c.lds_kb for c in taken} == {11, 13, 24}
    # every condition of the dispatch flipped once
    assert len([c for c in BLK if not c.taken]) == 14 and len({c.why for c in BLK if not c.taken}) == 14
    assert {c.F for c in taken if not c.f_valid} >= {2, 6, 46, 70, 76, 126, 128} and {c.f_valid for c in taken} == {0, 5, 75, 127}
    assert {c.lst.name for c in taken} == {l.name for l in G.HOT}
    assert {c.lst.name for c in taken if c.aux} == {l.name for l in G.HOT if B.aux_ok(l)} and len({c.lst.name for c in taken if c.aux}) == 10


def test_graph_cells_reach_every_tiling_and_the_refusal():
    taken = [c for c in GPH if c.taken]
    tiles = set()
    for c in GPH:
        g = BG.graph(c.graph)
        plan = B.graph_plan_of(c)
        if c.taken:
            assert plan is not None and g.route != "short" and g.n_src == g.N, c.name
            tiles.add(plan[0])
            assert plan[1] <= BG.GRAPH_LDS_MAX
    assert tiles == {1, 2, 3, 4}
    assert B.graph_plan_of(next(c for c in GPH if c.name == "gph-declined-lds")) is None
    assert B.graph_plan_of(next(c for c in GPH if c.name == "gph-big-F128"))[1] > 64 * 1024       # (beyond the default LDS of a workgroup)
    assert all(B.graph_plan_of(c) is None for c in GPH if c.name.startswith("gph-declined-no-aux"))
    assert {c.lst.name for c in taken} == {l.name for l in B.GRAPH_LISTS} and len(B.GRAPH_LISTS) == 9
    assert {c.F for c in taken} >= {2, 6, 30, 66, 70, 126, 128} and {c.xin for c in taken} == {"alias", "sep"} and {c.terms for c in taken} == {"s", "sd"}
    # the tilings the cells sweep: at least one cell where all four fit
    assert any(all(B.graph_plan_of(c, t) is not None for t in (1, 2, 3, 4)) for c in taken if not c.tiles_opt)


@pytest.mark.parametrize("cell", B.CELLS, ids=[c.name for c in B.CELLS])
def test_the_reference_is_conditioned_on_every_cell(cell):
    """agg_ref.sweep's facts on the cell's inputs: std / var conditioned everywhere, every abs-dx residual conditioned where x_in is a
    separate tensor; where it aliases x_src the entries left out of a gradient comparison stay at or below 0.5 % of a tensor"""
    p = G.problem(cell)
    assert p["ref"]["var_ok"].all() or not cell.lst.has_var
    bad = ~p["ref"]["dx_ok"]
    if cell.f_valid:
        bad[:, -1] = False
    assert p["alias"] or not bad.any()
    for k, v in p["skip"].items():
        if v is not None:
            assert v.mean() <= 0.005, (cell.name, k, float(v.mean()))
            assert p["alias"] or not v.any()
    x = p["x_src"]
    assert np.array_equal(np.round(x / G.LATTICE), x / G.LATTICE) and np.abs(x).max() <= 4.0          # the grid's lattice, unchanged
