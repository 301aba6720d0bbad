"""The two one-kernel backward routes of the sweep that ``dgn_agg_backward[_aux]`` tries before the staged kernels -- ``agg_bwd_block``
(csrc/dgn_agg_block.hpp: one wave owns a run of whole graphs, d x_src in LDS) and ``agg_bwd_graph`` (csrc/dgn_agg_graph.hpp: one
workgroup owns one graph) --, through the C ABI with structs this test fills, on the machinery of tests/test_agg_grid_gpu.py (inputs,
conditioning, NaN-framed views, poisoned workspaces, the kernel-name normaliser) and the graphs and restatements of
tests/agg_blk_graphs.py.  The descriptions handed to the library (blk_cut / blk_gap, gblk_desc / csc_order / dst_csr) are always the
truthful ones of that module.

Judgement in every cell: gradients against tests/agg_ref.py in fp64 at ``1e-4 max(1, max|r64|)``; a second call gives the same bits; a
third call with the description removed (the staged path) gives the same bits on the block route where d x_in does not alias d x_src,
agreement within 2e-6 of scale where it does, the fp64 tolerance alone on the graph route (d x_dst is a closed form there); on the
graph route every feature tiling that fits the LDS gives the same bits.  A declined cell (one condition of the dispatch flipped) gives
the staged path's own bits with and without the description.  ``test_every_cell_runs_the_kernels_it_was_designed_for`` proves the
instance of every cell by kernel name under the profiler.

``blk_min_nodes`` is 0 for this module (monkeypatch on ``_lib.options``); ``blk_lds_kb``, ``graph_bwd_tiles`` and
``bwd_rows_per_wave`` are set where a cell names them, and restored."""
import ctypes as C
import os
import re
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import pytest
import torch

import agg_blk_graphs as BG
import test_agg_grid_gpu as G
from test_agg_grid_gpu import AV, DN, DX, HOT, M, MN, MX, Buf, Bytes

pytestmark = pytest.mark.gpu

for _n in BG.ALL_GRAPHS:                      # (the grid's `problem` / `Launch` look graphs up by name)
    G._GRAPHS[_n] = BG.graph(_n)

ODD_LISTS = G.ODD_LISTS
GRAPH_LISTS = [l for l in HOT if not l.stats]                 # rows 3-9, 13, 14 of dgn_agg_hot.hpp: no max / min / std / var
DYN1 = next(l for l in G.DYN if l.n_ch == 1 and not l.stats and not l.av)


def has_dx(lst):
    return DX in lst.ops


def recomputes(lst):
    return any(o in (MX, MN, DX) for o in lst.ops)


def aux_ok(lst):
    """the lists that have an aux table at all (dgn_agg.hip: agg_aux_supported)"""
    return lst.hot and recomputes(lst) and not lst.has_var and lst.n_ch <= 2


@dataclass(frozen=True)
class BCell(G.Cell):
    route: str = "blk"                                  # blk | gph
    taken: bool = True
    opts: Tuple[Tuple[str, int], ...] = ()              # library options of the cell, besides blk_min_nodes = 0
    null: Tuple[str, ...] = ()                          # sinks (or log_deg) handed over as NULL
    why: str = ""                                       # declined cells: the flipped condition

    @property
    def lds_kb(self):
        return dict(self.opts).get("blk_lds_kb", 13)

    @property
    def tiles_opt(self):
        return dict(self.opts).get("graph_bwd_tiles", 0)


def blk_plan_of(c: BCell):
    return BG.blk_plan(c.F, BG.graph(c.graph).blk_gap, c.lds_kb)


def graph_plan_of(c: BCell, tiles=None):
    g = BG.graph(c.graph)
    alias = c.xin == "alias" and c.lst.needs_xin
    return BG.graph_plan(c.F, len(g.sizes), g.gblk_rows, c.lst.n_ch, c.lst.av, alias, c.tiles_opt if tiles is None else tiles,
                         need_signs=recomputes(c.lst), has_aux=c.aux)


# input seeds of the cells whose default (the list's row) does not condition the reference: more than 0.5 % of a [197, 6] tensor left out
# where x_in aliases x_src; the grid's 40 rounds of its std / var rule not enough
SEEDS = {"blk-hot1-mol23-aux": 41, "blk-hot4-mol23-aux": 41, "blk-hot9-mol37-plain": 64}


def _cells():
    cells, seen = [], set()

    def add(**kw):
        c = BCell(vec=kw.pop("vec", 2), **kw)
        assert c.name not in seen, c.name
        seen.add(c.name)
        cells.append(c)

    # ---- block route ----------------------------------------------------------------------------------------------------------------
    # 1. every row of dgn_agg_hot.hpp, plain and (where the list has one) with its aux table, on mol37 at F = 70 and mol23 at F = 6; the
    #    message forms take turns: x_src with x_in aliased, x_src with a separate x_in, x_src + x_dst, the pair form (x_src + x_dst of a
    #    P|Q buffer) with the x_in pass-through on rows 11-14
    forms = (("s", "alias"), ("s", "sep"), ("sd", "sep"))
    for i, lst in enumerate(HOT):
        for j, aux in enumerate((False, True)):
            if aux and not aux_ok(lst):
                continue
            for gi, (gname, F) in enumerate((("mol37", 70), ("mol23", 6))):
                terms, xin = ("sd", "sep") if i >= 10 else forms[(i + j + gi) % 3]
                # (aliased, the abs-dx residuals cannot be conditioned: with two channels or more the entries left out would pass 0.5 %)
                if xin == "alias" and (not lst.needs_xin or (has_dx(lst) and lst.n_ch >= 2)):
                    xin = "sep"
                name = f"blk-{lst.name}-{gname}-{'aux' if aux else 'plain'}"
                add(name=name, graph=gname, F=F, lst=lst, terms=terms, xin=xin, aux=aux, seed=SEEDS.get(name, i))
    # 2. widths at 8-byte lanes on a list of each AHEAD class (at most two upstream blocks: row 3, the only class that requests the
    #    group's operands a group early; more: row 1); from F = 126 on a wave's 13 KB hold 26 rows: mol23
    for lst in (HOT[2], HOT[0]):
        for k, F in enumerate((2, 6, 46, 70, 76, 126, 128)):
            gname = "mol37" if F <= 76 else "mol23"
            if (gname, F) in (("mol37", 70),):
                continue                                                       # (section 1)
            alias = lst is HOT[2] and k % 2 == 0
            add(name=f"blk-width-{lst.name}-{gname}-F{F}", graph=gname, F=F, lst=lst, terms="s" if alias or k % 3 else "sd", xin="alias" if alias else "sep", seed=k)
    # 3. rows of an odd width on the two lists with such kernels, NaN directly behind every row
    for lst in ODD_LISTS:
        for fv in (5, 75, 127):
            add(name=f"blk-odd-{lst.name}-{fv}", graph="mol37" if fv < 127 else "mol23", F=fv + 1, lst=lst, f_valid=fv,
                xin="alias" if fv == 75 and lst.ops == (M, DN) else "sep")
    add(name="blk-odd-aux-75", graph="mol37", F=76, lst=ODD_LISTS[1], f_valid=75, aux=True)
    # 4. towers
    for lst in (HOT[0], HOT[10]):
        for layout in ("tower", "tower_dense"):
            add(name=f"blk-towers-T5-{lst.name}-{layout}", graph="mol37", F=70, T=5, lst=lst, layout=layout, terms="sd", aux=layout == "tower")
    for layout in ("tower", "tower_dense"):
        add(name=f"blk-towers-T2-{HOT[7].name}-{layout}", graph="mol37", F=68, T=2, lst=HOT[7], layout=layout, terms="sd")
    # 5. sinks the caller does not want, no log_deg
    add(name="blk-no-gdst", graph="mol37", F=70, lst=HOT[0], terms="sd", null=("g_dst",))
    add(name="blk-no-gin", graph="mol37", F=70, lst=HOT[10], terms="sd", null=("g_in",), aux=True)
    add(name="blk-no-gdst-gin", graph="mol23", F=6, lst=HOT[3], terms="sd", null=("g_dst", "g_in"))
    add(name="blk-no-logdeg", graph="mol37", F=70, lst=HOT[1], terms="sd", null=("log_deg",))
    # 6. the LDS budget: 11 KB (bin == 4), 24 KB (rcap == gap + 15); 13 KB is everywhere else
    for kb in (11, 24):
        add(name=f"blk-lds{kb}-hot0", graph="mol37", F=70, lst=HOT[0], terms="sd", opts=(("blk_lds_kb", kb),), aux=kb == 11)
        add(name=f"blk-lds{kb}-hot2", graph="mol37", F=70, lst=HOT[2], xin="alias", opts=(("blk_lds_kb", kb),))
    # 7. the other graphs: the largest gap (rcap == kBlkRowsMax), one bin in total, a boundary that is no closed cut
    add(name="blk-mol52-hot0", graph="mol52", F=46, lst=HOT[0], terms="sd", aux=True)
    add(name="blk-mol52-hot2", graph="mol52", F=46, lst=HOT[2], xin="alias")
    add(name="blk-one-hot0", graph="mol_one", F=70, lst=HOT[0], terms="sd", aux=True)
    add(name="blk-one-hot2", graph="mol_one", F=70, lst=HOT[2], xin="alias")
    add(name="blk-chain-hot0", graph="mol_chain", F=46, lst=HOT[0], terms="sd")
    add(name="blk-chain-hot3", graph="mol_chain", F=46, lst=HOT[3], aux=True)
    # 8. row 10 (std, three scalers: every row through bwd_any_row<.., BLK> with the std term of emit_batch) at a third width
    add(name="blk-hot9-F30", graph="mol37", F=30, lst=HOT[9], terms="sd")
    # ---- block route, declined: one condition of dgn_agg_backward_aux / launch_backward_block_cfg flipped each -----------------------------
    base = dict(graph="mol37", F=70, lst=HOT[0], terms="sd", taken=False)
    add(name="blk-declined-accum", bwd="accum", why="accumulate mode", **base)
    add(name="blk-declined-hub", hub=(64, 64), why="a hub description", **base)
    wide = (("blk_lds_kb", 24),)                                      # (so that blk_plan would still accept rows of 130 floats)
    add(name="blk-declined-F130", **dict(base, graph="mol23", F=130), opts=wide, why="two feature tiles")
    add(name="blk-declined-vec1", vec=1, why="4-byte lanes", **base)
    add(name="blk-declined-vec4", vec=4, **dict(base, graph="mol23", F=132), opts=wide, why="16-byte lanes")
    add(name="blk-declined-medge", **dict(base, terms="se"), null=("g_edge",), why="m_edge")
    add(name="blk-declined-table", **dict(base, terms="st"), K=4, why="an edge-type table")
    add(name="blk-declined-no-gsrc", bwd="no_gsrc", why="g_src NULL", **base)
    add(name="blk-declined-bip", **dict(base, graph="mol_bip", F=6), why="n_src != n_nodes")
    add(name="blk-declined-gedge", **dict(base, terms="se"), why="g_edge wanted")
    add(name="blk-declined-dyn", **dict(base, lst=DYN1), why="a generic list")
    add(name="blk-declined-rpw1", opts=(("bwd_rows_per_wave", 1),), why="bwd_rows_per_wave = 1", **base)
    add(name="blk-declined-min-nodes", opts=(("blk_min_nodes", 1 << 20),), why="n_nodes below blk_min_nodes", **base)
    add(name="blk-declined-plan", **dict(base, graph="mol52"), why="blk_plan refuses (47 rows of LDS, a graph of 52)")
    # ---- graph route ----------------------------------------------------------------------------------------------------------------
    gph = dict(route="gph", graph="knn")
    # 1. the nine lists, with the aux table where the list has a dx aggregator (without it: the staged path, below); with and without
    #    x_dst in turn, and both on the lists with |w| coefficients (d x_dst is a closed form of the row's coefficients)
    for i, lst in enumerate(GRAPH_LISTS):
        alias = lst.ops == (M, DN)
        add(name=f"gph-{lst.name}", F=70, lst=lst, terms="s" if alias or i % 2 else "sd", xin="alias" if alias else "sep", aux=has_dx(lst), seed=i, **gph)
    for lst in (HOT[3], HOT[4], HOT[8], HOT[12]):
        c = next(c for c in cells if c.name == f"gph-{lst.name}")
        add(name=f"gph-{lst.name}-{'s' if c.terms == 'sd' else 'sd'}", F=70, lst=lst, terms="s" if c.terms == "sd" else "sd", aux=has_dx(lst), seed=20, **gph)
    add(name="gph-hot2-sep-sd", F=70, lst=HOT[2], terms="sd", **gph)
    # 2. widths: one to 64 feature pairs, every tiling the batch size chooses (1, 2, 4)
    for lst in (HOT[3], HOT[2]):
        for k, F in enumerate((2, 6, 30, 66, 126, 128)):
            alias = lst is HOT[2] and k % 2 == 0
            add(name=f"gph-width-{lst.name}-F{F}", F=F, lst=lst, terms="s" if alias or k % 2 else "sd", xin="alias" if alias else "sep", aux=has_dx(lst), seed=k, **gph)
    # 3. the tiling named by the option; one graph of 300 rows at F = 128: 115 KB of LDS with four tiles
    for t in (1, 2, 3):
        add(name=f"gph-tiles{t}", F=70, lst=HOT[4], terms="sd", aux=True, opts=(("graph_bwd_tiles", t),), **gph)
    add(name="gph-big-F128", F=128, lst=HOT[3], terms="sd", aux=True, route="gph", graph="knn_big")
    # ---- graph route, declined ------------------------------------------------------------------------------------------------------------
    add(name="gph-declined-lds", F=128, lst=HOT[3], terms="sd", aux=True, route="gph", graph="knn_big", opts=(("graph_bwd_tiles", 1),), taken=False,
        why="LDS: 300 rows x 3 coefficient vectors x 128 floats")
    add(name="gph-declined-short", F=70, lst=HOT[2], terms="sd", route="gph", graph="short_g", taken=False, why="a short-route graph")
    for lst in (HOT[3], HOT[12]):
        add(name=f"gph-declined-no-aux-{lst.name}", F=70, lst=lst, terms="sd", taken=False, why="a dx aggregator without its aux table", **gph)
    base = dict(F=70, lst=HOT[2], terms="sd", taken=False, **gph)
    add(name="gph-declined-accum", bwd="accum", why="accumulate mode", **base)
    add(name="gph-declined-hub", hub=(64, 64), why="a hub description", **base)
    add(name="gph-declined-F130", **dict(base, F=130), why="two feature tiles")
    add(name="gph-declined-vec1", vec=1, why="4-byte lanes", **base)
    add(name="gph-declined-vec4", vec=4, **dict(base, F=132), why="16-byte lanes")
    add(name="gph-declined-medge", **dict(base, terms="se"), null=("g_edge",), why="m_edge")
    add(name="gph-declined-table", **dict(base, terms="st"), K=4, why="an edge-type table")
    add(name="gph-declined-no-gsrc", bwd="no_gsrc", why="g_src NULL", **base)
    add(name="gph-declined-bip", **dict(base, graph="knn_bip"), why="n_src != n_nodes")
    add(name="gph-declined-gedge", **dict(base, terms="se"), why="g_edge wanted")
    add(name="gph-declined-dyn", **dict(base, lst=DYN1), why="a generic list")
    return cells


CELLS = _cells()


# ---- one launch -------------------------------------------------------------------------------------------------------------------
_DESC = {}


def _copy(struct):
    c = type(struct)()
    C.memmove(C.byref(c), C.byref(struct), C.sizeof(c))
    return c


def described(cell: BCell, base):
    """a copy of the grid's DgnGraph struct with the route's truthful description attached"""
    g = BG.graph(cell.graph)
    if cell.graph not in _DESC:
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(G._dev())
        _DESC[cell.graph] = dict(blk_cut=i32(g.blk_cut), gblk_desc=i32(g.gblk_desc), csc_order=i32(g.csc_order), dst_csr=i32(g.dst))
    t = _DESC[cell.graph]
    c = _copy(base)
    if cell.route == "blk":
        assert 0 < g.blk_gap <= BG.BLOCK_MAX_GAP and len(g.blk_cut) == g.N + 1
        c.blk_cut, c.blk_gap = t["blk_cut"].data_ptr(), g.blk_gap
    else:
        assert t["gblk_desc"].data_ptr() % 16 == 0
        c.gblk_desc, c.n_gblk, c.gblk_rows = t["gblk_desc"].data_ptr(), len(g.sizes), g.gblk_rows
        c.csc_order, c.dst_csr = t["csc_order"].data_ptr(), t["dst_csr"].data_ptr()
    return c


class BLaunch(G.Launch):
    def __init__(self, cell: BCell):
        super().__init__(cell)
        self.cg_plain = self.cg
        self.cg_desc = described(cell, self.cg)
        self.cg = self.cg_desc

    def _args(self, spec):
        a = super()._args(spec)
        return a[:5] + (None,) if "log_deg" in self.cell.null else a

    def sinks(self, accumulate):
        cell, g, F, vec, p = self.cell, self.g, self.cell.F, self.cell.vec, self.p
        null = set(cell.null) | ({"g_src"} if cell.bwd == "no_gsrc" else set())
        init = (lambda k: p["accum"][k]) if accumulate else (lambda k: None)
        s = {}
        if p["x_src"] is not None and "g_src" not in null:
            s["g_src"] = Buf(g.n_src, F, vec, init("g_src"))
        if p["x_dst"] is not None and "g_dst" not in null:
            s["g_dst"] = Buf(g.N, F, vec, init("g_dst"))
        if p["m_edge"] is not None and "g_edge" not in null:
            s["g_edge"] = Buf(p["m_edge"].shape[0], F, vec, init("g_src")[:1].repeat(p["m_edge"].shape[0], 0) if accumulate else None)
        if p["x_in"] is not None and "g_in" not in null:
            if p["alias"]:
                if "g_src" in s:
                    s["g_in"] = s["g_src"]
            else:
                s["g_in"] = Buf(g.N, F, vec, init("g_in"))
        gr = self.L.DgnMsgGrad()
        gr.accumulate = int(accumulate)
        for k, b in s.items():
            setattr(gr, k, b.ptr)
            setattr(gr, "ld_" + k[2:], b.ld)
        return s, gr


def _same(a, b, what, keep=None):
    for k in a:
        x, y = (a[k], b[k]) if keep is None or k != "g_dst" else (a[k][keep], b[k][keep])
        assert np.array_equal(x, y), f"{what} ({k}): {float(np.abs(x - y).max()):.3e}"


def run_cell(cell: BCell, monkeypatch, compare=True):
    """forward and backward of one cell; with compare=False one launch of each (the instance proof)"""
    L, _ = G._lib()
    with monkeypatch.context() as mp:
        for k, v in cell.opts:
            mp.setattr(L.options, k, v)
        ln = BLaunch(cell)
        p, g = ln.p, BG.graph(cell.graph)
        family = cell.route + ("" if cell.taken else "-declined")
        aux = None
        if cell.aux:
            n = ln.aux_bytes()
            assert n > 0, cell.name
            aux = Bytes(n)
        out = ln.forward(aux=aux)
        if aux is not None:
            aux.check("aux table")
        if compare:
            got = ln._from_layout(out.read(f"{cell.name} out"))
            G._close(got, p["ref"]["out"], 1e-5, f"{cell.name} out")
        accumulate, two_phase = cell.bwd == "accum", cell.two_phase
        s, _ = ln.backward(accumulate, two_phase, aux=aux)
        if not compare:
            return
        got = G._read_sinks(s, cell.name)
        G._check_grads(cell, p, got, accumulate, family + "-bwd")
        keep = (g.degs <= cell.hub[0]) if cell.hub else None       # (the slices of a hub row add their shares of d x_dst with atomics)
        again = G._read_sinks(ln.backward(accumulate, two_phase, aux=aux)[0], cell.name)
        _same(got, again, f"{cell.name}: two calls differ", keep)
        ln.cg = ln.cg_plain                                         # the description removed: the staged path
        staged = G._read_sinks(ln.backward(accumulate, two_phase, aux=aux)[0], cell.name)
        ln.cg = ln.cg_desc
        G._check_grads(cell, p, staged, accumulate, "staged-bwd")
        if not cell.taken:
            _same(got, staged, f"{cell.name}: declined, yet the description changed the bits", keep)
        elif cell.route == "blk":
            for k in got:
                if p["alias"] and k in ("g_src", "g_in"):           # d x_in joins d x_src at another position of the sum
                    scale = float(np.abs(staged[k]).max())
                    assert float(np.abs(got[k] - staged[k]).max()) <= 2e-6 * scale, (cell.name, k, float(np.abs(got[k] - staged[k]).max()), scale)
                else:
                    assert np.array_equal(got[k], staged[k]), f"{cell.name} {k}: the block backward and the staged path differ"
        if cell.taken and cell.route == "gph" and not cell.tiles_opt:      # every tiling that fits gives the same bits
            for tiles in (1, 2, 3, 4):
                if graph_plan_of(cell, tiles) is None:
                    continue
                mp.setattr(L.options, "graph_bwd_tiles", tiles)
                tiled = G._read_sinks(ln.backward(accumulate, two_phase, aux=aux)[0], cell.name)
                _same(got, tiled, f"{cell.name}: graph_bwd_tiles = {tiles} changed the bits")


@pytest.fixture(autouse=True)
def _blk_min_nodes_zero(monkeypatch):
    L, _ = G._lib()
    monkeypatch.setattr(L.options, "blk_min_nodes", 0)
    yield


@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_cell(cell, monkeypatch):
    run_cell(cell, monkeypatch)


def test_options_are_restored():
    L, _ = G._lib()
    assert L.options.blk_lds_kb == 13 and L.options.graph_bwd_tiles == 0 and L.options.bwd_rows_per_wave == 4


@pytest.mark.parametrize("n_nodes", [0, 7])
def test_no_rows_and_no_edges_with_the_descriptions_attached(n_nodes):
    """n_nodes == 0: nothing is launched or written; E == 0 (every node a graph of its own): zero gradients, the x_in pass-through apart"""
    L, lib = G._lib()
    dev = G._dev()
    c, keep = G._tiny(n_nodes, 0)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    cut, gap = BG.closed_cuts(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), n_nodes)
    assert gap == (1 if n_nodes else 0)
    desc = np.stack([np.arange(n_nodes), np.arange(n_nodes) + 1, np.zeros(n_nodes), np.zeros(n_nodes)], axis=1).reshape(-1, 4)
    keep.update(cut=i32(cut), desc=i32(desc if n_nodes else np.zeros((1, 4))), none=i32(np.zeros(1)), csc_ptr=i32(np.zeros(n_nodes + 1)))
    c.blk_cut, c.blk_gap = keep["cut"].data_ptr(), gap
    c.gblk_desc, c.n_gblk, c.gblk_rows = keep["desc"].data_ptr(), n_nodes, min(n_nodes, 1)
    c.csc_order = c.dst_csr = c.csc_pos = keep["none"].data_ptr()
    c.csc_ptr = keep["csc_ptr"].data_ptr()
    F = 6
    lst = HOT[12]                                                   # mean dir1-dx dir1-av __x_in__
    spec = L.DgnAggSpec()
    spec.n_agg, spec.n_ch, spec.n_scalers, spec.n_towers, spec.avg_log, spec.eps = len(lst.ops), lst.n_ch, 1, 1, G.AVG_LOG, G.EPS
    for a, (o, ch) in enumerate(zip(lst.ops, lst.chs)):
        spec.agg_op[a], spec.agg_ch[a] = o, ch
    A = len(lst.ops)
    x = G._lattice(np.random.default_rng(0), (max(n_nodes, 1), F))
    xs, xi, g_out = Buf(max(n_nodes, 1), F, 2, x), Buf(max(n_nodes, 1), F, 2, x + 1), Buf(n_nodes, A * F, 2, np.ones((n_nodes, A * F)))
    w = Buf(1, 1, 1, np.zeros((1, 1)), spare=1)
    msg = L.DgnMsg()
    msg.F, msg.x_src, msg.ld_src, msg.x_in, msg.ld_in = F, xs.ptr, xs.ld, xi.ptr, xi.ld
    sinks = dict(g_src=Buf(n_nodes, F, 2), g_in=Buf(n_nodes, F, 2))
    gr = L.DgnMsgGrad()
    gr.g_src, gr.ld_src, gr.g_in, gr.ld_in = sinks["g_src"].ptr, sinks["g_src"].ld, sinks["g_in"].ptr, sinks["g_in"].ld
    L.check(lib.dgn_agg_backward(C.byref(c), C.byref(spec), C.byref(msg), w.ptr, w.ld, None, g_out.ptr, g_out.ld, C.byref(gr), None, 0,
                                 L.stream_ptr(dev)), "backward")
    torch.cuda.synchronize()
    gs, gi = sinks["g_src"].read("g_src"), sinks["g_in"].read("g_in")
    if n_nodes:
        assert (gs == 0).all() and (gi == 1).all()


# ---- the instance proof -------------------------------------------------------------------------------------------------------------
_PACKS = {}
for _i, _l in enumerate(HOT):
    _PACKS[(len(_l.ops), sum(o << (4 * a) for a, o in enumerate(_l.ops)), sum(c << (3 * a) for a, c in enumerate(_l.chs)), len(_l.scalers),
            sum(s << (2 * k) for k, s in enumerate(_l.scalers)))] = _i
STAGED = ("agg_bwd_short", "agg_bwd_rows", "seg_sum_rows")


def _key(name):
    """'agg_bwd_block|2,1,1,1,0|hot0|1': kernel, Cfg arguments (ODD spelled out), the row of dgn_agg_hot.hpp (or 'dyn'), the flags behind"""
    key = G._kernel_key(name)
    if not key or not key.startswith("agg_"):
        return key
    parts = key.split("|")
    mt = re.search(r"StaticOps<(\d+),(\d+),(\d+),(\d+),(\d+)>", G._norm(name))
    parts[2] = f"hot{_PACKS[tuple(int(x) for x in mt.groups())]}" if mt else ("dyn" if parts[2] == "D" else "-")
    return "|".join(parts)


def expected_route_kernel(c: BCell):
    lst = c.lst
    cfg = f"2,{lst.n_ch},{int(lst.stats)},{int(lst.av)},{int(bool(c.f_valid))}"
    if c.route == "blk":
        return f"agg_bwd_block|{cfg}|{lst.name}|{int(c.aux)}"
    return f"agg_bwd_graph|2,{lst.n_ch},0,{int(lst.av)},0|{lst.name}|"


def test_every_cell_runs_the_kernels_it_was_designed_for(monkeypatch):
    """Every cell once more under the profiler (one forward and one backward each, a sort between cells as the separator).  A taken cell
    runs exactly its instance -- agg_bwd_block<Cfg<2, NCH, STATS, AV[, true]>, StaticOps<..>, AUX> or agg_bwd_graph<Cfg, StaticOps> -- and
    none of the staged kernels; a declined cell runs the staged kernels and neither of the two.  Together the cells name every instance
    the library can launch: the 14 lists, the 10 of them that have an aux table with AUX, the two odd-width kernels (the one with a dx
    aggregator also with AUX), and the nine graph lists."""
    from torch.profiler import ProfilerActivity, profile
    dev = G._dev()
    for c in CELLS:
        G.problem(c)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for c in CELLS:
            run_cell(c, monkeypatch, compare=False)
            torch.arange(64, device=dev, dtype=torch.float32).sort()
            torch.cuda.synchronize()
    evs = sorted((e for e in prof.profiler.kineto_results.events() if str(e.device_type()).endswith("CUDA")), key=lambda e: e.start_ns())
    names = [e.name() for e in evs]
    if G.DUMP:
        with open(os.path.join(G.DUMP, "agg_blk_grid_kernels.txt"), "w") as f:
            f.write("\n".join(names))
    got, cur = [], []
    for n in names:
        if "sort" in n.lower():
            if cur:
                got.append(cur)
                cur = []
            continue
        key = _key(n)
        if key:
            cur.append(key)
    assert len(got) == len(CELLS), (len(got), len(CELLS))
    tally, wrong = {}, []
    for c, keys in zip(CELLS, got):
        bwd = [k for k in keys if k.startswith(("agg_bwd_block", "agg_bwd_graph") + STAGED)]
        if c.taken:
            ok = bwd == [expected_route_kernel(c)]
        else:
            ok = not any(k.startswith(("agg_bwd_block", "agg_bwd_graph")) for k in bwd) and any(k.startswith(("agg_bwd_short", "agg_bwd_rows")) for k in bwd)
            ok = ok and (any(k.startswith("seg_sum_rows") for k in bwd) == (c.two_phase and "s" in c.terms))
        if not ok:
            wrong.append((c.name, bwd))
        for k in bwd:
            tally[k] = tally.get(k, 0) + 1
    if G.DUMP:
        with open(os.path.join(G.DUMP, "agg_blk_grid_tally.txt"), "w") as f:
            f.write("\n".join(f"{k} {v}" for k, v in sorted(tally.items())))
        with open(os.path.join(G.DUMP, "agg_blk_grid_ratios.txt"), "w") as f:
            f.write("\n".join(f"{k} error/tolerance {G.RATIOS[k]:.4f} error/fp32-error {G.VS_FP32.get(k, 0.0):.3f}" for k in sorted(G.RATIOS)))
    assert not wrong, wrong[:10]
    cfg = lambda l, odd=0: f"2,{l.n_ch},{int(l.stats)},{int(l.av)},{odd}"
    block = {f"agg_bwd_block|{cfg(l)}|{l.name}|0" for l in HOT} | {f"agg_bwd_block|{cfg(l)}|{l.name}|1" for l in HOT if aux_ok(l)}
    block |= {f"agg_bwd_block|{cfg(l, 1)}|{l.name}|0" for l in ODD_LISTS} | {f"agg_bwd_block|{cfg(l, 1)}|{l.name}|1" for l in ODD_LISTS if aux_ok(l)}
    graph = {f"agg_bwd_graph|{cfg(l)}|{l.name}|" for l in GRAPH_LISTS}
    assert len(block) == 14 + 10 + 2 + 1 and len(graph) == 9
    assert {k for k in tally if k.startswith("agg_bwd_block")} == block, sorted(block ^ {k for k in tally if k.startswith("agg_bwd_block")})
    assert {k for k in tally if k.startswith("agg_bwd_graph")} == graph, sorted(graph ^ {k for k in tally if k.startswith("agg_bwd_graph")})
    family = lambda pre: sum(v for k, v in tally.items() if k.startswith(pre))
    counts = {k: family(k) for k in ("agg_bwd_block|", "agg_bwd_graph|", "agg_bwd_short|", "agg_bwd_rows|", "seg_sum_rows|")}
    assert counts == LAUNCHES, counts


# launches of the backward kernels over all cells (one backward each): one agg_bwd_block / agg_bwd_graph per taken cell and nothing
# else; per declined cell one sweep kernel -- agg_bwd_short on the short-route graphs in define mode with x_src wanted and four rows per
# wave (blk: hub F130 vec1 vec4 medge table bip gedge min-nodes plan; gph: short), agg_bwd_rows otherwise (blk: accum no-gsrc dyn rpw1;
# gph: the other 14) -- and one seg_sum_rows wherever g_src is wanted (all but the two no-gsrc cells)
LAUNCHES = {"agg_bwd_block|": 88, "agg_bwd_graph|": 30, "agg_bwd_short|": 11, "agg_bwd_rows|": 18, "seg_sum_rows|": 27}
