"""The directional-aggregation sweep kernels (csrc/dgn_agg_kernels.hpp) themselves, through the C ABI (``dgn_agg_forward[_aux]`` /
``dgn_agg_backward[_aux]``) with structs this test fills: no ``DGNGraph``, ``make_plan`` or ``ops.py`` on the way.  Judged against
tests/agg_ref.py in fp64 (tied to the oracle by tests/test_agg_ref_cpu.py) at the project's tolerances:
values ``1e-5 max(1, max|r64|)``, gradients ``1e-4 max(1, max|r64|)`` -- no ``4 x |fp32 - fp64|`` clause.

CELLS is the grid, one launch description each; ``test_cell`` runs a cell's forward and backward, ``test_every_cell_runs_the_kernels_it_
was_designed_for`` runs all of them once more under the profiler and proves the instance by kernel name.

Graphs (numpy; hub description, csc view and log_deg built here and checked once against ``DGNGraph``): ``ladder`` (E >= 8 N: the row
kernels at one wave per workgroup; one row of every in-degree 0 1 2 3 4 5 7 8 9 12 13 16 17 63 64 65 127 128 129 200 -- the 4 + 4 half-groups of
``accumulate_batch``, the 64-slot batch -- plus mid-degree rows, N = 203), ``ladder4`` (the ladder plus rows of 0..4 slots, 3 N < E < 8 N:
four waves per workgroup, N = 401), ``short`` (E <= 3 N: ``agg_fwd_short`` / ``agg_bwd_short``; groups (4,4,4,4), (1,2,3,1), one with an empty
row, one with a row of 5 slots that sends the group to the per-row routine; N = 303 = 3 mod 4, 76 groups: ``xcd_grid`` pads), ``shorthub``
(a short-route graph with one row of 300 slots), ``bip_lt`` / ``bip_gt`` (``n_src`` below / above ``n_nodes``, sources beyond
``n_nodes``), and the ladder with hub descriptions (threshold, slice) = (127, 48), (100, 80), (16, 7).  Every graph has duplicated sources,
self loops, a source without out-edge and sources of 1, 3, 4, 5, 8, 9 out-edges (``seg_sum_rows``' groups of four).

Inputs: x_src / x_dst / x_in multiples of 2^-8 in [-4, 4), m_edge multiples of 8: every message is exact in fp32, so maxima, minima and
their first slots are the same in both precisions.  w and g_out ~ N(0, 1) (the first weight of a row whose weights sum to less than
0.5 in magnitude is moved by 1: otherwise x_in has no say in that row's residual).  Conditioning (agg_ref.sweep's facts): a separate x_in is
moved by lattice steps until every abs-valued dx residual keeps ``|r_c| >= 1e-3 (sum_j |w_jc m_j| + |(sum_j w_jc) x_in|)``; where x_in
aliases x_src those (row, feature) entries, and every gradient entry that sums over one, are left out of the GRADIENT comparison (at
most 0.5 % of a tensor, asserted).  Lists with std / var: the first slot's gathered term of a row whose E[m^2] - mean^2 is positive but
below 1e-3 (E[m^2] + mean^2) is moved by 1 (x_src) or 8 (m_edge) until no such row is left -- that cancellation is the formula's own
(aggregators.py:24-28), not the kernel's.

Traps: every operand is a view at a column offset inside a NaN-filled buffer with a padded row stride that keeps exactly the cell's
alignment; outputs and define-mode sinks arrive as NaN, have 16 spare rows, and everything outside the view must still be NaN afterwards;
accumulate-mode sinks arrive as a known tensor; workspaces and aux tables are exactly as long as the query says, arrive as 0xFF bytes and
have a guard behind them that must survive."""
import ctypes as C
import os
import re
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import pytest
import torch

import agg_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
LATTICE = 2.0 ** -8
GUARD = 256
SPARE = 16


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _lib():
    from dgn_amd import _lib
    return _lib, _lib.load()


# ---- graphs -----------------------------------------------------------------------------------------------------------------------
LADDER = [0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 63, 64, 65, 127, 128, 129, 200]
OUT_DEGS = (1, 3, 4, 5, 8, 9)


class Graph:
    def __init__(self, name, degs, seed, n_src=None, beyond=False):
        rng = np.random.default_rng(seed)
        self.name, self.degs = name, np.asarray(degs, dtype=np.int64)
        self.N = N = len(degs)
        self.n_src = n_src or N
        self.indptr = np.concatenate([[0], np.cumsum(self.degs)]).astype(np.int64)
        self.E = E = int(self.indptr[-1])
        self.dst = np.repeat(np.arange(N), self.degs)
        special = rng.permutation(self.n_src)[:len(OUT_DEGS) + 1]          # [0]: no out-edge; the rest: 1, 3, 4, 5, 8, 9 out-edges
        pool = np.setdiff1d(np.arange(self.n_src), special)
        if beyond:                                                         # n_src > N: most sources lie beyond the destination rows
            pool = pool[pool >= N - 5]
        src = pool[rng.integers(0, len(pool), E)]
        fixed = np.zeros(E, dtype=bool)
        for r in range(N):
            b, d = self.indptr[r], self.degs[r]
            if r % 4 == 1 and d >= 2:                                      # a duplicated source
                src[b + 1] = src[b]
                fixed[b:b + 2] = True
            elif r % 4 == 3 and d >= 2 and r < self.n_src and r not in special:      # a self loop
                src[b + d - 1] = r
                fixed[b + d - 1] = True
        free = rng.permutation(np.nonzero(~fixed)[0])
        k = 0
        for u, od in zip(special[1:], OUT_DEGS):
            src[free[k:k + od]] = u
            k += od
        self.src = src
        out_deg = np.bincount(src, minlength=self.n_src)
        assert out_deg[special[0]] == 0 and tuple(out_deg[special[1:]]) == OUT_DEGS, (name, out_deg[special])
        assert src.min() >= 0 and src.max() < self.n_src
        order = np.argsort(src, kind="stable")                             # slots by (source, slot)
        self.csc_pos = np.empty(E, dtype=np.int64)
        self.csc_pos[order] = np.arange(E)
        self.csc_ptr = np.concatenate([[0], np.cumsum(out_deg)])
        self.log_deg = np.log(self.degs.astype(np.float64) + 1.0).astype(np.float32)

    def hub(self, threshold, chunk):
        rows = np.nonzero(self.degs > threshold)[0]
        n_sl = (self.degs[rows] + chunk - 1) // chunk
        return dict(hub_rows=rows, hub_chunk_ptr=np.concatenate([[0], np.cumsum(n_sl)]), chunk_hub=np.repeat(np.arange(len(rows)), n_sl))

    @property
    def route(self):
        return "short" if self.E <= 3 * self.N else ("rows1" if self.E >= 8 * self.N else "rows4")


def _ladder_degs(rng, n_mid, mids=(6, 9, 10, 11, 12, 14, 8, 7, 15, 13)):
    mid = np.asarray(mids)[rng.integers(0, len(mids), n_mid)]
    return rng.permutation(np.concatenate([LADDER, mid]))


def _short_degs(groups, cycle):
    pats = {"a": (4, 4, 4, 4), "b": (1, 2, 3, 1), "c": (2, 0, 3, 1), "d": (1, 5, 2, 2), "e": (3, 3, 2, 1), "f": (2, 2, 2, 2), "g": (1, 1, 2, 1)}
    degs = []
    for g in range(groups):
        degs += pats[cycle[g % len(cycle)]]
    return degs + [2, 3, 1]                                                # a last group of three rows: N = 3 mod 4


def _build(name):
    rng = np.random.default_rng(11)
    if name == "ladder":
        g = Graph(name, _ladder_degs(rng, 183), 1)
        assert g.N == 203 and g.N % 8 and g.E >= 8 * g.N, (g.N, g.E)
    elif name == "ladder4":
        g = Graph(name, rng.permutation(np.concatenate([_ladder_degs(rng, 183, (5, 6, 7, 8)), rng.integers(0, 5, 198)])), 2)
        assert g.N == 401 and g.N % 4 == 1 and 3 * g.N < g.E < 8 * g.N, (g.N, g.E)
    elif name == "short":
        g = Graph(name, _short_degs(75, "abcdef"), 3)
        assert g.N == 303 and g.E <= 3 * g.N and ((g.N + 3) // 4) % 32, (g.N, g.E)
    elif name == "shorthub":
        degs = _short_degs(130, "bcgdefgb")
        degs[41] = 300
        g = Graph(name, degs, 4)
        assert g.N % 4 == 3 and g.E <= 3 * g.N, (g.N, g.E)
    elif name == "bip_lt":
        g = Graph(name, np.concatenate([LADDER[:14], rng.integers(1, 13, 87)]), 5, n_src=40)
        assert g.route == "rows4", (g.N, g.E)
    elif name == "bip_gt":
        g = Graph(name, _short_degs(30, "abcdef"), 6, n_src=123 + 70, beyond=True)
        assert g.route == "short" and g.src.max() >= g.N
    else:
        raise KeyError(name)
    assert g.route == {"ladder": "rows1", "ladder4": "rows4", "short": "short", "shorthub": "short", "bip_lt": "rows4", "bip_gt": "short"}[name]
    return g


_GRAPHS, _DEV_GRAPHS = {}, {}


def graph(name) -> Graph:
    if name not in _GRAPHS:
        _GRAPHS[name] = _build(name)
    return _GRAPHS[name]


def device_graph(name, hub):
    """(DgnGraph struct, the tensors it points to) for graph `name` with hub description `hub` = (threshold, slice) or None"""
    key = (name, hub)
    if key not in _DEV_GRAPHS:
        L, _ = _lib()
        g, dev = graph(name), _dev()
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        keep = dict(indptr=i32(g.indptr), src=i32(g.src), csc_ptr=i32(g.csc_ptr), csc_pos=i32(g.csc_pos))
        c = L.DgnGraph()
        c.n_nodes, c.n_edges, c.indptr, c.src = g.N, g.E, keep["indptr"].data_ptr(), keep["src"].data_ptr()
        c.csc_ptr, c.csc_pos = keep["csc_ptr"].data_ptr(), keep["csc_pos"].data_ptr()
        c.n_src = g.n_src if g.n_src != g.N else 0
        c.max_in_degree = int(g.degs.max())
        if hub:
            h = g.hub(*hub)
            assert len(h["hub_rows"]) > 0
            keep.update({k: i32(v) for k, v in h.items()})
            c.n_hub, c.n_chunks, c.hub_threshold, c.hub_chunk = len(h["hub_rows"]), len(h["chunk_hub"]), hub[0], hub[1]
            c.hub_rows, c.hub_chunk_ptr, c.chunk_hub = (keep[k].data_ptr() for k in ("hub_rows", "hub_chunk_ptr", "chunk_hub"))
        _DEV_GRAPHS[key] = (c, keep)
    return _DEV_GRAPHS[key]


# ---- aggregator lists -------------------------------------------------------------------------------------------------------------
M, SU, MX, MN, SD, VR, AV, WS, DX, DN, XI = range(11)
ID, AMP, ATT = range(3)
SCALER_SETS = {1: (ID,), 2: (ATT, ID), 3: (ID, AMP, ATT), 4: (AMP, ID, ATT, AMP)}


@dataclass(frozen=True)
class AggList:
    name: str
    ops: Tuple[int, ...]
    chs: Tuple[int, ...]
    n_ch: int
    scalers: Tuple[int, ...] = (ID,)
    hot: bool = False
    stats: bool = False
    av: bool = False

    @property
    def has_var(self):
        return SD in self.ops or VR in self.ops

    @property
    def needs_xin(self):
        return any(o in (DX, DN, XI) for o in self.ops)


def _dyn_lists():
    """one list per (NCH, STATS, AV) of launch_vec's table: 18, none of them a row of dgn_agg_hot.hpp (they start with sum), the channels
    referenced in descending order; together all ten ops and the x_in pass-through, 1 to 4 scalers"""
    out = []
    for nch in range(5):
        for stats in (False, True):
            for av in ((False, True) if nch else (False,)):
                ops, chs = [SU, M], [0, 0]
                if stats:
                    extra = [MX, MN, SD, VR] if nch == 0 else ([MX, VR] if (nch + av) % 2 == 0 else [MN, SD])
                    ops += extra
                    chs += [0] * len(extra)
                for c in reversed(range(nch)):
                    ops.append((DX, WS, DN)[(c + nch + stats) % 3])
                    chs.append(c)
                if av:
                    ops.append(AV)
                    chs.append((nch - 1) // 2)
                k = len(out)
                ns = 1 + k % 4
                if ns == 1:
                    ops.append(XI)
                    chs.append(0)
                out.append(AggList(f"dyn{nch}{'s' if stats else ''}{'a' if av else ''}", tuple(ops), tuple(chs), nch, SCALER_SETS[ns],
                                   stats=stats, av=av))
    assert len(out) == 18 and {o for l in out for o in l.ops} == set(range(11))
    assert {len(l.scalers) for l in out} == {1, 2, 3, 4}
    return out


def _hot_lists():
    """every row of csrc/dgn_agg_hot.hpp, read from the file"""
    out = []
    with open(os.path.join(ROOT, "dgn_amd", "csrc", "dgn_agg_hot.hpp")) as f:
        for line in f:
            mt = re.match(r"DGN_HOT\((\d+), (0x[0-9a-f]+)ull, (0x[0-9a-f]+)ull, (\d+), (0x[0-9a-f]+)u, (\d+), (true|false), (true|false)\)", line)
            if not mt:
                assert not line.startswith("DGN_HOT"), line
                continue
            na, opk, chk, ns, sck, nch = int(mt[1]), int(mt[2], 16), int(mt[3], 16), int(mt[4]), int(mt[5], 16), int(mt[6])
            out.append(AggList(f"hot{len(out)}", tuple((opk >> (4 * a)) & 15 for a in range(na)), tuple((chk >> (3 * a)) & 7 for a in range(na)),
                               nch, tuple((sck >> (2 * s)) & 3 for s in range(ns)), hot=True, stats=mt[7] == "true", av=mt[8] == "true"))
    assert len(out) == 14
    return out


DYN, HOT = _dyn_lists(), _hot_lists()
ODD_LISTS = [l for l in HOT if l.ops in ((M, DN), (M, DX, DX))]
SIXTEEN = AggList("sixteen", (SU, MX, DX, AV, M, WS, MN, DN, SD, DX, AV, VR, WS, DN, DX, AV), (0, 0, 3, 2, 0, 1, 0, 0, 0, 1, 0, 0, 2, 3, 2, 3), 4,
                  stats=True, av=True)
SIX = AggList("six", (SU, DX, MX, AV, DN, MN), (0, 1, 0, 0, 0, 0), 2, stats=True, av=True)


# ---- cells ------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Cell:
    name: str
    graph: str
    F: int
    vec: int
    lst: AggList
    hub: Optional[Tuple[int, int]] = None
    terms: str = "s"                  # s: x_src, d: x_dst, e: dense m_edge, t: edge-type table
    K: int = 0                        # edge types
    xin: str = "sep"                  # sep | alias
    bwd: str = "define"               # define | accum | atomic | atomic_accum | no_gsrc | no_gdst_gin | rpw | none
    T: int = 1
    layout: str = "node"              # node | node_dense | tower | tower_dense
    aux: bool = False
    f_valid: int = 0
    slices: Optional[Tuple[Tuple[int, int], ...]] = None
    seed: int = 0

    @property
    def two_phase(self):
        return self.bwd in ("define", "accum", "no_gdst_gin", "rpw")


def _cells():
    cells, seen = [], set()

    def add(**kw):
        c = Cell(**kw)
        assert c.name not in seen, c.name
        seen.add(c.name)
        cells.append(c)

    widths = {1: (5, 67, 131), 2: (6, 70, 128, 130, 132), 4: (132, 256, 260)}
    forms = ("s", "sd", "e", "sde", "s", "sd")
    routes = ("ladder", "ladder4", "short")
    modes = ("define", "accum", "atomic", "atomic_accum", "no_gsrc", "no_gdst_gin")
    # 1. every generic list, at every vector width, on a row route (ladder and ladder4 take turns) and on the short route; the backward
    #    modes, the widths of the vector width, the message forms and the x_in modes take turns
    for vec in (1, 2, 4):
        k = 0
        for i, lst in enumerate(DYN):
            for gname, mode in ((("ladder", "ladder4")[i % 2], modes[(i // 2) % 6]), ("short", modes[i % 6])):
                form = forms[k % 6]
                alias = (form == "s" and k % 6 == 4 and (DX not in lst.ops or gname == "short" and lst.n_ch <= 2))
                add(name=f"{mode}-{gname}-v{vec}-{lst.name}", graph=gname, F=widths[vec][k % len(widths[vec])], vec=vec, lst=lst, bwd=mode,
                    terms=form, xin="alias" if alias else "sep", seed=k)
                k += 1
    # 2. bwd_rows_per_wave 1 against 4 (baked-in lists: the only ones whose kernel the option changes)
    for vec in (1, 2, 4):
        for j, gname in enumerate(routes):
            add(name=f"rpw-{gname}-v{vec}", graph=gname, F=widths[vec][0 if vec != 2 else 1], vec=vec, lst=HOT[(3 * j + vec) % len(HOT)], bwd="rpw",
                terms="sd"[:1 + j % 2])
    # 3. 16 aggregators, the slice launches, bipartite graphs, hub descriptions
    for gname in ("ladder", "short"):
        add(name=f"sixteen-{gname}", graph=gname, F=70, vec=2, lst=SIXTEEN, terms="sd")
        add(name=f"slices-{gname}", graph=gname, F=6, vec=2, lst=SIX, slices=((0, 3), (3, 3)), terms="sd")
    for gname in ("bip_lt", "bip_gt"):
        for vec, F in ((1, 5), (2, 70), (4, 132)):
            for mode, lst in (("define", DYN[7]), ("atomic", DYN[13]), ("accum", HOT[0])):
                add(name=f"{gname}-v{vec}-{mode}", graph=gname, F=F, vec=vec, lst=lst, bwd=mode, terms="sd")
    for hub in ((127, 48), (100, 80), (16, 7)):
        for vec, F in ((1, 67), (2, 70), (4, 132)):
            for mode, lst in (("define", DYN[9]), ("atomic", DYN[17]), ("accum", DYN[2]), ("define", HOT[9])):
                add(name=f"hub{hub[0]}-v{vec}-{mode}-{lst.name}", graph="ladder", hub=hub, F=F, vec=vec, lst=lst, bwd=mode, terms="sd", seed=hub[1])
    for mode, lst in (("define", HOT[0]), ("atomic", DYN[9]), ("accum", DYN[16])):
        add(name=f"shorthub-{mode}-{lst.name}", graph="shorthub", hub=(64, 64), F=70, vec=2, lst=lst, bwd=mode, terms="sd")
    # 4. every baked-in list on the row and the short route: plain, with its aux table, with a dense m_edge (MEDGE), with an edge-type table
    for i, lst in enumerate(HOT):
        for gname in ("ladder", "short"):
            base = dict(graph=gname, F=6 if i % 2 else 70, vec=2, lst=lst, seed=i)
            add(name=f"{lst.name}-{gname}-plain", terms="sd" if i % 3 else "s", xin="alias" if (gname == "short" and i % 3 == 0 and lst.n_ch <= 2) else "sep", **base)
            add(name=f"{lst.name}-{gname}-aux", aux=True, **base)                 # (cells without a table fall back to the plain pair, asserted)
            add(name=f"{lst.name}-{gname}-medge", terms="se", **base)
            add(name=f"{lst.name}-{gname}-table", terms="st", K=(1, 4, 9)[i % 3], **base)
    add(name="hot0-short-aux-medge", graph="short", F=70, vec=2, lst=HOT[0], terms="se", aux=True)
    add(name="hot0-short-aux-table", graph="short", F=70, vec=2, lst=HOT[0], terms="st", K=4, aux=True)
    # 5. towers: node-major, tower-major (tower_stride a multiple of 4; K = A F/T a multiple of 4 or not; ld_out == K or padded)
    for gname in ("short", "ladder4"):
        for T, F, lst, layout in ((2, 68, HOT[7], "tower_dense"), (2, 68, HOT[7], "tower"), (5, 70, HOT[12], "tower_dense"), (5, 70, HOT[12], "tower"),
                                  (5, 70, HOT[0], "tower_dense"), (5, 70, HOT[0], "node"), (2, 132, DYN[11], "node"), (2, 132, DYN[3], "tower"),
                                  (1, 6, HOT[0], "node_dense"), (1, 70, HOT[3], "node_dense"), (5, 70, DYN[5], "tower_dense")):
            add(name=f"towers-{gname}-T{T}-F{F}-{lst.name}-{layout}", graph=gname, T=T, F=F, vec=2, lst=lst, layout=layout, terms="sd")
    # 6. rows of an odd width (f_valid) for the two lists with such kernels, both routes, NaN directly behind every row
    for lst in ODD_LISTS:
        for gname in ("ladder", "short"):
            for fv in (5, 75, 127):
                add(name=f"odd-{gname}-{lst.name}-{fv}", graph=gname, F=fv + 1, vec=2, lst=lst, f_valid=fv, xin="alias" if fv == 75 and lst.ops == (M, DN) else "sep")
    return cells


CELLS = _cells()


def test_the_grid_covers_what_it_claims():
    by = lambda f: {f(c) for c in CELLS}
    routes = {c.graph: graph(c.graph).route for c in CELLS}
    assert set(routes.values()) == {"rows1", "rows4", "short"}
    for mode in ("define", "accum", "atomic", "atomic_accum", "no_gsrc", "no_gdst_gin", "rpw"):
        assert {(routes[c.graph], c.vec) for c in CELLS if c.bwd == mode} >= {(r, v) for r in ("rows1", "rows4", "short") for v in (1, 2, 4)}, mode
    widths = {(1, 5), (1, 67), (1, 131), (2, 6), (2, 70), (2, 128), (2, 130), (2, 132), (4, 132), (4, 256), (4, 260)}
    for r in ("rows1", "rows4", "short"):
        assert {(c.vec, c.F) for c in CELLS if routes[c.graph] == r} >= widths, r
    for r in ("rows", "short"):
        for vec in (1, 2, 4):
            assert {c.lst.name for c in CELLS if c.vec == vec and routes[c.graph].startswith(r)} >= {l.name for l in DYN}, (r, vec)
    for vec in (1, 2, 4):
        assert {c.lst.name for c in CELLS if c.vec == vec} >= {l.name for l in DYN}
    assert {c.lst.name for c in CELLS} >= {l.name for l in HOT}
    assert by(lambda c: c.terms) >= {"s", "sd", "e", "sde", "se", "st"} and by(lambda c: c.xin) == {"sep", "alias"}
    assert by(lambda c: c.K) >= {1, 4, 9} and by(lambda c: c.T) == {1, 2, 5} and by(lambda c: c.f_valid) == {0, 5, 75, 127}
    assert by(lambda c: len(c.lst.scalers)) == {1, 2, 3, 4} and len(ODD_LISTS) == 2


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _lattice(rng, shape):
    return rng.integers(-1024, 1024, shape).astype(np.float64) * LATTICE


def _wrap(x):
    return (x + 4.0) % 8.0 - 4.0


_PROBLEMS = {}


def problem(cell: Cell):
    """host inputs of a cell (fp64 arrays holding fp32-exact values), conditioned as the module's docstring says; cached"""
    if cell.name in _PROBLEMS:
        return _PROBLEMS[cell.name]
    g, lst, F = graph(cell.graph), cell.lst, cell.F
    rng = np.random.default_rng(1000 + cell.seed)
    p = dict(x_src=None, x_dst=None, m_edge=None, edge_type=None, x_in=None)
    if "s" in cell.terms:
        p["x_src"] = _lattice(rng, (g.n_src, F))
    if "d" in cell.terms:
        p["x_dst"] = _lattice(rng, (g.N, F))
    if "e" in cell.terms:
        p["m_edge"] = rng.integers(-2, 3, (g.E, F)).astype(np.float64) * 8.0
    if "t" in cell.terms:
        p["m_edge"] = rng.integers(-2, 3, (cell.K, F)).astype(np.float64) * 8.0
        p["edge_type"] = rng.integers(0, cell.K, g.E)
    if cell.f_valid:                                                        # the zero-padded column the kernel makes up
        p["x_src"][:, -1] = 0.0
    w = rng.standard_normal((max(lst.n_ch, 1), g.E)).astype(np.float32)
    has = np.nonzero(g.degs > 0)[0]
    for c in range(w.shape[0]):             # a row whose weights cancel leaves x_in no say in its residual: such a row's first weight moves by 1
        sw = np.add.reduceat(w[c].astype(np.float64), g.indptr[:-1][has])
        low = np.abs(sw) < 0.5
        w[c, g.indptr[:-1][has][low]] += np.where(sw[low] >= 0, 1.0, -1.0).astype(np.float32)
    p["w"] = w.astype(np.float64)
    msg = lambda: dict(x_src=p["x_src"], x_dst=p["x_dst"], m_edge=p["m_edge"], edge_type=p["edge_type"])
    facts = lambda: ref.sweep(g.indptr, g.src, g.n_src, lst.ops, lst.chs, [ID], x_in=p["x_in"], w=p["w"], facts_only=True, **msg())
    if lst.has_var:
        for _ in range(40):
            bad = ~ref.sweep(g.indptr, g.src, g.n_src, [SD], [0], [ID], facts_only=True, **msg())["var_ok"]
            if not bad.any():
                break
            rows, cols = np.nonzero(bad)
            first = g.indptr[rows]
            if p["x_src"] is not None:
                p["x_src"][g.src[first], cols] = _wrap(p["x_src"][g.src[first], cols] + 1.0)
            else:
                p["m_edge"][first, cols] = (p["m_edge"][first, cols] + 24.0) % 40.0 - 16.0
        else:
            raise AssertionError(f"{cell.name}: std / var conditioning did not converge")
    p["alias"] = cell.xin == "alias" and lst.needs_xin
    if lst.needs_xin:
        if cell.xin == "alias":
            assert cell.terms == "s" and g.n_src == g.N
            p["x_in"] = p["x_src"]
        else:
            p["x_in"] = _lattice(rng, (g.N, F))
            if cell.f_valid:
                p["x_in"][:, -1] = 0.0
            cols_free = F - 1 if cell.f_valid else F
            for _ in range(40):                                             # lattice steps until every abs-dx residual is conditioned
                bad = ~facts()["dx_ok"]
                bad[:, cols_free:] = False
                if not bad.any():
                    break
                step = rng.integers(1, 512, int(bad.sum())) * LATTICE
                p["x_in"][bad] = _wrap(p["x_in"][bad] + step)
            else:
                raise AssertionError(f"{cell.name}: dx conditioning did not converge")
    S_, A_ = len(lst.scalers), len(lst.ops)
    p["g_out"] = rng.standard_normal((g.N, S_ * A_ * F)).astype(np.float32).astype(np.float64)
    p["accum"] = {k: rng.standard_normal(s).astype(np.float32) for k, s in (("g_src", (g.n_src, F)), ("g_dst", (g.N, F)), ("g_in", (g.N, F)))}
    r = ref.sweep(g.indptr, g.src, g.n_src, lst.ops, lst.chs, lst.scalers, AVG_LOG, EPS, cell.T, x_in=p["x_in"], w=p["w"], log_deg=g.log_deg,
                  g_out=p["g_out"], **msg())
    # unconditioned (row, feature) entries -- only where x_in aliases x_src -- and the gradient entries that sum over one
    bad = ~r["dx_ok"]
    if cell.f_valid:
        bad[:, -1] = False          # (the made-up column: messages and x_in are exact zeros, residual exactly zero in both precisions)
    assert r["var_ok"].all() or not lst.has_var, cell.name
    assert p["alias"] or not bad.any(), cell.name
    skip = dict(g_dst=bad, g_in=bad.copy(), g_edge=bad[g.dst] if "e" in cell.terms else None, g_src=np.zeros((g.n_src, F), dtype=bool))
    np.logical_or.at(skip["g_src"], g.src, bad[g.dst])
    if p["alias"]:
        skip["g_src"] |= bad
        skip["g_in"] = skip["g_src"]
    for k, v in skip.items():
        if v is not None:
            assert v.mean() <= 0.005, f"{cell.name}: {v.mean():.4f} of {k} unconditioned"
    p["ref"], p["skip"] = r, skip
    if DUMP:
        p["ref32"] = ref.sweep(g.indptr, g.src, g.n_src, lst.ops, lst.chs, lst.scalers, AVG_LOG, EPS, cell.T, x_in=p["x_in"], w=p["w"], log_deg=g.log_deg,
                               g_out=p["g_out"], dtype=np.float32, **msg())
    _PROBLEMS[cell.name] = p
    return p


AVG_LOG, EPS = 1.7, 1e-8


# ---- device buffers ---------------------------------------------------------------------------------------------------------------
class Buf:
    """A [rows, cols] fp32 view at column `off` of a NaN-filled [planes, rows + spare, ld] device buffer whose stride and offset keep
    exactly `vec` floats of alignment (vec 4: 16 bytes; 2: 8 bytes, stride = 2 mod 4; 1: 4 bytes, odd stride)."""

    def __init__(self, rows, cols, vec, data=None, planes=1, dense=False, spare=SPARE, fill=NAN):
        self.rows, self.cols, self.planes = rows, cols, planes
        if planes > 1:
            spare += -(rows + spare) % 4                 # (tower planes: a plane stride that is a multiple of 4)
        if dense:
            self.off, self.ld = 0, cols
        else:
            self.off = vec
            self.ld = cols + 5
            while self.ld % 4 != {4: 0, 2: 2, 1: 1}[vec]:
                self.ld += 1
        host = np.full((planes, rows + spare, self.ld), fill, dtype=np.float32)
        if data is not None:
            host[:, :rows, self.off:self.off + cols] = np.asarray(data, dtype=np.float32).reshape(planes, rows, cols)
        self.t = torch.from_numpy(host).to(_dev())
        self.plane_stride = (rows + spare) * self.ld

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.off

    def read(self, what):
        """the view as fp64 numpy [planes, rows, cols] after asserting that everything around it is still NaN"""
        host = self.t.cpu().numpy()
        inside = np.zeros(host.shape, dtype=bool)
        inside[:, :self.rows, self.off:self.off + self.cols] = True
        assert np.isnan(host[~inside]).all(), f"{what}: written outside its view"
        return host[:, :self.rows, self.off:self.off + self.cols].astype(np.float64)


class Bytes:
    """`n` bytes of 0xFF with a guard of 0xA5 behind them"""

    def __init__(self, n):
        self.n = int(n)
        self.t = torch.full((self.n + GUARD,), 0xFF, dtype=torch.uint8, device=_dev())
        self.t[self.n:] = 0xA5

    @property
    def ptr(self):
        return self.t.data_ptr() if self.n else None

    def check(self, what):
        assert bool((self.t[self.n:] == 0xA5).all()), f"{what}: written past its {self.n} bytes"


def _close(got, want, tol, what, skip=None, fp32=None, family=None):
    want = np.asarray(want, dtype=np.float64).reshape(got.shape)
    if fp32 is not None:                                 # (measuring: the kernel's error over that of an fp32 evaluation of the same formulas)
        e32 = np.abs(np.asarray(fp32, dtype=np.float64).reshape(got.shape) - want)
        e = np.abs(got - want)
        if skip is not None:
            e, e32 = np.where(skip.reshape(got.shape), 0.0, e), np.where(skip.reshape(got.shape), 0.0, e32)
        VS_FP32[family] = max(VS_FP32.get(family, 0.0), float(e.max()) / max(float(e32.max()), 1e-30))
    scale = max(1.0, float(np.abs(want).max())) if want.size else 1.0
    err = np.abs(got - want)
    err[np.isnan(got)] = np.inf
    if skip is not None:
        err = np.where(skip.reshape(got.shape), 0.0, err)
    worst = float(err.max()) if err.size else 0.0
    assert worst <= tol * scale, f"{what}: error {worst:.3e} > {tol:g} x {scale:.3e} at {np.unravel_index(int(err.argmax()), err.shape)}"
    return worst / scale


RATIOS, VS_FP32 = {}, {}
DUMP = os.environ.get("DGN_AGG_GRID_DUMP")              # a directory: kernel names, launch tally and error ratios are written there


def _note(family, ratio):
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)


# ---- one launch -------------------------------------------------------------------------------------------------------------------
class Launch:
    """structs and operand buffers of a cell on the device"""

    def __init__(self, cell: Cell):
        L, lib = _lib()
        self.cell, self.L, self.lib = cell, L, lib
        self.g, self.p = graph(cell.graph), problem(cell)
        self.cg, self._keep = device_graph(cell.graph, cell.hub)
        g, p, lst, F, vec = self.g, self.p, cell.lst, cell.F, cell.vec
        self.spec = self._spec(0, len(lst.ops))
        in_vec = 1 if cell.f_valid else vec
        fv = cell.f_valid or F
        self.ops = {}
        msg = self.msg = L.DgnMsg()
        msg.F, msg.f_valid = F, cell.f_valid
        if p["x_src"] is not None:
            b = self.ops["x_src"] = Buf(g.n_src, fv, in_vec, p["x_src"][:, :fv])
            msg.x_src, msg.ld_src = b.ptr, b.ld
        if p["x_dst"] is not None:
            b = self.ops["x_dst"] = Buf(g.N, F, vec, p["x_dst"])
            msg.x_dst, msg.ld_dst = b.ptr, b.ld
        if p["m_edge"] is not None:
            b = self.ops["m_edge"] = Buf(p["m_edge"].shape[0], F, vec, p["m_edge"])
            msg.m_edge, msg.ld_edge = b.ptr, b.ld
        if p["edge_type"] is not None:
            self.ops["edge_type"] = torch.from_numpy(p["edge_type"].astype(np.int32)).to(_dev())
            msg.edge_type, msg.n_edge_types = self.ops["edge_type"].data_ptr(), cell.K
        if p["x_in"] is not None:
            if p["alias"]:
                msg.x_in, msg.ld_in = msg.x_src, msg.ld_src
            else:
                b = self.ops["x_in"] = Buf(g.N, fv, in_vec, p["x_in"][:, :fv])
                msg.x_in, msg.ld_in = b.ptr, b.ld
        self.w = Buf(max(lst.n_ch, 1), g.E, 1, p["w"], spare=1)
        self.log_deg = Buf(1, g.N, 1, g.log_deg, spare=1)
        self.width = len(lst.scalers) * len(lst.ops) * F
        self.g_out = self._out_buf(self._to_layout(p["g_out"]))

    def _spec(self, offset, n):
        cell, lst = self.cell, self.cell.lst
        s = self.L.DgnAggSpec()
        s.n_agg, s.n_ch, s.n_scalers, s.avg_log, s.eps, s.n_towers = n, lst.n_ch, len(lst.scalers), AVG_LOG, EPS, cell.T
        for a in range(n):
            s.agg_op[a], s.agg_ch[a] = lst.ops[offset + a], lst.chs[offset + a]
        for i, k in enumerate(lst.scalers):
            s.scaler[i] = k
        if cell.slices:
            s.agg_total, s.agg_offset = len(lst.ops), offset
        return s

    @property
    def tower_major(self):
        return self.cell.layout.startswith("tower")

    def _to_layout(self, node_major):
        """reference order [N, T*K] -> the planes of the cell's layout"""
        N, T = self.g.N, self.cell.T
        return node_major.reshape(N, T, -1).transpose(1, 0, 2) if self.tower_major else node_major.reshape(1, N, -1)

    def _out_buf(self, data=None):
        planes, cols = (self.cell.T, self.width // self.cell.T) if self.tower_major else (1, self.width)
        # (tower-major: 16-byte aligned planes at a stride that is a multiple of 4 -- F / T keeps the kernel's vector width where it is)
        b = Buf(self.g.N, cols, 4 if self.tower_major else self.cell.vec, data, planes=planes, dense=self.cell.layout.endswith("dense"))
        assert not self.tower_major or b.plane_stride % 4 == 0
        return b

    def _from_layout(self, planes):
        return planes.transpose(1, 0, 2).reshape(self.g.N, -1) if self.tower_major else planes[0]

    def _set_stride(self, spec, buf):
        spec.tower_stride = buf.plane_stride if self.tower_major else 0

    def _args(self, spec):
        return (C.byref(self.cg), C.byref(spec), C.byref(self.msg), self.w.ptr, self.w.ld, self.log_deg.ptr)

    def aux_bytes(self):
        return self.lib.dgn_agg_aux_bytes(C.byref(self.cg), C.byref(self.spec), C.byref(self.msg))

    def forward(self, aux=None, out=None, spec=None):
        spec = spec or self.spec
        out = out or self._out_buf()
        self._set_stride(spec, out)
        ws = Bytes(self.lib.dgn_agg_workspace_bytes(C.byref(self.cg), C.byref(spec), self.cell.F))
        assert (ws.n > 0) == bool(self.cell.hub)
        stream = self.L.stream_ptr(_dev())
        if aux is not None:
            rc = self.lib.dgn_agg_forward_aux(*self._args(spec), out.ptr, out.ld, aux.ptr, ws.ptr, ws.n, stream)
        else:
            rc = self.lib.dgn_agg_forward(*self._args(spec), out.ptr, out.ld, ws.ptr, ws.n, stream)
        self.L.check(rc, f"{self.cell.name}: forward")
        torch.cuda.synchronize()
        ws.check("forward workspace")
        return out

    def sinks(self, accumulate):
        cell, g, F, vec = self.cell, self.g, self.cell.F, self.cell.vec
        null = {"no_gsrc": ("g_src",), "no_gdst_gin": ("g_dst", "g_in")}.get(cell.bwd, ())
        init = (lambda k: self.p["accum"][k]) if accumulate else (lambda k: None)
        s = {}
        if self.p["x_src"] is not None and "g_src" not in null:
            s["g_src"] = Buf(g.n_src, F, vec, init("g_src"))
        if self.p["x_dst"] is not None and "g_dst" not in null:
            s["g_dst"] = Buf(g.N, F, vec, init("g_dst"))
        if self.p["m_edge"] is not None:
            s["g_edge"] = Buf(self.p["m_edge"].shape[0], F, vec, init("g_src")[:1].repeat(self.p["m_edge"].shape[0], 0) if accumulate else None)
        if self.p["x_in"] is not None and "g_in" not in null:
            if self.p["alias"]:
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

    def backward(self, accumulate, two_phase, aux=None, spec=None, sinks=None):
        spec = spec or self.spec
        self._set_stride(spec, self.g_out)
        s, gr = sinks or self.sinks(accumulate)
        n = self.lib.dgn_agg_backward_workspace_bytes(C.byref(self.cg), C.byref(spec), self.cell.F, int(two_phase))
        if self.cell.K:
            n += self.lib.dgn_agg_edge_table_workspace_bytes(self.cell.F, self.cell.K)
        ws = Bytes(n)
        stream = self.L.stream_ptr(_dev())
        if aux is not None:
            rc = self.lib.dgn_agg_backward_aux(*self._args(spec), self.g_out.ptr, self.g_out.ld, aux.ptr, C.byref(gr), ws.ptr, ws.n, stream)
        else:
            rc = self.lib.dgn_agg_backward(*self._args(spec), self.g_out.ptr, self.g_out.ld, C.byref(gr), ws.ptr, ws.n, stream)
        self.L.check(rc, f"{self.cell.name}: backward")
        torch.cuda.synchronize()
        ws.check("backward workspace")
        return s, gr


def _read_sinks(s, what):
    return {k: b.read(f"{what} {k}")[0] for k, b in s.items()}


def _check_grads(cell, p, got, accumulate, family):
    for k, v in got.items():
        want = p["ref"][k]
        assert want is not None, k
        if p["alias"] and k in ("g_src", "g_in"):
            want = p["ref"]["g_src"] + p["ref"]["g_in"]
        if accumulate and k != "g_edge":                 # (g_edge is always overwritten)
            v = v - p["accum"]["g_src" if (p["alias"] and k == "g_in") else k].astype(np.float64)
        w32 = None
        if p.get("ref32") is not None:
            w32 = p["ref32"][k] if not (p["alias"] and k in ("g_src", "g_in")) else p["ref32"]["g_src"] + p["ref32"]["g_in"]
        _note(family, _close(v, want, 1e-4, f"{cell.name} {k}", p["skip"].get(k), w32, family) / 1e-4)


def run_cell(cell: Cell, compare=True):
    """forward and backward of one cell; with compare=False the launches alone (the instance proof)"""
    ln = Launch(cell)
    p, lst = ln.p, cell.lst
    family = ("hot" if lst.hot else "dyn") + "-" + graph(cell.graph).route + ("-hub" if cell.hub else "")
    aux = None
    if cell.aux:
        n = ln.aux_bytes()
        assert (n > 0) == _aux_supported(cell), (cell.name, n)
        aux = Bytes(n) if n else None
    if cell.slices:
        out = ln._out_buf()
        for i, (off, n) in enumerate(cell.slices):
            ln.forward(out=out, spec=ln._spec(off, n))
            if compare and i == 0:
                got = ln._from_layout(out.read(f"{cell.name} out")).reshape(graph(cell.graph).N, len(lst.scalers), len(lst.ops), cell.F)
                assert not np.isnan(got[:, :, off:off + n]).any() and np.isnan(got[:, :, off + n:]).all(), "the first slice launch wrote the other's columns"
    else:
        out = ln.forward(aux=aux)
        if aux is not None:
            aux.check("aux table")
    if compare:
        got = ln._from_layout(out.read(f"{cell.name} out"))
        _note(family + "-fwd", _close(got, p["ref"]["out"], 1e-5, f"{cell.name} out", None, p["ref32"]["out"] if p.get("ref32") else None, family + "-fwd") / 1e-5)
    if aux is not None and compare:                      # the table changes no value
        plain = ln.forward()
        assert np.array_equal(plain.read("out")[0], out.read("out")[0]), f"{cell.name}: forward with the aux table differs"
    if cell.bwd == "none":
        return
    accumulate, two_phase = cell.bwd in ("accum", "atomic_accum"), cell.two_phase
    if cell.slices:                                      # the first slice defines, the second accumulates
        sinks = ln.sinks(False)
        for i, (off, n) in enumerate(cell.slices):
            sinks[1].accumulate = int(i > 0)
            ln.backward(i > 0, True, spec=ln._spec(off, n), sinks=sinks)
        if compare:
            _check_grads(cell, p, _read_sinks(sinks[0], cell.name), False, family + "-bwd")
        return
    if cell.bwd == "rpw":
        L = ln.L
        default = L.options.bwd_rows_per_wave
        assert default == 4
        try:
            L.options.bwd_rows_per_wave = 1
            one = _read_sinks(ln.backward(False, True)[0], cell.name)
        finally:
            L.options.bwd_rows_per_wave = default
        s, _ = ln.backward(False, True)
        if compare:
            got = _read_sinks(s, cell.name)
            for k in got:
                assert np.array_equal(got[k], one[k]), f"{cell.name} {k}: bwd_rows_per_wave 1 and 4 differ"
            _check_grads(cell, p, got, False, family + "-bwd")
        return
    s, _ = ln.backward(accumulate, two_phase, aux=aux)
    if not compare:
        return
    got = _read_sinks(s, cell.name)
    _check_grads(cell, p, got, accumulate, family + "-bwd")
    if two_phase and cell.bwd != "no_gsrc":              # the two-phase scatter has a fixed summation order: equal bits, call after call
        again = _read_sinks(ln.backward(accumulate, two_phase, aux=aux)[0], cell.name)
        for k in got:
            a, b = got[k], again[k]
            if cell.hub and k == "g_dst":                # (the slices of a hub row add their shares of d x_dst with atomics, in any order)
                keep = graph(cell.graph).degs <= cell.hub[0]
                a, b = a[keep], b[keep]
            assert np.array_equal(a, b), f"{cell.name} {k}: two calls of the two-phase backward differ"
    if aux is not None:                                  # the aux backward recomputes nothing and still gives the same bits
        plain = _read_sinks(ln.backward(accumulate, two_phase)[0], cell.name)
        for k in got:
            assert np.array_equal(got[k], plain[k]), f"{cell.name} {k}: the aux backward differs from the recomputing one"


@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_cell(cell):
    run_cell(cell)


# ---- the graph description, the empty cases, the refusals ---------------------------------------------------------------------------
def test_numpy_graph_description_equals_DGNGraph():
    import dgn_amd
    g, dev = graph("ladder"), _dev()
    dg = dgn_amd.DGNGraph.from_csr(torch.from_numpy(g.indptr).to(dev), torch.from_numpy(g.src).to(dev), hub_threshold=100, hub_chunk=80)
    dg.ensure_csc()
    h = g.hub(100, 80)
    eq = lambda t, a: np.array_equal(t.cpu().numpy().astype(np.int64), np.asarray(a, dtype=np.int64))
    assert eq(dg.indptr, g.indptr) and eq(dg.src, g.src) and eq(dg.csc_ptr, g.csc_ptr) and eq(dg.csc_pos, g.csc_pos)
    assert np.array_equal(dg.log_deg.cpu().numpy(), g.log_deg)
    assert dg.n_hub == len(h["hub_rows"]) == 4 and dg.n_chunks == len(h["chunk_hub"]) == 2 + 2 + 2 + 3
    assert all(eq(t, h[k]) for t, k in zip(dg._keep, ("hub_rows", "hub_chunk_ptr", "chunk_hub")))
    c = device_graph("ladder", (100, 80))[0]
    for f in ("n_nodes", "n_edges", "n_hub", "n_chunks", "hub_threshold", "hub_chunk", "max_in_degree", "n_src"):
        assert getattr(c, f) == getattr(dg._c, f), f


def _tiny(n_nodes, E):
    L, lib = _lib()
    dev = _dev()
    keep = dict(indptr=torch.zeros(n_nodes + 1, dtype=torch.int32, device=dev), src=torch.zeros(max(E, 1), dtype=torch.int32, device=dev))
    c = L.DgnGraph()
    c.n_nodes, c.n_edges, c.indptr, c.src = n_nodes, E, keep["indptr"].data_ptr(), keep["src"].data_ptr()
    return c, keep


@pytest.mark.parametrize("n_nodes", [0, 7])
def test_no_rows_and_no_edges(n_nodes):
    """n_nodes == 0: nothing is launched or written; E == 0: rows of zeros (the x_in block apart), zero gradients"""
    L, lib = _lib()
    c, keep = _tiny(n_nodes, 0)
    F = 6
    spec = L.DgnAggSpec()
    spec.n_agg, spec.n_ch, spec.n_scalers, spec.n_towers, spec.avg_log, spec.eps = 3, 0, 1, 1, AVG_LOG, EPS
    spec.agg_op[0], spec.agg_op[1], spec.agg_op[2] = M, MX, XI
    x = _lattice(np.random.default_rng(0), (max(n_nodes, 1), F))
    xs, xi, out, g_out = Buf(max(n_nodes, 1), F, 2, x), Buf(max(n_nodes, 1), F, 2, x + 1), Buf(n_nodes, 3 * F, 2), Buf(n_nodes, 3 * F, 2, np.ones((n_nodes, 3 * F)))
    msg = L.DgnMsg()
    msg.F, msg.x_src, msg.ld_src, msg.x_in, msg.ld_in = F, xs.ptr, xs.ld, xi.ptr, xi.ld
    sinks = dict(g_src=Buf(n_nodes, F, 2), g_in=Buf(n_nodes, F, 2))
    gr = L.DgnMsgGrad()
    gr.g_src, gr.ld_src, gr.g_in, gr.ld_in = sinks["g_src"].ptr, sinks["g_src"].ld, sinks["g_in"].ptr, sinks["g_in"].ld
    args = (C.byref(c), C.byref(spec), C.byref(msg), None, 0, None)
    L.check(lib.dgn_agg_forward(*args, out.ptr, out.ld, None, 0, L.stream_ptr(_dev())), "forward")
    L.check(lib.dgn_agg_backward(*args, g_out.ptr, g_out.ld, C.byref(gr), None, 0, L.stream_ptr(_dev())), "backward")
    torch.cuda.synchronize()
    got = out.read("out")[0]
    if n_nodes:
        assert (got[:, :2 * F] == 0).all() and np.array_equal(got[:, 2 * F:], x + 1)
        assert (sinks["g_src"].read("g_src") == 0).all() and (sinks["g_in"].read("g_in") == 1).all()
    else:
        sinks["g_src"].read("g_src"), sinks["g_in"].read("g_in")


def test_refusals_are_host_side():
    """every refusal of validate(): DGN_ERR_INVALID before any launch -- `out` and the sinks keep their NaN"""
    L, lib = _lib()
    ln = Launch(Cell(name="refusals", graph="short", F=6, vec=2, lst=HOT[0], terms="sd"))
    out = ln._out_buf()
    sinks, gr = ln.sinks(False)
    err = lambda: lib.dgn_last_error().decode()

    def refused(word, spec=None, msg=None, cg=None, w=True, log_deg=True):
        args = (C.byref(cg or ln.cg), C.byref(spec or ln.spec), C.byref(msg or ln.msg), ln.w.ptr if w else None, ln.w.ld, ln.log_deg.ptr if log_deg else None)
        for rc in (lib.dgn_agg_forward(*args, out.ptr, out.ld, None, 0, None), lib.dgn_agg_backward(*args, ln.g_out.ptr, ln.g_out.ld, C.byref(gr), None, 0, None)):
            assert rc == L.DGN_ERR_INVALID and word in err(), (word, rc, err())

    def changed(struct, **kw):
        c = type(struct)()
        C.memmove(C.byref(c), C.byref(struct), C.sizeof(c))
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return c

    refused("gathered term", msg=changed(ln.msg, x_src=None))                       # x_dst alone
    refused("n_agg", spec=changed(ln.spec, n_agg=0))
    refused("n_agg", spec=changed(ln.spec, n_agg=17))
    refused("slice", spec=changed(ln.spec, agg_total=5, agg_offset=1))
    refused("n_ch", spec=changed(ln.spec, n_ch=5))
    refused("n_scalers", spec=changed(ln.spec, n_scalers=5))
    refused("n_towers", spec=changed(ln.spec, n_towers=4))
    refused("unknown scaler", spec=changed(ln.spec, scaler=(0, 3)))
    refused("log_deg", spec=changed(ln.spec, scaler=(0, AMP)), log_deg=False)
    refused("unknown aggregator", spec=changed(ln.spec, agg_op=(1, 11)))
    refused("channel", spec=changed(ln.spec, agg_ch=(3, 1)))
    refused("edge weights", w=False)
    refused("x_in", msg=changed(ln.msg, x_in=None))
    refused("pass-through", spec=changed(ln.spec, agg_op=(0, XI), scaler=(0, AMP)))
    refused("f_valid", msg=changed(ln.msg, f_valid=5))                               # (with x_dst)
    refused("edge_type", msg=changed(ln.msg, edge_type=ln.w.ptr, n_edge_types=2))    # (without the table)
    refused("edge-type table", msg=changed(ln.msg, m_edge=ln.w.ptr, ld_edge=8, edge_type=ln.w.ptr, n_edge_types=2000))
    refused("int32", msg=changed(ln.msg, ld_src=2 ** 31))
    refused("hub", cg=changed(ln.cg, n_hub=1))
    refused("null CSR", cg=changed(ln.cg, indptr=None))
    torch.cuda.synchronize()
    assert np.isnan(out.t.cpu().numpy()).all() and all(np.isnan(b.t.cpu().numpy()).all() for b in sinks.values())


# ---- the instance proof -------------------------------------------------------------------------------------------------------------
def _norm(name):
    name = name.replace("dgn::", "").replace("(anonymous namespace)::", "")
    name = re.sub(r"\((?:bool|int|unsigned long|unsigned int)\)", "", name)
    name = re.sub(r"\b(\d+)(?:ul|u|l)\b", r"\1", name)
    return name.replace("true", "1").replace("false", "0").replace(" ", "")


def _kernel_key(name):
    """'agg_fwd_short|2,1,1,1,0|S|1,0' : kernel, Cfg arguments (ODD spelled out), DynOps / StaticOps, the flags behind them"""
    n = _norm(name)
    mt = re.search(r"(agg_\w+|seg_sum_rows|edge_table_grad_\w+)", n)
    if not mt:
        return None
    base = mt[1]
    if base.startswith("edge_table"):
        return base
    if base == "seg_sum_rows":
        return base + "|" + re.search(r"seg_sum_rows<(\d)>", n)[1]
    cfg = re.search(r"Cfg<([\d,]+)>", n)[1].split(",")
    cfg += ["0"] * (5 - len(cfg))
    ops = "S" if "StaticOps" in n else ("D" if "DynOps" in n else "-")
    rest = re.sub(r"(Cfg|StaticOps)<[^<>]*>", "", n[mt.end():])
    rest = re.sub(r"\(.*$", "", rest).replace("DynOps", "")
    flags = ",".join(t for t in rest.strip("<>").split(",") if t)
    return f"{base}|{','.join(cfg)}|{ops}|{flags}"


def expected_kernels(cell: Cell):
    """the kernels the dispatch is designed to give the cell (launch_vec / launch_forward_cfg / launch_backward_cfg), as _kernel_key's"""
    g, lst = graph(cell.graph), cell.lst
    cfg = f"{cell.vec},{lst.n_ch},{int(lst.stats)},{int(lst.av)},{int(bool(cell.f_valid))}"
    ops = "S" if lst.hot else "D"
    if cell.slices:
        lists = [AggList("s", lst.ops[o:o + n], lst.chs[o:o + n], lst.n_ch) for o, n in cell.slices]
        cfgs = [f"{cell.vec},{lst.n_ch},{int(any(x in (MX, MN, SD, VR) for x in l.ops))},{int(AV in l.ops)},0" for l in lists]
    else:
        cfgs = [cfg]
    fwd, bwd = [], []
    short, dense_edge, table = g.route == "short", "e" in cell.terms, "t" in cell.terms
    has_aux = cell.aux and lst.hot and lst.n_ch <= 2 and _aux_supported(cell)
    for cf in cfgs:
        if short:
            medge = lst.hot and "s" in cell.terms and dense_edge
            fl = f"{int(has_aux)},{int(medge)}"
            fwd.append(f"agg_fwd_short|{cf}|{ops}|{fl}")
        else:
            fwd.append(f"agg_fwd_rows|{cf}|{ops}|")
        if cell.hub:
            fwd += [f"agg_hub_slices|{cf}|-|0", f"agg_fwd_hub_combine|{cf}|-|"]
        if cell.bwd == "none":
            continue
        fresh = cell.bwd in ("define", "no_gdst_gin", "rpw") and "s" in cell.terms
        if short and lst.hot and fresh and not cell.slices:
            edge = dense_edge or table
            bwd.append(f"agg_bwd_short|{cf}|{ops}|4,{int(edge)},{int(has_aux)}")
        else:
            bwd.append(f"agg_bwd_rows|{cf}|{ops}|")
        if cell.bwd == "rpw":
            bwd.append(f"agg_bwd_rows|{cf}|{ops}|")
        if cell.hub:
            bwd += [f"agg_hub_slices|{cf}|-|1", f"agg_bwd_hub_coef|{cf}|-|", f"agg_bwd_hub_emit|{cf}|-|"]
        if cell.two_phase and "s" in cell.terms:
            bwd.append(f"seg_sum_rows|{cell.vec}")
        if table:
            bwd += ["edge_table_grad_partial", "edge_table_grad_final"]
    return set(fwd), set(bwd)


def _aux_supported(cell):
    """dgn_agg_aux_bytes() > 0, by the header's description: a baked-in list that recomputes (max / min / dx) without std / var, at most
    two channels; on the short route with x_src and an even F, on the row route only the dx signs (no max / min, no hub rows)"""
    lst, g = cell.lst, graph(cell.graph)
    recomputes = any(o in (MX, MN, DX) for o in lst.ops)
    if not (lst.hot and recomputes and not lst.has_var and lst.n_ch <= 2):
        return False
    if g.route == "short":
        return "s" in cell.terms and cell.F % 2 == 0
    return lst.n_ch >= 1 and not any(o in (MX, MN) for o in lst.ops) and not cell.hub


def test_every_cell_runs_the_kernels_it_was_designed_for():
    """Every cell once more under the profiler (launches only, a sort between cells as the separator): the kernels of each cell are
    exactly the instances its description stands for, and the whole grid reaches every Cfg of launch_vec at every vector width, DynOps
    and StaticOps, the short kernels with their AUX / MEDGE / EDGE flags, the three hub kernels per direction, seg_sum_rows<1 | 2 | 4>
    and the edge-table kernels."""
    from torch.profiler import ProfilerActivity, profile
    dev = _dev()
    for c in CELLS:
        problem(c)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for c in CELLS:
            run_cell(c, compare=False)
            torch.arange(64, device=dev, dtype=torch.float32).sort()
            torch.cuda.synchronize()
    evs = sorted((e for e in prof.profiler.kineto_results.events() if str(e.device_type()).endswith("CUDA")), key=lambda e: e.start_ns())
    names = [e.name() for e in evs]
    out_dir = DUMP
    if out_dir:
        with open(os.path.join(out_dir, "agg_grid_kernels.txt"), "w") as f:
            f.write("\n".join(names))
    got, cur = [], []
    for n in names:
        if "sort" in n.lower():                          # (a sort is several kernels: the first one after a cell's kernels closes the cell)
            if cur:
                got.append(cur)
                cur = []
            continue
        key = _kernel_key(n)
        if key:
            cur.append(key)
    assert len(got) == len(CELLS), (len(got), len(CELLS))
    tally, wrong = {}, []
    for c, keys in zip(CELLS, got):
        fwd, bwd = expected_kernels(c)
        if set(keys) != fwd | bwd:
            wrong.append((c.name, sorted(set(keys) - (fwd | bwd)), sorted((fwd | bwd) - set(keys))))
        for k in keys:
            tally[k] = tally.get(k, 0) + 1
    assert not wrong, wrong[:10]
    if out_dir:
        with open(os.path.join(out_dir, "agg_grid_tally.txt"), "w") as f:
            f.write("\n".join(f"{k} {v}" for k, v in sorted(tally.items())))
        with open(os.path.join(out_dir, "agg_grid_ratios.txt"), "w") as f:
            f.write("\n".join(f"{k} error/tolerance {RATIOS[k]:.4f} error/fp32-error {VS_FP32.get(k, 0.0):.3f}" for k in sorted(RATIOS)))
    cfgs = {(n, int(s), int(a)) for n in range(5) for s in (0, 1) for a in ((0, 1) if n else (0,))}
    for vec in (1, 2, 4):
        for kern in ("agg_fwd_rows", "agg_bwd_rows", "agg_fwd_short"):
            have = {tuple(int(x) for x in k.split("|")[1].split(",")[1:4]) for k in tally if k.startswith(kern + f"|{vec},") and k.split("|")[2] == "D"}
            assert have >= cfgs, (vec, kern, sorted(cfgs - have))
        assert f"seg_sum_rows|{vec}" in tally
        for kern in ("agg_hub_slices", "agg_fwd_hub_combine", "agg_bwd_hub_coef", "agg_bwd_hub_emit"):
            assert any(k.startswith(kern + f"|{vec},") for k in tally), (vec, kern)
    flags = lambda kern: {k.split("|")[3] for k in tally if k.startswith(kern + "|")}
    assert flags("agg_fwd_short") >= {"0,0", "1,0", "0,1", "1,1"}, flags("agg_fwd_short")
    assert flags("agg_bwd_short") >= {"4,0,0", "4,1,0", "4,0,1", "4,1,1"}, flags("agg_bwd_short")
    assert flags("agg_hub_slices") == {"0", "1"}
    assert any(k.split("|")[1].endswith(",1") for k in tally if k.startswith("agg_fwd_short|")) and any(k.split("|")[1].endswith(",1") for k in tally if k.startswith("agg_fwd_rows|"))
    assert "edge_table_grad_partial" in tally and "edge_table_grad_final" in tally
    family = lambda pre: sum(v for k, v in tally.items() if k.startswith(pre))
    counts = {k: family(k) for k in ("agg_fwd_rows|", "agg_fwd_short|", "agg_bwd_rows|", "agg_bwd_short|", "agg_hub_slices|", "agg_fwd_hub_combine|",
                                     "agg_bwd_hub_coef|", "agg_bwd_hub_emit|", "seg_sum_rows|1", "seg_sum_rows|2", "seg_sum_rows|4", "edge_table_grad_partial",
                                     "edge_table_grad_final")}
    assert counts == LAUNCHES, counts


# launches of the whole grid per kernel (forward + backward of every cell, once): from the cells' descriptions, counted by hand of the
# dispatch rules in launch_forward_cfg / launch_backward_cfg -- a cell that lands on another kernel, or a kernel that runs twice, moves them
LAUNCHES = {"agg_fwd_rows|": 181, "agg_fwd_short|": 147, "agg_bwd_rows|": 261, "agg_bwd_short|": 76, "agg_hub_slices|": 78, "agg_fwd_hub_combine|": 39,
            "agg_bwd_hub_coef|": 39, "agg_bwd_hub_emit|": 39, "seg_sum_rows|1": 35, "seg_sum_rows|2": 191, "seg_sum_rows|4": 35,
            "edge_table_grad_partial": 29, "edge_table_grad_final": 29}
