"""Graphs and host-side restatements for the grid of the two one-kernel backward routes of the sweep (tests/test_agg_blk_grid_gpu.py):
the block backward (csrc/dgn_agg_block.hpp: one wave owns a run of whole graphs) and the graph backward (csrc/dgn_agg_graph.hpp: one
workgroup owns one graph).  numpy only; tests/test_agg_blk_graphs_cpu.py asserts every claim made here.

Every graph is a batch of whole graphs laid out one after the other: every source of a row lies inside the row's own graph, and inside
a graph row r > lo of at least one slot has r - 1 as its first source (a row without slots hands that duty to the row behind it), so
the closed cuts are exactly the graph boundaries.  All have duplicated sources (rows = 1 mod 4), self loops (rows = 3 mod 4) and a
source without an out-edge (the last row of the largest graph, and every isolated node).

Block graphs (E <= 3 N: the short route):
  mol37      sizes 1 2 3 4 5 7 8 9 23 37 and molecule-like ones up to 37, N = 3 mod 4, ordered (by its seed) so that the block
             boundaries of the default plan at F = 70 take all four residues mod 4; rows of 1..4 slots, a few of none, one of 7 (the
             per-row routine inside a group) and one of 70 slots from 7 sources (more than one 64-slot batch)
  mol23      largest graph 23, N = 1 mod 4       mol52  largest graph 52 (the largest the block route is tried for), N = 2 mod 4
  mol_one    a single graph of 5 rows            mol_chain  mol23 with one edge between two neighbouring graphs: that boundary is no
             closed cut any more, the gap grows to the two graphs' sum
  mol_bip    mol23 with three more source rows than destination rows (n_src != n_nodes: the block route declines)
Graph-route graphs (E > 3 N):
  knn        graphs of 9, 40, 85, 150 rows with 8 slots per row, a few rows of none, one row of 70 slots, one source of more than 64
             out-edges                           knn_big  one graph of 300 rows
  knn_bip    knn with three more source rows than destination rows
  short_g    mol23 carrying a gblk_desc (a short-route graph: the graph route declines)
"""
import numpy as np

K_BLK_ROWS_MAX = 56          # kBlkRowsMax
BLOCK_MAX_GAP = 52           # dgn_amd/graph.py
GRAPH_LDS_MAX = 160 * 1024   # launch_backward_graph_cfg
GRAPH_THREADS = 1024


class BatchGraph:
    """CSR of a batch of whole graphs from per-row source lists, with the transposed view and every description of include/dgn_hip.h"""

    def __init__(self, name, sizes, rows, n_src=None):
        self.name, self.sizes = name, np.asarray(sizes, dtype=np.int64)
        self.bounds = np.concatenate([[0], np.cumsum(self.sizes)])
        self.N = N = int(self.bounds[-1])
        assert len(rows) == N
        self.n_src = n_src or N
        self.degs = np.asarray([len(r) for r in rows], dtype=np.int64)
        self.indptr = np.concatenate([[0], np.cumsum(self.degs)]).astype(np.int64)
        self.E = E = int(self.indptr[-1])
        self.src = np.asarray([s for r in rows for s in r], dtype=np.int64).reshape(E)
        self.dst = np.repeat(np.arange(N), self.degs)
        self.rows = rows
        order = np.argsort(self.src, kind="stable")                     # slots by (source, slot)
        self.csc_order = order
        self.csc_pos = np.empty(E, dtype=np.int64)
        self.csc_pos[order] = np.arange(E)
        self.out_deg = np.bincount(self.src, minlength=self.n_src)
        self.csc_ptr = np.concatenate([[0], np.cumsum(self.out_deg)])
        self.log_deg = np.log(self.degs.astype(np.float64) + 1.0).astype(np.float32)
        self.blk_cut, self.blk_gap = closed_cuts(self.src, self.dst, N)
        self.gblk_desc = np.stack([self.bounds[:-1], self.bounds[1:], self.indptr[self.bounds[:-1]], self.indptr[self.bounds[1:]]], axis=1)
        self.gblk_rows = int(self.sizes.max())

    def hub(self, threshold, chunk):
        rows = np.nonzero(self.degs > threshold)[0]
        n_sl = (self.degs[rows] + chunk - 1) // chunk
        return dict(hub_rows=rows, hub_chunk_ptr=np.concatenate([[0], np.cumsum(n_sl)]), chunk_hub=np.repeat(np.arange(len(rows)), n_sl))

    @property
    def route(self):
        return "short" if self.E <= 3 * self.N else ("rows1" if self.E >= 8 * self.N else "rows4")

    def graph_of(self, row):
        return np.searchsorted(self.bounds, row, side="right") - 1


# ---- restatements -------------------------------------------------------------------------------------------------------------------
def closed_cuts(src, dst, N):
    """(blk_cut [N + 1], blk_gap) of dgn_graph_build_cuts: blk_cut[i] = the last closed cut <= i (a cut c is closed when no edge joins a
    node below c to a node at or above it), blk_gap = the largest distance between consecutive closed cuts"""
    diff = np.zeros(N + 2, dtype=np.int64)
    a, b = np.minimum(src, dst), np.maximum(src, dst)
    m = a < b
    np.add.at(diff, a[m] + 1, 1)
    np.add.at(diff, b[m] + 1, -1)
    cross = np.cumsum(diff)[: N + 1]
    closed = cross == 0
    last = np.maximum.accumulate(np.where(closed, np.arange(N + 1), 0))
    cuts = np.flatnonzero(closed)
    gap = int(np.diff(cuts).max()) if cuts.size > 1 else 0
    return last, gap


def blk_plan(F, gap, lds_kb=13):
    """(bin, rcap) of dgn_agg_block.hpp's blk_plan, or None where it refuses (bin < 4)"""
    rcap = min((lds_kb * 1024) // (4 * F), K_BLK_ROWS_MAX, gap + 15)
    bin_ = rcap - gap + 1
    return (bin_, rcap) if bin_ >= 4 else None


def blk_bins(blk_cut, N, bin_):
    """(lo, hi) of every bin of agg_bwd_block: the rows between the last closed cuts at or below the bin's two ends"""
    n_bins = (N + bin_ - 1) // bin_
    return [(int(blk_cut[b * bin_]), int(blk_cut[min((b + 1) * bin_, N)])) for b in range(n_bins)]


def graph_coef_slots(n_ch, av):
    return 1 + n_ch * (2 if av else 1)


def graph_plan(F, n_gblk, gblk_rows, n_ch, av, alias, tiles_opt=0, need_signs=False, has_aux=False):
    """(tiles, LDS bytes) of launch_backward_graph_cfg, or None where it refuses (LDS beyond 160 KB; a dx aggregator without its aux table)"""
    nco, nsw = graph_coef_slots(n_ch, av), n_ch * (2 if av else 1)
    pairs = (F + 1) >> 1
    tiles = tiles_opt
    if tiles <= 0:
        tiles = 1
        while tiles < 4 and n_gblk * tiles < 256 and (pairs + 2 * tiles - 1) // (2 * tiles) >= 8:
            tiles *= 2
    tiles = min(tiles, pairs)
    ppt = (pairs + tiles - 1) // tiles
    tiles = (pairs + ppt - 1) // ppt
    lds = (gblk_rows * (nco + (1 if alias else 0)) * ppt * 2 + gblk_rows * nsw) * 4
    if lds > GRAPH_LDS_MAX or (need_signs and not has_aux):
        return None
    return tiles, lds


# ---- generators ---------------------------------------------------------------------------------------------------------------------
def _rows(sizes, rng, deg_of, specials=()):
    """per-row source lists: `deg_of(rng, n)` slots per row of a graph of n rows; `specials`: {(graph, row in graph): source list
    builder}.  Chain first sources, duplicates, self loops as the module's docstring says; the last row of the largest graph is
    nobody's source."""
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    big = int(np.argmax(sizes))
    silent = int(bounds[big + 1] - 1) if sizes[big] > 2 else -1
    rows = []
    for gi, n in enumerate(sizes):
        lo = int(bounds[gi])
        degs = [int(deg_of(rng, n)) for _ in range(n)]
        if n == 1:
            degs = [0]
        degs[0] = max(degs[0], 1) if n > 1 else 0
        for i in range(1, n):                                   # a row without slots: never the last of its graph, never two in a row
            if degs[i] == 0 and (i == n - 1 or degs[i - 1] == 0):
                degs[i] = 1
        for i in range(n):
            r, d = lo + i, degs[i]
            if (gi, i) in specials:
                rows.append(specials[(gi, i)](lo, n, r))
                continue
            pool = np.setdiff1d(np.arange(lo, lo + n), [silent])
            s = [int(x) for x in pool[rng.integers(0, len(pool), d)]]
            if d >= 1 and i > 0:
                s[0] = r - 2 if degs[i - 1] == 0 else r - 1    # (the row before has no slot of its own: span both cuts)
            if d >= 1 and i == 0 and n > 1:
                s[0] = r + 1
            if r % 4 == 1 and d >= 2:
                s[1] = s[0]
            elif r % 4 == 3 and d >= 2 and r != silent:
                s[d - 1] = r
            rows.append(s)
    return rows


def _mol_degs(rng, n):
    return rng.choice([0, 1, 2, 3, 4], p=[0.04, 0.25, 0.38, 0.25, 0.08])


def _mol_sizes(rng, must, lo, hi, total, rem):
    sizes = list(must)
    while sum(sizes) < total:
        sizes.append(int(rng.integers(lo, hi + 1)))
    sizes = [int(s) for s in rng.permutation(sizes)]
    for i, s in enumerate(sizes):                               # the remainder mod 4 by shrinking one free graph
        if s not in must and s > lo + 3:
            sizes[i] = s - (sum(sizes) - rem) % 4
            break
    assert sum(sizes) % 4 == rem
    return sizes


def _mol(name, seed, must, lo, hi, total, rem, long_rows=True, extra_edge=False, n_src_extra=0):
    rng = np.random.default_rng(seed)
    sizes = _mol_sizes(rng, must, lo, hi, total, rem)
    specials = {}
    if long_rows:
        big = int(np.argmax(sizes))
        # a row of 7 slots (the per-row routine inside a group of four) and one of 70 slots from 7 sources (two slot batches)
        specials[(big, 5)] = lambda lo_, n, r: [r - 1] + [lo_ + (3 * k) % (n - 1) for k in range(6)]
        specials[(big, 11)] = lambda lo_, n, r: [r - 1 - k for k in range(7)] * 10
    rows = _rows(sizes, rng, _mol_degs, specials)
    if extra_edge:                                              # the first row of graph k + 1 also hears the last row of graph k
        bounds = np.concatenate([[0], np.cumsum(sizes)])
        k = int(np.argmax(sizes))
        k = k if k + 1 < len(sizes) else k - 1
        rows[int(bounds[k + 1])].append(int(bounds[k + 1]) - 1)
        sizes = sizes[:k] + [sizes[k] + sizes[k + 1]] + sizes[k + 2:]
    g = BatchGraph(name, sizes, rows, n_src=(sum(sizes) + n_src_extra) if n_src_extra else None)
    return g


def _knn(name, sizes, seed, n_src_extra=0):
    rng = np.random.default_rng(seed)
    big = int(np.argmax(sizes))
    specials = {(big, 17): lambda lo_, n, r: [r - 1] + [lo_ + (7 * k) % (n - 1) for k in range(69)]}
    rows = _rows(sizes, rng, lambda rng_, n: 0 if rng_.random() < 0.03 else 8, specials)
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    hub_src = int(bounds[big]) + 3                              # a source of more than 64 out-edges: the third slot of 80 rows of its graph
    n_big, k = sizes[big], 0
    for i in range(20, n_big):
        r = int(bounds[big]) + i
        if len(rows[r]) == 8 and k < 80:
            rows[r][2] = hub_src
            k += 1
    return BatchGraph(name, sizes, rows, n_src=(sum(sizes) + n_src_extra) if n_src_extra else None)


MOL37_MUST = (1, 2, 3, 4, 5, 7, 8, 9, 23, 37)


def _build(name):
    if name == "mol37":
        return _mol(name, 37, MOL37_MUST, 9, 37, 500, 3)
    if name == "mol23":
        return _mol(name, 23, (1, 2, 6, 23), 5, 23, 200, 1)
    if name == "mol52":
        return _mol(name, 52, (1, 3, 52), 20, 52, 250, 2)
    if name == "mol_one":                                       # row 1 a duplicated source, row 3 a self loop, source 4 without out-edge
        return BatchGraph(name, [5], [[1, 0], [0, 0], [1], [2, 3], [3]])
    if name == "mol_chain":
        return _mol(name, 23, (1, 2, 6, 23), 5, 23, 200, 1, extra_edge=True)
    if name == "mol_bip":
        return _mol(name, 23, (1, 2, 6, 23), 5, 23, 200, 1, n_src_extra=3)
    if name == "short_g":
        return _mol(name, 23, (1, 2, 6, 23), 5, 23, 200, 1)
    if name == "knn":
        return _knn(name, [9, 40, 85, 150], 8)
    if name == "knn_bip":
        return _knn(name, [9, 40, 85, 150], 8, n_src_extra=3)
    if name == "knn_big":
        return _knn(name, [300], 9)
    raise KeyError(name)


BLOCK_GRAPHS = ("mol37", "mol23", "mol52", "mol_one", "mol_chain")
GRAPH_GRAPHS = ("knn", "knn_big")
ALL_GRAPHS = BLOCK_GRAPHS + GRAPH_GRAPHS + ("mol_bip", "short_g", "knn_bip")
_CACHE = {}


def graph(name) -> BatchGraph:
    if name not in _CACHE:
        _CACHE[name] = _build(name)
    return _CACHE[name]
