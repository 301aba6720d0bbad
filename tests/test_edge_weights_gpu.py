"""The per-edge directional weights (csrc/dgn_edge_weights.hip) themselves, on every dispatch route, against their fp64 statement
``oracle.dgn_oracle.edge_weights_ref`` (tied to the oracle's aggregators by tests/test_edge_weights_oracle_cpu.py).

Every other test sees the weights through an aggregate, at whatever route its fixture's size selects, under layer-level tolerances.  Here
``dgn_amd.compute_edge_weights`` is called with raw ``Channel`` tuples on the smallest graphs at which every row class, class boundary and
hub-slice seam exists, and the routes are chosen through the option table (``ew_big_min``, ``ew_separate``, ``ew_no_flat8``).

Kernels reached, from the dispatch at the end of dgn_edge_weights.hip (``small`` = ``ew_rows_small``, which runs the bodies of
``ew_rows_flat``, ``ew_rows_g16<4>`` and -- largest in-degree unknown or > 16 -- ``ew_rows<1>`` in one launch; ``hub`` = ``ew_hub_slice_stats``
-> ``ew_hub_combine`` -> ``ew_hub_slice_write``, appended whenever the graph has hub rows):

    graph (largest in-degree)          defaults          ew_big_min=0                     ew_separate=1
    le4    (4)                         flat              flat                             flat
    le8    (8)                         flat8             flat8                            flat8
    le8    ew_no_flat8=1               small (f, g)      flat + g16<64>                   flat + g16<4>
    le16   (16)                        small (f, g)      flat + g16<64>                   flat + g16<4>
    mixed  (200)                       small (f, g, r)   flat + g16<64> + rows<64>        flat + g16<4> + rows<1>
    tiny1x5 (5)                        flat8             flat8                            flat8
    tiny1x5 ew_no_flat8=1              small (f, g)      flat + g16<64>                   flat + g16<4>
    tiny1x20, tiny3 (20)               small (f, g, r)   flat + g16<64> + rows<64>        flat + g16<4> + rows<1>
    hub    (1045, threshold 64)        small + hub       flat + g16<64> + rows<64> + hub  flat + g16<4> + rows<1> + hub
    hub_unsliced (threshold 2^30)      small (f, g, r)   flat + g16<64> + rows<64>        flat + g16<4> + rows<1>
    padded le8 / mixed (unknown: 0)    small (f, g, r)   flat + g16<64> + rows<64>        --

Rows of more than 64 slots (mixed: 65, 129, 200; hub_unsliced: up to 1045) take ``range_stats`` / ``range_write`` inside ``ew_rows``, the
rest of its class the one-slot-per-lane branch.  The ``eig`` layouts pick the vector width of the row loads (K = 4, 8, 12: 16 bytes; K = 2, 6
and the 8-byte aligned view: 8 bytes; K = 1, 3 and the 4-byte aligned view: 4 bytes), K = 8 reads the second ``float4`` of a row prefix and
column 9 of K = 12 the scalar fallback.

THE BOUND is derived, not tuned.  With u = 2^-24 and d the slots of the row, ``|w - w_ref| <= (d + 16) u |w_ref|``, and ``w == 0`` exactly
where ``w_ref == 0``: one rounding for the fp32 delta, at most d - 1 roundings in a sum of non-negative terms in any order, the eps add, the
divide, ``expf`` and its argument with ``|alpha delta| < 1``.  (A CPU emulation with strictly sequential fp32 sums, in-degrees 1..3000,
scales 1, 1e-3 and 3e-8 and all four channel kinds reached 0.16 of it.)  Every comparison records its worst ratio to the bound through
``parity_util.note`` (lines ``EDGE-WEIGHTS ...`` of the parity report, ``parity_util.REPORT_FILE``).

Values: ``eig`` ~ N(0, 1) in fp32, with planted rows in every class of every graph: rows whose neighbours all carry the destination's own
values (deltas exactly 0: ABSNORM and BALANCED exactly 0, softmax 1 / deg), rows whose deltas are all positive (``sneg = 0``), and rows that
live, with their neighbours, at a scale of 3e-8, where ``eps = 1e-8`` moves the result by tens of percent.  Sources are random, with
duplicates and self loops."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ABSNORM, BALANCED, SOFTMAX = 0, 1, 2
CLASSES = ((1, 4), (5, 8), (9, 16), (17, 64), (65, 1 << 30))      # the in-degree classes of the kernels (flat, flat8, g16, wave, > one slot batch)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def four_kinds(c0, c1, c2):
    return ((ABSNORM, c0, 0.0), (BALANCED, c1, 0.0), (SOFTMAX, c2, 0.1), (SOFTMAX, c1, -0.1))


MAIN = four_kinds(1, 2, 3)


# ---- graphs -----------------------------------------------------------------------------------------------------------------------
class G:
    """A destination-major CSR from seeded numpy, with the roles of its planted rows and the node pools their sources are drawn from."""

    def __init__(self, name, degs, seed, num_src=None, **graph_kw):
        rng = np.random.default_rng(seed)
        self.name, self.degs, self.graph_kw = name, np.asarray(degs, dtype=np.int64), graph_kw
        n = self.n = len(degs)
        self.num_src = N = num_src or n
        self.indptr = np.concatenate([[0], np.cumsum(self.degs)])
        self.E = int(self.indptr[-1])
        self.dst = np.repeat(np.arange(n), self.degs)
        src = rng.integers(0, N, self.E)
        loops = rng.random(self.E) < 0.03
        src[loops] = self.dst[loops]                                                  # self loops
        for r in range(n):                                                            # a duplicated source in every fourth row of >= 2 slots
            if r % 4 == 1 and self.degs[r] >= 2:
                src[self.indptr[r] + 1] = src[self.indptr[r]]
        # planted rows: per class one 'zero', one 'pos' and two 'tiny' rows, where the class has rows to spare
        self.zero, self.pos, self.tiny = [], [], []
        self.pool_zero = self.pool_pos = self.pool_tiny = np.zeros(0, dtype=np.int64)
        if n >= 100:
            free = np.ones(n, dtype=bool)
            for lo, hi in CLASSES:
                rows = rng.permutation(np.nonzero((self.degs >= lo) & (self.degs <= min(hi, 1000)))[0])      # (the 66-slice row keeps N(0, 1) values)
                take = 4 if len(rows) >= 8 else (3 if len(rows) >= 5 else 0)
                for r, role in zip(rows[:take], (self.zero, self.pos, self.tiny, self.tiny)):
                    role.append(int(r))
                    free[r] = False
            pool = rng.permutation(np.nonzero(free)[0])
            self.pool_zero, self.pool_pos, self.pool_tiny = pool[0:3], pool[3:7], pool[7:13]
            pick = lambda choices, k: np.asarray(choices)[rng.integers(0, len(choices), k)]
            for r in self.zero:        # neighbours: the zero rows themselves and their clones (all share one eig row)
                src[self.indptr[r]:self.indptr[r + 1]] = pick(list(self.pool_zero) + self.zero, self.degs[r])
            for r in self.pos:
                src[self.indptr[r]:self.indptr[r + 1]] = pick(self.pool_pos, self.degs[r])
            for r in self.tiny:
                src[self.indptr[r]:self.indptr[r + 1]] = pick(list(self.pool_tiny) + [t for t in self.tiny if t != r], self.degs[r])
        self.src = src
        self.slot_deg = self.degs[self.dst]                                           # d of the bound, per slot
        self._eig, self._ref = {}, {}

    def eig(self, K, seed=0):
        """fp32 [num_src, K] ~ N(0, 1) with the planted rows' values, the same in every column (cached: tests share it unchanged)."""
        if (K, seed) not in self._eig:
            rng = np.random.default_rng(1000 + 31 * K + seed)
            e = rng.standard_normal((self.num_src, K)).astype(np.float32)
            if self.zero:
                e[list(self.pool_zero) + self.zero] = e[self.zero[0]]
                e[self.pos] = np.minimum(e[self.pos], 2.5)
                e[self.pool_pos] = 3.0 + rng.random((len(self.pool_pos), K)).astype(np.float32)
                tiny = list(self.pool_tiny) + self.tiny
                e[tiny] = e[tiny] * np.float32(3e-8)
            self._eig[(K, seed)] = torch.from_numpy(e)
        return self._eig[(K, seed)]

    def ref(self, key, eig, channels, **kw):
        """edge_weights_ref, computed once per (eig layout, channels) and shared."""
        from oracle import dgn_oracle as orc
        k = (key, channels, tuple(sorted(kw)))
        if k not in self._ref:
            self._ref[k] = orc.edge_weights_ref(self.indptr, self.src, eig, channels, **kw)
        return self._ref[k]

    def device_graph(self, dev, **over):
        import dgn_amd
        kw = dict(self.graph_kw, **over)
        g = dgn_amd.DGNGraph.from_csr(torch.from_numpy(self.indptr).to(dev), torch.from_numpy(self.src).to(dev),
                                      num_src=self.num_src if self.num_src != self.n else None, **kw)
        assert g.max_in_degree == int(self.degs.max()) and g.num_edges == self.E
        return g


def _le4():
    rng = np.random.default_rng(4)
    degs = rng.integers(0, 5, 300)
    degs[0], degs[-1] = 0, 3
    assert set(degs.tolist()) == {0, 1, 2, 3, 4}
    return G("le4", degs, 40)


def _le8():
    rng = np.random.default_rng(8)
    degs = rng.integers(0, 9, 203)
    degs[[10, 70, 130]] = (4, 5, 8)
    degs[0], degs[-1] = 0, 8
    assert set(degs.tolist()) == set(range(9))
    return G("le8", degs, 80)


def _le16():
    rng = np.random.default_rng(16)
    degs = rng.integers(0, 17, 203)
    degs[[10, 70, 130]] = (8, 9, 16)
    degs[0], degs[-1] = 0, 16
    assert set(degs.tolist()) == set(range(17))
    return G("le16", degs, 160)


def _mixed():
    """203 rows from {0, 1, 4, 5, 8, 9, 16, 17, 63, 64, 65, 129, 200}, every value at least twice; rows 20..24 are five consecutive rows of
    the (4, 16] class (a g16 wave works on four rows at a time: looking at the 64 candidate rows 0..63 it takes a second trip through its
    list), rows 70 and 75 have 129 and 200 slots inside the candidate group 64..127 (a ballot wave walks a list of two rows of more than
    one slot batch)."""
    rng = np.random.default_rng(200)
    small = [0, 1, 4, 5, 8, 9, 16, 17]
    degs = np.asarray(small)[rng.integers(0, len(small), 203)]
    degs[20:25] = (5, 16, 9, 8, 16)
    long_rows = {30: 63, 31: 64, 40: 65, 70: 129, 75: 200, 100: 63, 101: 64, 140: 65, 141: 129, 190: 200, 191: 17, 192: 17}
    for r, d in long_rows.items():
        degs[r] = d
    degs[0], degs[-1] = 0, 9
    counts = {v: int((degs == v).sum()) for v in (0, 1, 4, 5, 8, 9, 16, 17, 63, 64, 65, 129, 200)}
    assert min(counts.values()) >= 2 and sum(counts.values()) == 203, counts
    return G("mixed", degs, 2000)


def _hub_degs():
    """120 rows: hub rows (more than 64 slots; slices of 16) of 65, 80 = 5 x 16, 81 and 1045 slots (66 slices: the lanes of ew_hub_combine
    make a second trip), three more of 65 / 81 / 80 to carry the planted values, the rest from the three lower classes up to 64 itself."""
    rng = np.random.default_rng(64)
    low = [0, 1, 2, 4, 5, 7, 8, 9, 12, 16, 17, 33, 63, 64]
    degs = np.asarray(low)[rng.integers(0, len(low), 120)]
    for r, d in {5: 65, 17: 80, 18: 81, 60: 1045, 61: 64, 90: 65, 91: 81, 119: 80, 3: 64, 4: 17}.items():
        degs[r] = d
    degs[0] = 0
    return degs


GRAPHS = {}


def graph(name):
    if name not in GRAPHS:
        if name in ("hub", "hub_unsliced"):
            degs = _hub_degs()
            GRAPHS["hub"] = G("hub", degs, 640, hub_threshold=64, hub_chunk=16)
            GRAPHS["hub_unsliced"] = G("hub_unsliced", degs, 640, hub_threshold=2 ** 30, hub_chunk=16)      # the same CSR (same seed)
        else:
            GRAPHS[name] = {"le4": _le4, "le8": _le8, "le16": _le16, "mixed": _mixed,
                            "tiny1x5": lambda: G("tiny1x5", [5], 15, num_src=9),
                            "tiny1x20": lambda: G("tiny1x20", [20], 120, num_src=9),
                            "tiny3": lambda: G("tiny3", [20, 0, 5], 320, num_src=9)}[name]()
    return GRAPHS[name]


ALL_GRAPHS = ("le4", "le8", "le16", "mixed", "tiny1x5", "tiny1x20", "tiny3", "hub", "hub_unsliced")
ROUTES = {"defaults": {}, "big0": {"ew_big_min": 0}, "separate": {"ew_separate": 1}, "no_flat8": {"ew_no_flat8": 1},
          "no_flat8+big0": {"ew_no_flat8": 1, "ew_big_min": 0}, "no_flat8+separate": {"ew_no_flat8": 1, "ew_separate": 1}}


def _set_route(monkeypatch, route):
    from dgn_amd import _lib
    assert (_lib.options.ew_big_min, _lib.options.ew_separate, _lib.options.ew_no_flat8) == (1 << 19, 0, 0), "the library's defaults"
    for k, v in ROUTES[route].items():
        monkeypatch.setattr(_lib.options, k, v)


# ---- the comparison ---------------------------------------------------------------------------------------------------------------
WORST = {}


def compare(w, ref, slot_deg, name):
    """``|w - w_ref| <= (d + 16) u |w_ref|`` per entry, exact zeros where the reference is exactly zero; the worst ratio goes on record."""
    from parity_util import note
    w = w.detach().cpu().double()
    assert w.shape == ref.shape, (name, tuple(w.shape), tuple(ref.shape))
    assert bool(torch.isfinite(w).all()), f"{name}: {int((~torch.isfinite(w)).sum())} entries not finite"
    bound = (torch.from_numpy(slot_deg).double() + 16.0).unsqueeze(0) * U * ref.abs()
    zero = ref == 0
    ratio = ((w - ref).abs() / bound.masked_fill(zero, 1.0)).masked_fill(zero, 0.0)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    at = np.unravel_index(int(ratio.argmax()), ratio.shape) if ratio.numel() else (0, 0)
    WORST[name] = worst
    note(f"EDGE-WEIGHTS {name}: n={w.numel()} exact zeros={int(zero.sum())} worst |w - w_ref| / ((d + 16) u |w_ref|) = {worst:.4f} "
         f"(channel {at[0]}, slot {at[1]}, d = {int(slot_deg[at[1]]) if len(slot_deg) else 0})")
    assert bool((w[zero] == 0).all()), f"{name}: {int((w[zero] != 0).sum())} entries not exactly 0 where the reference is"
    assert worst <= 1.0, f"{name}: worst ratio to the bound {worst:.4f} at channel {at[0]}, slot {at[1]}"


def run(g, dev, channels, eig=None, name="", graph_over=None, **slot):
    import dgn_amd
    dg = g.device_graph(dev, **(graph_over or {}))
    w = dgn_amd.compute_edge_weights(dg, channels, eig=eig, **slot)
    torch.cuda.synchronize()
    return dg, w


# ---- every graph on every route -------------------------------------------------------------------------------------------------
def _cases():
    out = [(gn, r) for gn in ALL_GRAPHS for r in ("defaults", "big0", "separate")]
    out += [(gn, r) for gn in ("le8", "tiny1x5") for r in ("no_flat8", "no_flat8+big0", "no_flat8+separate")]
    return out


@pytest.mark.parametrize("gname,route", _cases(), ids=lambda v: v)
def test_weights_on_every_route(gname, route, monkeypatch):
    dev = _dev()
    g = graph(gname)
    _set_route(monkeypatch, route)
    eig = g.eig(4)
    dg, w = run(g, dev, MAIN, eig=eig.to(dev))
    if gname == "hub":
        assert dg.n_hub == 7 and dg.n_chunks == 5 + 5 + 6 + 66 + 5 + 6 + 5
    elif gname == "hub_unsliced":
        assert dg.n_hub == 0
    compare(w, g.ref("K4", eig, MAIN), g.slot_deg, f"{gname} [{route}]")


def test_planted_rows_are_what_they_claim():
    """The reference on the planted rows (no GPU arithmetic involved): zero rows give exact zeros and 1 / deg, positive rows no backward
    field, and on the tiny rows eps takes at least 100 bounds of the row off sum |w| = 1 (tens of percent on the shortest rows) -- an eps
    error cannot hide."""
    for gname in ("le4", "le8", "le16", "mixed", "hub"):
        g = graph(gname)
        ref = g.ref("K4", g.eig(4), MAIN)
        a2 = g.ref("K4", g.eig(4), ((ABSNORM, 2, 0.0),))                                      # ABSNORM on BALANCED's column
        assert g.zero and g.pos and len(g.tiny) >= 2, gname
        for r in g.zero:
            sl = slice(int(g.indptr[r]), int(g.indptr[r + 1]))
            assert bool((ref[0, sl] == 0).all()) and bool((ref[1, sl] == 0).all())
            assert torch.allclose(ref[2, sl], torch.full_like(ref[2, sl], 1.0 / g.degs[r]), rtol=1e-14, atol=0)
        for r in g.pos:
            sl = slice(int(g.indptr[r]), int(g.indptr[r + 1]))
            assert bool((ref[0, sl] > 0).all()) and torch.equal(ref[1, sl], a2[0, sl] / 2)
        for r in g.tiny:
            sl = slice(int(g.indptr[r]), int(g.indptr[r + 1]))
            total = float(ref[0, sl].abs().sum())                                            # 1 without eps
            assert 0.0 < total < 1.0 - 100 * (g.degs[r] + 16) * U, (gname, r, total)


# ---- padded graphs: the largest in-degree is unknown ----------------------------------------------------------------------------
@pytest.mark.parametrize("gname", ["le8", "mixed"])
@pytest.mark.parametrize("route", ["defaults", "big0"])
def test_weights_on_a_padded_graph(gname, route, monkeypatch):
    """``DGNGraph.padded`` + ``rebuild``: ``max_in_degree`` is 0 (unknown), so no class is skipped and le8 does not take flat8; a larger batch
    is loaded first, so rows and slots beyond the tested batch hold its remains.  Slots [0, E) are compared."""
    import dgn_amd
    dev = _dev()
    g = graph(gname)
    _set_route(monkeypatch, route)
    n_cap, e_cap = g.n + 53, g.E + 517
    pg = dgn_amd.DGNGraph.padded(n_cap, e_cap, dev, eig_dim=4)
    rng = np.random.default_rng(9)
    pg.rebuild(torch.from_numpy(rng.integers(0, n_cap, e_cap)).to(dev), torch.from_numpy(rng.integers(0, n_cap, e_cap)).to(dev), n_cap,
               eig=torch.from_numpy(rng.standard_normal((n_cap, 4)).astype(np.float32)).to(dev))
    eig = g.eig(4)
    pg.rebuild(torch.from_numpy(g.src).to(dev), torch.from_numpy(g.dst).to(dev), g.n, eig=eig.to(dev))
    assert pg.max_in_degree == 0 and pg.num_edges == e_cap
    assert torch.equal(pg.indptr[:g.n + 1].cpu().long(), torch.from_numpy(g.indptr)) and torch.equal(pg.src[:g.E].cpu().long(), torch.from_numpy(g.src))
    w = dgn_amd.compute_edge_weights(pg, MAIN, eig=pg.ndata["eig"])
    torch.cuda.synchronize()
    pg.check_deferred()
    assert tuple(w.shape) == (4, e_cap)
    compare(w[:, :g.E], g.ref("K4", eig, MAIN), g.slot_deg, f"{gname} padded [{route}]")


# ---- eig layouts ------------------------------------------------------------------------------------------------------------------
# name: (columns of the tensor, view [a, b) of it or None, channel columns (c0, c1, c2) of the VIEW, expected bytes of a row load)
LAYOUTS = {
    "K1": (1, None, (0, 0, 0), 4), "K2": (2, None, (0, 1, 1), 8), "K3": (3, None, (0, 1, 2), 4), "K4": (4, None, (0, 2, 3), 16),
    "K6-col5": (6, None, (5, 1, 3), 8), "K8-col7": (8, None, (7, 4, 0), 16), "K12-cols3,9": (12, None, (3, 9, 3), 16),
    "view-1:4-of-8": (8, (1, 4), (0, 1, 2), 4), "view-2:6-of-8": (8, (2, 6), (3, 1, 2), 8),
}


@pytest.mark.parametrize("layout", list(LAYOUTS), ids=lambda v: v)
@pytest.mark.parametrize("gname", ["mixed", "hub"])
def test_eig_layouts(gname, layout, monkeypatch):
    dev = _dev()
    g = graph(gname)
    K, view, cols, nbytes = LAYOUTS[layout]
    channels = four_kinds(*cols)
    full = g.eig(K, seed=1)
    full_dev = full.to(dev)
    eig, eig_dev = (full, full_dev) if view is None else (full[:, view[0]:view[1]], full_dev[:, view[0]:view[1]])
    assert eig_dev.stride(0) == K and eig_dev.stride(1) == 1
    widest = max(v for v in (16, 8, 4) if (4 * K) % v == 0 and eig_dev.data_ptr() % v == 0)
    assert widest == nbytes, (layout, widest)
    ref = g.ref(layout, eig, channels)
    for route in ("defaults", "big0"):
        with monkeypatch.context() as mp:
            _set_route(mp, route)
            _, w = run(g, dev, channels, eig=eig_dev)
        compare(w, ref, g.slot_deg, f"{gname} eig {layout} [{route}]")


# ---- channel sets -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", ["mixed", "hub"])
@pytest.mark.parametrize("chset", ["absnorm-only", "six"])
def test_channel_sets(gname, chset, monkeypatch):
    """One ABSNORM channel (no softmax: the second pass of range_stats does not run) and six channels (two launches of at most DGN_MAX_CH,
    the second into planes 4 and 5)."""
    from dgn_amd import _lib
    dev = _dev()
    g = graph(gname)
    channels = ((ABSNORM, 2, 0.0),) if chset == "absnorm-only" else MAIN + ((ABSNORM, 3, 0.0), (SOFTMAX, 1, 0.1))
    assert (len(channels) > _lib.DGN_MAX_CH) == (chset == "six")
    eig = g.eig(4)
    ref = g.ref("K4", eig, channels)
    for route in ("defaults", "big0"):
        with monkeypatch.context() as mp:
            _set_route(mp, route)
            _, w = run(g, dev, channels, eig=eig.to(dev))
        compare(w, ref, g.slot_deg, f"{gname} channels {chset} [{route}]")


# ---- slot mode, shard -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", ["mixed", "hub"])
def test_slot_mode(gname, monkeypatch):
    """Both endpoints per slot (``eig_s_edge = eig[src]``, ``eig_d_edge = eig[dst of the slot]``) and no node table: the same weights."""
    dev = _dev()
    g = graph(gname)
    eig = g.eig(4)
    es, ed = eig[torch.from_numpy(g.src)].contiguous(), eig[torch.from_numpy(g.dst)].contiguous()
    ref = g.ref("K4-slots", None, MAIN, eig_s_edge=es, eig_d_edge=ed)
    assert torch.equal(ref, g.ref("K4", eig, MAIN))
    for route in ("defaults", "big0"):
        with monkeypatch.context() as mp:
            _set_route(mp, route)
            _, w = run(g, dev, MAIN, eig_s_edge=es.to(dev), eig_d_edge=ed.to(dev))
        compare(w, ref, g.slot_deg, f"{gname} slot mode [{route}]")


def test_destination_range_shard(monkeypatch):
    """Rows [70, 150) of ``mixed`` as a shard (``dist.shard_rows``: global source ids, ``row_base = 70``) with the whole ``eig``: the
    reference's slots of those rows, and the reference computed for the shard itself with ``row_base=70``."""
    import dgn_amd
    from dgn_amd import dist as ddist
    from oracle import dgn_oracle as orc
    dev = _dev()
    g = graph("mixed")
    eig = g.eig(4)
    r0, r1 = 70, 150
    e0, e1 = int(g.indptr[r0]), int(g.indptr[r1])
    ref = orc.edge_weights_ref(g.indptr[r0:r1 + 1] - e0, g.src[e0:e1], eig, MAIN, row_base=r0)
    assert torch.equal(ref, g.ref("K4", eig, MAIN)[:, e0:e1])
    for route in ("defaults", "big0"):
        with monkeypatch.context() as mp:
            _set_route(mp, route)
            shard = ddist.shard_rows(torch.from_numpy(g.indptr).to(dev), torch.from_numpy(g.src).to(dev), r0, r1)
            assert shard.row_base == r0 and shard.num_nodes == r1 - r0 and shard.num_edges == e1 - e0
            w = dgn_amd.compute_edge_weights(shard, MAIN, eig=eig.to(dev))
            torch.cuda.synchronize()
        compare(w, ref, g.slot_deg[e0:e1], f"mixed shard rows [70, 150) [{route}]")


# ---- footprint --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", ["mixed", "hub"])
@pytest.mark.parametrize("route", ["defaults", "big0"])
def test_footprint(gname, route, monkeypatch):
    """``dgn_edge_weights`` of the C ABI into a NaN-filled ``w`` with ``ld_w = E + 37``: every slot of the n_ch = 3 planes is written (no
    row falls between the classes), nothing beyond slot E of a plane and nothing of a fourth plane is (the deltas parked in ``w`` by rows
    of more than 64 slots and by hub slices included)."""
    from dgn_amd import _lib
    from dgn_amd.graph import _channel_array
    dev = _dev()
    g = graph(gname)
    _set_route(monkeypatch, route)
    lib = _lib.load()
    dg = g.device_graph(dev)
    channels = MAIN[:3]
    eig = g.eig(4)
    eig_dev = eig.to(dev)
    E, ld_w = g.E, g.E + 37
    w = torch.full((4, ld_w), float("nan"), dtype=torch.float32, device=dev)
    nbytes = lib.dgn_edge_weights_workspace_bytes(C.byref(dg.c_graph), 3)
    assert (nbytes > 0) == (gname == "hub")
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    rc = lib.dgn_edge_weights(C.byref(dg.c_graph), eig_dev.data_ptr(), None, None, 4, 3, _channel_array(channels), w.data_ptr(), ld_w,
                              ws.data_ptr() if nbytes else None, nbytes, _lib.stream_ptr(dev))
    _lib.check(rc, "dgn_edge_weights")
    torch.cuda.synchronize()
    w = w.cpu()
    assert bool(torch.isfinite(w[:3, :E]).all()), f"{int((~torch.isfinite(w[:3, :E])).sum())} slots never written"
    assert bool(torch.isnan(w[:3, E:]).all()), "a write beyond slot E of a plane"
    assert bool(torch.isnan(w[3]).all()), "a write into the plane after the last channel's"
    compare(w[:3, :E], g.ref("K4", eig, channels), g.slot_deg, f"{gname} footprint [{route}]")
