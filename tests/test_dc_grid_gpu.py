"""The degree-class products (dgn_dc_gemm / dgn_dc_wgrad / dgn_dc_fold: csrc/dgn_dc.hip, csrc/dgn_dc_kernels.hpp) through the C ABI, every
instantiated kernel against plain fp64, on class tables built here with numpy from a degree vector (the contract of include/dgn_hip.h:
stable sort by class, every class padded to 64 rows, classes ascending -- compared once with DGNGraph.degree_classes()):

  small   689 nodes in classes 0..6, class 3 absent, 5 nodes of class 0, one class of exactly 64 rows, one that ends in a 1-row unit
          (15 units: dc_gemm_small for tiles of up to 96 columns, dc_gemm<7> / <8> with one unit per workgroup; four strips per
          weight-gradient workgroup);
  long    13 * 2 * CUs + 5 units (6 661 units, 426 304 virtual rows on 256 CUs).  The host gives dc_gemm at most 2 * CUs row ranges (fewer
          with column tiles or towers) and dc_wgrad at most CUs, so every dc_gemm range holds at least 13 units -- three tiles of four
          units and a remainder -- and every dc_wgrad range at least 26 units = 104 strips.  Class 0 has 5 nodes (one unit, 59 padding
          rows), class 1 100 (two units), class 2 150 (three units), class 3 none; the bulk is classes 5, 9, 17 and 31 with sizes that
          are no multiples of 64 (the last unit of class 31 holds one row).  The first range therefore walks tiles of 1, 2, 3 and 4
          units; most ranges lie inside one class, a few hold a class change;
  towers  CUs + 45 units, for towers = 5: units * towers > 4 * CUs, so dc_gemm<NQ> runs (three units per range) with blockIdx.z > 0.

Traps: c is NaN-filled, 16 rows longer than N, ldc = n + 3 (all of it outside [N, n] must stay NaN); a lies in one buffer of row stride
K_MAX + 3; w has ldw = k + 4 and class_stride > n * ldw, the padding and every absent class's matrix NaN; g_wf is NaN-filled with ldw =
k + 4, ldg / ldx are padded, the weight gradient's workspace arrives filled with 0xFF bytes (dc_wgrad_finalize indexes `part` by x + c,
x < slots, c < 32, and `part` has slots + 32 blocks per slice: a stale mask reads NaN inside the buffer).

Bound: max|ours - r64| <= 1e-5 max|r64| (tests/test_dc_hip.py).  On the long table torch's own fp32 product of
the same operands is measured against fp64 as well; the largest ratio of our error to its error is printed per kernel family.

The instance proof (last test of the file) launches every cell once under torch.profiler and compares the kernel names and their counts
with literals worked out by hand from the host's plan arithmetic (gemm_stats / wgrad_plan in csrc/dgn_dc.hip)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
TOL = 1e-5
K_GEMM = (4, 5, 16, 33, 48, 70)                 # KB = 1, 1, 1, 3, 3, 5: a ragged last chunk (5, 33, 70), rows at 4-byte alignment
K_MAX = max(K_GEMM)
# n -> the tile width NQ the host picks (one tile), then the cells of several column tiles: (NQ, tiles)
N_ONE = (4, 16, 17, 32, 33, 45, 49, 64, 65, 75, 81, 96, 97, 112, 113, 128)            # NQ 1, 1, 2, 2, ... 8, 8
N_TILED = (250, 141, 230, 184, 270, 210, 420)                                        # (4, 4) (5, 2) (5, 3) (6, 2) (6, 3) (7, 2) (7, 4)
N_GEMM = N_ONE + N_TILED
GEMM_CELLS = [(n, k) for n in N_GEMM for k in K_GEMM]
TOWER_CELLS = [(32, 33), (75, 70), (112, 48)]                                        # NQ 2, 5, 7
TOWERS = 5

# weight gradient: n = 16 NTN - 3; k per KT from wgrad_plan's ranges (<= 128, .. 256, .. 384, .. 512), every k ragged (k % 4 != 0 in three of four)
K_OF_KT = {1: 70, 2: 201, 3: 302, 4: 500}
KT_MAX = {1: 4, 2: 4, 3: 4, 4: 4, 5: 4, 6: 3, 7: 2, 8: 2}
WGRAD_CELLS = [(ntn, K_OF_KT[kt]) for ntn in range(1, 9) for kt in range(1, KT_MAX[ntn] + 1)]
WGRAD_CELLS += [(3, 600), (5, 600), (8, 600)]        # two k slices of KT 3 (NTN 3, 5); three of KT 2, the last 88 columns wide (NTN 8)
WGRAD_CELLS += [(2, 420), (5, 420), (6, 420), (8, 420)]      # 27 k tiles: KT 4 with five waves on KTW 3 (NTN 2, 5); two slices of KT 2, the second
#                                                              with 11 tiles: five waves on KTW 1 (NTN 6, 8)
WGRAD_S = {cell: 1 + i % 3 for i, cell in enumerate(WGRAD_CELLS)}

# ---- the instance proof's literals: launches per kernel when every cell above runs once on every table -------------------------------
# gemm: 6 k values per n.  small table: NQ <= 6 on dc_gemm_small, NQ 7 / 8 on dc_gemm; long table: all on dc_gemm; towers: + 1 for NQ 2, 5, 7
EXPECT_GEMM_SMALL = {1: 12, 2: 12, 3: 12, 4: 18, 5: 24, 6: 24}
EXPECT_GEMM = {1: 12, 2: 13, 3: 12, 4: 18, 5: 25, 6: 24, 7: 49, 8: 24}
# weight gradient: every (NTN, KT) once per table, + k = 600 at (3, 3), (5, 3), (8, 2), + k = 420 at (2, 4), (5, 4), (6, 2), (8, 2)
EXPECT_WGRAD = {(ntn, kt): 2 for ntn in range(1, 9) for kt in range(1, KT_MAX[ntn] + 1)}
EXPECT_WGRAD.update({(3, 3): 4, (5, 3): 4, (8, 2): 6, (2, 4): 4, (5, 4): 4, (6, 2): 4})
EXPECT_FINALIZE = {1: 24, 2: 22, 3: 22}             # 34 cells, S = 1 + index % 3, two tables


def class_tables(deg):
    """vperm [64 n_units], unit_class [n_units], present [32] of a degree vector (include/dgn_hip.h: DgnDegreeClasses)."""
    deg = np.asarray(deg, dtype=np.int64)
    assert deg.min() >= 0 and deg.max() < 32
    present = np.bincount(deg, minlength=32)
    units = (present + 63) // 64
    first_row = 64 * (np.cumsum(units) - units)                        # virtual row at which a class begins
    vperm = np.full(64 * int(units.sum()), -1, dtype=np.int32)
    order = np.argsort(deg, kind="stable")                             # ascending node id inside a class
    at = 0
    for c in range(32):
        vperm[first_row[c]: first_row[c] + present[c]] = order[at: at + present[c]]
        at += present[c]
    unit_class = np.repeat(np.arange(32, dtype=np.int32), units)
    return vperm, unit_class, present.astype(np.int32)


class Table:
    def __init__(self, sizes, seed):
        deg = np.concatenate([np.full(cnt, c, dtype=np.int64) for c, cnt in sorted(sizes.items())])
        self.deg_np = deg[np.random.default_rng(seed).permutation(deg.size)]
        self.N = int(deg.size)
        vperm, uc, present = class_tables(self.deg_np)
        self.n_units = int(uc.size)
        self.np_tables = (vperm, uc, present)
        self.vperm, self.unit_class, self.present = (torch.from_numpy(t).cuda() for t in (vperm, uc, present))
        self.deg = torch.from_numpy(self.deg_np).cuda()
        self.classes = [c for c in range(32) if present[c]]
        self.rows = {c: torch.nonzero(self.deg == c).flatten() for c in self.classes}

    def struct(self, scale):
        from dgn_amd import _lib
        return _lib.DgnDegreeClasses(n_units=self.n_units, vperm=self.vperm.data_ptr(), unit_class=self.unit_class.data_ptr(),
                                     present=self.present.data_ptr(), scale=scale.data_ptr())


SMALL_SIZES = {0: 5, 1: 97, 2: 130, 4: 200, 5: 64, 6: 193}               # 1 + 2 + 3 + 4 + 1 + 4 = 15 units


def long_sizes(cus):
    bulk = 13 * 2 * cus + 5 - 6                                          # units of the four large classes
    u5, u9, u17 = bulk * 3 // 10, bulk // 4, bulk // 4
    u31 = bulk - u5 - u9 - u17
    return {0: 5, 1: 100, 2: 150, 5: 64 * u5 - 37, 9: 64 * u9 - 1, 17: 64 * u17 - 50, 31: 64 * u31 - 63}


def tower_sizes(cus):
    bulk = cus + 45 - 6
    u4, u7 = bulk // 3, bulk // 3
    return {0: 5, 1: 100, 2: 150, 4: 64 * u4 - 3, 7: 64 * u7 - 20, 31: 64 * (bulk - u4 - u7) - 63}


class Ctx:
    def __init__(self):
        from dgn_amd import _lib
        self._lib = _lib
        self.lib = _lib.load()
        self.dev = torch.device("cuda")
        self.cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.tab = {"small": Table(SMALL_SIZES, 1), "long": Table(long_sizes(self.cus), 2), "towers": Table(tower_sizes(self.cus), 3)}
        assert self.tab["long"].n_units == 13 * 2 * self.cus + 5 and self.tab["small"].n_units == 15
        assert self.tab["towers"].n_units * TOWERS > 4 * self.cus >= self.tab["small"].n_units
        n_long = self.tab["long"].N
        gen = torch.Generator(device=self.dev).manual_seed(99)
        self.p0 = torch.randn(n_long * 603, device=self.dev, generator=gen) * 1.5 + 0.3        # a / x rows (row strides up to 600 + 3)
        self.p1 = torch.randn(n_long * 131, device=self.dev, generator=gen)                    # g rows (row strides up to 125 + 3 .. 131)
        self.rs = torch.rand(n_long, device=self.dev, generator=gen) + 0.5
        self.ones = torch.ones(32, 1, device=self.dev)
        self.ratios = {}

    def st(self):
        return self._lib.stream_ptr(self.dev)

    def ratio(self, family, ours, theirs):
        if theirs > 0:
            self.ratios[family] = max(self.ratios.get(family, 0.0), ours / theirs)


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    print("\nlong table, largest error relative to torch's fp32 product against fp64, per kernel family:", {k: round(v, 3) for k, v in c.ratios.items()})


def P(t):
    return None if t is None else t.data_ptr()


def bits(t):
    return t.view(torch.int32)


def rel_err(a, r):
    return float((a.double() - r).abs().max()) / (float(r.abs().max()) + 1e-30)


def test_the_tables_equal_degree_classes_of_a_graph_with_these_in_degrees(ctx):
    import dgn_amd
    t = ctx.tab["small"]
    deg = torch.from_numpy(t.deg_np)
    dst = torch.repeat_interleave(torch.arange(t.N), deg)
    src = torch.randint(0, t.N, (dst.numel(),), generator=torch.Generator().manual_seed(0))
    dc = dgn_amd.DGNGraph(src.cuda(), dst.cuda(), t.N).degree_classes()
    vperm, uc, present = t.np_tables
    assert dc["n_units"] == t.n_units
    assert np.array_equal(dc["vperm"].cpu().numpy(), vperm)
    assert np.array_equal(dc["unit_class"].cpu().numpy(), uc)
    assert np.array_equal(dc["present"].cpu().numpy(), present)


def test_the_tables_have_the_stated_shape(ctx):
    for name, t in ctx.tab.items():
        vperm, uc, present = t.np_tables
        live = vperm[vperm >= 0]
        assert np.array_equal(np.sort(live), np.arange(t.N)), name                 # every node once
        assert np.array_equal(t.deg_np[vperm.reshape(-1, 64).max(1)], uc), name    # a unit holds its class (and is never empty)
        assert bool((uc[1:] >= uc[:-1]).all()) and present[3] == 0 and present[0] == 5
    uc = ctx.tab["long"].np_tables[1]
    assert [int((uc == c).sum()) for c in (0, 1, 2, 3)] == [1, 2, 3, 0] and uc[-1] == 31
    # dc_gemm's ranges (one column tile, one tower): at least three 4-unit tiles and a remainder each; some with a class change, some without
    upb = -(-uc.size // (2 * ctx.cus))
    assert upb >= 13 and upb % 4 != 0
    changes = [len(set(uc[i: i + upb])) for i in range(0, uc.size, upb)]
    assert max(changes) > 1 and min(changes) == 1
    assert -(-uc.size // ctx.cus) * 4 >= 12                                       # dc_wgrad: strips per range


# ---- A. dgn_dc_gemm -------------------------------------------------------------------------------------------------------------------

class GemmCall:
    """The operands of one dgn_dc_gemm cell: everything padded and poisoned as the module's docstring says."""

    def __init__(self, ctx, tab, n, k, T, bias, rs, poison=True):
        self.ctx, self.tab, self.n, self.k, self.T = ctx, tab, n, k, T
        N = tab.N
        dev = ctx.dev
        gen = torch.Generator(device=dev).manual_seed(1000 * n + k)
        self.lda, self.a_tower = K_MAX + 3, N * (K_MAX + 3) + (11 if T > 1 else 0)
        self.a_flat = ctx.p0[: T * self.a_tower]
        self.ldw = k + 4
        self.w_tower = n * self.ldw + 5
        self.class_stride = T * self.w_tower + 2
        self.w_flat = torch.full((32 * self.class_stride,), NAN, device=dev)
        vals = torch.randn(len(tab.classes), T, n, k, device=dev, generator=gen) / k ** 0.5
        for i, c in enumerate(tab.classes):
            for t in range(T):
                self.w(c, t).copy_(vals[i, t])
        self.bias = torch.randn(T, n, device=dev, generator=gen) if bias else None
        self.rs = ctx.rs[:N] if rs else None
        self.ldc = n + 3
        self.c_tower = (N + 16) * self.ldc + (9 if T > 1 else 0)
        self.c_elems = T * self.c_tower
        self.poison = poison
        self.s = tab.struct(ctx.ones)

    def a(self, t):
        return self.a_flat[t * self.a_tower: t * self.a_tower + self.tab.N * self.lda].view(self.tab.N, self.lda)[:, :self.k]

    def w(self, c, t):
        o = c * self.class_stride + t * self.w_tower
        return self.w_flat[o: o + self.n * self.ldw].view(self.n, self.ldw)[:, :self.k]

    def c_of(self, buf, t):
        return buf[t * self.c_tower: t * self.c_tower + (self.tab.N + 16) * self.ldc].view(self.tab.N + 16, self.ldc)[:self.tab.N, :self.n]

    def launch(self, stream_out):
        ctx = self.ctx
        buf = torch.full((self.c_elems,), NAN, device=ctx.dev) if self.poison else torch.empty(self.c_elems, device=ctx.dev)
        ctx._lib.check(ctx.lib.dgn_dc_gemm(C.byref(self.s), self.k, self.n, self.T, self.a_flat.data_ptr(), self.lda, self.a_tower, self.w_flat.data_ptr(),
                                           self.ldw, self.class_stride, self.w_tower, P(self.bias), P(self.rs), buf.data_ptr(), self.ldc, self.c_tower,
                                           stream_out, ctx.st()), "dgn_dc_gemm")
        return buf

    def reference(self, dtype):
        N, tab = self.tab.N, self.tab
        out = []
        for t in range(self.T):
            r = torch.zeros(N, self.n, dtype=dtype, device=self.ctx.dev)
            a = self.a(t)
            for c in tab.classes:
                r[tab.rows[c]] = a[tab.rows[c]].to(dtype) @ self.w(c, t).to(dtype).t()
            if self.bias is not None:
                r = r + self.bias[t].to(dtype)
            if self.rs is not None:
                r = r * self.rs.to(dtype).unsqueeze(1)
            out.append(r)
        return out


def gemm_flags(i_n, i_k):
    """bias, row_scale and the first call's stream_out, spread over the cells (each (NQ, k) sees bias on and off over its two widths)"""
    return (i_n + i_k) % 2 == 0, (i_n // 2 + i_k) % 2 == 0, (i_n + i_k // 2) % 2


def check_gemm(ctx, call, stream_out, family=None):
    N, n, T = call.tab.N, call.n, call.T
    first = call.launch(stream_out)
    for so in (1 - stream_out, stream_out):                                    # the other store flavour, then a repeat: same bits
        assert torch.equal(bits(first), bits(call.launch(so))), f"stream_out {so} differs from the first call ({stream_out})"
    assert int(torch.isnan(first).sum()) == first.numel() - T * N * n          # (with the next line: exactly the [N, n] blocks were written)
    r64 = call.reference(torch.float64)
    r32 = call.reference(torch.float32) if family else None
    for t in range(T):
        ours = call.c_of(first, t)
        assert not bool(torch.isnan(ours).any())
        err = rel_err(ours, r64[t])
        if family:
            theirs = rel_err(r32[t], r64[t])
            print(f"{family} n={n} k={call.k} tower {t}: err {err:.3e}, torch fp32 {theirs:.3e}")
            ctx.ratio(family, err, theirs)
        assert err <= TOL, (t, err)


@pytest.mark.parametrize("table", ["small", "long"])
@pytest.mark.parametrize("n,k", GEMM_CELLS)
def test_dc_gemm_vs_fp64(ctx, table, n, k):
    bias, rs, so = gemm_flags(N_GEMM.index(n), K_GEMM.index(k))
    check_gemm(ctx, GemmCall(ctx, ctx.tab[table], n, k, 1, bias, rs), so, "dc_gemm" if table == "long" else None)


@pytest.mark.parametrize("n,k", TOWER_CELLS)
def test_dc_gemm_towers_vs_fp64(ctx, n, k):
    """towers = 5 with distinct a_tower / w_tower / c_tower and a bias per tower, on dc_gemm<NQ> (units * towers > 4 CUs)"""
    check_gemm(ctx, GemmCall(ctx, ctx.tab["towers"], n, k, TOWERS, True, True), 0, "dc_gemm towers")


# ---- B. dgn_dc_wgrad ------------------------------------------------------------------------------------------------------------------

class WgradCall:
    def __init__(self, ctx, tab, n, k, S, layout=None):
        self.ctx, self.tab, self.n, self.k, self.S, self.layout = ctx, tab, n, k, S, layout
        N, dev = tab.N, ctx.dev
        gen = torch.Generator(device=dev).manual_seed(77 * n + k)
        self.ldg, self.ldx = n + 3, k + 3
        self.g = ctx.p1[: N * self.ldg].view(N, self.ldg)[:, :n]
        self.x = ctx.p0[: N * self.ldx].view(N, self.ldx)[:, :k]
        self.scale = torch.rand(32, S, device=dev, generator=gen) + 0.5
        self.s = tab.struct(self.scale)
        self.nbytes = ctx.lib.dgn_dc_wgrad_workspace_bytes(tab.n_units, k, n)
        self.ldw = k + 4

    def launch(self, poison=True):
        ctx, lay = self.ctx, self.layout
        ws = torch.full((self.nbytes,), 0xFF, dtype=torch.uint8, device=ctx.dev) if poison else torch.empty(self.nbytes, dtype=torch.uint8, device=ctx.dev)
        shape = (self.n, lay.ld) if lay is not None else (self.S * self.n, self.ldw)
        out = torch.full(shape, NAN, device=ctx.dev)
        ctx._lib.check(ctx.lib.dgn_dc_wgrad(C.byref(self.s), self.S, self.k, self.n, self.g.data_ptr(), self.ldg, self.x.data_ptr(), self.ldx, out.data_ptr(),
                                            self.ldw, C.byref(lay) if lay is not None else None, ws.data_ptr(), self.nbytes, ctx.st()), "dgn_dc_wgrad")
        return out

    def reference(self, dtype):
        sc = self.scale.to(dtype)[self.tab.deg]                                  # [N, S]
        x = self.x.to(dtype)
        return torch.cat([(self.g.to(dtype) * sc[:, j:j + 1]).t() @ x for j in range(self.S)], 0)


@pytest.mark.parametrize("table", ["small", "long"])
@pytest.mark.parametrize("ntn,k", WGRAD_CELLS)
def test_dc_wgrad_vs_fp64_and_reproducible(ctx, table, ntn, k):
    call = WgradCall(ctx, ctx.tab[table], 16 * ntn - 3, k, WGRAD_S[(ntn, k)])
    a, b = call.launch(), call.launch()
    assert torch.equal(bits(a), bits(b))
    assert bool(torch.isnan(a[:, k:]).all()) and not bool(torch.isnan(a[:, :k]).any())
    r64 = call.reference(torch.float64)
    err = rel_err(a[:, :k], r64)
    if table == "long":
        theirs = rel_err(call.reference(torch.float32), r64)
        print(f"dc_wgrad n={call.n} k={k} S={call.S}: err {err:.3e}, torch fp32 {theirs:.3e}")
        ctx.ratio("dc_wgrad", err, theirs)
    assert err <= TOL, err


# ---- C. the reference's weight layout (DgnDcLayout) and dgn_dc_fold -------------------------------------------------------------------

def layout_map(S, n_agg, f_pad, f_in, h_off, id_slot):
    """The header's statement of DgnDcLayout: for every (s, kk) of the folded matrix the column of W it stands for, or -1 (zero)."""
    k = (n_agg + (1 if h_off else 0)) * f_pad
    col = np.full((S, k), -1, dtype=np.int64)
    for s in range(S):
        for a in range(n_agg + (1 if h_off else 0)):
            for f in range(f_in):                                               # (padded columns f >= f_in: zero)
                if a < n_agg:
                    col[s, a * f_pad + f] = h_off + (s * n_agg + a) * f_in + f
                elif s == id_slot:                                              # the complex layer's h block, through the identity scaler
                    col[s, a * f_pad + f] = f
    return col


LAYOUTS = [("simple", 3, 6, 6, 0, 0), ("complex", 3, 6, 5, 5, 0), ("complex", 3, 6, 5, 5, 2), ("simple-odd", 4, 8, 7, 0, 0)]
#           name, n_agg, f_pad, f_in, h_off, id_slot


def make_layout(ctx, S, n_agg, f_pad, f_in, h_off, id_slot):
    cols = h_off + S * n_agg * f_in                                             # the nn.Linear's input width
    lay = ctx._lib.DgnDcLayout(n_agg=n_agg, f_pad=f_pad, f_in=f_in, h_off=h_off, id_slot=id_slot, ld=cols + 3)
    return lay, cols, layout_map(S, n_agg, f_pad, f_in, h_off, id_slot)


@pytest.mark.parametrize("name,n_agg,f_pad,f_in,h_off,id_slot", LAYOUTS)
def test_dc_fold_with_the_reference_layout(ctx, name, n_agg, f_pad, f_in, h_off, id_slot):
    S, n = 3, 20
    tab = ctx.tab["small"]
    lay, cols, col = make_layout(ctx, S, n_agg, f_pad, f_in, h_off, id_slot)
    k = col.shape[1]
    gen = torch.Generator(device=ctx.dev).manual_seed(5)
    W = torch.full((n, lay.ld), NAN, device=ctx.dev)
    W[:, :cols] = torch.randn(n, cols, device=ctx.dev, generator=gen)
    scale = torch.rand(32, S, device=ctx.dev, generator=gen) + 0.5
    s = tab.struct(scale)
    wc = torch.full((32, n, k), NAN, device=ctx.dev)
    wct = torch.full((32, k, n), NAN, device=ctx.dev)
    ctx._lib.check(ctx.lib.dgn_dc_fold(C.byref(s), S, n, k, 1, W.data_ptr(), C.byref(lay), wc.data_ptr(), wct.data_ptr(), ctx.st()), "dgn_dc_fold")
    Wn, sc = W.double().cpu().numpy(), scale.double().cpu().numpy()
    wf = np.where(col[:, None, :] >= 0, Wn[:, np.maximum(col, 0)].transpose(1, 0, 2), 0.0)       # [S, n, k]
    ref = torch.from_numpy(np.einsum("cs,sok->cok", sc, wf)).to(ctx.dev)
    present = tab.present.bool()
    assert rel_err(wc[present], ref[present]) <= 1e-6
    assert torch.equal(wct[present], wc[present].transpose(1, 2))
    assert bool(torch.isnan(wc[~present]).all()) and bool(torch.isnan(wct[~present]).all())


@pytest.mark.parametrize("name,n_agg,f_pad,f_in,h_off,id_slot", LAYOUTS)
def test_dc_wgrad_into_the_reference_layout(ctx, name, n_agg, f_pad, f_in, h_off, id_slot):
    S, n = 3, 20
    tab = ctx.tab["small"]
    lay, cols, col = make_layout(ctx, S, n_agg, f_pad, f_in, h_off, id_slot)
    k = col.shape[1]
    call = WgradCall(ctx, tab, n, k, S, layout=lay)
    a, b = call.launch(), call.launch()
    assert torch.equal(bits(a), bits(b))
    folded = call.reference(torch.float64).view(S, n, k).cpu().numpy()
    ref = np.full((n, cols), np.nan)
    for s_ in range(S):
        for kk in range(k):
            if col[s_, kk] >= 0:
                assert np.isnan(ref[0, col[s_, kk]])                            # (the map addresses an element once)
                ref[:, col[s_, kk]] = folded[s_, :, kk]
    assert not np.isnan(ref).any()                                              # the layout addresses every column of the nn.Linear
    assert not bool(torch.isnan(a[:, :cols]).any()), "an element the layout addresses was not written"
    assert bool(torch.isnan(a[:, cols:]).all())
    assert rel_err(a[:, :cols], torch.from_numpy(ref).to(ctx.dev)) <= TOL


def test_dc_fold_towers(ctx):
    S, n, k, T = 3, 21, 37, 3
    tab = ctx.tab["small"]
    gen = torch.Generator(device=ctx.dev).manual_seed(6)
    wf = torch.randn(T, S * n, k, device=ctx.dev, generator=gen)
    scale = torch.rand(32, S, device=ctx.dev, generator=gen) + 0.5
    s = tab.struct(scale)
    wc = torch.full((32, T, n, k), NAN, device=ctx.dev)
    wct = torch.full((32, T, k, n), NAN, device=ctx.dev)
    ctx._lib.check(ctx.lib.dgn_dc_fold(C.byref(s), S, n, k, T, wf.data_ptr(), None, wc.data_ptr(), wct.data_ptr(), ctx.st()), "dgn_dc_fold")
    present = tab.present.bool()
    for t in range(T):
        ref = torch.einsum("cs,sok->cok", scale.double(), wf[t].double().view(S, n, k))
        assert rel_err(wc[present, t], ref[present]) <= 1e-6
    assert torch.equal(wct[present], wc[present].transpose(2, 3))
    assert bool(torch.isnan(wc[~present]).all()) and bool(torch.isnan(wct[~present]).all())      # absent classes are not touched


# ---- E. edges and refusals ------------------------------------------------------------------------------------------------------------

def test_no_units(ctx):
    lib, _lib = ctx.lib, ctx._lib
    empty = _lib.DgnDegreeClasses(n_units=0, vperm=None, unit_class=None, present=None, scale=None)
    c = torch.full((8, 16), NAN, device=ctx.dev)
    assert lib.dgn_dc_gemm(C.byref(empty), 16, 16, 1, None, 16, 0, None, 16, 256, 0, None, None, c.data_ptr(), 16, 0, 0, ctx.st()) == _lib.DGN_OK
    assert bool(torch.isnan(c).all())
    S, n, k = 2, 20, 18
    out = torch.full((S * n, k + 4), NAN, device=ctx.dev)
    assert lib.dgn_dc_wgrad(C.byref(empty), S, k, n, None, n, None, k, out.data_ptr(), k + 4, None, None, 0, ctx.st()) == _lib.DGN_OK
    assert float(out[:, :k].abs().max()) == 0.0
    lay, cols, _ = make_layout(ctx, S, 3, 6, 6, 0, 0)
    out = torch.full((n, lay.ld), NAN, device=ctx.dev)
    assert lib.dgn_dc_wgrad(C.byref(empty), S, k, n, None, n, None, k, out.data_ptr(), 0, C.byref(lay), None, 0, ctx.st()) == _lib.DGN_OK
    assert float(out[:, :cols].abs().max()) == 0.0


def test_refusals(ctx):
    lib, _lib, tab = ctx.lib, ctx._lib, ctx.tab["small"]
    INVALID, WORKSPACE = _lib.DGN_ERR_INVALID, _lib.DGN_ERR_WORKSPACE
    N, dev = tab.N, ctx.dev
    s = tab.struct(torch.ones(32, 4, device=dev))
    a = torch.zeros(N, 160, device=dev)                 # (every buffer is large enough for the call it would be, were it accepted)
    w = torch.zeros(32 * 65 * 160 * 2, device=dev)
    c = torch.full((65, N, 160), NAN, device=dev)
    ws = torch.zeros(1 << 24, dtype=torch.uint8, device=dev)
    out = torch.full((4 * 160, 160), NAN, device=dev)

    def gemm(k, n, towers=1, lda=160):
        return lib.dgn_dc_gemm(C.byref(s), k, n, towers, a.data_ptr(), lda, 0, w.data_ptr(), k, n * k * towers, n * k, None, None, c.data_ptr(), 160, N * 160, 0, ctx.st())

    def wgrad(k, n, S=1, ws_bytes=None):
        need = ws.numel() if ws_bytes is None else ws_bytes
        return lib.dgn_dc_wgrad(C.byref(s), S, k, n, a.data_ptr(), 160, a.data_ptr(), 160, out.data_ptr(), 160, None, ws.data_ptr(), need, ctx.st())

    def fold(S, towers, layout=None):
        return lib.dgn_dc_fold(C.byref(s), S, 20, 18, towers, w.data_ptr(), layout, w.data_ptr(), w.data_ptr(), ctx.st())

    assert gemm(3, 16) == INVALID and gemm(16, 3) == INVALID
    assert wgrad(3, 16) == INVALID and wgrad(16, 3) == INVALID
    assert wgrad(16, 129) == INVALID
    assert wgrad(16, 16, S=4) == INVALID and fold(4, 1) == INVALID
    assert gemm(16, 16, towers=65) == INVALID and fold(3, 65) == INVALID
    lay, _, _ = make_layout(ctx, 3, 3, 6, 6, 0, 0)
    assert fold(3, 2, C.byref(lay)) == INVALID
    assert gemm(16, 16, lda=15) == INVALID
    need = lib.dgn_dc_wgrad_workspace_bytes(tab.n_units, 16, 16)
    assert 0 < need <= ws.numel() and wgrad(16, 16, ws_bytes=need - 1) == WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(c).all()) and bool(torch.isnan(out).all())          # nothing was launched
    assert wgrad(16, 16, ws_bytes=need) == _lib.DGN_OK                          # (and the exact size is accepted)


# ---- the instance proof ---------------------------------------------------------------------------------------------------------------

def _launches(step):
    """Name of every device kernel launch of ``step`` (torch.profiler, device activities: tests/test_bench_sizes_gpu.py _device_kernels)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return [e.name() for e in prof.profiler.kineto_results.events() if str(e.device_type()).endswith("CUDA")]


def test_every_instance_ran(ctx):
    def every_cell_once():
        for table in ("small", "long"):
            for n, k in GEMM_CELLS:
                GemmCall(ctx, ctx.tab[table], n, k, 1, False, False, poison=False).launch(0)
            for ntn, k in WGRAD_CELLS:
                WgradCall(ctx, ctx.tab[table], 16 * ntn - 3, k, WGRAD_S[(ntn, k)]).launch(poison=False)
        for n, k in TOWER_CELLS:
            GemmCall(ctx, ctx.tab["towers"], n, k, TOWERS, False, False, poison=False).launch(0)

    names = [n for n in _launches(every_cell_once) if "dgn::dc::" in n]
    assert names, "torch.profiler saw no device kernel of the degree-class family"
    got = {"small": {}, "gemm": {}, "wgrad": {}, "finalize": {}}
    patterns = [("small", r"dc_gemm_small<(\d+)>"), ("gemm", r"dc_gemm<(\d+)>"), ("finalize", r"dc_wgrad_finalize<(\d+)>"), ("wgrad", r"dc_wgrad<(\d+),\s*(\d+)>")]
    for name in names:
        for what, pat in patterns:
            m = re.search(pat, name)
            if m:
                key = tuple(int(v) for v in m.groups())
                key = key[0] if len(key) == 1 else key
                got[what][key] = got[what].get(key, 0) + 1
                break
        else:
            raise AssertionError("a kernel of the family this file does not know: " + name)
    assert got["small"] == EXPECT_GEMM_SMALL
    assert got["gemm"] == EXPECT_GEMM
    assert len(EXPECT_WGRAD) == 27 and got["wgrad"] == EXPECT_WGRAD
    assert got["finalize"] == EXPECT_FINALIZE
