"""The wide GEMM family (dgn_gemm_forward / dgn_gemm_wgrad: csrc/dgn_gemm.hip, csrc/dgn_gemm_kernels.hpp) through the C ABI, every
instantiated kernel against plain fp64 on the device, in steady state.  These entry points carry the simple / complex layers' posttrans
product whenever the degree-class route is not taken (the library's default below 16 384 nodes); tests/conftest.py lowers that threshold,
so the layer tests of the suite run dc_gemm and this family is left with its direct tests.

Row counts, from the device's CU count and never from the plan under test (a count derived from the plan would shrink with a bug in it):

  M_SMALL = 37                          two full 16-row strips and one of five rows; one row block, one 64-row tile.  ts_gemm's column
                                        split narrows every width to NT = 1 here (the single-block cell);
  M_TS    = 128 * 3 * (2 CUs + 1) + 5   (196 997 rows on 256 CUs) ts_gemm launches at most 2 CUs / gy + 1 workgroups of 128 rows per pass, so
                                        every workgroup of any column split owns at least three row blocks (the grid-stride loop's second
                                        and later iterations: the barrier in front of the next block's first commit, the accumulators
                                        re-initialised from the bias) and the batch ends in a block of five rows; no column split happens
                                        (more row blocks than CUs), so the width alone picks NT.  The weight gradients have at most CUs
                                        slots: dozens of strips per workgroup;
  M_TILE  = 256 * 3 * 2 CUs + 5         (393 221 rows) tile_gemm sizes its grid for two resident workgroups per CU: every workgroup walks
                                        at least three tiles (832 rows: heights 4, 3, 3, 3), a ragged last one apart;
  M_T320  = 320 * 2 CUs - 315           ranges of 320 rows: heights 3 then 2, and a last range of five rows (height 1);
  M_T448  = 448 * 2 CUs - 443           ranges of 448 rows: heights 4 then 3, and a last range of five rows.

tile_pass<NQ, RT> and tw_run<NTc, KTc> do not appear in kernel names: the walk of tile_gemm and the deal of tile_wgrad are restated here
in Python, and test_the_row_counts_and_shapes_reach_what_they_are_for asserts that the cells reach all 16 (NQ, RT) pairs (with a walk of
three or more tiles per NQ) and all nine tw_run variants, for the CU count of the device the suite runs on.

Traps, in every cell: A / X is a view at column offset 1 of a buffer of row stride k + 3 (rows at 4-byte alignment) whose other columns
are NaN; W lies in a NaN-filled buffer of row stride cols + 2; C is NaN-filled, ldc = n + 2, 16 rows longer than M (all of that must
still be NaN afterwards); the bias is the last n floats of a NaN-padded vector; G has ldg = n + 2 with NaN padding; dw is NaN-filled
with lddw = k + 2; the workspace is exactly dgn_gemm_wgrad_workspace_bytes long, handed over as 0xFF bytes, with a poisoned guard
behind it.  A clamped 16-byte load that leaks a neighbouring column is a NaN, not a tolerance miss.

Tolerances: products 1e-5 max|ref| (tests/test_linear_hip.py _close); weight gradients the rule of tests/test_hip_parity.py _as_good --
within 1e-5 max|ref| of fp64, or no further from it than four times torch's own fp32 product of the same operands; bias gradients
2e-6 max_col(sum |g|) + 1e-6.  Weight gradients are called twice everywhere, products twice at the long row counts: same bits.

The instance proof (last test) launches every cell once under torch.profiler: all 32 ts_gemm<NT, WKN>, four tile_gemm<NQ>, sixteen
ts_gemm_wgrad<KT>, tile_wgrad and both finalize kernels by name, launches per kernel against literals worked out by hand."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

M_SMALL = 37
NAN = float("nan")
K_SMALL = (4, 5, 16, 33, 70)         # KB = 1, 1, 1, 3, 5: one (ragged) chunk, both LDS buffers, a ragged last chunk
K_LONG = (5, 33, 70)
GUARD = 1 << 20                      # poisoned bytes behind the workspace
TILE_MIN_ROWS = 131072               # dgn_gemm_forward: tile_gemm by default from this many rows on, for n >= 64


def cdiv(a, b):
    return -(-a // b)


# ---- the cells --------------------------------------------------------------------------------------------------------------------------
# ts_gemm: (label, n); every NT at its ragged width, three full widths, two outputs of two column slices with a ragged last one
TS_WIDTHS = [(f"nt{t}", 16 * t - 2) for t in range(1, 17)] + [(f"full{t}", 16 * t) for t in (1, 8, 16)] + [("slices11", 330), ("slices16", 500)]
TS_NT_LONG = {**{f"nt{t}": t for t in range(1, 17)}, **{f"full{t}": t for t in (1, 8, 16)}, "slices11": 11, "slices16": 16}     # at M_TS
# tile_gemm: n -> (NQ, column tiles)
TILE_WIDTHS = {62: (4, 1), 78: (5, 1), 94: (6, 1), 110: (7, 1), 210: (7, 2), 225: (5, 3)}
TILE_ROWS = ("small", "t320", "t448", "tile")
# ts_gemm_wgrad: (label, k, dbias, KT); one k slice of KT tiles with and without the ones column, the ones column as the first column of
# a tile of its own (k a multiple of 16), and two k slices with a ragged last one (300: 160 + 140 (+ 1), 420: 224 + 196 (+ 1))
STRIP_CELLS = [(f"kt{t}" + ("-dbias" if db else ""), 16 * t - 2, db, t) for t in range(1, 17) for db in (False, True)]
STRIP_CELLS += [("ones-opens-tile-2", 16, True, 2), ("ones-opens-tile-8", 112, True, 8), ("ones-opens-tile-16", 240, True, 16)]
STRIP_CELLS += [(f"k{k}" + ("-dbias" if db else ""), k, db, kt) for k, kt in ((300, 10), (420, 14)) for db in (False, True)]
STRIP_N = (5, 78, 256)               # one wave with a tile, five waves, all sixteen
# tile_wgrad: (k, n) -> the tw_run variants its deal gives (0, 0: a wave without tiles), with and without the ones column unless stated
TW_SHAPES = {(7, 5): {(1, 1), (0, 0)}, (128, 64): {(1, 1), (1, 2)}, (96, 330): {(2, 1), (3, 1)}, (250, 130): {(2, 2), (3, 2)},
             (100, 200): {(4, 1)}, (255, 250): {(4, 2)}, (256, 256): {(4, 1), (4, 2)}, (880, 1320): None}
TW_SMALL_ONLY = {(880, 1320)}        # 6 x 4 blocks of 7 x 7 tiles
TW_VARIANTS = {(a, b) for a in (1, 2, 3, 4) for b in (1, 2)} | {(0, 0)}


# ---- the host plans and the kernels' walks, restated (csrc/dgn_gemm.hip, csrc/dgn_gemm_kernels.hpp) ---------------------------------------
def ts_plan(M, n, cus):
    """(NT, gy, gx) of the strip product"""
    slices = cdiv(n, 256)
    want = cus // max(1, cdiv(M, 128))
    if want > slices:
        slices = min(want, cdiv(n, 16))
    nt = cdiv(cdiv(n, slices), 16)
    gy = cdiv(n, 16 * nt)
    return nt, gy, max(1, min(cdiv(M, 128), 2 * cus // gy + 1))


def tile_plan(M, n, cus):
    """(NQ, column tiles, rows_per_block) of the tile product"""
    nq, tiles = 7, cdiv(n, 112)
    pad = tiles * 112 - n
    for q in (7, 6, 5, 4):
        t = cdiv(n, 16 * q)
        if t * 16 * q - n < pad:
            nq, tiles, pad = q, t, t * 16 * q - n
    slots_x = max(1, 2 * cus // tiles)
    return nq, tiles, max(64, cdiv(cdiv(M, slots_x), 64) * 64)


def tile_walks(M, rpb):
    """the tile heights (64-row units) every workgroup of tile_gemm walks: a tuple per workgroup, in blockIdx.x order"""
    walks = []
    for r in range(0, M, rpb):
        end, hs = min(M, r + rpb), []
        while r < end:
            left = end - r
            h = min(4, cdiv(cdiv(left, cdiv(left, 256)), 64))
            hs.append(h)
            r += 64 * h
        walks.append(tuple(hs))
    return walks


def strip_plan(kk):
    """(KT, k slices) of the strip weight gradient"""
    kt = cdiv(cdiv(kk, cdiv(kk, 256)), 16)
    return kt, cdiv(kk, 16 * kt)


def tw_deal(kk, n):
    """the (NTc, KTc) of every wave of every block of tile_wgrad; (0, 0) for a wave without tiles"""
    nt, kt = cdiv(n, 32), cdiv(kk, 32)
    n_blocks, k_blocks = cdiv(nt, 8), cdiv(kt, 8)
    nb_tiles, kb_tiles = cdiv(nt, n_blocks), cdiv(kt, k_blocks)
    out = set()
    for bn in range(n_blocks):
        for bk in range(k_blocks):
            nt_blk = cdiv(min(nb_tiles * 32, n - bn * nb_tiles * 32), 32)
            kt_blk = cdiv(min(kb_tiles * 32, kk - bk * kb_tiles * 32), 32)
            for wn in range(2):
                for wk in range(4):
                    nt_w = nt_blk * (wn + 1) // 2 - nt_blk * wn // 2
                    kt_w = kt_blk * (wk + 1) // 4 - kt_blk * wk // 4
                    out.add((nt_w, kt_w) if nt_w > 0 and kt_w > 0 else (0, 0))
    return out, n_blocks * k_blocks


# ---- the module's operands ----------------------------------------------------------------------------------------------------------------
class Ctx:
    """Operand pools drawn once (read-only), the NaN-padded buffers built from them per (rows, width), the library handle."""

    def __init__(self):
        from dgn_amd import _lib
        self._lib = _lib
        self.lib = _lib.load()
        self.dev = torch.device("cuda")
        self.cus = cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.rows = {"small": M_SMALL, "ts": 128 * 3 * (2 * cus + 1) + 5, "tile": 256 * 3 * 2 * cus + 5, "t320": 320 * 2 * cus - 315,
                     "t448": 448 * 2 * cus - 443}
        gen = torch.Generator(device=self.dev).manual_seed(4321)
        self.p0 = torch.randn(max(self.rows["ts"] * 423, self.rows["tile"] * 73), device=self.dev, generator=gen) * 1.5 + 0.3      # a / x
        self.p1 = torch.randn(self.rows["ts"] * 332, device=self.dev, generator=gen)                                              # g
        self.w = torch.randn(512, 512, device=self.dev, generator=gen)
        self.v = torch.randn(512, device=self.dev, generator=gen)
        self._a, self._g = {}, {}
        self.ratios = {}                 # kernel -> largest (our error / the error of torch's fp32 product), both against fp64
        self.cells = {}                  # mode -> cells run

    def st(self):
        return self._lib.stream_ptr(self.dev)

    def a(self, M, k):
        """[M, k] at column offset 1 of a buffer of row stride k + 3, the other three columns NaN"""
        if (M, k) not in self._a:
            buf = self.p0[:M * (k + 3)].view(M, k + 3).clone()
            buf[:, 0] = NAN
            buf[:, k + 1:] = NAN
            self._a[(M, k)] = buf
        return self._a[(M, k)][:, 1:k + 1]

    def g(self, M, n):
        """[M, n] in a buffer of row stride n + 2, the padding NaN"""
        if (M, n) not in self._g:
            buf = self.p1[:M * (n + 2)].view(M, n + 2).clone()
            buf[:, n:] = NAN
            self._g[(M, n)] = buf
        return self._g[(M, n)][:, :n]

    def weight(self, rows, cols, red):
        """[rows, cols] in a NaN-filled buffer of row stride cols + 2, scaled by 1 / sqrt(reduction width)"""
        buf = torch.full((rows, cols + 2), NAN, device=self.dev)
        buf[:, :cols] = self.w[:rows, :cols] / red ** 0.5
        return buf[:, :cols]

    def bias(self, n):
        """the last n floats of a NaN-padded vector (4-byte aligned)"""
        buf = torch.full((n + 3,), NAN, device=self.dev)
        buf[3:] = self.v[:n]
        return buf[3:]

    def ratio(self, kernel, ours, theirs):
        if theirs > 0:
            self.ratios[kernel] = max(self.ratios.get(kernel, 0.0), ours / theirs)

    def count(self, mode, n=1):
        self.cells[mode] = self.cells.get(mode, 0) + n


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    print("\nlargest error relative to torch's fp32 product of the same operands (both against fp64), per kernel:", {k: round(v, 3) for k, v in c.ratios.items()})
    print("cells run per mode:", c.cells)


def P(t):
    return None if t is None else t.data_ptr()


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- A. dgn_gemm_forward ------------------------------------------------------------------------------------------------------------------
def forward(c, M, k, n, kn, a, w, b, poison=True):
    """-> the whole C buffer ([M + 16, n + 2])"""
    cbuf = torch.full((M + 16, n + 2), NAN, device=c.dev) if poison else torch.empty(M + 16, n + 2, device=c.dev)
    c._lib.check(c.lib.dgn_gemm_forward(M, k, n, a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), kn, P(b), cbuf.data_ptr(), n + 2, c.st()), "dgn_gemm_forward")
    return cbuf


def forward_operands(c, M, k, n, kn):
    a = c.a(M, k)
    w = c.weight(k, n, k) if kn else c.weight(n, k, k)
    assert a.stride(0) == k + 3 and a.data_ptr() % 16 == 4 and w.stride(0) == (n if kn else k) + 2
    return a, w, c.bias(n)


def check_forward(c, M, k, n, kn, long, kernel, fails):
    """both bias settings of one (M, k, n, layout) against fp64; at the long row counts twice (same bits) and with torch's fp32 product measured"""
    a, w, b = forward_operands(c, M, k, n, kn)
    w64 = w.double() if kn else w.double().T
    r0 = a.double() @ w64
    lib_err = float(((a @ (w if kn else w.T)).double() - r0).abs().max()) if long else 0.0
    for bias in (None, b):
        label = f"{kernel} M={M} k={k} n={n} w_is_kn={kn} bias={bias is not None}"
        ref = r0 if bias is None else r0 + bias.double()
        cbuf = forward(c, M, k, n, kn, a, w, bias)
        out = cbuf[:M, :n]
        if int(torch.isnan(cbuf).sum()) != cbuf.numel() - M * n or bool(torch.isnan(out).any()):
            fails.append(f"{label}: NaN in the output, or the padding columns / the rows past M were written")
        err, scale = float((out.double() - ref).abs().max()), float(ref.abs().max()) + 1e-30
        if long:
            c.ratio(kernel, err, lib_err)
            if not same_bits(out, forward(c, M, k, n, kn, a, w, bias)[:M, :n]):
                fails.append(f"{label}: a second call returned other bits")
        if not err <= 1e-5 * scale:                   # (a NaN fails every comparison)
            fails.append(f"{label}: error {err:.3e} at max|ref| {scale:.3e}")
        c.count(kernel)


@pytest.mark.parametrize("kn", [0, 1])
@pytest.mark.parametrize("label,n", TS_WIDTHS, ids=[w[0] for w in TS_WIDTHS])
def test_ts_gemm_vs_fp64(ctx, monkeypatch, label, n, kn):
    """ts_gemm<NT, WKN> (option tile_gemm = 0): M_SMALL (NT = 1 by the column split) with k = 4, 5, 16, 33, 70, and M_TS -- where the
    width's own NT runs and every workgroup owns three or more row blocks -- with k = 5, 33, 70; with and without bias"""
    monkeypatch.setattr(ctx._lib.options, "tile_gemm", 0)
    fails = []
    for k in K_SMALL:
        check_forward(ctx, M_SMALL, k, n, kn, False, "ts_gemm", fails)
    for k in K_LONG:
        check_forward(ctx, ctx.rows["ts"], k, n, kn, True, "ts_gemm", fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("rows", TILE_ROWS)
@pytest.mark.parametrize("n", list(TILE_WIDTHS))
def test_tile_gemm_vs_fp64(ctx, monkeypatch, n, rows):
    """tile_gemm<NQ> (option tile_gemm = 1, W as [n, k]): one width per NQ, two and three column tiles with a ragged last one, at the
    row counts whose walks cover every tile height (module docstring); k = 5, 33, 70, with and without bias"""
    monkeypatch.setattr(ctx._lib.options, "tile_gemm", 1)
    fails = []
    for k in K_LONG:
        check_forward(ctx, ctx.rows[rows], k, n, 0, rows != "small", "tile_gemm", fails)
    assert not fails, "\n".join(fails)


# ---- B. dgn_gemm_wgrad --------------------------------------------------------------------------------------------------------------------
def wgrad(c, M, k, n, dbias, g, x, poison=True):
    """-> (dw buffer [n, k + 2], dbias buffer [n + 16] or None); the workspace exactly as long as the query says, a guard behind it"""
    nb = c.lib.dgn_gemm_wgrad_workspace_bytes(M, k, n)
    assert nb > 0
    dw = torch.full((n, k + 2), NAN, device=c.dev)
    db = torch.full((n + 16,), NAN, device=c.dev) if dbias else None
    if poison:
        buf = torch.full((nb + GUARD,), 0xFF, dtype=torch.uint8, device=c.dev)
        buf[nb:] = 0xA5
    else:
        buf = torch.empty(nb, dtype=torch.uint8, device=c.dev)
    c._lib.check(c.lib.dgn_gemm_wgrad(M, k, n, g.data_ptr(), g.stride(0), x.data_ptr(), x.stride(0), dw.data_ptr(), k + 2, P(db), buf.data_ptr(), nb, c.st()),
                 "dgn_gemm_wgrad")
    if poison:
        assert bool((buf[nb:] == 0xA5).all()), f"dgn_gemm_wgrad wrote behind its workspace (M={M} k={k} n={n} dbias={dbias})"
    return dw, db


def check_wgrad(c, M, k, n, dbias, kernel, fails):
    g, x = c.g(M, n), c.a(M, k)
    assert g.stride(0) == n + 2 and x.stride(0) == k + 3
    label = f"{kernel} M={M} k={k} n={n} dbias={dbias}"
    dw, db = wgrad(c, M, k, n, dbias, g, x)
    dw2, db2 = wgrad(c, M, k, n, dbias, g, x)
    g64, x64 = g.double(), x.double()
    ref = g64.T @ x64
    lib_err = float(((g.T @ x).double() - ref).abs().max())
    if not bool(torch.isnan(dw[:, k:]).all()):
        fails.append(f"{label}: the padding columns of dw were written")
    if not same_bits(dw[:, :k], dw2[:, :k]):
        fails.append(f"{label}: a second call returned other bits")
    err, scale = float((dw[:, :k].double() - ref).abs().max()), float(ref.abs().max()) + 1e-30
    c.ratio(kernel, err, lib_err)
    if not (err <= 1e-5 * scale or err <= 4 * lib_err):
        fails.append(f"{label}: dw error {err:.3e} at max|ref| {scale:.3e}, torch's fp32 product {lib_err:.3e}")
    if dbias:
        if not bool(torch.isnan(db[n:]).all()):
            fails.append(f"{label}: dbias was written past its n entries")
        if not same_bits(db[:n], db2[:n]):
            fails.append(f"{label}: a second call returned other dbias bits")
        berr = float((db[:n].double() - g64.sum(0)).abs().max())
        if not berr <= 2e-6 * float(g64.abs().sum(0).max()) + 1e-6:
            fails.append(f"{label}: dbias error {berr:.3e}")
    c.count(kernel)


@pytest.mark.parametrize("label,k,dbias,kt", STRIP_CELLS, ids=[s[0] for s in STRIP_CELLS])
def test_strip_wgrad_vs_fp64_and_reproducible(ctx, monkeypatch, label, k, dbias, kt):
    """ts_gemm_wgrad<KT> (option tile_wgrad = 0): n = 5, 78, 256 at M_SMALL (at most one strip per workgroup) and M_TS (dozens)"""
    assert strip_plan(k + 1 if dbias else k)[0] == kt
    monkeypatch.setattr(ctx._lib.options, "tile_wgrad", 0)
    fails = []
    for M in (M_SMALL, ctx.rows["ts"]):
        for n in STRIP_N:
            check_wgrad(ctx, M, k, n, dbias, "ts_gemm_wgrad", fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("k,n", list(TW_SHAPES))
def test_tile_wgrad_vs_fp64_and_reproducible(ctx, monkeypatch, k, n):
    """tile_wgrad: option tile_wgrad = 1 up to n = 256, the library's default beyond; the shapes whose deal gives every tw_run variant"""
    if n <= 256:
        monkeypatch.setattr(ctx._lib.options, "tile_wgrad", 1)
    else:
        assert ctx._lib.options.tile_wgrad == -1
    fails = []
    for M in (M_SMALL,) if (k, n) in TW_SMALL_ONLY else (M_SMALL, ctx.rows["ts"]):
        for dbias in (False, True):
            check_wgrad(ctx, M, k, n, dbias, "tile_wgrad", fails)
    assert not fails, "\n".join(fails)


# ---- C. what the cells reach ----------------------------------------------------------------------------------------------------------------
def test_the_row_counts_and_shapes_reach_what_they_are_for(ctx):
    """The restated plans on this device's CU count: NT per ts_gemm cell and three row blocks per workgroup at M_TS; all 16 (NQ, RT) pairs of
    tile_pass with a walk of three or more tiles per NQ; KT per strip cell; all nine tw_run variants"""
    cus, M_TS = ctx.cus, ctx.rows["ts"]
    assert M_TS % 128 == 5 and ctx.rows["tile"] % 64 == 5
    for label, n in TS_WIDTHS:
        nt, gy, gx = ts_plan(M_TS, n, cus)
        assert nt == TS_NT_LONG[label] and gy == cdiv(n, 256), (label, nt, gy)
        assert cdiv(M_TS, 128) >= 3 * gx + 1, label                     # every workgroup: three row blocks or more
        assert ts_plan(M_SMALL, n, cus)[0] == 1 or cus < 32, label
    pairs, long_walk = set(), set()
    for n, (nq, tiles) in TILE_WIDTHS.items():
        for rows in TILE_ROWS:
            q, t, rpb = tile_plan(ctx.rows[rows], n, cus)
            assert (q, t) == (nq, tiles), (n, q, t)
            for walk in tile_walks(ctx.rows[rows], rpb):
                pairs |= {(nq, h) for h in walk}
                if len(walk) >= 3:
                    long_walk.add(nq)
            if rows == "tile":
                assert min(len(w) for w in tile_walks(ctx.rows[rows], rpb)[:-1]) >= 3, n      # every workgroup but the ragged last one: three tiles or more
    assert pairs == {(nq, h) for nq in (4, 5, 6, 7) for h in (1, 2, 3, 4)}, sorted(pairs)
    assert long_walk == {4, 5, 6, 7}
    assert set(tile_walks(ctx.rows["t320"], 320)) == {(3, 2), (1,)} and set(tile_walks(ctx.rows["t448"], 448)) == {(4, 3), (1,)}
    assert cdiv(M_TS, 16) >= 3 * cus                                    # weight gradients: at most CUs slots
    for label, k, dbias, kt in STRIP_CELLS:
        got = strip_plan(k + 1 if dbias else k)
        assert got == (kt, 2 if k in (300, 420) else 1), (label, got)
    assert sorted(set(s[3] for s in STRIP_CELLS)) == list(range(1, 17))
    seen = set()
    for (k, n), want in TW_SHAPES.items():
        for dbias in (False, True):
            deal, blocks = tw_deal(k + 1 if dbias else k, n)
            seen |= deal
            if (k, n) == (880, 1320):
                assert blocks == 24
        if want is not None:
            assert want <= tw_deal(k, n)[0] | tw_deal(k + 1, n)[0], ((k, n), want)
    assert seen >= TW_VARIANTS, sorted(TW_VARIANTS - seen)
    assert tw_deal(257, 256)[1] == 2 and tw_deal(256, 256)[1] == 1      # the ones column of (256, 256) makes a second k block


# ---- D. the default dispatch ------------------------------------------------------------------------------------------------------------------
def _launches(step):
    """Name of every device kernel launch of ``step`` (torch.profiler, device activities: tests/test_bench_sizes_gpu.py _device_kernels)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return [e.name() for e in prof.profiler.kineto_results.events() if str(e.device_type()).endswith("CUDA")]


def _gemm_kernels(step):
    return [n for n in _launches(step) if "dgn::gemm::" in n]


@pytest.mark.parametrize("M,n,kn,kernel", [(TILE_MIN_ROWS, 78, 0, "tile_gemm<5>"), (TILE_MIN_ROWS, 64, 0, "tile_gemm<4>"), (TILE_MIN_ROWS, 62, 0, "ts_gemm<4, 0>"),
                                           (TILE_MIN_ROWS, 78, 1, "ts_gemm<5, 1>"), (TILE_MIN_ROWS - 1, 78, 0, "ts_gemm<5, 0>"), (M_SMALL, 78, 0, "ts_gemm<1, 0>")])
def test_default_options_pick_the_kernel_by_shape(ctx, M, n, kn, kernel):
    """option tile_gemm at its default: tile_gemm for n >= 64 on 131 072 rows or more of an [n, k] weight, ts_gemm otherwise"""
    assert ctx._lib.options.tile_gemm == -1
    k = 33
    a, w, b = forward_operands(ctx, M, k, n, kn)
    out = []
    names = _gemm_kernels(lambda: out.append(forward(ctx, M, k, n, kn, a, w, b)))
    assert len(names) == 1 and kernel in re.sub(r",\s*", ", ", names[0]), names
    cbuf = out[0]
    ref = a.double() @ (w.double() if kn else w.double().T) + b.double()
    assert int(torch.isnan(cbuf).sum()) == cbuf.numel() - M * n
    assert float((cbuf[:M, :n].double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


# ---- E. edges and refusals ----------------------------------------------------------------------------------------------------------------
def test_no_rows(ctx):
    lib, OK = ctx.lib, ctx._lib.DGN_OK
    k, n = 18, 21
    c = torch.full((16, n + 2), NAN, device=ctx.dev)
    assert lib.dgn_gemm_forward(0, k, n, None, k, None, k, 0, None, c.data_ptr(), n + 2, ctx.st()) == OK
    dw = torch.full((n + 1, k + 2), NAN, device=ctx.dev)
    db = torch.full((n + 16,), NAN, device=ctx.dev)
    assert lib.dgn_gemm_wgrad(0, k, n, None, n, None, k, dw.data_ptr(), k + 2, db.data_ptr(), None, 0, ctx.st()) == OK
    assert float(dw[:n, :k].abs().max()) == 0.0 and float(db[:n].abs().max()) == 0.0          # exactly the n x k entries and dbias
    assert bool(torch.isnan(dw[:n, k:]).all()) and bool(torch.isnan(dw[n:]).all()) and bool(torch.isnan(db[n:]).all())
    dw.fill_(NAN)
    assert lib.dgn_gemm_wgrad(0, k, n, None, n, None, k, dw.data_ptr(), k + 2, None, None, 0, ctx.st()) == OK
    assert float(dw[:n, :k].abs().max()) == 0.0 and int(torch.isnan(dw).sum()) == dw.numel() - n * k
    assert bool(torch.isnan(c).all())
    assert lib.dgn_gemm_wgrad_workspace_bytes(0, k, n) == 0 and lib.dgn_gemm_wgrad_workspace_bytes(-1, k, n) == 0
    assert lib.dgn_gemm_wgrad_workspace_bytes(100, 3, n) == 0 and lib.dgn_gemm_wgrad_workspace_bytes(100, k, 4097) == 0
    assert lib.dgn_gemm_wgrad_workspace_bytes(1, k, n) > 0


def test_supported_at_the_corners(ctx):
    ok = ctx.lib.dgn_gemm_supported
    assert ok(4, 4) and ok(4, 4096) and ok(4096, 4) and ok(4096, 4096)
    assert not ok(3, 4) and not ok(4, 3) and not ok(4097, 4) and not ok(4, 4097) and not ok(3, 4096) and not ok(4096, 4097)


def test_refusals(ctx, monkeypatch):
    lib, _lib, dev = ctx.lib, ctx._lib, ctx.dev
    INVALID, WORKSPACE = _lib.DGN_ERR_INVALID, _lib.DGN_ERR_WORKSPACE
    M, W = 16, 4100                                      # (every buffer is large enough for the call it would be, were it accepted)
    a = torch.zeros(M, W, device=dev)
    w = torch.zeros(W, W, device=dev)
    c = torch.full((M, W), NAN, device=dev)
    dw = torch.full((W, W), NAN, device=dev)
    ws = torch.zeros(1 << 26, dtype=torch.uint8, device=dev)
    pa, pw, pc, pd, pws = a.data_ptr(), w.data_ptr(), c.data_ptr(), dw.data_ptr(), ws.data_ptr()

    def fwd(k, n, a=pa, lda=W, w=pw, ldw=W, kn=0, c=pc, ldc=W, rows=M):
        return lib.dgn_gemm_forward(rows, k, n, a, lda, w, ldw, kn, None, c, ldc, ctx.st())

    def wg(k, n, g=pa, ldg=W, x=pa, ldx=W, dw=pd, lddw=W, ws=pws, nb=ws.numel(), rows=M):
        return lib.dgn_gemm_wgrad(rows, k, n, g, ldg, x, ldx, dw, lddw, None, ws, nb, ctx.st())

    for k, n in ((3, 16), (16, 3), (4097, 16), (16, 4097)):
        assert fwd(k, n) == INVALID and wg(k, n) == INVALID, (k, n)
        assert fwd(k, n, rows=0) == INVALID and wg(k, n, rows=0) == INVALID, (k, n)
    assert fwd(16, 16, rows=-1) == INVALID and wg(16, 16, rows=-1) == INVALID
    assert fwd(20, 24, lda=19) == INVALID and fwd(20, 24, ldc=23) == INVALID
    assert fwd(20, 24, ldw=19) == INVALID and fwd(20, 24, ldw=23, kn=1) == INVALID       # [n, k]: ldw >= k; [k, n]: ldw >= n
    assert fwd(24, 20, ldw=23) == INVALID and fwd(24, 20, ldw=19, kn=1) == INVALID
    assert fwd(20, 24, a=None) == INVALID and fwd(20, 24, w=None) == INVALID and fwd(20, 24, c=None) == INVALID
    assert wg(20, 24, lddw=19) == INVALID and wg(20, 24, dw=None) == INVALID and wg(20, 24, dw=None, rows=0) == INVALID
    assert wg(20, 24, g=None) == INVALID and wg(20, 24, x=None) == INVALID and wg(20, 24, ldg=23) == INVALID and wg(20, 24, ldx=19) == INVALID
    need = lib.dgn_gemm_wgrad_workspace_bytes(M, 20, 24)
    assert 0 < need <= ws.numel()
    assert wg(20, 24, nb=need - 1) == WORKSPACE and wg(20, 24, ws=None) == WORKSPACE
    for tile in (0, 1):
        monkeypatch.setattr(_lib.options, "tile_wgrad", tile)
        assert wg(20, 24, nb=need - 1) == WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(c).all()) and bool(torch.isnan(dw).all())            # nothing was launched
    assert fwd(20, 24, lda=20, ldc=24, ldw=20) == _lib.DGN_OK and fwd(20, 24, lda=20, ldc=24, ldw=24, kn=1) == _lib.DGN_OK      # (the exact strides
    assert wg(20, 24, ldg=24, ldx=20, lddw=20, nb=need) == _lib.DGN_OK                                                           #  and size are accepted)
    torch.cuda.synchronize()


# ---- F. the instance proof ------------------------------------------------------------------------------------------------------------------
# Launches per kernel when every cell runs once (by hand from the cell lists above).
#   ts_gemm<NT, W>, per layout W: M_SMALL -- 21 widths x 5 k x 2 bias settings = 210, all on NT = 1 (the column split); M_TS -- 3 k x 2 bias
#     = 6 per width: NT 1 .. 16 once each (ragged), NT 1, 8, 16 once more (full), n = 330 on NT 11, n = 500 on NT 16
#   tile_gemm<NQ>: 4 row counts x 3 k x 2 bias = 24 per width; NQ 5 and 7 have two widths each
#   ts_gemm_wgrad<KT>: 2 row counts x 3 n = 6 per cell and k slice grid (one launch whatever the number of slices); KT t: two cells;
#     KT 2, 8, 16: the ones-opens-tile cell; KT 10, 14: k = 300, 420 with and without dbias
#   tile_wgrad: 7 shapes x 2 row counts x 2 + (880, 1320) x 2 = 30
EXPECT_TS = {nt: 6 for nt in range(1, 17)}
EXPECT_TS.update({1: 210 + 12, 8: 12, 11: 12, 16: 18})
EXPECT_TILE = {4: 24, 5: 48, 6: 24, 7: 48}
EXPECT_STRIP = {kt: 12 for kt in range(1, 17)}
EXPECT_STRIP.update({2: 18, 8: 18, 16: 18, 10: 24, 14: 24})
EXPECT_CELLS = {"ts_gemm": 672, "tile_gemm": 144, "ts_gemm_wgrad": 234, "tile_wgrad": 30}


def test_the_cell_lists_have_the_stated_sizes():
    assert len(TS_WIDTHS) == 21 and len(TILE_WIDTHS) == 6 and len(STRIP_CELLS) == 39 and len(TW_SHAPES) == 8
    assert 2 * sum(EXPECT_TS.values()) == EXPECT_CELLS["ts_gemm"] == 21 * 2 * (5 + 3) * 2
    assert sum(EXPECT_TILE.values()) == EXPECT_CELLS["tile_gemm"] == 6 * 4 * 3 * 2
    assert sum(EXPECT_STRIP.values()) == EXPECT_CELLS["ts_gemm_wgrad"] == 39 * 3 * 2
    assert EXPECT_CELLS["tile_wgrad"] == 7 * 2 * 2 + 2


def test_every_instance_ran(ctx, monkeypatch):
    cells = {}

    def option(name, value):
        monkeypatch.setattr(ctx._lib.options, name, value)

    def fwd_cell(mode, M, k, n, kn):
        a, w, b = forward_operands(ctx, M, k, n, kn)
        for bias in (None, b):
            forward(ctx, M, k, n, kn, a, w, bias, poison=False)
            cells[mode] = cells.get(mode, 0) + 1

    def wg_cell(mode, M, k, n, dbias):
        wgrad(ctx, M, k, n, dbias, ctx.g(M, n), ctx.a(M, k), poison=False)
        cells[mode] = cells.get(mode, 0) + 1

    def every_cell_once():
        option("tile_gemm", 0)
        for _, n in TS_WIDTHS:
            for kn in (0, 1):
                for M, ks in ((M_SMALL, K_SMALL), (ctx.rows["ts"], K_LONG)):
                    for k in ks:
                        fwd_cell("ts_gemm", M, k, n, kn)
        option("tile_gemm", 1)
        for n in TILE_WIDTHS:
            for rows in TILE_ROWS:
                for k in K_LONG:
                    fwd_cell("tile_gemm", ctx.rows[rows], k, n, 0)
        option("tile_wgrad", 0)
        for _, k, dbias, _ in STRIP_CELLS:
            for M in (M_SMALL, ctx.rows["ts"]):
                for n in STRIP_N:
                    wg_cell("ts_gemm_wgrad", M, k, n, dbias)
        for k, n in TW_SHAPES:
            option("tile_wgrad", 1 if n <= 256 else -1)
            for M in (M_SMALL,) if (k, n) in TW_SMALL_ONLY else (M_SMALL, ctx.rows["ts"]):
                for dbias in (False, True):
                    wg_cell("tile_wgrad", M, k, n, dbias)

    assert ctx._lib.options.tile_gemm == -1 and ctx._lib.options.tile_wgrad == -1
    names = _gemm_kernels(every_cell_once)
    assert names, "torch.profiler saw no device kernel of the wide GEMM family"
    assert cells == EXPECT_CELLS
    got = {"ts": {}, "tile": {}, "strip": {}, "other": {}}
    for name in names:
        for what, pat in (("other", r"(ts_gemm_wgrad_finalize|tile_wgrad_finalize)"), ("strip", r"ts_gemm_wgrad<(\d+)>"), ("ts", r"ts_gemm<(\d+),\s*(\d+)>"),
                          ("tile", r"tile_gemm<(\d+)>"), ("other", r"(tile_wgrad)")):
            m = re.search(pat, name)
            if m:
                key = tuple(int(v) if v.isdigit() else v for v in m.groups())
                key = key[0] if len(key) == 1 else key
                got[what][key] = got[what].get(key, 0) + 1
                break
        else:
            raise AssertionError("a kernel of the family this file does not know: " + name)
    assert got["ts"] == {(nt, kn): EXPECT_TS[nt] for nt in range(1, 17) for kn in (0, 1)}
    assert got["tile"] == EXPECT_TILE
    assert got["strip"] == EXPECT_STRIP
    assert got["other"] == {"ts_gemm_wgrad_finalize": 234, "tile_wgrad": 30, "tile_wgrad_finalize": 30}
    assert len(got["ts"]) + len(got["tile"]) + len(got["strip"]) == 52 and len(got["other"]) == 3          # 32 + 4 + 16 templated instances by name
