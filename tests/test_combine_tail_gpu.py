"""The scale-combine and BatchNorm-tail kernels (csrc/dgn_combine.hip, csrc/dgn_bn_tail.hip) themselves, through the C ABI, against their
fp64 statements ``tests/combine_tail_ref.py`` (tied to torch's autograd by tests/test_combine_tail_ref_cpu.py).

Every other test sees these kernels through ``ops.*`` wrappers and whole layers: contiguous 256-byte aligned tensors, widths 65-130, a
few thousand rows, layer-level tolerances.  Only the C ABI lets a test choose ``ld``, the alignment of a base, ``n_valid``, NULL outputs
and a prefilled ``g_bias``.  Every output buffer is prefilled with NaN (``g_bias`` with a known non-zero vector), lives ``off`` floats
into a larger NaN-filled allocation (``off`` = 1: a 4-byte aligned base, 2: 8-byte) and is checked to be untouched outside its [N, F]
window (the slack columns of ``ld > F``, the floats in front of and behind it).  ``mean``, ``invstd`` and -- where they are inputs --
``sums`` come from the test (fp64, rounded to fp32; the same fp32 values go to the kernel and to the reference): the kernel's own
arithmetic is what is judged.

ROUTES: the kernel the dispatch code selects, per case.

  A  dgn_scale_combine_forward: ``combine_fwd<S>`` for S = 1, 2, 3, ``combine_fwd<0>`` (runtime S) for S >= 4.  width = T fo <= 256:
     256 / width row phases, one trip of the column loop; width > 256 (257, 300, 4096): ceil(width / 256) trips, one phase.  Slab height
     ``fwd_slab_rows``: 8 rows up to N = 16384, 16 at N = 16385.
  B  dgn_scale_combine_backward, bn == NULL: ``combine_bwd`` (+ ``bias_finalize`` with g_bias); even fo: the float2 stores, odd fo: scalar.
     (1, 4096, 1, 4099): slabs of 2 rows, 2050 slabs on 2048 workgroups -- workgroups 0 and 1 take a second trip of the slab loop.
  C  dgn_scale_combine_backward with a DgnBnGrad: ``combine_bwd_flat4`` when T == 1, S == 1, no table, bn.ld == wy, 2 <= wy <= 256,
     wy mod 4 != 0 and bn.y, bn.g_out, g_z 16-byte aligned (widths 2, 3, 5, 75, 130, 254, 255); ``combine_bwd`` otherwise: its pairs branch
     on even wy and bn.ld with 8-byte aligned bn.y / bn.g_out (258, 510, 514, 70 with ld 72, 1024 x 16391: 2049 slabs on 2048 workgroups), its
     scalar branch else (1, 257, 75 at a 4-byte base, 70 with bn.g_out at a 4-byte base; an 8-byte aligned bn.g_out leaves the flat
     route but keeps the pairs branch).
  D  dgn_bn_tail_forward: statistics ``bn_stats<true>`` (even F and ld, 8-byte aligned x) or ``bn_stats<false>``; F > 256 (pairs: > 512)
     takes a second trip of the column loop; ``stat_groups`` reaches its cap of 2048 at N = 16391 for F >= 129.  Apply: ``bn_apply_flat4``
     (dense, F mod 4 != 0, x / y / residual 16-byte aligned), else ``bn_apply_vec<4 | 2 | 1>`` by F, ld and the three addresses.
  E  dgn_bn_tail_backward: ``bn_bwd_stats_flat4`` (odd F, N >= 131072, dense, x and g_y 16-byte aligned), else ``bn_bwd_stats<true>``
     (pairs_ok) or ``bn_bwd_stats<false>``; then ``bn_bwd_finalize`` and, with g_x, ``bn_bwd_apply``.

THE BOUNDS are derived, not tuned: ``|ours - ref| <= k u magnitude`` with u = 2^-24, magnitude the reference's expression with every term
replaced by its absolute value, and k the fp32 roundings on the longest path from an input to the output.  The library is built with
``-ffp-contract=off`` (csrc/Makefile) and without ``-ffast-math`` or ``-fno-hip-fp32-correctly-rounded-divide-sqrt``, so hipcc's default
holds: fp32 division and square root are correctly rounded -- one rounding each.

  forward combine     k = S + 2: the product, the S adds onto the bias, the row scale.
  g_z without bn      k = 2: the row scale, the scaler.
  g_z with bn         k = 8 (+ 1 with row_scale, + 1 with a table) on the path of xhat sums[F + c] / n: xhat 2 (difference, invstd),
                      inv_n 1, sums inv_n 1, the product 1, the bracket's second difference 1, gamma invstd 1, its product 1.
                      (dgn_bn_tail_backward's g_x: the same count, (xhat sums) inv_n.)
  apply               k = 5: difference, invstd, gamma, beta, residual; eval k = 8: + the eps add, the square root, the division.
  sums over rows      fp64 accumulation of fp32 terms: the final rounding u |sum| + (rows) 2^-53 sum |term| for the accumulation, and the
                      roundings of each term: none for sum g' and sum x, 3 for g' xhat (xhat 2, product 1), 1 for x^2.
  save_invstd         relative u (1 + 0.5 E[x^2] / (var + eps)) + the fp64 accumulation.
  running statistics  k = 4 on momentum * statistic (its own final rounding, 1 - momentum, product, add) + the statistic's error.
  bias gradient       fp32 sums: (k of a term + chain) u sum |term|, chain = the adds in a row: ``combine_bwd`` rows-per-slab x slab trips,
                      ``combine_bwd_flat4`` period trips of a thread + the (rows per period) x (periods per workgroup) terms of the
                      epilogue + the remainder rows; ``bias_finalize`` ceil(G / 256) strided adds + 8 shuffle / LDS levels; + the add
                      into the caller's vector.

The routes named above and the chain lengths (``takes_flat4``, ``bwd_slab_rows``, ``flat4_geometry``, ``finalize_chain``, the ``flat``
expression of ``check_bn_backward``) are COPIES of the host conditions and constants of csrc/dgn_combine.hip and csrc/dgn_bn_tail.hip --
nothing in the C ABI reports the kernel a call took -- and must be kept in step with them.

Every comparison records its worst ratio to its bound as ``COMBINE-TAIL <entry> <case> <ratio>`` (``parity_util.note``).  Entries whose
bound is zero (rows >= n_valid, untouched slack) are compared for equality."""
import ctypes as C

import pytest
import torch

import combine_tail_ref as ref
from combine_tail_ref import U, EPS, f32

pytestmark = pytest.mark.gpu

NAN = float("nan")
ERR_INVALID, ERR_WORKSPACE = -1, -2      # DGN_ERR_INVALID, DGN_ERR_WORKSPACE of include/dgn_hip.h
D53 = 2.0 ** -53


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _lib():
    from dgn_amd import _lib
    return _lib, _lib.load()


class Buf:
    """An [N, F] window with row stride ``ld`` that starts ``off`` floats into a NaN-filled device allocation (8 more floats behind it)."""

    def __init__(self, dev, N, F, ld=None, off=0, src=None):
        self.N, self.F, self.ld, self.off = N, F, ld or F, off
        self.back = torch.full((off + N * self.ld + 8,), NAN, dtype=torch.float32, device=dev)
        assert self.back.data_ptr() % 16 == 0
        self.view = self.back.as_strided((N, F), (self.ld, 1), off)
        if src is not None:
            self.view.copy_(src.reshape(N, F))
        assert self.view.data_ptr() % 16 == (4 * off) % 16

    @property
    def ptr(self):
        return self.view.data_ptr()

    def get(self):
        return self.view.cpu()

    def untouched_outside(self):
        back = self.back.cpu()
        outside = torch.ones(back.shape, dtype=torch.bool)
        outside.as_strided((self.N, self.F), (self.ld, 1), self.off).fill_(False)
        return bool(torch.isnan(back[outside]).all())


def stream():
    return _lib()[0].stream_ptr(_dev())


def P(b):
    return None if b is None else (b.ptr if isinstance(b, Buf) else b.data_ptr())


def compare(entry, case, got, want, bound):
    """``|got - want| <= bound`` per entry (equality where the bound is 0); the worst ratio goes on record."""
    from parity_util import note
    got, want, bound = got.detach().cpu().double().reshape(-1), want.reshape(-1), bound.reshape(-1)
    assert got.shape == want.shape == bound.shape, (entry, case, got.shape, want.shape, bound.shape)
    assert bool(torch.isfinite(got).all()), f"{entry} {case}: {int((~torch.isfinite(got)).sum())} entries not finite (never written?)"
    err = (got - want).abs()
    exact = bound == 0
    ratio = (err / bound.masked_fill(exact, 1.0)).masked_fill(exact, 0.0)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    note(f"COMBINE-TAIL {entry} {case} {worst:.4f}")
    n_off = int((err[exact] != 0).sum())
    assert n_off == 0, f"{entry} {case}: {n_off} entries differ where equality is required"
    at = int(ratio.argmax()) if ratio.numel() else 0
    assert worst <= 1.0, f"{entry} {case}: worst ratio to the bound {worst:.4f} at flat index {at} (got {float(got[at])!r}, want {float(want[at])!r})"


def sum_bound(total, total_mag, rows, k_term):
    """fp64 accumulation of fp32 terms, rounded to fp32 at the end."""
    return U * total.abs() + (k_term * U + rows * D53) * total_mag


# ==== A. dgn_scale_combine_forward ==================================================================================================
# id: (T, fo, S, table, N, bias, row_scale, ld_extra)
FWD = {
    "S1-no-table-3x7-N257": (3, 7, 1, False, 257, True, True, 0),
    "S1-table-3x7-N257": (3, 7, 1, True, 257, True, True, 0),
    "S2-3x7-N7": (3, 7, 2, True, 7, True, True, 0),
    "S2-3x7-N257-ld+3": (3, 7, 2, True, 257, True, True, 3),
    "S3-5x14-N257": (5, 14, 3, True, 257, True, True, 0),
    "S4-runtime-5x14-N257": (5, 14, 4, True, 257, True, True, 0),
    "S4-runtime-3x7-N1": (3, 7, 4, True, 1, True, True, 3),
    "S2-1x256-N7-one-phase": (1, 256, 2, True, 7, True, True, 0),
    "S3-1x257-N257-two-trips": (1, 257, 3, True, 257, True, True, 0),
    "S1-3x100-N7-two-trips": (3, 100, 1, False, 7, True, True, 3),
    "S4-2x2048-N9-limit": (2, 2048, 4, True, 9, True, True, 0),
    "S2-3x7-N1": (3, 7, 2, True, 1, True, True, 0),
    "S2-1x3-N16385-slab16": (1, 3, 2, True, 16385, True, True, 0),
    "S3-5x14-N7-no-bias": (5, 14, 3, True, 7, False, True, 0),
    "S3-5x14-N7-no-row-scale": (5, 14, 3, True, 7, True, False, 0),
    "S1-1x257-N7-nothing": (1, 257, 1, False, 7, False, False, 0),
}


def combine_inputs(T, fo, S, table, N, seed):
    z = ref.values((T, N, S * fo), seed)
    scale = ref.uniform((N, S), seed + 1) if table else None
    bias = ref.values((T * fo,), seed + 2)
    rs = ref.uniform((N,), seed + 3)
    return z, scale, bias, rs


@pytest.mark.parametrize("case", list(FWD))
def test_scale_combine_forward(case):
    """k = S + 2 (S = 1 without a table: the product is exact, the bound stays)."""
    dev = _dev()
    _, lib = _lib()
    T, fo, S, table, N, use_bias, use_rs, ld_extra = FWD[case]
    z, scale, bias, rs = combine_inputs(T, fo, S, table, N, 100 + len(case))
    bias, rs = (bias if use_bias else None), (rs if use_rs else None)
    want, mag = ref.scale_combine_forward(z, scale, bias, rs)
    zd = z.to(dev)
    sd, bd, rd = (None if t is None else t.to(dev) for t in (scale, bias, rs))
    y = Buf(dev, N, T * fo, ld=T * fo + ld_extra)
    rc = lib.dgn_scale_combine_forward(N, T, S, fo, zd.data_ptr(), P(sd), P(bd), P(rd), y.ptr, y.ld, stream())
    assert rc == 0, lib.dgn_last_error()
    torch.cuda.synchronize()
    compare("scale_combine_forward", case, y.get(), want, (S + 2) * U * mag)
    assert y.untouched_outside(), "a write outside the [N, T fo] window of y"


def test_scale_combine_forward_refuses_a_row_wider_than_4096():
    dev = _dev()
    _, lib = _lib()
    z, y = torch.zeros(1, 1, 4097, device=dev), torch.full((1, 4097), NAN, device=dev)
    assert lib.dgn_scale_combine_forward(1, 1, 1, 4097, z.data_ptr(), None, None, None, y.data_ptr(), 4097, stream()) == ERR_INVALID
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())


# ==== bias-gradient chains (from the kernels' loop structure) ========================================================================
def bwd_slab_rows(wy):
    return max(1, min(32, 8192 // wy))      # kTileFloats / wy, at most 32


def finalize_chain(G):
    return -(-G // 256) + 8 + 1            # bias_finalize: strided adds, shuffle / LDS levels, the add into g_bias


def combine_bwd_chain(N, wy, G):
    rows = bwd_slab_rows(wy)
    slabs = -(-N // rows)
    return rows * -(-slabs // G) + finalize_chain(G)


def flat4_geometry(N, wy, G):
    g4 = 1 if wy & 1 else 2
    Pc, R = wy // g4, 4 // g4
    Pw = 256 // Pc
    periods = N // R
    Gf = max(1, min(G, -(-periods // (Pw * 8))))
    return R, Pw, periods, Gf


def flat4_chain(N, wy, G):
    R, Pw, periods, Gf = flat4_geometry(N, wy, G)
    return -(-periods // (Gf * Pw)) + R * Pw + (R - 1) + finalize_chain(Gf)


def takes_flat4(T, S, table, wy, ld, *ptrs):
    return T == 1 and S == 1 and not table and wy % 4 != 0 and 2 <= wy <= 256 and ld == wy and all(p % 16 == 0 for p in ptrs)


PREFILL_SEED = 77


def run_combine_backward(dev, T, fo, S, N, g_y, ld_gy, scale, rs, want_bias, bn=None, gz_off=0, ws_short=0):
    """-> (rc, g_z Buf, g_bias (device, prefilled) | None, prefill | None, G)."""
    _, lib = _lib()
    wy = T * fo
    g_z = Buf(dev, T * N, S * fo, off=gz_off)
    nbytes = lib.dgn_scale_combine_backward_workspace_bytes(N, T, fo)
    assert nbytes % (4 * wy) == 0
    G = nbytes // (4 * wy)
    prefill = ref.values((wy,), PREFILL_SEED) if want_bias else None
    g_b = prefill.clone().to(dev) if want_bias else None
    ws = torch.full((nbytes // 4 + 4,), NAN, dtype=torch.float32, device=dev) if want_bias else None
    rc = lib.dgn_scale_combine_backward(N, T, S, fo, P(g_y), ld_gy, P(scale), P(rs), g_z.ptr, P(g_b), P(ws), (nbytes - ws_short) if want_bias else 0,
                                        C.byref(bn) if bn is not None else None, stream())
    torch.cuda.synchronize()
    return rc, g_z, g_b, prefill, G


# ==== B. dgn_scale_combine_backward without bn ======================================================================================
# id: (T, fo, S, table, N, row_scale, ld_extra, g_bias)
BWD = {
    "T1-fo7-S1-no-table": (1, 7, 1, False, 257, True, 0, True),
    "T3-fo7-S2": (3, 7, 2, True, 257, True, 3, True),
    "T5-fo7-S3": (5, 7, 3, True, 131, True, 0, True),
    "T3-fo7-S4": (3, 7, 4, True, 33, True, 1, True),
    "T1-fo14-S1-table": (1, 14, 1, True, 257, True, 0, True),
    "T3-fo14-S2": (3, 14, 2, True, 257, True, 2, True),
    "T5-fo14-S3": (5, 14, 3, True, 131, True, 0, True),
    "T5-fo14-S4": (5, 14, 4, True, 7, True, 0, True),
    "T3-fo14-S2-no-row-scale": (3, 14, 2, True, 257, False, 0, True),
    "T3-fo7-S1-no-table-no-row-scale": (3, 7, 1, False, 1, False, 0, True),
    "T5-fo14-S3-no-bias-no-ws": (5, 14, 3, True, 257, True, 0, False),
    "T1-fo4096-N4099-2050-slabs": (1, 4096, 1, False, 4099, True, 0, True),
}


@pytest.mark.parametrize("case", list(BWD))
def test_scale_combine_backward(case):
    """g_z: k = 2.  g_bias: the prefilled vector + sum_n row_scale g_y, (1 + chain) u (sum |term| + |prefill|)."""
    dev = _dev()
    T, fo, S, table, N, use_rs, ld_extra, want_bias = BWD[case]
    wy = T * fo
    gy = ref.values((N, wy), 300 + len(case))
    scale = ref.uniform((N, S), 301 + len(case)) if table else None
    rs = ref.uniform((N,), 302 + len(case)) if use_rs else None
    want = ref.scale_combine_backward(gy, scale, rs, T, S, fo)
    gyd = Buf(dev, N, wy, ld=wy + ld_extra, src=gy)
    sd, rd = (None if t is None else t.to(dev) for t in (scale, rs))
    rc, g_z, g_b, prefill, G = run_combine_backward(dev, T, fo, S, N, gyd, gyd.ld, sd, rd, want_bias)
    assert rc == 0
    if case.endswith("2050-slabs"):
        assert bwd_slab_rows(wy) == 2 and G == 2048 and -(-N // 2) == 2050
    compare("scale_combine_backward", case + ":g_z", g_z.get(), want["g_z"], 2 * U * want["g_z_mag"])
    assert g_z.untouched_outside()
    if want_bias:
        k = 1 + combine_bwd_chain(N, wy, G)
        compare("scale_combine_backward", case + ":g_bias", g_b, prefill.double() + want["g_bias"], k * U * (want["g_bias_mag"] + prefill.double().abs()))


def test_scale_combine_backward_workspace_one_byte_short():
    dev = _dev()
    gy = torch.ones(33, 21, device=dev)
    rc, g_z, g_b, prefill, _ = run_combine_backward(dev, 3, 7, 1, 33, gy, 21, None, None, True, ws_short=1)
    assert rc == ERR_WORKSPACE
    assert torch.equal(g_b.cpu(), prefill) and bool(torch.isnan(g_z.back).all()), "something ran although the workspace was refused"


# ==== C. dgn_scale_combine_backward with a DgnBnGrad ================================================================================
FLAT_WIDTHS = (1, 2, 3, 5, 75, 130, 254, 255, 258, 510)
FLAT_ROWS = (1, 2, 3, 5, 1003, 6001)


def n_valid_values(N):
    """NULL, N, N - 3, a value inside a period of four rows (4 k + 1), 1."""
    out = [None, N]
    if N > 3:
        out.append(N - 3)
    if N > 5:
        out.append(4 * (N // 8) + 1)
    out.append(1)
    return out


def flat_variants(N):
    """(row_scale, relu, n_valid): every n_valid with both on, and the other three on / off pairs."""
    out = [(True, True, nv) for nv in n_valid_values(N)]
    out += [(False, False, None), (True, False, N - 3 if N > 3 else None), (False, True, None)]
    return out


def bn_struct(dev, d, sums, relu, nv, ld=None, off_y=0, off_g=0, gamma=True, beta=True):
    """DgnBnGrad over TailData ``d`` (+ the buffers it points into)."""
    lib_mod, _ = _lib()
    y, g = Buf(dev, d.N, d.F, ld=ld, off=off_y, src=d.x), Buf(dev, d.N, d.F, ld=ld, off=off_g, src=d.g)
    keep = dict(y=y, g=g, gamma=d.gamma.to(dev) if gamma else None, beta=d.beta.to(dev) if beta else None, mean=d.mean.to(dev), invstd=d.invstd.to(dev),
                sums=sums.to(dev), nv=None if nv is None else torch.tensor([nv], dtype=torch.int64, device=dev))
    bn = lib_mod.DgnBnGrad(g_out=g.ptr, y=y.ptr, ld=y.ld, gamma=P(keep["gamma"]), beta=P(keep["beta"]), mean=P(keep["mean"]), invstd=P(keep["invstd"]),
                           sums=P(keep["sums"]), relu=1 if relu else 0, n_valid=P(keep["nv"]))
    return bn, keep


def bn_dict(d, sums, relu, nv, gamma=True, beta=True):
    return dict(g_out=d.g, y=d.x, gamma=d.gamma if gamma else None, beta=d.beta if beta else None, mean=d.mean, invstd=d.invstd, sums=sums, relu=relu, n_valid=nv)


def check_bn_combine(case, dev, d, T, fo, S, scale, rs, relu, nv, expect_flat, ld=None, off_y=0, off_g=0, gz_off=0, gamma=True, beta=True):
    wy, N = T * fo, d.N
    sums = d.sums(relu, nv, gamma, beta)
    want = ref.scale_combine_backward(None, scale, rs, T, S, fo, bn=bn_dict(d, sums, relu, nv, gamma, beta))
    bn, keep = bn_struct(dev, d, sums, relu, nv, ld, off_y, off_g, gamma, beta)
    sd, rd = (None if t is None else t.to(dev) for t in (scale, rs))
    rc, g_z, g_b, prefill, G = run_combine_backward(dev, T, fo, S, N, None, 0, sd, rd, True, bn=bn, gz_off=gz_off)
    assert rc == 0
    flat = takes_flat4(T, S, scale is not None, wy, bn.ld, keep["y"].ptr, keep["g"].ptr, g_z.ptr)
    assert flat == expect_flat, f"{case}: the dispatch condition as this test restates it selects {'flat4' if flat else 'combine_bwd'}"
    k = 8 + (rs is not None) + (scale is not None)
    compare("scale_combine_backward_bn", case + ":g_z", g_z.get(), want["g_z"], k * U * want["g_z_mag"])
    assert g_z.untouched_outside()
    chain = flat4_chain(N, wy, G) if flat else combine_bwd_chain(N, wy, G)
    compare("scale_combine_backward_bn", case + ":g_bias", g_b, prefill.double() + want["g_bias"],
            (k + chain) * U * (want["g_bias_mag"] + prefill.double().abs()))


@pytest.mark.parametrize("N", FLAT_ROWS)
@pytest.mark.parametrize("W", FLAT_WIDTHS)
def test_one_tower_combine_backward_behind_batchnorm(W, N):
    """T = 1, S = 1, no table, dense, 16-byte aligned: ``combine_bwd_flat4`` for 2 <= W <= 256, ``combine_bwd`` for 1, 258 and 510 (at W = 1
    a 16-byte chunk spans four rows of row_scale; at W > 256 the flat kernel's epilogue has no thread for the columns from 256 on)."""
    dev = _dev()
    d = ref.tail_data(N, W)
    rs = ref.uniform((N,), 500 + N + W)
    for use_rs, relu, nv in flat_variants(N):
        check_bn_combine(f"W{W}-N{N}-rs{int(use_rs)}-relu{int(relu)}-nv{nv}", dev, d, 1, W, 1, None, rs if use_rs else None, relu, nv, expect_flat=2 <= W <= 256)


# id: (T, fo, S, table, N, ld_extra, off_y, off_g, gz_off)
OFF_FLAT = {
    "W257-scalar": (1, 257, 1, False, 131, 0, 0, 0, 0),
    "W514-pairs": (1, 514, 1, False, 67, 0, 0, 0, 0),
    "W70-ld72-pairs": (1, 70, 1, False, 1003, 2, 0, 0, 0),
    "W75-y-4-byte-aligned": (1, 75, 1, False, 1003, 0, 1, 0, 0),
    "W70-g_out-8-byte-aligned-pairs": (1, 70, 1, False, 1003, 0, 0, 2, 0),
    "W70-g_out-4-byte-aligned-scalar": (1, 70, 1, False, 1003, 0, 0, 1, 0),
    "W75-g_z-8-byte-aligned": (1, 75, 1, False, 1003, 0, 0, 0, 2),
    "T5-fo14": (5, 14, 1, False, 1003, 0, 0, 0, 0),
    "W70-S1-table": (1, 70, 1, True, 1003, 0, 0, 0, 0),
    "W70-S3": (1, 70, 3, True, 1003, 0, 0, 0, 0),
    "T5-fo14-S3": (5, 14, 3, True, 257, 0, 0, 0, 0),
    "W1024-N16391-2049-slabs": (1, 1024, 1, False, 16391, 0, 0, 0, 0),
}


@pytest.mark.parametrize("case", list(OFF_FLAT))
def test_combine_backward_behind_batchnorm_off_the_flat_route(case):
    """The same arithmetic through ``combine_bwd``: its pairs branch (even wy and bn.ld, bn.y and bn.g_out 8-byte aligned) and its scalar one.
    An 8-byte aligned g_out keeps the pairs branch; the scalar branch needs a 4-byte aligned one."""
    dev = _dev()
    T, fo, S, table, N, ld_extra, off_y, off_g, gz_off = OFF_FLAT[case]
    wy = T * fo
    d = ref.tail_data(N, wy)
    scale = ref.uniform((N, S), 600 + len(case)) if table else None
    rs = ref.uniform((N,), 601 + len(case))
    if case.endswith("2049-slabs"):
        assert bwd_slab_rows(wy) == 8 and -(-N // 8) == 2049
        variants = [(True, N - 3)]
    else:
        variants = [(True, None), (False, N - 3)]
    for relu, nv in variants:
        check_bn_combine(f"{case}-relu{int(relu)}-nv{nv}", dev, d, T, fo, S, scale, rs, relu, nv, expect_flat=False, ld=wy + ld_extra if ld_extra else None,
                         off_y=off_y, off_g=off_g, gz_off=gz_off)
    if N < 2000:      # gamma / beta NULL, no row_scale on the same route
        check_bn_combine(f"{case}-no-affine", dev, d, T, fo, S, scale, None, True, None, expect_flat=False, ld=wy + ld_extra if ld_extra else None,
                         off_y=off_y, off_g=off_g, gz_off=gz_off, gamma=False, beta=False)


def test_combine_backward_behind_batchnorm_refuses_a_row_wider_than_1024():
    dev = _dev()
    d = ref.tail_data(*TOO_WIDE)
    bn, keep = bn_struct(dev, d, d.sums(True), True, None)
    rc, g_z, g_b, prefill, _ = run_combine_backward(dev, 1, d.F, 1, d.N, None, 0, None, None, True, bn=bn)
    assert rc == ERR_INVALID
    assert torch.equal(g_b.cpu(), prefill) and bool(torch.isnan(g_z.back).all())


TAIL_WIDTHS = (1, 3, 70, 75, 301, 600, 1024)      # D and E: dense, aligned
TAIL_ROWS = (1, 2, 9, 1003)
TOO_WIDE = (3, 1025)                               # (N, F) of the refusals


# ==== D. dgn_bn_tail_forward ========================================================================================================
def run_bn_forward(dev, d, ld=None, off_x=0, off_y=0, off_r=0, training=True, relu=True, residual=True, gamma=True, beta=True, nv=None, momentum=0.1,
                   y_null=False, running=True):
    _, lib = _lib()
    N, F = d.N, d.F
    x = Buf(dev, N, F, ld=ld, off=off_x, src=d.x)
    r = Buf(dev, N, F, ld=ld, off=off_r, src=d.residual) if residual else None
    y = None if y_null else Buf(dev, N, F, ld=ld, off=off_y)
    ga, be = (d.gamma.to(dev) if gamma else None), (d.beta.to(dev) if beta else None)
    rm, rv = (d.running_mean.clone().to(dev), d.running_var.clone().to(dev)) if running else (None, None)      # (updated in place)
    sm, si = torch.full((F,), NAN, device=dev), torch.full((F,), NAN, device=dev)
    nbytes = lib.dgn_bn_tail_workspace_bytes(N, F)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
    nvd = None if nv is None else torch.tensor([nv], dtype=torch.int64, device=dev)
    rc = lib.dgn_bn_tail_forward(N, F, x.ptr, x.ld, P(ga), P(be), P(rm), P(rv), momentum, EPS, 1 if training else 0, 1 if relu else 0, P(r), P(y), sm.data_ptr(),
                                 si.data_ptr(), ws.data_ptr(), nbytes, P(nvd), stream())
    torch.cuda.synchronize()
    return rc, dict(x=x, y=y, r=r, rm=rm, rv=rv, mean=sm, invstd=si)


def check_bn_forward(case, dev, d, **kw):
    """Training in two steps -- the statistics against fp64, y against the fp64 apply formula on the RETURNED fp32 statistics (k = 5) -- then
    eval on the running statistics the test supplies (k = 8)."""
    relu, residual, gamma, beta = kw.get("relu", True), kw.get("residual", True), kw.get("gamma", True), kw.get("beta", True)
    nv, momentum, y_null = kw.get("nv"), kw.get("momentum", 0.1), kw.get("y_null", False)
    N, F = d.N, d.F
    mom = float(f32(torch.tensor(momentum, dtype=torch.float64)))          # (the fp32 value the C ABI receives)
    rc, out = run_bn_forward(dev, d, training=True, **kw)
    assert rc == 0
    ga, be, res = (d.gamma if gamma else None), (d.beta if beta else None), (d.residual if residual else None)
    want = ref.bn_tail_forward(d.x, ga, be, d.running_mean, d.running_var, mom, EPS, True, relu, res, nv, stats=(out["mean"], out["invstd"]))
    st = want["stats"]
    n = st["n"]
    e_mean = U * st["mean"].abs() + n * D53 * st["abs_mean"]
    compare("bn_tail_forward", case + ":save_mean", out["mean"], st["mean"], e_mean)
    var_err = (U + n * D53 * 4) * st["ex2"]                                  # the fp32 squares, the fp64 accumulation of sum x^2 and mean * sum x
    rel_is = U + 0.5 * var_err / (st["var"] + EPS)
    compare("bn_tail_forward", case + ":save_invstd", out["invstd"], st["invstd"], rel_is * st["invstd"])
    compare("bn_tail_forward", case + ":running_mean", out["rm"], want["running_mean"], 4 * U * want["running_mean_mag"] + mom * e_mean)
    unb_err = var_err * (n / (n - 1) if n > 1 else 1.0)
    compare("bn_tail_forward", case + ":running_var", out["rv"], want["running_var"], 4 * U * want["running_var_mag"] + mom * unb_err)
    if not y_null:
        compare("bn_tail_forward", case + ":y", out["y"].get(), want["y"], 5 * U * want["y_mag"])
        assert out["y"].untouched_outside()
        kw_eval = {k: v for k, v in kw.items() if k not in ("nv", "momentum", "y_null")}
        rc, ev = run_bn_forward(dev, d, training=False, **kw_eval)
        assert rc == 0
        want_ev = ref.bn_tail_forward(d.x, ga, be, d.running_mean, d.running_var, mom, EPS, False, relu, res)
        compare("bn_tail_forward", case + ":eval-y", ev["y"].get(), want_ev["y"], 8 * U * want_ev["y_mag"])
        assert ev["y"].untouched_outside()
        assert torch.equal(ev["rm"].cpu(), d.running_mean) and torch.equal(ev["rv"].cpu(), d.running_var), "eval mode wrote the running statistics"


@pytest.mark.parametrize("N", TAIL_ROWS)
@pytest.mark.parametrize("F", TAIL_WIDTHS)
def test_bn_tail_forward_widths_and_rows(F, N):
    """Dense, aligned.  Statistics: ``bn_stats<true>`` for 70, 600 (two trips of the pair loop), 1024; ``bn_stats<false>`` for 1, 3, 75, 301
    (two trips).  Apply: ``bn_apply_flat4`` for 1, 3, 70, 75 (N F mod 4 != 0 where N and F are odd: the ragged last chunk), ``bn_apply_vec<1>``
    for 301 (a period of 301 chunks does not fit a workgroup), ``bn_apply_vec<4>`` for 600 and 1024.  ReLU and residual on for odd N + F, off otherwise; momentum 1.0 at N = 9."""
    on = bool((N + F) & 1)
    check_bn_forward(f"F{F}-N{N}", _dev(), ref.tail_data(N, F), relu=on, residual=on, momentum=1.0 if N == 9 else 0.1)


# id: (N, F, kwargs): the apply kernel named is what launch_bn_apply selects
FWD_LAYOUT = {
    "F600-ld604-vec4": (257, 600, dict(ld=604)),
    "F70-ld72-pairs-vec2": (1003, 70, dict(ld=72)),
    "F70-ld71-scalar-vec1": (1003, 70, dict(ld=71)),
    "F75-ld77-vec1": (1003, 75, dict(ld=77)),
    "F600-ld602-vec2": (257, 600, dict(ld=602)),
    "F600-ld601-vec1": (257, 600, dict(ld=601)),
    "F70-x-4-byte-stats-scalar-vec1": (1003, 70, dict(off_x=1)),
    "F70-x-8-byte-vec2": (1003, 70, dict(off_x=2)),
    "F70-y-8-byte-vec2": (1003, 70, dict(off_y=2)),
    "F70-residual-8-byte-vec2": (1003, 70, dict(off_r=2)),
    "F75-x-8-byte-vec1": (1003, 75, dict(off_x=2)),
    "F600-x-8-byte-vec2": (257, 600, dict(off_x=2)),
    "F600-y-8-byte-vec2": (257, 600, dict(off_y=2)),
    "F600-residual-8-byte-vec2": (257, 600, dict(off_r=2)),
    "F600-x-4-byte-vec1": (257, 600, dict(off_x=1)),
    "F600-y-4-byte-vec1": (257, 600, dict(off_y=1)),
    "F600-residual-4-byte-vec1": (257, 600, dict(off_r=1)),
    "F75-no-gamma": (1003, 75, dict(gamma=False)),
    "F70-ld72-no-beta": (1003, 70, dict(ld=72, beta=False)),
    "F600-no-affine-no-relu-no-residual": (257, 600, dict(gamma=False, beta=False, relu=False, residual=False)),
    "F75-n_valid-1000": (1003, 75, dict(nv=1000)),
    "F70-n_valid-1": (1003, 70, dict(nv=1)),
    "F3-N9-n_valid-5": (9, 3, dict(nv=5)),
    "F70-statistics-only": (1003, 70, dict(y_null=True)),
    "F75-momentum-1": (1003, 75, dict(momentum=1.0)),
    "F257-N16391-2048-groups": (16391, 257, dict()),
    "F512-N16391-2048-groups": (16391, 512, dict(relu=False)),
}


@pytest.mark.parametrize("case", list(FWD_LAYOUT))
def test_bn_tail_forward_layouts(case):
    dev = _dev()
    N, F, kw = FWD_LAYOUT[case]
    _, lib = _lib()
    d = ref.tail_data(N, F, n_valid=kw.get("nv"))
    if case.endswith("2048-groups"):
        P_ = max(1, 256 // F)
        assert -(-N // (P_ * 8)) > 2048 and lib.dgn_bn_tail_workspace_bytes(N, F) == 2 * F * 2048 * 8 + 2 * F * 4
    check_bn_forward(case, dev, d, **kw)


def test_bn_tail_forward_refuses_a_row_wider_than_1024():
    dev = _dev()
    _, lib = _lib()
    assert lib.dgn_bn_tail_workspace_bytes(*TOO_WIDE) == 0
    rc, out = run_bn_forward(dev, ref.tail_data(*TOO_WIDE))
    assert rc == ERR_INVALID and bool(torch.isnan(out["y"].back).all()) and bool(torch.isnan(out["mean"]).all())


# ==== E. dgn_bn_tail_backward =======================================================================================================
def check_bn_backward(case, dev, d, ld=None, off_x=0, off_g=0, off_gx=0, relu=True, nv=None, gamma=True, beta=True, want_gx=True, want_sums=True,
                      want_ggamma=True, want_gbeta=True):
    """sums, g_gamma, g_beta against fp64 (fp64 accumulation: the terms' roundings + the final one); g_x against the fp64 formula on the
    RETURNED fp32 sums (k = 8) -- or, with sums == NULL, on the fp64 sums with their error carried into the bound."""
    _, lib = _lib()
    N, F = d.N, d.F
    x, g = Buf(dev, N, F, ld=ld, off=off_x, src=d.x), Buf(dev, N, F, ld=ld, off=off_g, src=d.g)
    gx = Buf(dev, N, F, ld=ld, off=off_gx) if want_gx else None
    ga, be = (d.gamma.to(dev) if gamma else None), (d.beta.to(dev) if beta else None)
    mean, invstd = d.mean.to(dev), d.invstd.to(dev)
    sums = torch.full((2 * F,), NAN, device=dev) if want_sums else None
    gg = torch.full((F,), NAN, device=dev) if want_ggamma else None
    gb = torch.full((F,), NAN, device=dev) if want_gbeta else None
    nbytes = lib.dgn_bn_tail_workspace_bytes(N, F)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
    nvd = None if nv is None else torch.tensor([nv], dtype=torch.int64, device=dev)
    rc = lib.dgn_bn_tail_backward(N, F, g.ptr, x.ptr, x.ld, P(ga), P(be), mean.data_ptr(), invstd.data_ptr(), 1 if relu else 0, P(gx), P(gg), P(gb), P(sums),
                                  ws.data_ptr(), nbytes, P(nvd), stream())
    assert rc == 0, lib.dgn_last_error()
    torch.cuda.synchronize()
    flat = bool(F & 1) and N >= 131072 and (ld or F) == F and F <= 256 and x.ptr % 16 == 0 and g.ptr % 16 == 0
    gam, bet = (d.gamma if gamma else None), (d.beta if beta else None)
    want = ref.bn_tail_backward(d.g, d.x, gam, bet, d.mean, d.invstd, relu, nv, sums=sums)
    n = N if nv is None else min(nv, N)
    k_term = torch.cat([torch.zeros(F, dtype=torch.float64), torch.full((F,), 3.0, dtype=torch.float64)])
    s_bound = U * want["sums"].abs() + (k_term * U + n * D53) * want["sums_mag"]
    if want_sums:
        compare("bn_tail_backward", case + ":sums", sums, want["sums"], s_bound)
    if want_gbeta:
        compare("bn_tail_backward", case + ":g_beta", gb, want["g_beta"], s_bound[:F])
    if want_ggamma:
        compare("bn_tail_backward", case + ":g_gamma", gg, want["g_gamma"], s_bound[F:])
    if want_gx:
        bound = 8 * U * want["g_x_mag"]
        if not want_sums:      # the kernel's own (unseen) fp32 sums: |gamma invstd| (d sums[c] + |xhat| d sums[F + c]) / n
            xh = ((d.x.double() - d.mean.double()) * d.invstd.double()).abs()
            carried = (d.invstd.double() * (d.gamma.double() if gamma else 1.0)).abs() * (s_bound[:F] + xh * s_bound[F:]) / n
            carried[n:] = 0.0
            bound = bound + carried
        compare("bn_tail_backward", case + ":g_x", gx.get(), want["g_x"], bound)
        assert gx.untouched_outside()
    return flat


@pytest.mark.parametrize("N", TAIL_ROWS)
@pytest.mark.parametrize("F", TAIL_WIDTHS)
def test_bn_tail_backward_widths_and_rows(F, N):
    """Dense, aligned, fewer than 131072 rows: ``bn_bwd_stats<true>`` for 70, 600, 1024, ``bn_bwd_stats<false>`` for 1, 3, 75, 301; ReLU on for
    odd N + F."""
    assert not check_bn_backward(f"F{F}-N{N}", _dev(), ref.tail_data(N, F), relu=bool((N + F) & 1))


# id: (N, F, kwargs)
BWD_LAYOUT = {
    "F70-ld72-pairs": (1003, 70, dict(ld=72)),
    "F70-ld71-scalar": (1003, 70, dict(ld=71)),
    "F75-ld77": (1003, 75, dict(ld=77)),
    "F600-ld602-pairs": (257, 600, dict(ld=602)),
    "F70-x-4-byte-scalar": (1003, 70, dict(off_x=1)),
    "F70-g_y-4-byte-scalar": (1003, 70, dict(off_g=1)),
    "F70-x-8-byte-pairs": (1003, 70, dict(off_x=2, off_g=2)),
    "F70-g_x-4-byte-pairs": (1003, 70, dict(off_gx=1)),
    "F75-n_valid-1000": (1003, 75, dict(nv=1000)),
    "F70-n_valid-1": (1003, 70, dict(nv=1)),
    "F3-N9-n_valid-5": (9, 3, dict(nv=5)),
    "F75-sums-only": (1003, 75, dict(want_gx=False)),
    "F75-g_x-without-sums": (1003, 75, dict(want_sums=False)),
    "F70-g_x-without-sums-n_valid": (1003, 70, dict(want_sums=False, nv=700)),
    "F75-no-g_gamma": (1003, 75, dict(want_ggamma=False)),
    "F75-no-g_beta": (1003, 75, dict(want_gbeta=False)),
    "F70-no-gamma-no-beta": (1003, 70, dict(gamma=False, beta=False)),
    "F75-no-relu": (1003, 75, dict(relu=False)),
    "F257-N16391-2048-groups": (16391, 257, dict()),
    "F512-N16391-2048-groups": (16391, 512, dict()),
}


@pytest.mark.parametrize("case", list(BWD_LAYOUT))
def test_bn_tail_backward_layouts(case):
    N, F, kw = BWD_LAYOUT[case]
    assert not check_bn_backward(case, _dev(), ref.tail_data(N, F), **kw)


# id: (N, F, kwargs): bn_bwd_stats_flat4 unless named otherwise
BWD_FLAT = {
    "F1-N131072": (131072, 1, dict()),
    "F1-N131075": (131075, 1, dict(relu=False)),
    "F3-N131072": (131072, 3, dict(relu=False)),
    "F3-N131075": (131075, 3, dict()),
    "F75-N131072": (131072, 75, dict()),
    "F75-N131075": (131075, 75, dict(relu=False)),
    "F75-N131075-n_valid-N-2": (131075, 75, dict(nv=131073)),
    "F75-N131075-n_valid-1000": (131075, 75, dict(nv=1000)),
    "F129-N131072": (131072, 129, dict(relu=False)),
    "F129-N131075": (131075, 129, dict()),
    "F255-N131075-sums-only": (131075, 255, dict(want_gx=False)),
    "F75-N131071-below-the-threshold": (131071, 75, dict()),
    "F75-N131075-x-8-byte-off-the-flat-route": (131075, 75, dict(off_x=2)),
}


@pytest.mark.parametrize("case", list(BWD_FLAT))
def test_bn_tail_backward_flat_chunks_of_large_batches(case):
    """``bn_bwd_stats_flat4``: odd F, N >= 131072, dense rows, x and g_y 16-byte aligned.  131072 rows are whole periods of four rows, 131075
    leave three remainder rows to workgroup 0's column threads; n_valid cuts the flat array short (N - 2: one remainder row; 1000: most
    workgroups idle)."""
    N, F, kw = BWD_FLAT[case]
    flat = check_bn_backward(case, _dev(), ref.tail_data(N, F), **kw)
    assert flat == ("131071" not in case and "off-the-flat" not in case)
