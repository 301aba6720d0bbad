"""The streaming fp32 Linear family (dgn_linear_*: ts_linear / ts_wgrad of csrc/dgn_linear_kernels.hpp) over its whole instantiated
(NT, KB) grid, every entry point against a plain fp64 evaluation of its definition (include/dgn_hip.h), at two row counts:

  M_SMALL = 37                        two full 16-row strips and a partial one of five rows -- every wave owns at most one strip;
  M_LONG  = 16 * 3 * 32 * CUs + 5     (393 221 rows on a 256-CU part) -- the kernels are persistent and software-pipelined (results stored
                                      one iteration late, row factors double-buffered on the iteration's parity, the next strip's prefetch
                                      crossing the MFMA block), so their first, middle and last iterations are three code paths, and a
                                      wave sees a second strip only when there are more strips than wave slots.  No launch can place
                                      more than 32 waves on a CU (the hardware's limit; 16 for the block-diagonal kernels, 8 for the
                                      weight gradients), so with 3 * 32 * CUs strips and five rows more EVERY wave of ANY plan owns at
                                      least three strips and the batch ends in a partial strip.  The bound is the hardware's, not the plan
                                      the library computes: a smaller count does not reach the steady-state loop, and a count derived from
                                      the code under test would shrink with a bug in its plan.  (Two towers share the wave slots: M_LONG / 2
                                      rows per tower.)

A mode is the library's own predicate (which cells it takes -- the others must be refused with an error code, and the number taken is
asserted against a literal worked out by hand from linear_shape_ok / kMaxWgradTiles), the call through the C ABI, and the fp64 reference.
Widths: a tile count t stands for the ragged width 16 t - 2 (padding columns and the bias gradient's ones column live); plain forward /
weight gradient also run the full width 16 t (no padding: the bias gradient must be refused) and the thin width 16 (t - 1) + 2.

Traps: weights sit in buffers two floats wider than the matrix with NaN padding; outputs are NaN-filled and 16 rows longer than M (the extra
rows must stay NaN); weight gradients have row stride k + 2 (the padding stays NaN).  At M_LONG every call is made twice: same bits.

Tolerances: products 1e-5 max|ref| (tests/test_linear_hip.py _close); bias gradients 2e-6 max_col(sum |g|) + 1e-6 (the same file); weight
gradients the rule of tests/test_hip_parity.py _as_good -- within 1e-5 max|ref| of fp64, or no further from it than four times torch's own
fp32 product; masks bit for bit.

The operands are drawn once per module into pools (three fp32 pools of M_LONG * 160 floats, a pool of mask bytes, the row factors); a case
takes views of them and converts the views for its reference."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

M_SMALL = 37
NAN = float("nan")
SLOPE = 0.01
EPS = 1e-5
TILES = range(1, 11)
CELLS = [(nt, kb) for nt in TILES for kb in TILES]


def ragged(t):
    return 16 * t - 2


def full(t):
    return 16 * t


def thin(t):
    return 16 * (t - 1) + 2


WIDTHS = {"ragged": ragged, "full": full, "thin": thin}


def combine_width(t, S):
    """S * f_out with f_out even, as close to the ragged width of tile count t as that allows: the largest multiple of 2 S up to 16 t - 2."""
    n = (ragged(t) // (2 * S)) * (2 * S)
    assert (n + 15) // 16 == t
    return n


class Ctx:
    """The module's operands (read-only) and the library handle."""

    def __init__(self):
        from dgn_amd import _lib
        self._lib = _lib
        self.lib = _lib.load()
        self.dev = torch.device("cuda")
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.m_long = 16 * 3 * 32 * cus + 5
        gen = torch.Generator(device=self.dev).manual_seed(1234)
        n = self.m_long * 160
        self.p0 = torch.randn(n, device=self.dev, generator=gen) * 1.5 + 0.3      # operands a / x / z / y
        self.p1 = torch.randn(n, device=self.dev, generator=gen)                  # gradients g / first addend / residual
        self.p2 = torch.randn(n, device=self.dev, generator=gen)                  # second addend
        self.mask = torch.randint(0, 4, (n // 2,), device=self.dev, generator=gen, dtype=torch.uint8)      # two sign bits per byte
        self.sc = torch.rand(self.m_long * 3, device=self.dev, generator=gen) + 0.5                       # scale table rows
        self.rs = torch.rand(self.m_long, device=self.dev, generator=gen) + 0.5                           # graph norm
        self.w = torch.randn(2, 160, 160, device=self.dev, generator=gen)
        self.v = torch.randn(8, 320, device=self.dev, generator=gen)                                      # bias / gamma / beta vectors
        self.st = torch.cuda.current_stream().cuda_stream
        self.ratios = {}                 # family -> largest (our error / the library GEMM's error) of a weight gradient
        self.ran = {}                    # mode -> cells run

    def rows(self, long, towers=1):
        return (self.m_long // towers) if long else M_SMALL

    def view(self, pool, *shape):
        n = 1
        for s in shape:
            n *= s
        return pool[:n].view(*shape)

    def weight(self, rows, cols, red, towers=None):
        """[rows, cols] (per tower) in a NaN-filled buffer of row stride cols + 2, scaled by 1 / sqrt(reduction width) -> (matrix view, buffer)"""
        T = towers or 1
        buf = torch.full((T, rows, cols + 2), NAN, device=self.dev)
        buf[:, :, :cols] = self.w[:T, :rows, :cols] / red ** 0.5
        return (buf[:, :, :cols] if towers else buf[0, :, :cols]), buf

    def vec(self, i, n, positive=False):
        return (self.v[i, :n].abs() + 0.5) if positive else self.v[i, :n].clone()

    def out(self, M, *w, towers=None):
        """NaN-filled, 16 rows longer than M (per tower) -> (the M rows, the whole buffer)"""
        buf = torch.full(((towers,) if towers else ()) + (M + 16,) + tuple(w), NAN, device=self.dev)
        return (buf[:, :M] if towers else buf[:M]), buf

    def bits(self, M, k):
        """the mask bytes of a dense [M, k] tensor and the bits they describe (byte i: elements 2 i and 2 i + 1)"""
        nb = self.lib.dgn_linear_act_mask_bytes(M, k)
        by = self.mask[:max(nb, M * k // 2)]
        b = by[:M * k // 2]
        return by, torch.stack([b & 1, (b >> 1) & 1], dim=1).view(M, k).bool()

    def call(self, what, rc):
        self._lib.check(rc, what)


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    print("\nweight gradients, largest error relative to torch's fp32 product against fp64, per family:", {k: round(v, 3) for k, v in c.ratios.items()})
    print("cells run per mode:", {k: len(v) for k, v in c.ran.items()})


def P(t):
    return None if t is None else t.data_ptr()


def act_grad(bit, act):
    off = SLOPE if act == 2 else (0.0 if act == 1 else 1.0)
    return torch.where(bit, 1.0, off).double()


def act_fwd(v, act):
    return torch.clamp_min(v, 0) if act == 1 else (torch.where(v > 0, v, v * SLOPE) if act == 2 else v)


def bn_stats(x):
    mean = x.mean(0)
    return mean, (x.var(0, unbiased=False) + EPS).rsqrt()


def bn64(x, mean, invstd, gamma, beta):
    xh = (x.double() - mean.double()) * invstd.double()
    if gamma is not None:
        xh = xh * gamma.double()
    return xh + beta.double() if beta is not None else xh


def ws_for(c, M, k, n, T=1):
    nb = c.lib.dgn_linear_wgrad_workspace_bytes(M, k, n, T)
    return torch.empty(max(nb, 1), dtype=torch.uint8, device=c.dev), nb


def colsum_abs(g):
    return float(g.abs().sum(-2).max())


# ---- the modes: prepare(c, M, k, n, var) -> inputs; run(c, I) -> {name: (value, guard)}; ref64(c, I) -> {name: (kind, ref, aux)} ------------
# kinds: "prod" (1e-5 max|ref|), "bias" (aux = max column sum of |g|), "wgrad" (aux = torch's fp32 product), "bits" (ref has the bits)
class Mode:
    towers = 1

    def cells_widths(self, nt, kb, var):
        """(k, n) of cell (NT, KB)"""
        f = WIDTHS[var[0]] if var and var[0] in WIDTHS else ragged
        return f(kb), f(nt)


class Forward(Mode):
    name, count, family = "forward", 100, None
    variants = [(wk, kn) for wk in ("ragged", "full", "thin") for kn in (0, 1)]

    def supported(self, c, k, n):
        return c.lib.dgn_linear_supported(k, n, 0)

    def prepare(self, c, M, k, n, var):
        kn = var[1]
        w, wbuf = c.weight(k, n, k) if kn else c.weight(n, k, k)
        return dict(M=M, k=k, n=n, kn=kn, a=c.view(c.p0, M, k), w=w, wbuf=wbuf, b=c.vec(0, n))

    def run(self, c, I):
        o, ob = c.out(I["M"], I["n"])
        c.call("forward", c.lib.dgn_linear_forward(I["M"], I["k"], I["n"], 1, P(I["a"]), I["k"], 0, P(I["wbuf"]), I["wbuf"].shape[-1], 0, I["kn"], P(I["b"]), 0,
                                                   P(o), I["n"], 0, c.st))
        return {"c": (o, ob[I["M"]:])}

    def ref64(self, c, I):
        w = I["w"].double()
        return {"c": ("prod", I["a"].double() @ (w if I["kn"] else w.T) + I["b"].double(), None)}


class Wgrad(Mode):
    name, count, family = "wgrad", 76, "ts_wgrad"
    variants = [(wk, db) for wk in ("ragged", "full", "thin") for db in (True, False)]

    def supported(self, c, k, n):
        return c.lib.dgn_linear_supported(k, n, 1)

    def refused(self, k, n, var):
        return var[1] and k % 16 == 0                 # the bias gradient rides in X's padding column

    def prepare(self, c, M, k, n, var):
        return dict(M=M, k=k, n=n, db=var[1], g=c.view(c.p1, M, n), x=c.view(c.p0, M, k))

    def operands(self, c, I):
        return I["g"], I["x"]

    def launch(self, c, I, dw, db, ws, nb):
        return c.lib.dgn_linear_wgrad(I["M"], I["k"], I["n"], 1, P(I["g"]), I["n"], 0, P(I["x"]), I["k"], 0, P(dw), I["k"] + 2, 0, P(db), 0, P(ws), nb, c.st)

    def run(self, c, I):
        k, n = I["k"], I["n"]
        dw = torch.full((n, k + 2), NAN, device=c.dev)
        db = torch.full((n + 16,), NAN, device=c.dev) if I["db"] else None
        ws, nb = ws_for(c, I["M"], k, n)
        c.call(self.name, self.launch(c, I, dw, db, ws, nb))
        res = {"dw": (dw[:, :k], dw[:, k:])}
        if I["db"]:
            res["db"] = (db[:n], db[n:])
        return res

    def ref64(self, c, I):
        g, x = self.operands(c, I)
        g64, x64 = g.double(), x.double()
        res = {"dw": ("wgrad", g64.T @ x64, g64.float().T @ x64.float())}
        if I["db"]:
            res["db"] = ("bias", g64.sum(0), colsum_abs(g64))
        return res


class ForwardBn(Mode):
    name, count, family = "forward_bn", 100, None
    variants = [("ragged", True), ("ragged", False)]

    def supported(self, c, k, n):
        return c.lib.dgn_linear_supported(k, n, 0)

    def prepare(self, c, M, k, n, var):
        x = c.view(c.p0, M, k)
        mean, invstd = bn_stats(x)
        w, wbuf = c.weight(n, k, k)
        return dict(M=M, k=k, n=n, a=x, mean=mean, invstd=invstd, gamma=c.vec(1, k, True) if var[1] else None, beta=c.vec(2, k) if var[1] else None,
                    w=w, wbuf=wbuf, b=c.vec(0, n))

    def run(self, c, I):
        o, ob = c.out(I["M"], I["n"])
        c.call(self.name, c.lib.dgn_linear_forward_bn(I["M"], I["k"], I["n"], P(I["a"]), P(I["wbuf"]), I["k"] + 2, 0, P(I["b"]), P(o), P(I["mean"]), P(I["invstd"]),
                                                      P(I["gamma"]), P(I["beta"]), c.st))
        return {"c": (o, ob[I["M"]:])}

    def ref64(self, c, I):
        return {"c": ("prod", bn64(I["a"], I["mean"], I["invstd"], I["gamma"], I["beta"]) @ I["w"].double().T + I["b"].double(), None)}


class WgradBn(Wgrad):
    name, count, family = "wgrad_bn", 76, "ts_wgrad"
    variants = [("ragged", db, aff) for db in (True, False) for aff in (True, False)]

    def prepare(self, c, M, k, n, var):
        I = Wgrad.prepare(self, c, M, k, n, var)
        I["mean"], I["invstd"] = bn_stats(I["x"])
        I["gamma"], I["beta"] = (c.vec(1, k, True), c.vec(2, k)) if var[2] else (None, None)
        return I

    def operands(self, c, I):
        return I["g"], bn64(I["x"], I["mean"], I["invstd"], I["gamma"], I["beta"])

    def launch(self, c, I, dw, db, ws, nb):
        return c.lib.dgn_linear_wgrad_bn(I["M"], I["k"], I["n"], P(I["g"]), P(I["x"]), P(dw), I["k"] + 2, P(db), P(I["mean"]), P(I["invstd"]), P(I["gamma"]),
                                         P(I["beta"]), P(ws), nb, c.st)


class WgradBnActMask(WgradBn):
    name, count, family = "wgrad_bn_act_mask", 76, "ts_wgrad gmask"
    variants = [("ragged", True, False), ("ragged", False, True)]

    def prepare(self, c, M, k, n, var):
        I = WgradBn.prepare(self, c, M, k, n, var)
        I["mask"], I["bit"] = c.bits(M, n)
        return I

    def operands(self, c, I):
        return I["g"].double() * act_grad(I["bit"], 2), bn64(I["x"], I["mean"], I["invstd"], I["gamma"], I["beta"])

    def launch(self, c, I, dw, db, ws, nb):
        return c.lib.dgn_linear_wgrad_bn_act_mask(I["M"], I["k"], I["n"], P(I["g"]), P(I["mask"]), 2, SLOPE, P(I["x"]), P(dw), I["k"] + 2, P(db), P(I["mean"]),
                                                  P(I["invstd"]), P(I["gamma"]), P(I["beta"]), P(ws), nb, c.st)


class ForwardAct(Mode):
    """c = (g * act'(z + b)) . w, side output the formed operand (k: the reduction width)"""
    name, count, family = "forward_act", 94, None
    variants = [("ragged", act, side) for act in (0, 1, 2) for side in (True, False)]

    def supported(self, c, k, n):
        return c.lib.dgn_linear_act_supported(k, n)

    def prepare(self, c, M, k, n, var):
        w, wbuf = c.weight(k, n, k)
        return dict(M=M, k=k, n=n, act=var[1], side=var[2], g=c.view(c.p1, M, k), z=c.view(c.p0, M, k), b=c.vec(0, k), w=w, wbuf=wbuf)

    def launch(self, c, I, o, gz):
        return c.lib.dgn_linear_forward_act(I["M"], I["k"], I["n"], P(I["g"]), P(I["z"]), P(I["b"]), I["act"], SLOPE, P(I["wbuf"]), I["n"] + 2, 1, P(o), P(gz), c.st)

    def run(self, c, I):
        o, ob = c.out(I["M"], I["n"])
        gz, gzb = c.out(I["M"], I["k"]) if I["side"] else (None, None)
        c.call(self.name, self.launch(c, I, o, gz))
        res = {"c": (o, ob[I["M"]:])}
        if I["side"]:
            res["gz"] = (gz, gzb[I["M"]:])
        return res

    def derivative(self, I):
        return act_grad((I["z"].double() + I["b"].double()) > 0, I["act"])

    def ref64(self, c, I):
        gz = I["g"].double() * self.derivative(I)
        res = {"c": ("prod", gz @ I["w"].double(), None)}
        if I["side"]:
            res["gz"] = ("prod", gz, None)
        return res


class ForwardActMask(ForwardAct):
    """the same with the derivative read from a byte mask (an input: built from random sign bits)"""
    name, count, family = "forward_act_mask", 94, None

    def prepare(self, c, M, k, n, var):
        I = ForwardAct.prepare(self, c, M, k, n, var)
        I["mask"], I["bit"] = c.bits(M, k)
        return I

    def launch(self, c, I, o, gz):
        return c.lib.dgn_linear_forward_act_mask(I["M"], I["k"], I["n"], P(I["g"]), P(I["mask"]), I["act"], SLOPE, P(I["wbuf"]), I["n"] + 2, 1, P(o), P(gz), c.st)

    def derivative(self, I):
        return act_grad(I["bit"], I["act"])


class ForwardAdd(Mode):
    name, count, family = "forward_add", 62, None
    variants = [("ragged", True), ("ragged", False)]

    def supported(self, c, k, n):
        return c.lib.dgn_linear_add_supported(k, n)

    def prepare(self, c, M, k, n, var):
        w, wbuf = c.weight(k, n, k)
        return dict(M=M, k=k, n=n, a=c.view(c.p0, M, k), w=w, wbuf=wbuf, e1=c.view(c.p1, M, n), e2=c.view(c.p2, M, n) if var[1] else None)

    def run(self, c, I):
        o, ob = c.out(I["M"], I["n"])
        c.call(self.name, c.lib.dgn_linear_forward_add(I["M"], I["k"], I["n"], P(I["a"]), P(I["wbuf"]), I["n"] + 2, 1, P(I["e1"]), P(I["e2"]), P(o), c.st))
        return {"c": (o, ob[I["M"]:])}

    def ref64(self, c, I):
        r = I["e1"].double() + I["a"].double() @ I["w"].double()
        return {"c": ("prod", r + I["e2"].double() if I["e2"] is not None else r, None)}


class ForwardBnAct(Mode):
    """z = bn(x) w^T, out = act(z + b) + residual"""
    name, count, family = "forward_bn_act", 62, None
    variants = [("ragged", 2, True), ("ragged", 1, True), ("ragged", 2, False)]

    def supported(self, c, k, n):
        return c.lib.dgn_linear_add_supported(k, n)

    def prepare(self, c, M, k, n, var):
        x = c.view(c.p0, M, k)
        mean, invstd = bn_stats(x)
        w, wbuf = c.weight(n, k, k)
        return dict(M=M, k=k, n=n, act=var[1], a=x, mean=mean, invstd=invstd, gamma=c.vec(1, k, True), beta=c.vec(2, k), w=w, wbuf=wbuf, b=c.vec(0, n),
                    res=c.view(c.p1, M, n) if var[2] else None)

    def z_and_out(self, c, I):
        z, zb = c.out(I["M"], I["n"])
        o, ob = c.out(I["M"], I["n"])
        c.call("forward_bn_act", c.lib.dgn_linear_forward_bn_act(I["M"], I["k"], I["n"], P(I["a"]), P(I["wbuf"]), I["k"] + 2, P(I["mean"]), P(I["invstd"]), P(I["gamma"]),
                                                                 P(I["beta"]), P(I["b"]), I["act"], SLOPE, P(I["res"]), P(z), P(o), c.st))
        return (z, zb), (o, ob)

    def run(self, c, I):
        (z, zb), (o, ob) = self.z_and_out(c, I)
        return {"z": (z, zb[I["M"]:]), "out": (o, ob[I["M"]:])}

    def ref64(self, c, I):
        z = bn64(I["a"], I["mean"], I["invstd"], I["gamma"], I["beta"]) @ I["w"].double().T
        out = act_fwd(z + I["b"].double(), I["act"])
        res = {"out": ("prod", out + I["res"].double() if I["res"] is not None else out, None)}
        if "z" in self.outputs:
            res["z"] = ("prod", z, None)
        return res

    outputs = ("z", "out")


class ForwardBnActMask(ForwardBnAct):
    """`out` against fp64; the mask bit for bit against (z + b) > 0 of dgn_linear_forward_bn_act's own z_out on the same inputs (sign bits
    near zero cannot be compared with fp64)"""
    name, count, family = "forward_bn_act_mask", 62, None
    outputs = ("out", "mask")

    def run(self, c, I):
        M, n = I["M"], I["n"]
        nb = c.lib.dgn_linear_act_mask_bytes(M, n)
        assert nb >= M * n // 2 and nb % 16 == 0
        mask = torch.full((nb + 16,), 0xAA, dtype=torch.uint8, device=c.dev)
        o, ob = c.out(M, n)
        c.call(self.name, c.lib.dgn_linear_forward_bn_act_mask(M, I["k"], n, P(I["a"]), P(I["wbuf"]), I["k"] + 2, P(I["mean"]), P(I["invstd"]), P(I["gamma"]), P(I["beta"]),
                                                               P(I["b"]), I["act"], SLOPE, P(I["res"]), P(mask), P(o), c.st))
        assert bool((mask[M * n // 2:] == 0xAA).all()), "mask bytes written past the tensor"
        return {"out": (o, ob[M:]), "mask": (mask[:M * n // 2], None)}

    def ref64(self, c, I):
        res = ForwardBnAct.ref64(self, c, I)
        (z, _), _ = self.z_and_out(c, I)
        pos = ((z + I["b"]) > 0).reshape(-1, 2)
        res["mask"] = ("bits", pos[:, 0].to(torch.uint8) | (pos[:, 1].to(torch.uint8) << 1), None)
        return res


class ActMaskBnb(Mode):
    """The formula of test_mixing_backward_kernels_of_round_6_vs_the_separate_passes in fp64: g_y1 = (g * act'(mask)) . w,
    gz[t][m][o] = rs[m] * gamma[c] invstd[c] (g_y1[m][c] - sums[c] / M - xhat[m][c] sums[n + c] / M), c = t f_out + o, tower-major.
    k == n; the widths: the ragged width where an even f_out divides it into 2 .. 15 towers, else the nearest width below that has one (and the
    ragged width itself as a single tower)."""
    name, count, family = "forward_act_mask_bnb", 5, None
    shapes = {1: [(14, 2)], 2: [(30, 6)], 3: [(46, 46), (44, 4)], 4: [(62, 62), (60, 10)], 5: [(78, 6)],
              6: [(94, 94)], 7: [(110, 10)], 8: [(126, 14)], 9: [(142, 142)], 10: [(158, 158)]}      # (6 .. 10: refused)
    variants = [("ragged", i, rs) for i in (0, 1) for rs in (True, False)]

    def supported(self, c, k, n):
        return k == n and c.lib.dgn_linear_bnb_supported(k, n)

    def cells_widths(self, nt, kb, var):
        w = self.shapes[nt][min(var[1], len(self.shapes[nt]) - 1)][0]
        return w, w

    def prepare(self, c, M, k, n, var):
        sh = self.shapes[(n + 15) // 16]
        if var[1] >= len(sh):
            return None
        fo = sh[var[1]][1]
        w, wbuf = c.weight(k, n, k)
        y = c.view(c.p0, M, n)
        mean, invstd = bn_stats(y)
        mask, bit = c.bits(M, k)
        I = dict(M=M, k=k, n=n, fo=fo, g=c.view(c.p1, M, k), mask=mask, bit=bit, w=w, wbuf=wbuf, y=y, mean=mean, invstd=invstd, gamma=c.vec(1, n, True),
                 rs=c.view(c.rs, M) if var[2] else None)
        gy1 = (I["g"].double() * act_grad(bit, 2)) @ w.double()
        xh = (y.double() - mean.double()) * invstd.double()
        I["gy1"], I["xh"] = gy1, xh
        I["sums"] = torch.cat([gy1.sum(0), (gy1 * xh).sum(0)]).float().contiguous()      # (the fp32 values the kernel receives)
        return I

    def run(self, c, I):
        M, n, fo = I["M"], I["n"], I["fo"]
        gz, gzb = c.out(M, fo, towers=n // fo)
        c.call(self.name, c.lib.dgn_linear_forward_act_mask_bnb(M, I["k"], n, P(I["g"]), P(I["mask"]), 2, SLOPE, P(I["wbuf"]), n + 2, 1, P(I["y"]), P(I["mean"]), P(I["invstd"]),
                                                                P(I["gamma"]), P(I["sums"]), P(I["rs"]), fo, P(gzb), (M + 16) * fo, c.st))
        return {"gz": (gz, gzb[:, M:])}

    def ref64(self, c, I):
        M, n, fo = I["M"], I["n"], I["fo"]
        s = I["sums"].double()
        want = (I["gamma"].double() * I["invstd"].double()) * ((I["gy1"] - s[:n] / M) - I["xh"] * (s[n:] / M))
        if I["rs"] is not None:
            want = want * I["rs"].double().unsqueeze(1)
        return {"gz": ("prod", want.view(M, n // fo, fo).permute(1, 0, 2), None)}


class Combine(Mode):
    """The scale-combine of the per-tower product as tests/combine_tail_ref.py states it (scale_combine_forward), on the GPU in fp64:
    y[m, t fo + o] = rs[m] (bias[t fo + o] + sum_s scale[m, s] (a[t] w[t]^T)[m, s fo + o]).  Two towers: blockIdx % T addressing is live."""
    towers = 2
    T = 2

    def cells_widths(self, nt, kb, var):
        return ragged(kb), combine_width(nt, var[1])

    def expand(self, I, gy):
        """G[t][m][s fo + o] = scale[m, s] gy[t][m][o]"""
        if I["sc"] is None:
            return gy.double()
        return torch.cat([gy.double() * I["sc"].double()[:, s].view(1, -1, 1) for s in range(I["S"])], dim=2)


class CombineForward(Combine):
    name, count, family = "combine_forward", 100, None
    variants = [("ragged", S, dressed) for S in (1, 2, 3) for dressed in (True, False)]
    wreg = True

    def supported(self, c, k, n):
        return c.lib.dgn_linear_supported(k, n, 0)

    def prepare(self, c, M, k, n, var):
        S, T = var[1], self.T
        fo = n // S
        w, wbuf = c.weight(n, k, k, towers=T)
        return dict(M=M, k=k, n=n, S=S, fo=fo, a=c.view(c.p0, T, M, k), w=w, wbuf=wbuf, sc=c.view(c.sc, M, S) if S > 1 else None,
                    b=c.vec(0, T * fo) if var[2] else None, rs=c.view(c.rs, M) if var[2] else None)

    def run(self, c, I):
        M, k, T, fo = I["M"], I["k"], self.T, I["fo"]
        y, yb = c.out(M, T * fo)
        c.call(self.name, c.lib.dgn_linear_combine_forward(M, k, T, I["S"], fo, P(I["a"]), M * k, P(I["wbuf"]), k + 2, I["n"] * (k + 2), P(I["sc"]), P(I["b"]), P(I["rs"]),
                                                           P(y), T * fo, c.st))
        return {"y": (y, yb[M:])}

    def ref64(self, c, I):
        M, T, S, fo = I["M"], self.T, I["S"], I["fo"]
        z = torch.bmm(I["a"].double(), I["w"].double().transpose(1, 2))
        y = torch.zeros(M, T * fo, dtype=torch.float64, device=c.dev)
        for t in range(T):
            for s in range(S):
                y[:, t * fo:(t + 1) * fo] += z[t][:, s * fo:(s + 1) * fo] * (I["sc"].double()[:, s:s + 1] if I["sc"] is not None else 1.0)
        if I["b"] is not None:
            y = y + I["b"].double()
        if I["rs"] is not None:
            y = y * I["rs"].double().unsqueeze(1)
        return {"y": ("prod", y, None)}


class CombineBackwardInput(Combine):
    """g_a[t] = G[t] . w[t]: the reduction runs over the expanded width S f_out (KB), the output is k wide (NT).  S = 2, 3: the expand
    kernels; S = 1: the plain kernel over two towers."""
    name, count, family = "combine_backward_input", 100, None
    variants = [("ragged", S) for S in (1, 2, 3)]
    wreg = True

    def cells_widths(self, nt, kb, var):
        return ragged(nt), combine_width(kb, var[1])       # (k, the output width; n = S f_out, the reduction width)

    def supported(self, c, k, n):
        return c.lib.dgn_linear_supported(n, k, 0)

    def prepare(self, c, M, k, n, var):
        S, T = var[1], self.T
        fo = n // S
        w, wbuf = c.weight(n, k, n, towers=T)
        return dict(M=M, k=k, n=n, S=S, fo=fo, gy=c.view(c.p1, T, M, fo), w=w, wbuf=wbuf, sc=c.view(c.sc, M, S) if S > 1 else None)

    def run(self, c, I):
        M, k, T, fo = I["M"], I["k"], self.T, I["fo"]
        ga, gab = c.out(M, k, towers=T)
        c.call(self.name, c.lib.dgn_linear_combine_backward_input(M, T, I["S"], fo, k, P(I["gy"]), M * fo, P(I["sc"]), P(I["wbuf"]), k + 2, I["n"] * (k + 2), P(gab),
                                                                  (M + 16) * k, c.st))
        return {"g_a": (ga, gab[:, M:])}

    def ref64(self, c, I):
        return {"g_a": ("prod", torch.bmm(self.expand(I, I["gy"]), I["w"].double()), None)}


class CombineBackwardWeight(Combine):
    """dw[t] = G[t]^T . a[t], g_sum[t] = column sums of G[t]"""
    name, count, family = "combine_backward_weight_bias", 76, "ts_wgrad expand"
    variants = [("ragged", S, gs) for S in (1, 2, 3) for gs in (True, False)]

    def supported(self, c, k, n):
        return c.lib.dgn_linear_supported(k, n, 1)

    def prepare(self, c, M, k, n, var):
        S, T = var[1], self.T
        fo = n // S
        return dict(M=M, k=k, n=n, S=S, fo=fo, gs=var[2], gy=c.view(c.p1, T, M, fo), a=c.view(c.p0, T, M, k), sc=c.view(c.sc, M, S) if S > 1 else None)

    def run(self, c, I):
        M, k, n, T, fo = I["M"], I["k"], I["n"], self.T, I["fo"]
        dw = torch.full((T, n, k + 2), NAN, device=c.dev)
        gs = torch.full((T * n + 16,), NAN, device=c.dev) if I["gs"] else None
        ws, nb = ws_for(c, M, k, n, T)
        c.call(self.name, c.lib.dgn_linear_combine_backward_weight_bias(M, T, I["S"], fo, k, P(I["gy"]), M * fo, P(I["sc"]), P(I["a"]), M * k, P(dw), k + 2, n * (k + 2), P(gs),
                                                                        P(ws), nb, c.st))
        res = {"dw": (dw[:, :, :k], dw[:, :, k:])}
        if I["gs"]:
            res["g_sum"] = (gs[:T * n].view(T, n), gs[T * n:])
        return res

    def ref64(self, c, I):
        G, a = self.expand(I, I["gy"]), I["a"].double()
        res = {"dw": ("wgrad", torch.bmm(G.transpose(1, 2), a), torch.bmm(G.float().transpose(1, 2), a.float()))}
        if I["gs"]:
            res["g_sum"] = ("bias", G.sum(1), colsum_abs(G))
        return res


MODES = [Forward(), Wgrad(), ForwardBn(), WgradBn(), ForwardAct(), ForwardAdd(), ForwardBnAct(), ForwardBnActMask(), ForwardActMask(), WgradBnActMask(),
         ActMaskBnb(), CombineForward(), CombineBackwardInput(), CombineBackwardWeight()]
BY_NAME = {m.name: m for m in MODES}


def compare(c, mode, got, ref, label, fails):
    for name, (kind, r, aux) in ref.items():
        v, guard = got[name]
        if guard is not None and guard.numel() and not bool(torch.isnan(guard).all()):
            fails.append(f"{label} {name}: wrote outside its rows / columns")
        if kind == "bits":
            if not torch.equal(v, r):
                fails.append(f"{label} {name}: {int((v != r).sum())} bytes differ")
            continue
        err = float((v.double() - r).abs().max())
        scale = float(r.abs().max())
        if kind == "prod":
            ok = err <= 1e-5 * scale
        elif kind == "bias":
            ok = err <= 2e-6 * aux + 1e-6
        else:
            lib_err = float((aux.double() - r).abs().max())
            ratio = err / max(lib_err, 1e-300)
            c.ratios[mode.family] = max(c.ratios.get(mode.family, 0.0), ratio)
            ok = err <= 1e-5 * scale or err <= 4 * lib_err
        if not ok:                                   # (a NaN in the output fails every comparison)
            fails.append(f"{label} {name}: error {err:.3e} at max|ref| {scale:.3e} ({kind})")


def run_cell(c, mode, nt, kb, monkeypatch=None):
    """every variant of the mode on cell (NT, KB) at both row counts; the WREG-eligible cells of the combine / expand products (12 .. 18
    tiles) with the option off and on"""
    fails = []
    ran = 0
    wreg = (0, 3) if getattr(mode, "wreg", False) and 12 <= nt * kb <= 18 else (None,)
    for var, long, wr in itertools.product(mode.variants, (False, True), wreg):
        k, n = mode.cells_widths(nt, kb, var)
        if not mode.supported(c, k, n):
            continue
        M = c.rows(long, mode.towers)
        I = mode.prepare(c, M, k, n, var)
        if I is None:
            continue
        label = f"{mode.name} {var} M={M} k={k} n={n}" + (f" lin_wreg={wr}" if wr is not None else "")
        if wr is not None:
            monkeypatch.setattr(c._lib.options, "lin_wreg", wr)
        if getattr(mode, "refused", None) and mode.refused(k, n, var):
            with pytest.raises(c._lib.DgnError):
                mode.run(c, I)
            continue
        got = mode.run(c, I)
        compare(c, mode, got, mode.ref64(c, I), label, fails)
        if long:                                     # a fixed summation order: the second call returns the same bits
            again = mode.run(c, I)
            for name, (v, _) in got.items():
                if not torch.equal(v, again[name][0]):
                    fails.append(f"{label} {name}: a second call returned other bits")
        ran += 1
    if ran:
        c.ran.setdefault(mode.name, set()).add((nt, kb))
    assert not fails, "\n".join(fails)
    return ran


def _cell_params():
    out = []
    for m in MODES:
        for nt, kb in CELLS:
            if m.name == "forward_act_mask_bnb" and nt != kb:
                continue                              # (k == n)
            out.append(pytest.param(m.name, nt, kb, id=f"{m.name}-{nt}x{kb}"))
    return out


@pytest.mark.parametrize("mode,nt,kb", _cell_params())
def test_cell_vs_fp64(ctx, monkeypatch, mode, nt, kb):
    """One (NT, KB) cell of one entry point: every variant, at M_SMALL and at M_LONG (the steady-state loop: see the module's docstring),
    against fp64, with the NaN traps around weights and outputs and, at M_LONG, bitwise repeatability.  A cell the library's predicate
    rejects must be refused with an error code instead."""
    m = BY_NAME[mode]
    ran = run_cell(ctx, m, nt, kb, monkeypatch)
    if not ran:
        refused = 0
        for var in m.variants:
            k, n = m.cells_widths(nt, kb, var)
            assert not m.supported(ctx, k, n)
            I = m.prepare(ctx, M_SMALL, k, n, var)          # the cell's operands all the same: the entry point must return an error, not launch
            if I is None:
                continue
            with pytest.raises(ctx._lib.DgnError):
                m.run(ctx, I)
            refused += 1
        assert refused


# Cells per mode, by hand from the shape rules of csrc/dgn_linear_kernels.hpp (tile counts 1 .. 10 each way):
#   every cell                                            100   plain / BatchNorm-prologue / combine / expand products
#   NT * KT <= 45 (kMaxWgradTiles)                         76   = 4 * 10 (NT <= 4) + 9 + 7 + 6 + 5 + 5 + 4 (NT = 5 .. 10)
#   4 NT + 8 KB <= 104 (two prefetched strips)             94   = 6 * 10 (NT <= 6) + 9 + 9 + 8 + 8 (NT = 7 .. 10)
#   16 NT + 4 KB <= 128 (two result-shaped strips)         62   = 5 * 10 (NT <= 5) + 8 (NT = 6) + 4 (NT = 7)
#   both, NT <= 5, KB <= 7, NT + KB <= 11, and k == n       5   the diagonal cells 1 .. 5
EXPECTED_CELLS = {"forward": 100, "wgrad": 76, "forward_bn": 100, "wgrad_bn": 76, "forward_act": 94, "forward_add": 62, "forward_bn_act": 62,
                  "forward_bn_act_mask": 62, "forward_act_mask": 94, "wgrad_bn_act_mask": 76, "forward_act_mask_bnb": 5, "combine_forward": 100,
                  "combine_backward_input": 100, "combine_backward_weight_bias": 76}


@pytest.mark.parametrize("mode", [m.name for m in MODES])
def test_the_predicates_accept_the_cells_the_shape_rules_imply(ctx, mode):
    """A predicate that wrongly shrank would thin test_cell_vs_fp64 silently: the number of cells each mode's predicate accepts (at every
    width of every variant) against the literal above."""
    m = BY_NAME[mode]
    assert m.count == EXPECTED_CELLS[mode]
    for var in m.variants:
        cells = [(nt, kb) for nt, kb in CELLS if (mode != "forward_act_mask_bnb" or nt == kb) and m.supported(ctx, *m.cells_widths(nt, kb, var))]
        assert len(cells) >= EXPECTED_CELLS[mode], (var, len(cells))


WREG_CELLS = [(nt, kb) for nt, kb in CELLS if 12 <= nt * kb <= 18]


def test_the_wreg_cells_include_the_hand_written_exclusions():
    """(2, 9) for the combine product, (2, 8), (2, 9), (3, 6) and (9, 2) for the expanded one, and their neighbours: all inside the 12 .. 18 tile
    band that test_cell_vs_fp64 runs with option lin_wreg off and on"""
    assert len(WREG_CELLS) == 15                     # 12: 4 cells, 14: 2, 15: 2, 16: 3, 18: 4
    for cell in ((2, 9), (2, 8), (3, 6), (9, 2), (2, 7), (3, 5), (6, 3), (2, 6), (3, 4), (4, 4), (6, 2), (8, 2)):
        assert cell in WREG_CELLS, cell


# plain forward: 1024 threads (8 NT + 4 KB + 52 <= 116), 512 threads, and the widest cell, whose weights leave LDS for two waves only
@pytest.mark.parametrize("nt,kb", [(2, 2), (9, 5), (10, 10)])
@pytest.mark.parametrize("min_waves", [1, 2, 4, 8, 16])
def test_small_batch_wave_plan_vs_fp64(ctx, monkeypatch, nt, kb, min_waves):
    """M = 2 970 (the row count launch_linear's small-batch comment speaks of: 186 strips), every value of option linear_small_min_waves"""
    monkeypatch.setattr(ctx._lib.options, "linear_small_min_waves", min_waves)
    m = BY_NAME["forward"]
    fails = []
    for kn in (0, 1):
        I = m.prepare(ctx, 2970, ragged(kb), ragged(nt), ("ragged", kn))
        compare(ctx, m, m.run(ctx, I), m.ref64(ctx, I), f"min_waves={min_waves} w_is_kn={kn}", fails)
    assert not fails, "\n".join(fails)
