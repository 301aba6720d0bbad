"""Restatement of the eigenvector augmentations (csrc/dgn_eig_augment.hip, dgn_amd.EigAugment) for the tests: a numpy Philox4x32-10, the
random stream of the kernel as include/dgn_hip.h defines it, and the two training loops' arithmetic in fp64 with the random numbers as
ARGUMENTS -- so the same lines check against the reference's own recorded draws (tests/golden/g20_eig_augment.npz) and against the kernel's
Philox draws.

    molecule loop      train/train_molecules_graph_regression.py:29-33     sign[u >= 0.5] = +1, sign[u < 0.5] = -1; eig = sign * eig
    superpixel loop    train/train_superpixels_graph_classification.py:29-37
                           angle = (u - 0.5) * 2 * augmentation; sine = sin(angle * pi / 180)
                           eig[:, 1] = (1 - sine^2)^0.5 * eig1 + sine * eig2;  eig[:, 2] = (1 - sine^2)^0.5 * eig2 - sine * eig1
                       :38-42  the sign of the molecule loop, one per node, on column 2 -- after the rotation
"""
import math

import numpy as np

_M0, _M1 = 0xD2511F53, 0xCD9E8D57          # Random123's Philox4x32 multipliers ...
_W0, _W1 = 0x9E3779B9, 0xBB67AE85          # ... and Weyl key increments
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """``counter`` uint32 ``[..., 4]``, ``key`` uint32 ``[..., 2]`` (broadcast against each other) -> the ten-round output, uint32 ``[..., 4]``."""
    counter, key = np.asarray(counter, dtype=np.uint64), np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (counter[..., i] for i in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    sh = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2              # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & _LO, (p0 >> sh) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + np.uint64(_W0)) & _LO, (k1 + np.uint64(_W1)) & _LO
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def kernel_draws(n_rows: int, key: int, calls: int):
    """What row i of call number ``calls`` of a stream with ``key`` draws: ``(u [n_rows] -- the rotation's uniform (r[0] >> 8) 2^-24, exact in
    fp32 --, plus [n_rows, 32] bool -- bit j of r[1]: column j keeps its sign)``.  Counter (lo32 i, hi32 i, lo32 calls, hi32 calls), key
    (lo32 key, hi32 key)."""
    i = np.arange(n_rows, dtype=np.uint64)
    key, calls = int(key) & (2 ** 64 - 1), int(calls) & (2 ** 64 - 1)
    counter = np.stack([i & _LO, i >> np.uint64(32), np.full_like(i, calls & 0xFFFFFFFF), np.full_like(i, calls >> 32)], axis=-1)
    r = philox4x32_10(counter, np.array([key & 0xFFFFFFFF, key >> 32], dtype=np.uint64))
    u = (r[:, 0] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    plus = ((r[:, 1:2] >> np.arange(32, dtype=np.uint32)[None, :]) & np.uint32(1)).astype(bool)
    return u, plus


def augment(eig, rotate_deg=0.0, u=None, flip_cols=(), plus=None):
    """The two loops in fp64: ``eig [N, K]``; a rotation when ``rotate_deg != 0`` with the uniforms ``u [N]``; then, for the columns
    ``flip_cols``, the product with +1 where ``plus [N, len(flip_cols)]`` holds and -1 where not.  Returns ``(out [N, K] fp64, 1 - sine^2 [N])``
    (ones without a rotation): where that is small the reference's fp32 square root has lost digits already."""
    x = np.asarray(eig, dtype=np.float64)
    out = x.copy()
    safe = np.ones(x.shape[0])
    if rotate_deg != 0:
        angle = (np.asarray(u, dtype=np.float64) - 0.5) * 2 * rotate_deg
        sine = np.sin(angle * math.pi / 180)
        safe = 1 - sine ** 2
        cos = safe ** 0.5
        out[:, 1] = cos * x[:, 1] + sine * x[:, 2]
        out[:, 2] = cos * x[:, 2] - sine * x[:, 1]
    flip_cols = list(flip_cols)
    if flip_cols:
        sign = np.where(np.asarray(plus, dtype=bool), 1.0, -1.0).reshape(x.shape[0], len(flip_cols))
        out[:, flip_cols] = sign * out[:, flip_cols]                  # a product: 0 -> -0 under a minus sign, as torch.mul
    return out, safe


def same_bits(a, b) -> bool:
    """fp32 arrays equal bit for bit (-0.0 is not +0.0)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
