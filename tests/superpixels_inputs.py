"""The inputs the superpixel GPU tests share with the CPU test of their rank gaps (tests/test_superpixels_cpu.py): one batch of graph sizes on
either side of every branch of the kernel -- sigma's (k + 1 nodes), the neighbour rule's (1, k + 1, k + 2) and the 64-column groups of a wave
(63 / 64 / 65, 128 / 129, 256) -- with uniform random coordinates and features that fp32 holds exactly."""
import numpy as np

SIZES = [1, 2, 8, 9, 10, 11, 63, 64, 65, 128, 129, 150, 256]
SEED = 2015


def points(sizes, channels, seed=SEED):
    """(coord [N, 2] fp64, feat [N, channels] fp64 or None) for graphs of ``sizes`` nodes."""
    rng = np.random.default_rng(seed)
    N = int(sum(sizes))
    coord = rng.random((N, 2), dtype=np.float32).astype(np.float64)
    feat = rng.random((N, channels), dtype=np.float32).astype(np.float64) if channels else None
    return coord, feat


def batch(channels):
    coord, feat = points(SIZES, channels)
    return coord, feat, list(SIZES)


def grid(side=12):
    """A side x side regular grid in the unit square: many exactly equal distances."""
    t = (np.arange(side, dtype=np.float64) + 0.5) / side
    x, y = np.meshgrid(t, t, indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1)], axis=1)
