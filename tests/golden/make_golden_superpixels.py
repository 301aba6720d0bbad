#!/usr/bin/env python3
"""Generate ``g15_superpixels.npz`` by IMPORTING the reference (build container only, like make_golden.py, whose stub
modules this file reuses; numeric arrays only, no reference source or bytecode is copied).

    python tests/golden/make_golden_superpixels.py

The UNMODIFIED ``compute_adjacency_matrix_images`` / ``compute_edges_list`` and ``sort_eig`` of ``realworld_benchmark/data/superpixels.py``
(:17-69, :371-420) are called as ``SuperPixDGL._prepare`` and ``get_eig`` call them.  Stored per graph: the inputs (``coord`` already divided
by the image size, ``feat`` where the adjacency uses the mean pixel values), ``A`` (graphs over 40 nodes: its first 8 rows, ``A_head``),
``knns`` and ``knn_values`` -- for n > 1 with the self-edge of every row removed the way ``_prepare`` does (:145).  Coordinates and features
are uniform random numbers that fp32 holds exactly.  For ``sort_eig``: (eig, feat) pairs built so that every arm of its if-chain is taken, a
few random ones, and the eig it leaves behind.  (Its two "exchanging" arms assign ``eigs[:, 1] = eig2`` and then ``eigs[:, 2] = eig1`` with
``eig1`` a VIEW of column 1: what they leave is column 2 in both columns.  The fixture records that, as the reference's datasets hold it.)
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (sets sys.dont_write_bytecode before anything of the reference is imported)

import numpy as np  # noqa: E402
import torch  # noqa: E402

GRAPHS = ((1, 0), (2, 1), (8, 3), (9, 0), (9, 3), (10, 0), (10, 1), (11, 3), (40, 1), (75, 0), (150, 3))   # (nodes, channels)
A_FULL_MAX, A_HEAD = 40, 8


def knn_cases(SP, out):
    rng = np.random.default_rng(15)
    out["n_graphs"] = np.array(len(GRAPHS))
    for i, (n, C) in enumerate(GRAPHS):
        coord = rng.random((n, 2), dtype=np.float32).astype(np.float64)
        feat = rng.random((n, max(C, 1)), dtype=np.float32).astype(np.float64)
        A = SP.compute_adjacency_matrix_images(coord, feat, use_feat=C > 0)
        knns, values = SP.compute_edges_list(A)
        if n > 9:                                   # (the branch for n <= 9 has removed the self-edges already)
            keep = knns != np.arange(n)[:, None]
            assert keep.all(), "a row of the reference lists the node itself"
        out[f"g{i}/n"], out[f"g{i}/channels"] = np.array(n), np.array(C)
        out[f"g{i}/coord"] = coord
        if C:
            out[f"g{i}/feat"] = feat
        out[f"g{i}/A" if n <= A_FULL_MAX else f"g{i}/A_head"] = A if n <= A_FULL_MAX else A[:A_HEAD]
        out[f"g{i}/knns"], out[f"g{i}/knn_values"] = np.asarray(knns, dtype=np.int64), np.asarray(values, dtype=np.float64)


def _sort_eig_inputs():
    """(eig [n, 7] fp32, x, y fp32) cases: four with the signs of columns 1 and 2 laid out for one arm each, then random ones."""
    rng = np.random.default_rng(151)
    n = 12
    right, up = np.arange(n) >= n // 2, np.arange(n) % 2 == 1
    few_h = np.zeros(n, dtype=bool); few_h[[n // 2, n // 2 + 1]] = True          # two right nodes, one up one down: hor 2, ver 0
    few_v = np.zeros(n, dtype=bool); few_v[[1, n // 2 + 1]] = True              # two up nodes, one left one right: ver 2, hor 0
    layouts = ((right, up), (few_h, up), (up, few_h), (few_v, right))          # positive entries of (column 1, column 2)
    cases = []
    for p1, p2 in layouts:
        eig = np.abs(rng.standard_normal((n, 7))).astype(np.float32) + 0.01
        eig[:, 1] *= np.where(p1, 1, -1)
        eig[:, 2] *= np.where(p2, 1, -1)
        x = np.where(right, 0.75, 0.25).astype(np.float32) + rng.uniform(-0.2, 0.2, n).astype(np.float32)
        y = np.where(up, 0.75, 0.25).astype(np.float32) + rng.uniform(-0.2, 0.2, n).astype(np.float32)
        cases.append((eig, x, y))
    for n in (3, 40, 75, 150):
        cases.append((rng.standard_normal((n, 7)).astype(np.float32), rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)))
    return cases


def sort_eig_cases(SP, out):
    cases = _sort_eig_inputs()
    out["n_sort"] = np.array(len(cases))
    for i, (eig, x, y) in enumerate(cases):
        n = eig.shape[0]
        feat = np.zeros((n, 5), dtype=np.float32)
        feat[:, 3], feat[:, 4] = x, y
        g = types.SimpleNamespace(ndata={"feat": torch.from_numpy(feat.copy()), "eig": torch.from_numpy(eig.copy())})
        res = SP.sort_eig(g)
        out[f"s{i}/eig"], out[f"s{i}/x"], out[f"s{i}/y"] = eig, x, y
        out[f"s{i}/sorted"] = res.ndata["eig"].numpy().copy()


def main():
    mg._install_stubs()
    import data.superpixels as SP
    out = {}
    knn_cases(SP, out)
    sort_eig_cases(SP, out)
    path = os.path.join(HERE, "g15_superpixels.npz")
    np.savez_compressed(path, **out)
    print("wrote g15_superpixels.npz:", sum(v.nbytes for v in out.values()), "bytes of arrays,", os.path.getsize(path), "on disk")


if __name__ == "__main__":
    main()
