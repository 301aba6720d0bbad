#!/usr/bin/env python3
"""Generate ``g14_pos_enc.npz`` by IMPORTING the reference (build container only, like make_golden.py, whose stub
modules this file reuses; numeric arrays only, no reference source or bytecode is copied).

    python tests/golden/make_golden_eig.py

The UNMODIFIED ``positional_encoding`` of ``realworld_benchmark/data/molecules.py`` (:18-32) is driven with a fake graph
that supplies the three DGL methods it calls -- the way ``make_golden.py::g9_laplacian`` drives ``get_eig``.  The routine
solves with ``np.linalg.eig`` (dense, exact), so nothing is intercepted: stored are its ``pos_enc`` (fp32 columns
1 .. pos_enc_dim of the sym-normalised Laplacian's eigenvectors), and, restated here from the same three methods, the
dense ``L`` and its sorted eigenvalues.  Five connected symmetric graphs of 5 .. 40 nodes (a random spanning tree plus a few extra edges
each); the tests compare eigen-SUBSPACES, clustered at 1e-6.
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (sets sys.dont_write_bytecode before anything of the reference is imported)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def g14_pos_enc(out, pos_enc_dim=4):
    import scipy.sparse as sp
    dgl = sys.modules["dgl"]
    dgl.backend = types.SimpleNamespace(asnumpy=lambda t: t.numpy() if torch.is_tensor(t) else np.asarray(t))
    dgl.DGLGraph = object
    import data.molecules as M

    class G:
        def __init__(self, src, dst, n):
            self.src, self.dst, self.n, self.ndata = np.asarray(src), np.asarray(dst), n, {}

        def number_of_nodes(self):
            return self.n

        def in_degrees(self):
            return torch.from_numpy(np.bincount(self.dst, minlength=self.n))

        def adjacency_matrix_scipy(self, return_edge_ids=False):
            return sp.coo_matrix((np.ones(len(self.src)), (self.dst, self.src)), shape=(self.n, self.n)).tocsr()

    rng = np.random.default_rng(14)
    graphs = []
    for n in (5, 12, 26, 33, 40):
        und = [(int(rng.integers(0, v)), v) for v in range(1, n)]           # a random spanning tree: connected
        for _ in range(4):
            a, b = sorted(int(x) for x in rng.integers(0, n, 2))
            if a != b and (a, b) not in und:
                und.append((a, b))
        und = np.asarray(und)
        graphs.append((np.concatenate([und[:, 0], und[:, 1]]), np.concatenate([und[:, 1], und[:, 0]]), n))
    out["n_graphs"] = np.array(len(graphs))
    out["pos_enc_dim"] = np.array(pos_enc_dim)
    for i, (src, dst, n) in enumerate(graphs):
        g = M.positional_encoding(G(src, dst, n), pos_enc_dim)
        A = g.adjacency_matrix_scipy().toarray().astype(float)
        d = np.clip(np.bincount(dst, minlength=n), 1, None) ** -0.5
        L = np.eye(n) - d[:, None] * A * d[None, :]
        out[f"g{i}/src"], out[f"g{i}/dst"], out[f"g{i}/n"] = src, dst, np.array(n)
        out[f"g{i}/pos_enc"] = g.ndata["pos_enc"].numpy()
        out[f"g{i}/L"] = L
        out[f"g{i}/eigval"] = np.sort(np.linalg.eigvalsh(L))


def main():
    mg._install_stubs()
    out = {}
    g14_pos_enc(out)
    np.savez_compressed(os.path.join(HERE, "g14_pos_enc.npz"), **out)
    print("wrote g14_pos_enc.npz:", sum(v.nbytes for v in out.values()), "bytes of arrays")


if __name__ == "__main__":
    main()
