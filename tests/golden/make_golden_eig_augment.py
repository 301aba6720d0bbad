#!/usr/bin/env python3
"""Generate g20_eig_augment.npz by IMPORTING the reference's two training-loop modules (see make_golden.py for the rules: arrays only, no
reference source or bytecode).

    python tests/golden/make_golden_eig_augment.py            # rewrites g20_eig_augment.npz

``train_epoch`` of train/train_molecules_graph_regression.py (the sign flip of its lines 29-33) and of
train/train_superpixels_graph_classification.py (the rotation of lines 29-37, the sign flip of column 2 of lines 38-42) each run ONE batch:
a 40-node, K = 6 fake graph object (``ndata`` / ``edata`` dictionaries are all the loops touch), a stub model whose ``forward`` records
``batch_graphs.ndata['eig']`` as the model sees it, a stub optimizer, and ``torch.rand`` wrapped so that every uniform the loop draws is
recorded.  Stored per configuration: ``eig`` in, every drawn uniform in call order (``u0``, ``u1``), and ``eig`` as the model saw it.
Configurations: molecules ``flip=True``; superpixels ``(augmentation, flip)`` = (30, False), (0, True), (30, True), ``distortion`` 0.

``train/metrics.py`` needs scikit-learn for metrics the two loops never call: replaced by an empty module where it is not installed."""
import importlib
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as mg

torch.set_num_threads(1)

N, K, F_IN = 40, 6, 3
CONFIGS = (("molecules_flip", "molecules", dict(flip=True)),
           ("superpixels_rot30", "superpixels", dict(augmentation=30, flip=False, distortion=0)),
           ("superpixels_flip", "superpixels", dict(augmentation=0, flip=True, distortion=0)),
           ("superpixels_rot30_flip", "superpixels", dict(augmentation=30, flip=True, distortion=0)))
MODULES = {"molecules": "train.train_molecules_graph_regression", "superpixels": "train.train_superpixels_graph_classification"}


def _placeholder_modules():
    for name in ("sklearn", "sklearn.metrics"):
        try:
            importlib.import_module(name)
        except Exception:
            mod = types.ModuleType(name)
            mod.__getattr__ = lambda attr: type(attr, (), {})
            sys.modules[name] = mod


class _Model(torch.nn.Module):
    """Records the eigenvectors the forward pass is handed; scores and loss are whatever lets the loop's bookkeeping run."""

    def __init__(self, n_out):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(n_out))
        self.seen = []

    def forward(self, g, h, e, snorm_n, snorm_e):
        self.seen.append(g.ndata["eig"].detach().clone())
        return self.w.unsqueeze(0) * torch.ones(2, 1)

    def loss(self, scores, targets):
        return scores.sum()


class _Optimizer:
    def zero_grad(self):
        pass

    def step(self):
        pass


def _eig_in(seed):
    gen = torch.Generator().manual_seed(seed)
    eig = torch.randn(N, K, generator=gen)
    eig[7, 1] = eig[11, 4] = 0.0                                              # zeros: a flipped zero is -0.0
    eig[12:20, 2] = 0.0
    return eig


def main():
    mg._install_stubs()
    _placeholder_modules()
    out = {"cases": np.array([c[0] for c in CONFIGS])}
    real_rand = torch.rand
    for i, (case, which, kw) in enumerate(CONFIGS):
        mod = importlib.import_module(MODULES[which])
        eig = _eig_in(2000 + i)
        gen = torch.Generator().manual_seed(2100 + i)
        graph = types.SimpleNamespace(ndata={"feat": torch.randn(N, F_IN, generator=gen), "eig": eig.clone()},
                                      edata={"feat": torch.randn(2 * N, 1, generator=gen)})
        classes = which == "superpixels"
        targets = torch.zeros(2, dtype=torch.int64) if classes else torch.zeros(2, 1)
        loader = [(graph, targets, torch.ones(N, 1), torch.ones(2 * N, 1))]
        model, drawn = _Model(4 if classes else 1), []

        def recording_rand(*args, **kwargs):
            u = real_rand(*args, **kwargs)
            drawn.append(u.clone())
            return u

        torch.manual_seed(2200 + i)
        torch.rand = recording_rand
        try:
            mod.train_epoch(model, _Optimizer(), torch.device("cpu"), loader, 0, **kw)
        finally:
            torch.rand = real_rand
        assert len(model.seen) == 1
        out[f"{case}/eig_in"], out[f"{case}/eig_seen"] = eig.numpy(), model.seen[0].numpy()
        out[f"{case}/augmentation"], out[f"{case}/flip"] = np.array(float(kw.get("augmentation", 0))), np.array(bool(kw["flip"]))
        out[f"{case}/n_draws"] = np.array(len(drawn))
        for j, u in enumerate(drawn):
            out[f"{case}/u{j}"] = u.numpy()
    path = os.path.join(HERE, "g20_eig_augment.npz")
    np.savez_compressed(path, **out)
    print("wrote g20_eig_augment.npz:", sum(v.nbytes for v in out.values()), "bytes of arrays,", os.path.getsize(path), "on disk")


if __name__ == "__main__":
    main()
