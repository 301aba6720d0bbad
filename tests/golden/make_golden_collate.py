#!/usr/bin/env python3
"""Generate g19_collate.npz by IMPORTING the reference's data modules (see make_golden.py for the rules: arrays only, no reference source
or bytecode).

    python tests/golden/make_golden_collate.py            # rewrites g19_collate.npz

The five ``collate`` methods (data/molecules.py:219-230, data/SBMs.py:167-179, data/HIV.py:113-125, data/PCBA.py:266-278,
data/superpixels.py:316-330) are called unbound -- none reads ``self`` -- on the dozen fake samples of tests/collate_ref.py::fake_samples.
DGL is not installed: ``dgl.batch`` is a RECORDING stub that concatenates the samples' nodes and edges in sample order, shifts the node
ids by the nodes before and concatenates ndata / edata -- DGL 0.4's documented meaning, fixed here by definition like the mailbox order
of make_golden.py.  Stored per dataset: the reference's ``labels``, ``snorm_n``, ``snorm_e`` and the stub's concatenation.

All five modules import under the stubs: ``data/HIV.py`` and ``data/PCBA.py`` need ``ogb``, ``networkx``, ``tqdm``, ``pandas`` and
``dgl.data.utils`` only for downloading and reading the datasets; whichever of them is not installed is replaced by an empty module whose
attributes are placeholders."""
import importlib
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))          # tests/: collate_ref

import numpy as np
import torch

import make_golden as mg
from collate_ref import DATASETS, fake_samples

torch.set_num_threads(1)

CLASSES = {"molecules": "MoleculeDataset", "SBMs": "SBMsDataset", "HIV": "HIVDataset", "PCBA": "PCBADataset", "superpixels": "SuperPixDataset"}
SEEDS = {name: 1900 + i for i, name in enumerate(DATASETS)}


def _placeholder_modules():
    for name in ("ogb", "ogb.graphproppred", "ogb.utils", "ogb.utils.url", "ogb.io", "ogb.io.read_graph_dgl", "networkx", "tqdm", "pandas",
                 "dgl.data", "dgl.data.utils"):
        try:
            importlib.import_module(name)
        except Exception:
            mod = types.ModuleType(name)
            mod.__getattr__ = lambda attr: type(attr, (), {})
            sys.modules[name] = mod


class _Graph:
    def __init__(self, g):
        self.src, self.dst, self.n = torch.from_numpy(g["src"]), torch.from_numpy(g["dst"]), int(g["num_nodes"])
        self.ndata = {k: torch.from_numpy(np.asarray(v)) for k, v in g["ndata"].items()}
        self.edata = {k: torch.from_numpy(np.asarray(v)) for k, v in g["edata"].items()}

    def number_of_nodes(self):
        return self.n

    def number_of_edges(self):
        return self.src.numel()


def _recording_batch(graphs):
    off, src, dst = 0, [], []
    for g in graphs:
        src.append(g.src + off)
        dst.append(g.dst + off)
        off += g.n
    return types.SimpleNamespace(src=torch.cat(src), dst=torch.cat(dst), num_nodes=off,
                                 ndata={k: torch.cat([g.ndata[k] for g in graphs]) for k in graphs[0].ndata},
                                 edata={k: torch.cat([g.edata[k] for g in graphs]) for k in graphs[0].edata})


def main():
    mg._install_stubs()
    _placeholder_modules()
    sys.modules["dgl"].batch = _recording_batch
    out = {"datasets": np.array(DATASETS)}
    for name in DATASETS:
        mod = importlib.import_module("data." + name)
        samples = []
        for g, y in fake_samples(name, SEEDS[name]):
            samples.append((_Graph(g), y if name in ("molecules", "superpixels") else torch.from_numpy(np.asarray(y))))
        batched, labels, snorm_n, snorm_e = getattr(mod, CLASSES[name]).collate(None, samples)
        out[f"{name}/seed"] = np.array(SEEDS[name])
        out[f"{name}/labels"], out[f"{name}/snorm_n"], out[f"{name}/snorm_e"] = labels.numpy(), snorm_n.numpy(), snorm_e.numpy()
        out[f"{name}/src"], out[f"{name}/dst"], out[f"{name}/num_nodes"] = batched.src.numpy(), batched.dst.numpy(), np.array(batched.num_nodes)
        for k, v in batched.ndata.items():
            out[f"{name}/ndata::{k}"] = v.numpy()
        for k, v in batched.edata.items():
            out[f"{name}/edata::{k}"] = v.numpy()
    path = os.path.join(HERE, "g19_collate.npz")
    np.savez_compressed(path, **out)
    print("wrote g19_collate.npz:", sum(v.nbytes for v in out.values()), "bytes of arrays,", os.path.getsize(path), "on disk")


if __name__ == "__main__":
    main()
