"""Numpy restatement (the graph norms apart: see ``snorm``) of the reference's five ``collate`` methods (data/molecules.py:219-230, data/SBMs.py:167-179, data/HIV.py:113-125,
data/PCBA.py:266-278, data/superpixels.py:316-330) and of what they get from DGL 0.4's ``dgl.batch``: the samples' nodes and edges
concatenated in sample order, node ids shifted by the nodes before, ndata / edata concatenated.  Pinned to the reference by
tests/golden/g19_collate.npz (tests/test_collate_cpu.py); the device collate (dgn_amd/data.py) is compared with it bit for bit.

A graph is a dict ``src``, ``dst`` (local ids, edge-id order), ``num_nodes``, ``ndata``, ``edata`` (name -> array); a sample is a
``(graph, label)`` pair."""
import numpy as np

DATASETS = ("molecules", "SBMs", "HIV", "PCBA", "superpixels")


def dgl_batch(graphs):
    sizes = np.asarray([int(g["num_nodes"]) for g in graphs], dtype=np.int64)
    edges = np.asarray([len(g["src"]) for g in graphs], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)])
    cat = lambda xs, like: np.concatenate(xs) if xs else like
    src = cat([np.asarray(g["src"], dtype=np.int64) + off[i] for i, g in enumerate(graphs)], np.zeros(0, dtype=np.int64))
    dst = cat([np.asarray(g["dst"], dtype=np.int64) + off[i] for i, g in enumerate(graphs)], np.zeros(0, dtype=np.int64))
    ndata = {k: np.concatenate([np.asarray(g["ndata"][k]) for g in graphs]) for k in (graphs[0]["ndata"] if graphs else {})}
    edata = {k: np.concatenate([np.asarray(g["edata"][k]) for g in graphs]) for k in (graphs[0]["edata"] if graphs else {})}
    return dict(src=src, dst=dst, num_nodes=int(off[-1]), batch_num_nodes=sizes, batch_num_edges=edges, ndata=ndata, edata=edata)


def snorm(sizes):
    """The reference's expression itself, evaluated by torch on the host as the reference evaluates it.  Not restated in numpy on purpose:
    torch's CPU square root and numpy's differ in the last bit for some sizes (66 is the first), and the value a training run of the
    reference sees is torch's."""
    import torch
    if len(sizes) == 0:
        return np.zeros((0, 1), dtype=np.float32)
    tab = [torch.FloatTensor(int(size), 1).fill_(1. / float(size)) for size in sizes]
    return torch.cat(tab).sqrt().numpy()


def collate(dataset, samples):
    """``(batched_graph, labels, snorm_n, snorm_e)`` of the reference's ``collate`` of ``dataset`` (one of DATASETS)."""
    graphs, labels = [s[0] for s in samples], [s[1] for s in samples]
    if dataset == "molecules":
        labels = np.array(labels)[:, None]                          # torch.tensor(np.array(labels)).unsqueeze(1)
    elif dataset in ("SBMs", "HIV"):
        labels = np.concatenate([np.asarray(y) for y in labels]).astype(np.int64)      # torch.cat(labels).long()
    elif dataset == "PCBA":
        labels = np.concatenate([np.asarray(y)[None] for y in labels])                 # torch.cat([label.unsqueeze(0) ...])
    elif dataset == "superpixels":
        labels = np.array(labels)
        graphs = [dict(g, ndata=dict(g["ndata"], feat=np.asarray(g["ndata"]["feat"], dtype=np.float32)),
                       edata=dict(g["edata"], feat=np.asarray(g["edata"]["feat"], dtype=np.float32))) for g in graphs]
    else:
        raise KeyError(dataset)
    snorm_n = snorm([g["num_nodes"] for g in graphs])
    snorm_e = snorm([len(g["src"]) for g in graphs])
    return dgl_batch(graphs), labels, snorm_n, snorm_e


def fake_samples(dataset, seed, n_graphs=12):
    """A dozen small samples shaped like ``dataset``'s (every graph has an edge: the reference's ``1. / float(size)`` divides by the
    edge count).  The SAME generator feeds tests/golden/make_golden_collate.py and the tests."""
    rng = np.random.default_rng(seed)
    sizes = [1, 2, 3, 9, 17, 5] + [int(x) for x in rng.integers(2, 24, max(0, n_graphs - 6))]
    samples = []
    for n in sizes[:n_graphs]:
        e = int(rng.integers(1, 3 * n + 1))
        g = dict(src=rng.integers(0, n, e), dst=rng.integers(0, n, e), num_nodes=n, ndata={}, edata={})
        g["ndata"]["eig"] = rng.standard_normal((n, 4)).astype(np.float32)
        if dataset == "molecules":
            g["ndata"]["feat"], g["edata"]["feat"] = rng.integers(0, 28, n), rng.integers(0, 4, e)
            y = np.float32(rng.standard_normal())
        elif dataset == "SBMs":
            g["ndata"]["feat"], g["edata"]["feat"] = rng.integers(0, 3, n), np.ones((e, 1), dtype=np.float32)
            y = rng.integers(0, 2, n).astype(np.int16)
        elif dataset == "HIV":
            g["ndata"]["feat"], g["edata"]["feat"] = rng.integers(0, 5, (n, 9)), rng.integers(0, 3, (e, 3))
            y = rng.integers(0, 2, 1)
        elif dataset == "PCBA":
            g["ndata"]["feat"], g["edata"]["feat"] = rng.integers(0, 5, (n, 9)), rng.integers(0, 3, (e, 3))
            y = np.where(rng.random(7) < 0.3, np.nan, rng.integers(0, 2, 7)).astype(np.float32)
        else:
            g["ndata"]["feat"], g["edata"]["feat"] = rng.random((n, 5)).astype(np.float16), rng.random((e, 1)).astype(np.float16)
            y = int(rng.integers(0, 10))
        samples.append((g, y))
    return samples
