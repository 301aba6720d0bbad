#!/usr/bin/env python3
"""Time ``knn_graph(check=False)`` (one workgroup per graph, csrc/dgn_superpixels.hip) on 128 and on 8 192 CIFAR10-sized graphs (85 to 150
nodes, k = 8, the reference's neighbour choice), coordinates only and with 3 feature channels, against the numpy restatement of the
reference's per-graph host code (tests/superpixels_oracle.py: cdist, partition, exp, ranking) on the same inputs, and ``sort_eig`` on the
same batches.  Per case: warm-up, then the median of ``--reps`` calls, each between two device synchronisations (host clock); ``knn_graph``
is timed as a data loader calls it, with host sizes: two cumsums, two small H2D copies, one launch.  The restatement is timed on the first
128 graphs (median of ``--host-reps`` passes) and reported per graph.
usage: tools/superpixels_time.py [--reps 25] [--out profiles/superpixels_times.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def host_timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: at least 20")
    import dgn_amd
    import superpixels_oracle as so
    dev = torch.device("cuda:0")
    fmt = lambda t: f"{t[0]:9.3f} ({t[1]:.3f} .. {t[2]:.3f})"
    lines = [f"$ python tools/superpixels_time.py --reps {args.reps}    # {torch.cuda.get_device_name(0)}, k = 8, skip_nearest, ms per call: median (min .. max)",
             f"{'graphs':>7} {'nodes':>8} {'channels':>8} {'knn_graph(check=False)':>30} {'us / graph':>10} {'numpy restatement us / graph':>28} {'ratio':>7} "
             f"{'sort_eig':>28}"]
    for G in (128, 8192):
        rng = np.random.default_rng(41)
        sizes = rng.integers(85, 151, G).tolist()
        N = int(sum(sizes))
        coord = rng.random((N, 2), dtype=np.float32)
        feat = rng.random((N, 3), dtype=np.float32)
        eig = torch.from_numpy(rng.standard_normal((N, 7)).astype(np.float32)).to(dev)
        c_dev, f_dev = torch.from_numpy(coord).to(dev), torch.from_numpy(feat).to(dev)
        head, n_head = sizes[:128], int(sum(sizes[:128]))
        srt = timed(lambda: dgn_amd.sort_eig(eig, c_dev, sizes), args.reps)
        for channels in (0, 3):
            f = f_dev if channels else None
            new = timed(lambda: dgn_amd.knn_graph(c_dev, sizes, f, check=False), args.reps)
            host = host_timed(lambda: so.knn_graph(coord[:n_head].astype(np.float64), head, feat[:n_head].astype(np.float64) if channels else None),
                              args.host_reps)
            per_new, per_host = new[0] * 1e3 / G, host * 1e3 / len(head)
            lines.append(f"{G:7d} {N:8d} {channels:8d} {fmt(new):>30} {per_new:10.2f} {per_host:28.1f} {per_host / per_new:7.0f} {fmt(srt):>28}")
    text = "\n".join(lines) + "\nratio = numpy restatement / knn_graph, per graph (the restatement: one host thread, first 128 graphs of the batch)\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
