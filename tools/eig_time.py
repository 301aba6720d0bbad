#!/usr/bin/env python3
"""Time ``batch_eig(check=False)`` (one Jacobi workgroup per graph, csrc/dgn_eig_small.hip) against ``laplacian_eigvecs`` (bucketed
``torch.linalg.eigh``) on the same device tensors: ``molecule_batch(128)`` and ``molecule_batch(12000)``, k = 6, 'none' and 'sym'.
Per case: warm-up, then the median of ``--reps`` calls, each between two device synchronisations (host clock).  ``batch_eig`` is timed as a
data loader calls it, on a ``DGNGraph`` that exists already (the layer needs it anyway): host cumsum of the sizes, one small H2D copy, two
launches.  Also prints the largest difference of the eigenvector residuals so that the two are seen to solve the same problem.
usage: tools/eig_time.py [--reps 25] [--out profiles/eig_small_times.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: at least 20")
    import dgn_amd
    from dgn_amd import synth
    from dgn_amd.eig import laplacian_eig_small
    dev = torch.device("cuda:0")
    lines = [f"$ python tools/eig_time.py --reps {args.reps}    # {torch.cuda.get_device_name(0)}, k = 6, ms per call: median (min .. max)",
             f"{'batch':>22} {'norm':>5} {'batch_eig(check=False)':>28} {'laplacian_eigvecs':>28} {'ratio':>7} {'max sweeps':>10}"]
    for n_graphs in (128, 12000):
        b = synth.molecule_batch(n_graphs, seed=41, laplacian_eig=False)
        src, dst, sizes = b["src"].to(dev), b["dst"].to(dev), b["sizes"].tolist()
        graph = dgn_amd.DGNGraph(src, dst, int(b["num_nodes"]))
        off = torch.zeros(len(sizes) + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(b["sizes"].long(), 0)
        for norm in ("none", "sym"):
            new = timed(lambda: dgn_amd.batch_eig(graph, sizes, 6, norm, check=False), args.reps)
            old = timed(lambda: dgn_amd.laplacian_eigvecs(src, dst, sizes, 6, norm=norm), args.reps)
            status = laplacian_eig_small(graph, off.to(dev), 6, norm)[2]
            fmt = lambda t: f"{t[0]:9.3f} ({t[1]:.3f} .. {t[2]:.3f})"
            lines.append(f"{'molecule_batch(%d)' % n_graphs:>22} {norm:>5} {fmt(new):>28} {fmt(old):>28} {old[0] / new[0]:7.2f} {int(status.max()):10d}")
    text = "\n".join(lines) + "\nratio = laplacian_eigvecs / batch_eig (above 1: the Jacobi kernel is faster)\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
