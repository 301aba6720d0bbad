#!/usr/bin/env python3
"""Time ``batch_eig(check=False)`` (one Jacobi workgroup per graph, csrc/dgn_eig_small.hip) against ``laplacian_eigvecs`` (bucketed
``torch.linalg.eigh``) on the same device tensors: ``molecule_batch(128)`` and ``molecule_batch(12000)``, k = 6, 'none' and 'sym'; and
``batch_eig(check=False, mid=True)`` (csrc/dgn_eig_mid.hip for the graphs of 65 to 192 nodes) on ``sbm_batch(128)`` (PATTERN-sized, 44 to 188
nodes) and ``knn_batch(128)`` (CIFAR10-sized, 85 to 150 nodes).
Per case: warm-up, then the median of ``--reps`` calls, each between two device synchronisations (host clock).  ``batch_eig`` is timed as a
data loader calls it, on a ``DGNGraph`` that exists already (the layer needs it anyway): host cumsum of the sizes, one small H2D copy, two
launches.  Also prints the largest difference of the eigenvector residuals so that the two are seen to solve the same problem.
usage: tools/eig_time.py [--reps 25] [--only small|mid] [--out profiles/eig_small_times.txt] [--mid-out profiles/eig_mid_times.txt]"""
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


def table(title, cases, mid, reps):
    import dgn_amd
    from dgn_amd.eig import laplacian_eig_mid, laplacian_eig_small
    dev = torch.device("cuda:0")
    name = "batch_eig(check=False, mid=True)" if mid else "batch_eig(check=False)"
    lines = [title, f"{'batch':>22} {'norm':>5} {name:>34} {'laplacian_eigvecs':>28} {'ratio':>7} {'max sweeps':>10}"]
    for label, b in cases:
        src, dst, sizes = b["src"].to(dev), b["dst"].to(dev), b["sizes"].tolist()
        graph = dgn_amd.DGNGraph(src, dst, int(b["num_nodes"]))
        off = torch.zeros(len(sizes) + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(b["sizes"].long(), 0)
        for norm in ("none", "sym"):
            new = timed(lambda: dgn_amd.batch_eig(graph, sizes, 6, norm, check=False, mid=mid), reps)
            old = timed(lambda: dgn_amd.laplacian_eigvecs(src, dst, sizes, 6, norm=norm), reps)
            out, values, status = laplacian_eig_small(graph, off.to(dev), 6, norm)
            if mid:
                laplacian_eig_mid(graph, off.to(dev), 6, norm, out=out, values=values, status=status)
            fmt = lambda t: f"{t[0]:9.3f} ({t[1]:.3f} .. {t[2]:.3f})"
            lines.append(f"{label:>22} {norm:>5} {fmt(new):>34} {fmt(old):>28} {old[0] / new[0]:7.2f} {int(status.max()):10d}")
    return "\n".join(lines) + "\nratio = laplacian_eigvecs / batch_eig (above 1: the Jacobi kernels are faster)\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--only", choices=("small", "mid"), default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mid-out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: at least 20")
    from dgn_amd import synth
    head = f"$ python tools/eig_time.py --reps {args.reps}{' --only ' + args.only if args.only else ''}    # {torch.cuda.get_device_name(0)}, k = 6, ms per call: median (min .. max)"
    runs = []
    if args.only != "mid":
        cases = [("molecule_batch(%d)" % n, synth.molecule_batch(n, seed=41, laplacian_eig=False)) for n in (128, 12000)]
        runs.append((table(head, cases, False, args.reps), args.out))
    if args.only != "small":
        cases = [("sbm_batch(128)", synth.sbm_batch(128, seed=41)), ("knn_batch(128)", synth.knn_batch(128, seed=41))]
        text = table(head, cases, True, args.reps)
        n_mid = [sum(1 for n in b["sizes"].tolist() if 64 < n <= 192) for _, b in cases]
        text += (f"graphs of 65 .. 192 nodes: {n_mid[0]} of 128 (sbm), {n_mid[1]} of 128 (knn); log workspace at max_sweeps = 30: "
                 f"{n_mid[0] * 30 * 191 * 96 * 8 / 1e6:.0f} MB / {n_mid[1] * 30 * 191 * 96 * 8 / 1e6:.0f} MB, allocated and freed inside every call\n")
        runs.append((text, args.mid_out))
    for text, path in runs:
        print(text, end="")
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
