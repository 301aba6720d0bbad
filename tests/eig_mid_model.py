"""A numpy model of ``csrc/dgn_eig_mid.hip`` with the kernel's own index arithmetic: the packed lower triangle, the round-robin schedule,
the merged tile pass with its (row, offset) -> (P, Q) map, the rotation log and its backward replay.  The GPU cannot be used to hunt a
wrong index, so the arithmetic is held to the dense oracle here (tests/test_eig_mid_cpu.py); the model also gives the sweep counts that
DESIGN.md section 5 quotes beside the GPU's."""
import numpy as np

TOL2 = 1e-28


def pidx(i, j):
    hi, lo = np.maximum(i, j), np.minimum(i, j)
    return hi * (hi + 1) // 2 + lo


def build_packed(src, dst, n, norm):
    """(packed L of the padded m x m matrix, dsc): every edge j -> i adds -w to cell {i, j}, a self-loop -2w to its diagonal cell"""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    m = n + (n & 1)
    deg = np.clip(np.bincount(dst, minlength=n).astype(np.float64), 1, None)
    normalised = norm != "none"
    dsc = 1.0 / np.sqrt(deg) if normalised else deg
    A = np.zeros(m * (m + 1) // 2)
    w = (0.5 * dsc[dst]) * dsc[src] if normalised else np.full(src.size, 0.5)
    np.add.at(A, pidx(dst, src), np.where(src == dst, -2.0 * w, -w))
    i = np.arange(n)
    A[pidx(i, i)] += 1.0 if normalised else dsc
    return A, dsc


def schedule(m, r):
    """the step's m / 2 pairs (p < q) by pair slot, as the kernel's threads compute them"""
    t = np.arange(m // 2)
    x = np.where(t == 0, m - 1, (r + t) % (m - 1))
    y = np.where(t == 0, r, (r - t + (m - 1)) % (m - 1))
    return np.minimum(x, y), np.maximum(x, y)


def tile_map(npairs):
    """all unordered {P, Q} of a step, P == Q included: row P, offset c in [0, npairs / 2], Q = (P + c) mod npairs; an even npairs covers
    the offset npairs / 2 twice, so only its rows below npairs / 2 count"""
    hc = npairs // 2
    P, c = np.divmod(np.arange(npairs * (hc + 1)), hc + 1)
    keep = ~((npairs % 2 == 0) & (c == hc) & (P >= hc))
    P, c = P[keep], c[keep]
    Q = (P + c) % npairs
    assert P.size == npairs * (npairs + 1) // 2
    return P[c > 0], Q[c > 0]


def solve(A, n, max_sweeps=30):
    """diagonalise the packed matrix in place -> (sweeps, log): log[sweep][r] = t per pair slot (0: skipped pair or the idle slot)"""
    m = n + (n & 1)
    npairs = m // 2
    TP, TQ = tile_map(npairs)
    ii, jj = np.tril_indices(n, -1)
    offd, diag = pidx(ii, jj), pidx(np.arange(n), np.arange(n))
    norm2 = 2.0 * (A[offd] ** 2).sum() + (A[diag] ** 2).sum()
    log, sweeps = [], 0
    while True:
        steps = []
        for r in range(m - 1):
            p, q = schedule(m, r)
            apq, app, aqq = A[pidx(q, p)], A[pidx(p, p)], A[pidx(q, q)]
            live = apq != 0
            with np.errstate(divide="ignore", invalid="ignore"):
                theta = np.where(live, (aqq - app) / (2.0 * np.where(live, apq, 1.0)), 0.0)
            t = np.where(live, np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.hypot(theta, 1.0)), 0.0)
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            steps.append(t)
            p1, q1, p2, q2 = p[TP], q[TP], p[TQ], q[TQ]
            i00, i01, i10, i11 = pidx(p1, p2), pidx(p1, q2), pidx(q1, p2), pidx(q1, q2)
            b00, b01, b10, b11 = A[i00], A[i01], A[i10], A[i11]
            cP, sP, cQ, sQ = c[TP], s[TP], c[TQ], s[TQ]
            x0, y0 = cQ * b00 - sQ * b01, sQ * b00 + cQ * b01
            x1, y1 = cQ * b10 - sQ * b11, sQ * b10 + cQ * b11
            A[i00], A[i10] = cP * x0 - sP * x1, sP * x0 + cP * x1
            A[i01], A[i11] = cP * y0 - sP * y1, sP * y0 + cP * y1
            A[pidx(p, p)], A[pidx(q, q)], A[pidx(q, p)] = app - t * apq, aqq + t * apq, 0.0
        log.append(steps)
        sweeps += 1
        off2 = 2.0 * (A[offd] ** 2).sum()
        if not (off2 > TOL2 * norm2 and sweeps < max_sweeps):
            return sweeps, log


def replay(log, cols, n):
    """V e_c for the columns `cols`: the log applied backwards to unit vectors, [m, len(cols)]"""
    m = n + (n & 1)
    X = np.zeros((m, len(cols)))
    X[np.asarray(cols), np.arange(len(cols))] = 1.0
    for steps in reversed(log):
        for r in range(m - 2, -1, -1):
            p, q = schedule(m, r)
            t = steps[r]
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            xp, xq = X[p].copy(), X[q].copy()
            X[p] = c[:, None] * xp + s[:, None] * xq
            X[q] = -s[:, None] * xp + c[:, None] * xq
    return X


def eig_mid(src, dst, n, k, norm="none", max_sweeps=30):
    """(vec [n, k] fp32, val [k] fp64, sweeps) of one graph, as the kernel writes them"""
    A, dsc = build_packed(src, dst, n, "sym" if norm == "walk" else norm)
    sweeps, log = solve(A, n, max_sweeps)
    lam = A[pidx(np.arange(n), np.arange(n))]
    order = np.argsort(lam, kind="stable")                 # ties by column index
    kk = min(k, n)
    X = replay(log, order[:kk], n)[:n]
    if norm == "walk":
        X = X * dsc[:, None]
        X = X * (1.0 / np.sqrt(np.maximum((X * X).sum(0), 1e-300)))
    vec, val = np.zeros((n, k), dtype=np.float32), np.full(k, np.nan)
    vec[:, :kk], val[:kk] = X.astype(np.float32), lam[order[:kk]]
    return vec, val, sweeps


def split(b):
    """a synth batch -> list of per-graph (src, dst, n) with local node ids (numpy)"""
    src, dst, out, off = b["src"].numpy(), b["dst"].numpy(), [], 0
    for n in b["sizes"].tolist():
        m = (dst >= off) & (dst < off + n)
        out.append((src[m] - off, dst[m] - off, int(n)))
        off += n
    return out


def mid_graphs():
    """The test graphs of the 65-192-node solver as (name, (src, dst, n)): both sides of each class limit (the odd sizes have an idle slot),
    directed graphs, and the degenerate cases."""
    from dgn_amd import synth
    out = []
    for i, n in enumerate((65, 127, 128, 129, 191, 192)):
        out.append((f"sbm{n}", split(synth.sbm_batch(1, seed=40 + i, n_lo=n, n_hi=n))[0]))
    out += [(f"knn{i}", g) for i, g in enumerate(split(synth.knn_batch(3, seed=5, n_lo=85, n_hi=150)))]      # directed, symmetrised
    p = np.arange(192)
    out.append(("path192", (np.concatenate([p[:-1], p[1:]]), np.concatenate([p[1:], p[:-1]]), 192)))          # sparse, small gaps
    a = np.arange(40)
    rs, rd = np.concatenate([a, (a + 1) % 40]), np.concatenate([(a + 1) % 40, a])
    out.append(("rings2x40", (np.concatenate([rs, rs + 40]), np.concatenate([rd, rd + 40]), 80)))            # double eigenvalues throughout
    out.append(("edgeless70", (np.zeros(0, np.int64), np.zeros(0, np.int64), 70)))
    p = np.arange(65)
    out.append(("loop66", (np.concatenate([p[:-1], p[1:], [2]]), np.concatenate([p[1:], p[:-1], [2]]), 66)))  # a self-loop, an isolated node
    return out


def assert_unambiguous_clusters(w, k):
    """the comparison's cluster rule (eigenvalues closer than 1e-6 form one cluster) must not sit next to a gap of the test graph"""
    gaps = np.diff(w[:k + 1])
    assert not np.any((gaps > 1e-7) & (gaps < 1e-5)), gaps
