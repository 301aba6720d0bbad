"""CPU restatement, in numpy fp64, of the superpixel graph construction of the reference's ``data/superpixels.py`` -- ``sigma``,
``compute_adjacency_matrix_images``, ``compute_edges_list`` with the self-edge removal of ``SuperPixDGL._prepare`` (:17-69, :139-145) -- generalised
to k neighbours, and of ``sort_eig`` (:371-420).  Pinned to the reference by fixture G15 (tests/test_superpixels_cpu.py).

The neighbour rule: with n >= k + 2 nodes, the n - 1 other nodes of row i are ranked by A descending, equal values by lower column; the reference's
``np.argpartition(A, n - 10)[:, n - 9:-1]`` keeps ranks 1 .. 8 (``skip_nearest``), a plain k-NN ranks 0 .. k - 1.  2 <= n <= k + 1: every other node in
ascending order.  n == 1: one self-loop of value 0.

``sort_eig``: the reference's two exchanging arms run ``eigs[:, 1] = eig2; eigs[:, 2] = eig1`` with ``eig1`` a view of column 1, so what they leave
is the OLD COLUMN 2 IN BOTH COLUMNS (column 1 is lost), not an exchange.  The fixture records it and this restatement states it that way."""
import numpy as np


def pairwise(p: np.ndarray) -> np.ndarray:
    """[n, n] Euclidean distances of the rows of p [n, C], the squares summed in ascending channel order (scipy's cdist)."""
    p = np.asarray(p, dtype=np.float64).reshape(p.shape[0], -1)
    s = np.zeros((p.shape[0], p.shape[0]))
    for c in range(p.shape[1]):
        d = p[:, None, c] - p[None, :, c]
        s = s + d * d
    return np.sqrt(s)


def sigma(d: np.ndarray, k: int = 8) -> np.ndarray:
    """[n, 1]: (sum of the k + 1 smallest entries of every row, the zero diagonal included) / k + 1e-8; 1 + 1e-8 for n < k + 1 (sigma()'s
    ValueError branch).  The k + 1 terms are added in numpy's own order -- np.partition's placement, read backwards, summed by ``sum`` -- as
    the reference adds them: a one-ulp change of sigma moves an entry of A by |log A| ulps, which in the far tail of a 150-node graph
    (A ~ 1e-76) is more than the fixture's rtol of 1e-13 allows (adding in ascending order, as the kernel does, gave 1.14e-13 on one of
    its entries)."""
    n = d.shape[0]
    if n < k + 1:
        return np.full((n, 1), 1.0) + 1e-8
    low = np.partition(d, k, axis=1)[:, :k + 1][:, ::-1]
    return (low.sum(axis=1) / k).reshape(n, 1) + 1e-8


def adjacency(coord: np.ndarray, feat=None, k: int = 8) -> np.ndarray:
    """A [n, n] fp64 of compute_adjacency_matrix_images (``feat=None``: its use_feat=False)."""
    coord = np.asarray(coord, dtype=np.float64).reshape(-1, 2)
    c = pairwise(coord)
    if feat is not None:
        f = pairwise(np.asarray(feat, dtype=np.float64).reshape(coord.shape[0], -1))
        E = np.exp(-(c / sigma(c, k)) ** 2 - (f / sigma(f, k)) ** 2)
    else:
        E = np.exp(-(c / sigma(c, k)) ** 2)
    A = 0.5 * (E + E.T)
    A[np.diag_indices_from(A)] = 0
    return A


def edge_count(n: int, k: int = 8) -> int:
    if n < 1:
        raise ValueError("a graph has at least one node")
    return 1 if n == 1 else n * (n - 1 if n <= k + 1 else k)


def ranked(A: np.ndarray) -> np.ndarray:
    """[n, n - 1]: the other nodes of every row by A descending, equal values by lower column."""
    n = A.shape[0]
    out = np.empty((n, n - 1), dtype=np.int64)
    cols = np.arange(n)
    for i in range(n):
        others = cols[cols != i]
        out[i] = others[np.lexsort((others, -A[i, others]))]
    return out


def neighbours(A: np.ndarray, k: int = 8, skip_nearest: bool = True):
    """(dst [n, per_node] local column indices, value [n, per_node] fp64) in the edge order of the rule above."""
    n = A.shape[0]
    if n == 1:
        return np.zeros((1, 1), dtype=np.int64), np.zeros((1, 1))
    order = ranked(A)
    if n >= k + 2:
        lo = 1 if skip_nearest else 0
        dst = order[:, lo:lo + k]
    else:
        dst = np.sort(order, axis=1)
    return dst, np.take_along_axis(A, dst, axis=1)


def knn_graph(coord, sizes, feat=None, k: int = 8, skip_nearest: bool = True):
    """(src, dst int64 global ids, value fp64, list of per-graph A) of a batch: graph g owns the rows sum(sizes[:g]) .. of coord / feat."""
    coord = np.asarray(coord, dtype=np.float64)
    srcs, dsts, vals, As, off = [], [], [], [], 0
    for n in sizes:
        A = adjacency(coord[off:off + n], None if feat is None else np.asarray(feat)[off:off + n], k)
        d, v = neighbours(A, k, skip_nearest)
        srcs.append(np.repeat(np.arange(n), d.shape[1]) + off)
        dsts.append(d.reshape(-1) + off)
        vals.append(v.reshape(-1))
        As.append(A)
        off += n
    return np.concatenate(srcs), np.concatenate(dsts), np.concatenate(vals), As


def rank_gaps(A: np.ndarray, k: int = 8, skip_nearest: bool = True):
    """Per row of a graph with n >= k + 2 nodes, the relative gaps (a_hi - a_lo) / a_hi between rank 0 and rank 1 and between the last kept rank
    and the first one not kept (inf where every other node is kept or dropped): the margins by which the neighbour SET is decided."""
    n = A.shape[0]
    if n < k + 2:
        return np.full(n, np.inf), np.full(n, np.inf)
    v = np.take_along_axis(A, ranked(A), axis=1)
    rel = lambda hi, lo: np.where(hi > 0, (hi - lo) / np.where(hi > 0, hi, 1.0), 0.0)
    first = rel(v[:, 0], v[:, 1])
    last = k if skip_nearest else k - 1
    tail = rel(v[:, last], v[:, last + 1]) if last + 1 < n - 1 else np.full(n, np.inf)
    return first, tail


def sort_eig_scores(eig: np.ndarray, x: np.ndarray, y: np.ndarray):
    """(hor1, ver1, hor2, ver2) of get_scores for columns 1 and 2."""
    out = []
    for c in (1, 2):
        pos = eig[:, c] > 0
        out.append(abs(int(np.sum(np.where(x[pos] > 0.5, 1, -1)))))
        out.append(abs(int(np.sum(np.where(y[pos] > 0.5, 1, -1)))))
    return tuple(out)


def sort_eig_branch(eig: np.ndarray, x: np.ndarray, y: np.ndarray) -> int:
    """Which arm of sort_eig's if-chain a graph takes: 0 (hor1 is the maximum) and 1 (ver2) keep, 2 (ver1) and 3 (hor2) overwrite column 1 with column 2."""
    hor1, ver1, hor2, ver2 = sort_eig_scores(eig, x, y)
    m = max(hor1, ver2, ver1, hor2)
    return 0 if hor1 == m else 1 if ver2 == m else 2 if ver1 == m else 3


def sort_eig(eig: np.ndarray, x: np.ndarray, y: np.ndarray, sizes) -> np.ndarray:
    """A copy of eig [N, K] with columns 1 and 2 of every graph's rows as sort_eig leaves them."""
    out, off = np.array(eig, copy=True), 0
    for n in sizes:
        blk = out[off:off + n]
        if sort_eig_branch(blk, x[off:off + n], y[off:off + n]) >= 2:
            blk[:, 1] = blk[:, 2]
        off += n
    return out
