"""CPU restatement of the node-classification tail, in plain torch, dtype-generic (fp32 / fp64): the batch-balanced cross-entropy of the
reference's ``DGNNet.loss`` (nets/SBMs_node_classification/dgn_net.py:67-81), its gradient in closed form, and the confusion matrix and
accuracy of ``accuracy_SBM`` (train/metrics.py:37-54).  Labels < 0 mark rows that do not exist (padding): they are ignored everywhere and
their gradient rows are zero.  Pinned to the reference by fixture G12 (tests/test_node_ce_oracle_vs_golden.py)."""
import numpy as np
import torch


def class_counts(labels: torch.Tensor, n_classes: int) -> torch.Tensor:
    valid = labels >= 0
    return torch.bincount(labels[valid], minlength=n_classes)


def class_weights(labels: torch.Tensor, n_classes: int, dtype=torch.float64) -> torch.Tensor:
    """(V - count_c) / V for the classes present, 0 for the others (integer subtract, convert, divide: dgn_net.py:74-75)."""
    count = class_counts(labels, n_classes)
    V = int(count.sum())
    if V == 0:
        return torch.zeros(n_classes, dtype=dtype)
    w = (V - count).to(dtype) / torch.tensor(float(V), dtype=dtype)
    return w * (count > 0).to(dtype)


def loss_and_grad(scores: torch.Tensor, labels: torch.Tensor, n_classes: int):
    """(loss 0-dim, d loss / d scores [N, C]) in ``scores.dtype``.  One class only: nan (0 / 0), padding rows' gradient still 0;
    no valid row: 0, 0."""
    dtype = scores.dtype
    valid = labels >= 0
    grad = torch.zeros_like(scores)
    if int(valid.sum()) == 0:
        return torch.zeros((), dtype=dtype), grad
    x, y = scores[valid], labels[valid]
    count = class_counts(labels, n_classes).to(dtype)
    w = class_weights(labels, n_classes, dtype)
    den = (w * count).sum()
    lse = torch.logsumexp(x, dim=1)
    wy = w[y]
    loss = (wy * (lse - x.gather(1, y[:, None])[:, 0])).sum() / den
    onehot = torch.zeros_like(x)
    onehot.scatter_(1, y[:, None], 1.0)
    grad[valid] = wy[:, None] * (torch.softmax(x, dim=1) - onehot) / den
    return loss, grad


def margins(scores: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """Per valid row, scores[n, c] - logsumexp over the valid NODES of column c: the log of metrics.py:39's Softmax(dim=0)."""
    x = scores[labels >= 0]
    return x - torch.logsumexp(x, dim=0, keepdim=True)


def predictions(scores: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """The reference's predicted class per valid row (first maximum on ties, numpy.argmax)."""
    return torch.from_numpy(np.argmax(margins(scores, labels).numpy(), axis=1))


def prediction_gap(scores: torch.Tensor, labels: torch.Tensor) -> float:
    """Smallest distance between the best and the second-best margin over the valid rows (inf without rows or with one class)."""
    m = margins(scores, labels)
    if m.shape[0] == 0 or m.shape[1] < 2:
        return float("inf")
    top = torch.topk(m, 2, dim=1).values
    return float((top[:, 0] - top[:, 1]).min())


def nudge_scores(scores: torch.Tensor, labels: torch.Tensor, gap: float = 1e-4, step: float = 1e-2, rounds: int = 20) -> torch.Tensor:
    """A copy of ``scores`` in which every valid row whose two best margins (evaluated in fp64) are closer than 4 x ``gap`` got ``step``
    added to its best class (repeated: a nudge moves the column log-sum-exps a little), so that fp32 and fp64 evaluations agree on every
    prediction and the fp32 evaluation still sees at least ``gap`` (the factor four is headroom for its rounding of O(10) margins)."""
    scores = scores.clone()
    rows = torch.nonzero(labels >= 0).flatten()
    for _ in range(rounds):
        m = margins(scores.double(), labels)
        if m.shape[0] == 0 or m.shape[1] < 2:
            return scores
        top = torch.topk(m, 2, dim=1)
        close = (top.values[:, 0] - top.values[:, 1]) < 4 * gap
        if not bool(close.any()):
            return scores
        scores[rows[close], top.indices[close, 0]] += step
    raise AssertionError("nudge_scores: prediction gaps stay below the bound")


def confusion_matrix(scores: torch.Tensor, labels: torch.Tensor, n_classes: int) -> torch.Tensor:
    """[C, C] int64: rows = label, columns = the reference's prediction; always the full matrix."""
    y = labels[labels >= 0]
    if y.numel() == 0:
        return torch.zeros(n_classes, n_classes, dtype=torch.int64)
    pred = predictions(scores, labels)
    return torch.bincount(y * n_classes + pred, minlength=n_classes * n_classes).reshape(n_classes, n_classes)


def accuracy(confusion: torch.Tensor) -> float:
    """100 * sum of the per-class recalls over the classes present / number of classes with at least one hit (metrics.py:41-53);
    0 where no class has a hit (the reference divides by zero)."""
    cm = confusion.to(torch.float64)
    count, hit = cm.sum(1), cm.diagonal()
    recall = torch.where(count > 0, hit / count.clamp_min(1.0), torch.zeros_like(hit))
    scored = int((hit > 0).sum())
    return 100.0 * float(recall.sum()) / scored if scored else 0.0
