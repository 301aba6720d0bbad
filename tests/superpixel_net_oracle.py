"""CPU restatement of the superpixel net's loss tail, in plain torch, dtype-generic (fp32 / fp64): the mean cross-entropy of the
reference's ``DGNNet.loss`` (nets/superpixels_graph_classification/dgn_net.py:75-78: ``nn.CrossEntropyLoss()``), its gradient in closed
form, and the hit count of ``accuracy_MNIST_CIFAR`` (train/metrics.py:25-28).  Labels < 0 mark rows that do not exist (padding): they are
ignored everywhere and their gradient rows are zero.  Pinned to the reference by fixture G17
(tests/test_superpixel_net_oracle_vs_golden.py)."""
import numpy as np
import torch


def loss_and_grad(scores: torch.Tensor, labels: torch.Tensor):
    """(loss 0-dim, d loss / d scores [G, C]) in ``scores.dtype``: the mean over the valid rows of logsumexp(row) - row[label] and
    (softmax - onehot) / V.  No valid row: nan (0 / 0) with an all-zero gradient."""
    valid = labels >= 0
    grad = torch.zeros_like(scores)
    V = int(valid.sum())
    if V == 0:
        return torch.full((), float("nan"), dtype=scores.dtype), grad
    x, y = scores[valid], labels[valid]
    loss = (torch.logsumexp(x, dim=1) - x.gather(1, y[:, None])[:, 0]).sum() / V
    onehot = torch.zeros_like(x)
    onehot.scatter_(1, y[:, None], 1.0)
    grad[valid] = (torch.softmax(x, dim=1) - onehot) / V
    return loss, grad


def predictions(scores: torch.Tensor) -> torch.Tensor:
    """The column of every row's FIRST maximal score (numpy.argmax's rule, which is torch.argmax's documented one)."""
    return torch.from_numpy(np.argmax(scores.numpy(), axis=1).astype(np.int64)).reshape(-1)


def hits(scores: torch.Tensor, labels: torch.Tensor) -> int:
    """Number of valid rows whose prediction is their label."""
    valid = labels >= 0
    if int(valid.sum()) == 0:
        return 0
    return int((predictions(scores[valid]) == labels[valid]).sum())


def top_gap(scores: torch.Tensor, labels: torch.Tensor) -> float:
    """Smallest distance between the best and the second-best score over the valid rows (inf without rows)."""
    x = scores[labels >= 0]
    if x.shape[0] == 0:
        return float("inf")
    top = torch.topk(x, 2, dim=1).values
    return float((top[:, 0] - top[:, 1]).min())


def nudge_scores(scores: torch.Tensor, gap: float = 1e-4, step: float = 1e-2) -> torch.Tensor:
    """A copy of ``scores`` in which every row whose two best scores (in fp64) are closer than 4 x ``gap`` got ``step`` added to its best
    class: fp32 and fp64 evaluations then agree on every prediction (a row's scores are independent of the other rows: one pass)."""
    scores = scores.clone()
    top = torch.topk(scores.double(), 2, dim=1)
    close = (top.values[:, 0] - top.values[:, 1]) < 4 * gap
    rows = torch.nonzero(close).flatten()
    scores[rows, top.indices[close, 0]] += step
    return scores
