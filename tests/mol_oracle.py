"""CPU restatement (fp32 / fp64) of what the OGB molecule nets add around the layers: ogb's AtomEncoder / BondEncoder (a sum of embedding
lookups in column order), the binary cross-entropy with logits over the labelled entries (NaN label = not measured:
train/train_PCBA_graph_classification.py:32-33 + nets/PCBA_graph_classification/dgn_net.py:99-102) with its gradient, and the two metrics
of ogb's evaluator (ROC-AUC for ogbg-molhiv, average precision for ogbg-molpcba) written task by task in numpy, on purpose in another
form than ``dgn_amd.nets.rocauc_ogb`` / ``ap_ogb``.  Pinned to fixtures G13 / G14 by tests/test_mol_oracle_vs_golden.py."""
import numpy as np
import torch


def encoder_sum(weights, idx):
    """``x_embedding = 0; x_embedding += emb_c(idx[:, c])`` (ogb.graphproppred.mol_encoder)"""
    h = 0
    for c, w in enumerate(weights):
        h = h + w[idx[:, c]]
    return h


def encoder_grads(weights, idx, g):
    """d/d weights of <encoder_sum, g>: g's rows added up per index, in row order"""
    out = []
    for c, w in enumerate(weights):
        gw = torch.zeros_like(w)
        gw.index_add_(0, idx[:, c], g.to(w.dtype))
        out.append(gw)
    return out


def masked_bce(scores, labels):
    """(loss, gradient) in ``scores``' dtype: the mean over the labelled entries of max(x, 0) - x y + log1p(exp(-|x|)); the gradient is
    (sigmoid(x) - y) / n_labelled on them and exactly 0 elsewhere; no labelled entry: nan and zeros."""
    x = scores
    y = labels.to(x.dtype)
    lab = y == y
    n = int(lab.sum())
    y0 = torch.where(lab, y, torch.zeros_like(y))
    term = torch.clamp_min(x, 0) - x * y0 + torch.log1p(torch.exp(-x.abs()))
    loss = torch.where(lab, term, torch.zeros_like(term)).sum() / n if n else torch.full((), float("nan"), dtype=x.dtype)
    grad = torch.where(lab, (torch.sigmoid(x) - y0) / max(n, 1), torch.zeros_like(x))
    return loss, grad


def _scorable(labels):
    labels = np.asarray(labels, dtype=np.float64)
    labels = labels.reshape(len(labels), -1)
    for t in range(labels.shape[1]):
        y = labels[:, t]
        if (y == 1).sum() > 0 and (y == 0).sum() > 0:
            yield t, y == y


def rocauc(scores, labels):
    """ogb's rule: per task over its labelled rows, tasks with a positive and a negative only; the probability that a positive outranks a
    negative, ties counting one half (the average-rank form); mean over the tasks; nan where ogb raises"""
    s = np.asarray(scores, dtype=np.float64).reshape(len(scores), -1)
    y_all = np.asarray(labels, dtype=np.float64).reshape(len(labels), -1)
    vals = []
    for t, lab in _scorable(y_all):
        y, x = y_all[lab, t], s[lab, t]
        pos, neg = x[y == 1], x[y == 0]
        neg_sorted = np.sort(neg)
        below = np.searchsorted(neg_sorted, pos, side="left")
        upto = np.searchsorted(neg_sorted, pos, side="right")
        vals.append(float((below + 0.5 * (upto - below)).sum()) / (len(pos) * len(neg)))
    return float(np.mean(vals)) if vals else float("nan")


def average_precision(scores, labels):
    """ogb's rule around scikit-learn's definition: sum over the distinct thresholds, descending, of (recall step) x precision"""
    s = np.asarray(scores, dtype=np.float64).reshape(len(scores), -1)
    y_all = np.asarray(labels, dtype=np.float64).reshape(len(labels), -1)
    vals = []
    for t, lab in _scorable(y_all):
        y, x = y_all[lab, t], s[lab, t]
        n_pos = float((y == 1).sum())
        ap, prev_recall = 0.0, 0.0
        for thr in np.unique(x)[::-1]:
            sel = x >= thr
            tp = float(((y == 1) & sel).sum())
            recall, precision = tp / n_pos, tp / float(sel.sum())
            ap += (recall - prev_recall) * precision
            prev_recall = recall
        vals.append(ap)
    return float(np.mean(vals)) if vals else float("nan")
