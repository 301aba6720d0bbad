"""Numpy restatement, in fp32 and fp64, of the input stage of the nets with positional encodings and of the masked L1 loss, written from
the reference's lines:

* ``h = embedding_h(h); h = in_feat_dropout(h); h = h + embedding_pos_enc(g.ndata['pos_enc'])`` -- nets/molecules_graph_regression/
  dgn_net.py:58-62, nets/SBMs_node_classification/dgn_net.py:55-59, nets/HIV_graph_classification/dgn_net.py:62-66 (there ``embedding_h``
  is ogb's AtomEncoder: the sum of one lookup per index column) -- with the dropout inactive;
* ``nn.L1Loss()(scores, targets)`` -- nets/molecules_graph_regression/dgn_net.py:90-92, = ``MAE`` of train/metrics.py:14-16 -- over the
  entries whose target is not NaN (``ops.masked_bce_with_logits``' convention for "does not count").

``dtype`` selects the arithmetic of every function: np.float32 (sums taken row by row, in index order: the order of torch's CPU
``embedding_dense_backward``) or np.float64 (the judge of the GPU tests)."""
import numpy as np


def _idx2(idx):
    idx = np.asarray(idx)
    return idx.reshape(-1, 1) if idx.ndim == 1 else idx


def input_stage(idx, tables, pos_enc, weight, bias, dtype=np.float64):
    """``sum_c tables[c][idx[:, c]] + (pos_enc @ weight.T + bias)``: the table terms added in column order, the linear terms in increasing
    k from the bias on, the two partial results added last."""
    idx, pe, w = _idx2(idx), np.asarray(pos_enc, dtype=dtype), np.asarray(weight, dtype=dtype)
    emb = np.zeros((idx.shape[0], w.shape[0]), dtype=dtype)
    for c, t in enumerate(tables):
        emb = emb + np.asarray(t, dtype=dtype)[idx[:, c]]
    lin = np.zeros_like(emb) if bias is None else np.broadcast_to(np.asarray(bias, dtype=dtype), emb.shape).copy()
    for k in range(w.shape[1]):
        lin = lin + pe[:, k:k + 1] * w[:, k][None, :]
    return emb + lin


def input_stage_magnitude(idx, tables, pos_enc, weight, bias):
    """``sum_c |T_c[i_c]| + |b| + sum_k |W[f, k] pe[n, k]|`` in fp64: what the forward's rounding bound scales with."""
    abs_tables = [np.abs(np.asarray(t, dtype=np.float64)) for t in tables]
    return input_stage(idx, abs_tables, np.abs(np.asarray(pos_enc, dtype=np.float64)), np.abs(np.asarray(weight, dtype=np.float64)),
                       None if bias is None else np.abs(np.asarray(bias, dtype=np.float64)))


def input_stage_grads(idx, dims, pos_enc, g, dtype=np.float64):
    """The three gradients of ``input_stage`` for the upstream gradient ``g [N, F]``: the tables' (row ``r`` of table ``c`` collects the
    rows ``n`` with ``idx[n, c] == r``, in row order), ``dW [F, K] = g^T pos_enc`` and ``db [F] = sum_n g[n]``."""
    idx, pe, g = _idx2(idx), np.asarray(pos_enc, dtype=dtype), np.asarray(g, dtype=dtype)
    g_tables = []
    for c, d in enumerate(dims):
        t = np.zeros((int(d), g.shape[1]), dtype=dtype)
        np.add.at(t, idx[:, c], g)                      # unbuffered: the rows added one by one in row order
        g_tables.append(t)
    d_w = np.zeros((g.shape[1], pe.shape[1]), dtype=dtype)
    d_b = np.zeros(g.shape[1], dtype=dtype)
    for n in range(g.shape[0]):
        d_w = d_w + g[n][:, None] * pe[n][None, :]
        d_b = d_b + g[n]
    return g_tables, d_w, d_b


def masked_l1(scores, targets, dtype=np.float64):
    """``(loss, gradient)``: the mean of ``|s - t|`` over the entries whose target is not NaN and ``sign(s - t) / count`` there (0 at a
    tie and at the masked entries).  fp32: the terms in fp32, their sum in fp64, ``loss = float32(sum / count)`` and the gradient's
    ``float32(1 / count)`` -- the arithmetic the kernels state.  No counted entry: ``nan`` and an all-zero gradient."""
    s, t = np.asarray(scores, dtype=dtype), np.asarray(targets, dtype=dtype)
    keep = ~np.isnan(t)
    count = int(keep.sum())
    d = np.where(keep, s - np.where(keep, t, 0), 0).astype(dtype)
    total = np.abs(d).astype(np.float64).sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = dtype(np.float64(total) / np.float64(count))
        inv = dtype(np.float64(1.0) / np.float64(count))
    grad = np.zeros(s.shape, dtype=dtype)
    if count:
        grad = (np.sign(d) * inv).astype(dtype) * keep
    return loss, grad.astype(dtype)
