# -*- coding: utf-8 -*-
"""numpy oracle of similar_items() / similar_users() (csrc/retrieve.hip neighbour_fold_kernel + the fused top-k with
each query's own row excluded; include/trs.h "nearest neighbours").

  representation   item i: S_i = item_i + sum_m meta_m(i) (the row item_fold_kernel writes); user u: its table row
  metric 'dot'     <x_q, x_j>
  metric 'cosine'  <x^_q, x^_j>, x^ = x * (1 / |x|), a zero row -> 0
  ranking          similarity descending, ties by ascending dense row, the query's own row removed, -1 / -inf padding

Everything is float64 numpy except normalise_f32, the bit-level restatement of the kernel's fp32 normalisation, and
neighbours_int, which ranks exact integer keys (torch.topk on the CPU, for the one large catalogue)."""
import numpy as np
import torch

KMAX = 128  # TRS_RETRIEVE_KMAX


def dp(D):
    """Padded width of a D-factor row in the folded buffers: 16, 32, 64, 128 or 256."""
    p = 16
    while p < D:
        p <<= 1
    return p


def tol(D):
    """Bound on |fp32 cosine - float64 cosine|: the gamma bound of a Dp-term fp32 inner product of unit vectors plus the
    roundings of the normalisation, doubled."""
    return (dp(D) + 8) * 2.0 ** -23


def item_rows(m):
    """S (n_items, D) float64 of a Linear / FM model: item rows plus the rows of their metadata."""
    net = m.net
    f = lambda t: t.detach().cpu().double().numpy()
    S = f(net.item.weight).copy()
    if net.n_meta_tables():
        meta_ids = m.data_processor.item_meta_table
        for j, l in enumerate(net.metadata):
            S += f(l.weight)[meta_ids[:, j]]
    return S


def user_rows(m):
    return m.net.user.weight.detach().cpu().double().numpy().copy()


def normalise(X):
    """float64 unit rows; a zero row stays zero."""
    nrm = np.sqrt((X * X).sum(1))
    inv = np.where(nrm > 0, 1.0 / np.where(nrm > 0, nrm, 1.0), 0.0)
    return X * inv[:, None]


def normalise_f32(X):
    """The kernel's normalisation, bit for bit: lane l of a 64-lane wave holds columns 4l .. 4l+3 of the row padded with
    zeros to 256 columns; per lane the squares are added in ascending column order from 0 (product and sum rounded
    separately); the lane sums go through the xor butterfly of strides 32, 16, 8, 4, 2, 1 (every lane adds its partner's
    value); inv = 1 / sqrt(sum) in fp32, 0 for a zero sum; x^ = x * inv."""
    X = np.asarray(X, dtype=np.float32)
    n, D = X.shape
    assert D <= 256
    P = np.zeros((n, 256), np.float32)
    P[:, :D] = X
    L = P.reshape(n, 64, 4)
    sq = np.zeros((n, 64), np.float32)
    for c in range(4):
        sq = (sq + (L[:, :, c] * L[:, :, c]).astype(np.float32)).astype(np.float32)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        sq = (sq + sq[:, lanes ^ o]).astype(np.float32)
    tot = sq[:, 0]
    with np.errstate(divide="ignore"):
        inv = np.where(tot > 0, np.float32(1.0) / np.sqrt(tot, dtype=np.float32), np.float32(0.0)).astype(np.float32)
    return (X * inv[:, None]).astype(np.float32)


def similarities(X, queries, metric="dot", block=2048):
    """(len(queries), n) float64 similarities of rows `queries` of X to every row."""
    X = np.asarray(X, dtype=np.float64)
    if metric == "cosine":
        X = normalise(X)
    elif metric != "dot":
        raise ValueError(metric)
    q = np.asarray(queries, dtype=np.int64)
    return np.concatenate([X[q[s:s + block]] @ X.T for s in range(0, len(q), block)]) if len(q) else \
        np.zeros((0, X.shape[0]))


def rank(vals, queries, k):
    """Stable descending ranking of each row of vals (ties by ascending id) with the query's own id removed:
    (ids (n, k) int64 padded with -1, values (n, k) float64 padded with -inf)."""
    n = vals.shape[1]
    ids = np.full((len(queries), k), -1, np.int64)
    out = np.full((len(queries), k), -np.inf)
    for r, q in enumerate(queries):
        v = vals[r]
        order = np.argsort(-v, kind="stable")  # stable: equal values keep ascending ids
        order = order[order != q][:k]
        ids[r, :len(order)] = order
        out[r, :len(order)] = v[order]
    assert n >= 1
    return ids, out


def neighbours_int(X, queries, k, block=2048):
    """neighbours(X, queries, k, 'dot') for integer-valued rows without sorting whole rows (large catalogues): the k + 1
    largest of the integer keys value * n + (n - 1 - id) — descending value, ascending id, all distinct — per row, in
    blocks (torch on the CPU: threaded matmul and top-k)."""
    X = np.asarray(X, dtype=np.float64)
    assert np.array_equal(X, np.rint(X))
    n = X.shape[0]
    q = torch.as_tensor(np.asarray(queries, dtype=np.int64))
    kk = min(k + 1, n)
    ids = torch.full((len(q), k), -1, dtype=torch.int64)
    out = torch.full((len(q), k), -np.inf, dtype=torch.float64)
    small = float(np.abs(X).sum(1).max()) ** 2 * n < 2 ** 24  # products and sums exact in fp32, keys within int32
    Xt = torch.from_numpy(X).to(torch.float32 if small else torch.float64)
    tie = torch.arange(n - 1, -1, -1, dtype=torch.int32 if small else torch.int64)[None, :]
    cols = torch.arange(kk - 1)[None, :]
    for s in range(0, len(q), block):
        qs = q[s:s + block]
        key = (Xt[qs] @ Xt.T).to(tie.dtype) * n + tie
        order = torch.topk(key, kk, dim=1).indices  # (rows, kk), keys descending
        is_self = order == qs[:, None]
        at = torch.where(is_self.any(1), is_self.int().argmax(1), torch.tensor(kk))
        if kk > 1:  # drop the query's own column, keep the order
            kept = torch.where(cols >= at[:, None], order[:, 1:], order[:, :-1])
        else:
            kept = order[:, :0]
        w = min(k, kept.shape[1])
        ids[s:s + len(qs), :w] = kept[:, :w]
        vals = torch.div(torch.gather(key, 1, kept[:, :w]).to(torch.int64), n, rounding_mode="floor")
        out[s:s + len(qs), :w] = vals.to(torch.float64)
    return ids.numpy(), out.numpy()


def neighbours(X, queries, k, metric="dot", block=2048):
    """rank() of similarities(), computed in blocks of queries (large catalogues)."""
    q = np.asarray(queries, dtype=np.int64)
    parts = [rank(similarities(X, q[s:s + block], metric), q[s:s + block], k) for s in range(0, len(q), block)]
    if not parts:
        return np.zeros((0, k), np.int64), np.zeros((0, k))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
