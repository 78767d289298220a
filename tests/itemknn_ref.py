# -*- coding: utf-8 -*-
"""numpy restatement of the item-kNN model as include/trs.h "item kNN" states it: the oracle of
tests/test_itemknn_host.py (which ties it to a brute-force dense X^T X) and of tests/test_gpu_itemknn.py.

    c(i, j) = users holding both items;  sim from (c, n_i, n_j, h) in float64, rounded to float32 once;
    row i keeps the K candidates j != i, c > 0 with the largest (sim descending, j ascending);
    score(u, j) = sum over the items i of hist(u), in list order, of the weight row i gives j: one float32 add each.
"""
import numpy as np

KINDS = ("cosine", "jaccard", "conditional", "count")
FIRST_LENGTHS = (0, 1, 2, 63, 64, 65)  # the rest random in 0..20


def histories(n_users, n_items, seed):
    """n_users sorted lists of distinct items drawn over the whole range: lengths 0, 1, 2, 63, 64, 65 (each clipped to
    n_items), then random lengths in 0..20 (clipped)."""
    rs = np.random.RandomState(seed)
    lens = [min(v, n_items) for v in FIRST_LENGTHS][:n_users]
    lens += [min(int(v), n_items) for v in rs.randint(0, 21, size=max(n_users - len(lens), 0))]
    return [np.sort(rs.choice(n_items, size=v, replace=False)).astype(np.int64) for v in lens]


def csr(lists):
    """(offsets int64 (n + 1,), ids int32)."""
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(v) for v in lists])
    ids = np.concatenate([np.asarray(v, dtype=np.int64) for v in lists]) if off[-1] else np.zeros(0, np.int64)
    return off, ids.astype(np.int32)


def inverse(lists, n_items):
    """item -> sorted users, as lists."""
    users = np.repeat(np.arange(len(lists), dtype=np.int64), [len(v) for v in lists])
    items = np.concatenate([np.asarray(v, dtype=np.int64) for v in lists]) if users.size else np.zeros(0, np.int64)
    o = np.lexsort((users, items))
    by_item, cuts = users[o], np.searchsorted(items[o], np.arange(n_items + 1))
    return [by_item[cuts[i]:cuts[i + 1]] for i in range(n_items)]


def cocounts(lists, n_items):
    """(i, j, c, deg): every ordered pair i != j with c(i, j) > 0, sorted by (i, j), and the items' degrees.  Pair
    expansion per user and np.unique: nothing of size n_items^2."""
    n = int(n_items)
    keys = []
    deg = np.zeros(n, dtype=np.int64)
    for v in lists:
        v = np.asarray(v, dtype=np.int64)
        if v.size:
            deg[v] += 1
            keys.append((v[:, None] * n + v[None, :]).ravel())
    if not keys:
        e = np.zeros(0, dtype=np.int64)
        return e, e, e, deg
    uniq, c = np.unique(np.concatenate(keys), return_counts=True)
    i, j = uniq // n, uniq % n
    keep = i != j
    return i[keep], j[keep], c[keep].astype(np.int64), deg


def similarity(kind, c, ni, nj, h):
    """float32 similarity from the integer arrays (c, n_i, n_j) and the shrinkage h: float64, one rounding per
    operation, then one rounding to float32."""
    c64, ni64, nj64 = (np.asarray(a).astype(np.float64) for a in (c, ni, nj))
    h = np.float64(h)
    if kind == "cosine":
        s = c64 / (np.sqrt(ni64 * nj64) + h)
    elif kind == "jaccard":
        s = c64 / ((np.asarray(ni) + np.asarray(nj) - np.asarray(c)).astype(np.float64) + h)
    elif kind == "conditional":
        s = c64 / (ni64 + h)
    elif kind == "count":
        s = c64
    else:
        raise ValueError(kind)
    return s.astype(np.float32)


def neighbours(pairs, n_items, kind, h, K):
    """(ids (n, K) int32 with -1 padding, w (n, K) float32 with 0 padding) from cocounts(): rows in key order."""
    i, j, c, deg = pairs
    n = int(n_items)
    ids = np.full((n, K), -1, dtype=np.int32)
    w = np.zeros((n, K), dtype=np.float32)
    if i.size == 0:
        return ids, w
    s = similarity(kind, c, deg[i], deg[j], h)
    o = np.lexsort((j, -s.astype(np.float64), i))  # i ascending, then sim descending, then j ascending
    i, j, s = i[o], j[o], s[o]
    start = np.searchsorted(i, np.arange(n))
    slot = np.arange(i.size) - start[i]
    keep = slot < K
    ids[i[keep], slot[keep]] = j[keep]
    w[i[keep], slot[keep]] = s[keep]
    return ids, w


def score_rows(ids, w, lists, n_items):
    """float32 score rows: per history item, in list order, one float32 add to every column its list holds."""
    out = np.zeros((len(lists), int(n_items)), dtype=np.float32)
    for r, v in enumerate(lists):
        acc = out[r]
        for i in v:
            row = ids[int(i)]
            ok = row >= 0
            acc[row[ok]] = (acc[row[ok]] + w[int(i)][ok]).astype(np.float32)  # a row lists a column once
    return out


def item_weights(ids, w, item, k):
    """The first k stored neighbours of `item`: (ids (k,) int64 with -1 padding, weights with -inf padding)."""
    K = ids.shape[1]
    oi = np.full(k, -1, dtype=np.int64)
    ow = np.full(k, -np.inf, dtype=np.float32)
    m = min(k, K)
    oi[:m] = ids[item, :m]
    ow[:m] = np.where(ids[item, :m] >= 0, w[item, :m], -np.inf)
    return oi, ow
