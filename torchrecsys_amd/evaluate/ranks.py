# -*- coding: utf-8 -*-
"""Per-user ranking metrics from exact ranks (TorchRecSys.evaluate_ranks): float64 host arithmetic on int64 ranks.

With a user's ranks sorted ascending r_0 < ... < r_{m-1}, m = |T_u| relevant items and n_c = |C_u| candidates:
  auc         = 1 - sum_j (r_j - j) / (m (n_c - m))        the share of (relevant, irrelevant) pairs in the right order
  mrr         = 1 / (r_0 + 1)                              mean_rank = sum_j r_j / m
  hits@k      = #{j : r_j < k}                             hit_rate@k = 1[hits >= 1]
  precision@k = hits / k                                   recall@k   = hits / m
  ndcg@k      = sum_{r_j < k} 1/log2(r_j + 2)  /  sum_{r < min(k, m)} 1/log2(r + 2)
  map@k       = 1/min(k, m) * sum_{j : r_j < k} (j + 1) / (r_j + 1)
k > n_items behaves as n_items.  A user without relevant items, or whose candidates are all relevant, has no value.
"""
import numpy as np

PLAIN = ('auc', 'mrr', 'mean_rank')
AT_K = ('hit_rate', 'precision', 'recall', 'ndcg', 'map')


def check(metrics, ks):
    """ValueError for an unknown metric name or a k below 1."""
    unknown = set(metrics) - set(PLAIN) - set(AT_K)
    if unknown:
        raise ValueError(f"unknown ranking metrics {sorted(unknown)}")
    for k in ks:
        if k < 1:
            raise ValueError(f"k must be >= 1, got {k}")


def entries(metrics, ks):
    """Result keys in the order of `metrics`: the name itself, or name@k for every k."""
    out = []
    for m in metrics:
        out += [m] if m in PLAIN else [f'{m}@{k}' for k in ks]
    return out


def per_user(ranks, off, n_cand, ks, metrics, n_items):
    """ranks (n_t,) int64 in any order within a user's segment; off (n + 1,) the users' segment offsets; n_cand (n,)
    |C_u|.  Returns (keep (n,) bool: the users that have a value, {entry: (keep.sum(),) float64})."""
    ranks = np.asarray(ranks, dtype=np.int64)
    off = np.asarray(off, dtype=np.int64)
    n_c = np.asarray(n_cand, dtype=np.int64)
    m = np.diff(off)
    n = m.size
    keep = (m > 0) & (n_c > m)
    seg = np.repeat(np.arange(n), m)
    r = ranks[np.lexsort((ranks, seg))]  # ascending within each user
    j = np.arange(r.size, dtype=np.int64) - off[:-1][seg]
    md = np.where(keep, m, 1).astype(np.float64)

    def seg_sum(w):
        return np.bincount(seg, weights=w, minlength=n)[keep]

    out = {}
    rf = r.astype(np.float64)
    for name in metrics:
        if name == 'auc':
            pairs = np.where(keep, m * (n_c - m), 1).astype(np.float64)
            out[name] = 1.0 - seg_sum((r - j).astype(np.float64)) / pairs[keep]
        elif name == 'mrr':
            out[name] = 1.0 / (r[off[:-1][keep]] + 1.0)
        elif name == 'mean_rank':
            out[name] = seg_sum(rf) / md[keep]
    if any(name in AT_K for name in metrics):
        disc = 1.0 / np.log2(np.arange(max(int(m.max()) if n else 0, 1), dtype=np.float64) + 2.0)
        ideal = np.concatenate([[0.0], np.cumsum(disc)])  # ideal[x] = sum_{r < x} 1/log2(r + 2)
    for k in ks:
        kk = min(int(k), int(n_items))
        top = r < kk
        hits = seg_sum(top.astype(np.float64))
        depth = np.minimum(kk, m)[keep]
        for name in metrics:
            if name == 'hit_rate':
                out[f'{name}@{k}'] = (hits >= 1).astype(np.float64)
            elif name == 'precision':
                out[f'{name}@{k}'] = hits / kk
            elif name == 'recall':
                out[f'{name}@{k}'] = hits / md[keep]
            elif name == 'ndcg':
                out[f'{name}@{k}'] = seg_sum(np.where(top, 1.0 / np.log2(rf + 2.0), 0.0)) / ideal[depth]
            elif name == 'map':
                out[f'{name}@{k}'] = seg_sum(np.where(top, (j + 1.0) / (rf + 1.0), 0.0)) / depth
    return keep, out
