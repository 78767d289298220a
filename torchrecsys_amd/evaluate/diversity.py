# -*- coding: utf-8 -*-
"""Beyond-accuracy metrics of top-k lists (TorchRecSys.evaluate_diversity): float64 host arithmetic on dense item ids.

For the lists R_u (n, k) of the evaluated users, -1 = no item:
  coverage@k = |union of the returned ids| / n_items                    the share of the catalogue that is ever shown
  novelty@k  = mean_u mean_{i in R_u} -log2((c_i + 1) / (n_users + 1))   c_i = the distinct train users of item i; the
               self-information of an item's popularity, add-one smoothed; a user without any returned item adds 0
  ild@k      = mean_u ild(R_u), ild = the mean of 1 - cosine over the unordered pairs of a list (trs_list_ild on the
               device, include/trs.h "diversified re-ranking"); 0 for a list with fewer than two items
The arguments of recommend_diverse / evaluate_diversity are checked here too, before any device work.
"""
import numbers

import numpy as np

METRICS = ('cosine', 'dot')


def check(what, net_type, n_factors, n_items, top_k, diversity, pool, metric, kmax, dmax):
    """ValueError for arguments recommend_diverse / evaluate_diversity do not take; returns (k, pool) clamped to the
    catalogue: k = min(top_k, n_items), pool = min(TRS_RETRIEVE_KMAX, max(4 top_k, 32), n_items) unless given."""
    if metric not in METRICS:
        raise ValueError(f"metric must be 'cosine' or 'dot', got {metric!r}")
    if net_type not in ('linear', 'fm'):
        raise ValueError(f"{what} needs net_type 'linear' or 'fm': with net_type={net_type!r} the metadata embeddings "
                         "are concatenated, not summed, so an item has no folded row to compare")
    if n_factors > dmax:
        raise ValueError(f"{what} takes n_factors <= {dmax} (TRS_RETRIEVE_DMAX), got {n_factors}")
    if isinstance(diversity, bool) or not isinstance(diversity, numbers.Real) or not 0.0 <= float(diversity) <= 1.0:
        raise ValueError(f"diversity must be a number in [0, 1], got {diversity!r}")
    k = min(int(top_k), int(n_items))
    if pool is None:
        pool = min(kmax, max(4 * int(top_k), 32))
    elif isinstance(pool, bool) or not isinstance(pool, numbers.Integral) or pool < 1:
        raise ValueError(f"pool must be an integer >= 1, got {pool!r}")
    elif pool > kmax:
        raise ValueError(f"pool={pool} is above {kmax} (TRS_RETRIEVE_KMAX), the most candidates the fused top-k keeps "
                         "per user")
    pool = min(int(pool), int(n_items))
    if k > pool:
        raise ValueError(f"top_k={top_k} > pool={pool}: the list is picked out of the pool")
    return k, pool


def coverage(ids, n_items):
    """|union of the ids >= 0| / n_items."""
    ids = np.asarray(ids, dtype=np.int64)
    return float(np.unique(ids[ids >= 0]).size) / float(n_items)


def novelty_per_user(ids, item_users, n_users):
    """(n,) float64: per list the mean over its ids >= 0 of -log2((c_i + 1) / (n_users + 1)), summed in list order; 0 for
    a list without one."""
    ids = np.asarray(ids, dtype=np.int64)
    c = np.asarray(item_users, dtype=np.float64)
    real = ids >= 0
    info = np.where(real, -np.log2((c[np.where(real, ids, 0)] + 1.0) / (float(n_users) + 1.0)), 0.0)
    total = np.zeros(ids.shape[0], dtype=np.float64)
    for col in range(ids.shape[1]):
        total += info[:, col]
    cnt = real.sum(1)
    return np.where(cnt > 0, total / np.maximum(cnt, 1), 0.0)
