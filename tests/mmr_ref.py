# -*- coding: utf-8 -*-
"""numpy oracle of recommend_diverse() / evaluate_diversity() (csrc/rerank.hip; the rule is the contract in
include/trs.h "diversified re-ranking").

  rerank        the greedy MMR selection in np.float32, operation by operation, with similarities from a given matrix
                (bit-exact against the kernel wherever the kernel's fp32 inner products are exact)
  check_greedy  a returned list verified step by step against float64 similarities of the stored fp32 fold rows: every
                pick's m is at least the best unselected m - eps
  ild, coverage, novelty   the metrics of evaluate_diversity in float64
"""
import numpy as np

KMAX = 128  # TRS_RETRIEVE_KMAX


def dp(D):
    """Padded width of a D-factor row in the folded buffers: 16, 32, 64, 128 or 256."""
    p = 16
    while p < D:
        p <<= 1
    return p


def eps(lam, D):
    """Slack of check_greedy.  The fp32 inner product of two unit-length rows errs by at most (Dp + 2) * 2**-24 in any
    summation order, and m carries it times lambda; rel is reproduced bit for bit; 3 * 2**-24 covers the three roundings
    of m (|m| <= 1); the factor 2 covers both sides of the comparison."""
    return 2.0 * (float(lam) * (dp(D) + 2) + 3.0) * 2.0 ** -24


def ild_tol(D):
    """Bound on |trs_list_ild - ild()|: the inner-product bound above (a mean of such errors) plus float64 rounding."""
    return (dp(D) + 2) * 2.0 ** -24 + 1e-12


def relevance(v, valid):
    """rel (N,) float32 of one pool: min-max scaled over the valid entries (scan with < / > from the first valid one),
    0 everywhere when v_max == v_min, then the running minimum along the valid entries; invalid entries hold 0."""
    v = np.asarray(v, dtype=np.float32)
    rel = np.zeros(v.shape, np.float32)
    idx = np.nonzero(valid)[0]
    if idx.size == 0:
        return rel
    vmin = vmax = v[idx[0]]
    for i in idx[1:]:
        x = v[i]
        vmin = x if x < vmin else vmin
        vmax = x if x > vmax else vmax
    if vmax != vmin:
        rel[idx] = (v[idx] - vmin) / (vmax - vmin)  # float32 arrays: a rounded difference, a rounded quotient
    run = rel[idx[0]]
    for i in idx:
        run = rel[i] if rel[i] < run else run
        rel[i] = run
    return rel


def _pick(m, taken):
    """The contract's scan over the unselected entries: the largest m, ties to the lowest position, a NaN below every
    number (argmax returns the first maximum; -0.0 == +0.0 compare equal)."""
    cand = np.nonzero(~taken)[0]
    num = cand[~np.isnan(m[cand])]
    return int(num[np.argmax(m[num])]) if num.size else int(cand[0])


def rerank(pool_ids, pool_scores, X, k, lam, n_items=None):
    """MMR lists of pools (n, N): ids int64 (-1 / an id >= n_items: no item), scores float32; X (n_items, n_items) the
    similarity matrix (cast to float32 as given).  Returns (ids (n, k) int64, scores (n, k) float32, pool positions
    (n, k) int32), padded with -1 / -inf / -1 from min(k, n_valid) on."""
    pool_ids = np.asarray(pool_ids, dtype=np.int64)
    pool_scores = np.asarray(pool_scores, dtype=np.float32)
    X = np.asarray(X).astype(np.float32)
    n_items = X.shape[0] if n_items is None else n_items
    n, N = pool_ids.shape
    assert 1 <= k <= N <= KMAX
    a, b = np.float32(1.0) - np.float32(lam), np.float32(lam)
    ids = np.full((n, k), -1, np.int64)
    sc = np.full((n, k), -np.inf, np.float32)
    pos = np.full((n, k), -1, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(n):
            p = pool_ids[q]
            valid = (p >= 0) & (p < n_items)
            n_pick = min(k, int(valid.sum()))
            if n_pick == 0:
                continue
            rel = relevance(pool_scores[q], valid)
            ar = a * rel
            safe = np.where(valid, p, 0)
            taken = ~valid
            pen = np.full(N, -np.inf, np.float32)
            s = int(np.nonzero(valid)[0][0])
            for t in range(n_pick):
                ids[q, t], sc[q, t], pos[q, t] = p[s], pool_scores[q, s], s
                if t + 1 == n_pick:
                    break
                taken[s] = True
                sim = X[p[s], safe]
                pen = np.where(sim > pen, sim, pen)
                s = _pick(ar - b * pen, taken)
    return ids, sc, pos


def check_greedy(pool_ids, pool_scores, rows, k, lam, D, got_ids, got_scores, got_pos, n_items=None):
    """Every returned list is a greedy MMR list up to rounding: picks are distinct valid pool positions, pick 0 is the
    first valid one, ids / scores are the pool's at those positions, the tail is -1 / -inf / -1, and at every step t >= 1
    the chosen entry's m (float64 similarities of `rows`, the stored fp32 fold rows; rel bit for bit) is at least the
    best unselected m - eps(lam, D).  Returns the largest shortfall met (<= eps), for printing."""
    pool_ids = np.asarray(pool_ids, dtype=np.int64)
    pool_scores = np.asarray(pool_scores, dtype=np.float32)
    rows = np.asarray(rows, dtype=np.float64)
    n_items = rows.shape[0] if n_items is None else n_items
    n, N = pool_ids.shape
    slack = eps(lam, D)
    a, b = float(np.float32(1.0) - np.float32(lam)), float(np.float32(lam))
    worst = 0.0
    for q in range(n):
        p = pool_ids[q]
        valid = (p >= 0) & (p < n_items)
        n_pick = min(k, int(valid.sum()))
        gp = np.asarray(got_pos[q])
        assert np.all(gp[n_pick:] == -1) and np.all(got_ids[q][n_pick:] == -1), q
        assert np.all(np.isneginf(got_scores[q][n_pick:])), q
        if n_pick == 0:
            continue
        sel = gp[:n_pick]
        assert np.all((sel >= 0) & (sel < N)) and valid[sel].all() and len(set(sel.tolist())) == n_pick, (q, sel)
        assert sel[0] == np.nonzero(valid)[0][0], q
        assert np.array_equal(got_ids[q][:n_pick], p[sel]), q
        assert np.array_equal(got_scores[q][:n_pick], pool_scores[q][sel]), q
        rel = relevance(pool_scores[q], valid).astype(np.float64)
        R = rows[np.where(valid, p, 0)]
        taken = ~valid
        pen = np.full(N, -np.inf)
        for t in range(1, n_pick):
            s = sel[t - 1]
            taken[s] = True
            pen = np.maximum(pen, R @ R[s])
            m = a * rel - b * pen
            short = float(np.max(m[~taken]) - m[sel[t]])
            assert not taken[sel[t]] and short <= slack, (q, t, short, slack)
            worst = max(worst, short)
    return worst


def ild(ids, rows, n_items=None):
    """(n,) float64: per list the mean over the unordered pairs of valid entries of 1 - <row_a, row_b>; 0.0 with fewer
    than two valid entries.  rows: the fold rows the similarity is defined on (float64 arithmetic)."""
    ids = np.asarray(ids, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.float64)
    n_items = rows.shape[0] if n_items is None else n_items
    out = np.zeros(ids.shape[0])
    for q in range(ids.shape[0]):
        v = ids[q][(ids[q] >= 0) & (ids[q] < n_items)]
        if v.size < 2:
            continue
        G = rows[v] @ rows[v].T
        iu = np.triu_indices(v.size, 1)
        out[q] = np.mean(1.0 - G[iu])
    return out


def coverage(ids, n_items):
    ids = np.asarray(ids, dtype=np.int64)
    return len(set(ids[ids >= 0].tolist())) / float(n_items)


def novelty(ids, item_users, n_users):
    """Mean over the lists of the mean over their valid entries of -log2((c_i + 1) / (n_users + 1)); a list without a
    valid entry adds 0."""
    ids = np.asarray(ids, dtype=np.int64)
    c = np.asarray(item_users, dtype=np.float64)
    per = []
    for row in ids:
        v = row[row >= 0]
        per.append(float(np.mean(-np.log2((c[v] + 1.0) / (n_users + 1.0)))) if v.size else 0.0)
    return float(np.mean(per)) if per else 0.0
