# -*- coding: utf-8 -*-
"""numpy restatement of EASE as include/trs.h "EASE" states it: the oracle of tests/test_ease_host.py (which ties it to
the real reference's output, tests/golden/g5_ease.npz) and of tests/test_gpu_ease.py.

    X binary (n_users, n_items);  A = X^T X + lambda I;  P = A^-1;  B[i][j] = -P[i][j] / P[j][j], B[i][i] = 0;
    score(u, :) = sum of the rows of B that the history of u lists.
"""
import numpy as np

FIRST_LENGTHS = (0, 1, 2, 63, 64, 65)  # then n_items; the rest random in 0..20


def byte_planes(a):
    """A float64 array as (8, a.size) uint8, plane k = byte k of every value (lossless; tests/golden/g5_ease.npz)."""
    return np.ascontiguousarray(np.ascontiguousarray(a, dtype='<f8').reshape(-1).view(np.uint8).reshape(-1, 8).T)


def from_byte_planes(planes, shape):
    return np.ascontiguousarray(planes.T).reshape(-1).view('<f8').reshape(shape).astype(np.float64)


def histories(n_users, n_items, seed):
    """n_users sorted lists of distinct items: lengths 0, 1, 2, 63, 64, 65 and n_items (each clipped to n_items), then
    random lengths in 0..20 (clipped)."""
    rs = np.random.RandomState(seed)
    lens = [min(v, n_items) for v in FIRST_LENGTHS + (n_items,)][:n_users]
    lens += [min(int(v), n_items) for v in rs.randint(0, 21, size=max(n_users - len(lens), 0))]
    return [np.sort(rs.choice(n_items, size=v, replace=False)).astype(np.int64) for v in lens]


def csr(lists):
    """(offsets int64 (n + 1,), items int32)."""
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(v) for v in lists])
    items = np.concatenate([np.asarray(v, dtype=np.int64) for v in lists]) if off[-1] else np.zeros(0, np.int64)
    return off, items.astype(np.int32)


def dense_x(lists, n_items):
    X = np.zeros((len(lists), n_items), dtype=np.float64)
    for u, v in enumerate(lists):
        X[u, np.asarray(v, dtype=np.int64)] = 1.0
    return X


def gram(X, lam):
    """A = X^T X + lam I (float64; the counts are exact integers)."""
    A = X.T @ X
    A[np.diag_indices(A.shape[0])] += lam
    return A


def padded(A, nb):
    """A beside an identity block, edge a multiple of nb (what trs_ease_gram writes)."""
    n = A.shape[0]
    nbar = -(-n // nb) * nb
    out = np.eye(nbar, dtype=np.float64)
    out[:n, :n] = A
    return out


def weights(P):
    """B (float64) from P: column j divided by -P[j][j], diagonal 0."""
    B = P / (-np.diag(P))
    B[np.diag_indices(B.shape[0])] = 0.0
    return B


def _factor_block(a):
    """(L, W = L^-1) of one diagonal block: left-looking Cholesky column by column, forward substitution row by row."""
    nb = a.shape[0]
    L = np.zeros_like(a)
    for j in range(nb):
        s = a[j:, j] - L[j:, :j] @ L[j, :j]
        L[j, j] = np.sqrt(s[0])
        L[j + 1:, j] = s[1:] / L[j, j]
    W = np.zeros_like(a)
    for r in range(nb):
        W[r, r] = 1.0 / L[r, r]
        W[r, :r] = -(L[r, :r] @ W[:r, :r]) / L[r, r]
    return L, W


def blocked_inverse(A, nb):
    """A^-1 (float64) by the route of trs_ease_invert with block size nb: right-looking blocked Cholesky with explicit
    inverses of the diagonal factors, M = L^-1 by block forward substitution, P = M^T M."""
    n = A.shape[0]
    a = padded(A, nb)
    nblk = a.shape[0] // nb
    blk = lambda i: slice(i * nb, (i + 1) * nb)  # noqa: E731
    W = [None] * nblk
    for k in range(nblk):
        Lkk, W[k] = _factor_block(a[blk(k), blk(k)])
        a[blk(k), blk(k)] = Lkk
        lo = (k + 1) * nb
        a[lo:, blk(k)] = a[lo:, blk(k)] @ W[k].T
        a[lo:, lo:] -= a[lo:, blk(k)] @ a[lo:, blk(k)].T
    M = np.zeros_like(a)
    for i in range(nblk):
        M[blk(i), blk(i)] = W[i]
        for k in range(i):
            T = np.zeros((nb, nb))
            for j in range(k, i):
                T += a[blk(i), blk(j)] @ M[blk(j), blk(k)]
            M[blk(i), blk(k)] = -W[i] @ T
    P = M.T @ M
    return P[:n, :n]


def residual(A, P):
    """max |A P - I| in long double."""
    A, P = A.astype(np.longdouble), P.astype(np.longdouble)
    return float(np.abs(A @ P - np.eye(A.shape[0], dtype=np.longdouble)).max())


def score_rows(B32, lists):
    """float32 score rows: one float32 add per item, in list order, from 0."""
    B32 = np.asarray(B32, dtype=np.float32)
    out = np.zeros((len(lists), B32.shape[1]), dtype=np.float32)
    for r, v in enumerate(lists):
        acc = np.zeros(B32.shape[1], dtype=np.float32)
        for j in v:
            acc = (acc + B32[int(j)]).astype(np.float32)
        out[r] = acc
    return out


def order(row, excluded=()):
    """Candidate items by (value descending, id ascending), the excluded ones left out."""
    row = np.asarray(row)
    keep = np.ones(row.size, dtype=bool)
    keep[np.asarray(list(excluded), dtype=np.int64)] = False
    ids = np.nonzero(keep)[0]
    return ids[np.lexsort((ids, -row[ids].astype(np.float64)))]


def recommend(rows, seen_lists, k, exclude_seen):
    """(ids (n, k) int64 with -1 padding, scores (n, k) float32 with -inf padding)."""
    n = rows.shape[0]
    ids = np.full((n, k), -1, dtype=np.int64)
    sc = np.full((n, k), -np.inf, dtype=np.float32)
    for r in range(n):
        o = order(rows[r], seen_lists[r] if exclude_seen else ())[:k]
        ids[r, :o.size] = o
        sc[r, :o.size] = rows[r][o]
    return ids, sc


def rank(row, target, seen, exclude_seen):
    """0-based rank of `target`: candidates other than it that order before it (a seen target counts as a candidate)."""
    out = set(int(v) for v in seen) - {int(target)} if exclude_seen else set()
    o = order(row, sorted(out))
    return int(np.nonzero(o == int(target))[0][0])


def item_weights(B32, item, k):
    """Top-k of row `item` of B without the item itself: (ids (k,) with -1 padding, values with -inf padding)."""
    o = order(B32[item], (item,))[:k]
    ids = np.full(k, -1, dtype=np.int64)
    sc = np.full(k, -np.inf, dtype=np.float32)
    ids[:o.size] = o
    sc[:o.size] = B32[item][o]
    return ids, sc
