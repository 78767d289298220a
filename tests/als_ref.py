# -*- coding: utf-8 -*-
"""numpy restatement of the implicit-ALS rule of include/trs.h ("implicit ALS": trs_als_gram / trs_als_solve) and of the
objective fit_als(return_loss=True) reports.

half_sweep(..., dtype=float64)                 the reference the GPU tests compare against
half_sweep(..., dtype=float32, order=...)      every product and sum rounded to fp32 as the kernel does, the sums over the
                                               factors (y . v, r . r, p . A p, and the e of G v) taken sequentially in
                                               ascending ('asc') or descending ('desc') column order.  The kernel's
                                               butterfly is a third order; the spread between these two and float64 is
                                               what the GPU tolerance is derived from (tests/test_gpu_als.py).
The sums over the neighbours (acc, s) always run sequentially in CSR order, as the rule fixes them."""
import numpy as np

RHO_STOP = 1e-20


def random_lists(n_rows, n_other, seed, fixed=()):
    """n_rows sorted, distinct id lists over [0, n_other): the lengths `fixed`, then random lengths 0..20."""
    rs = np.random.RandomState(seed)
    lens = list(fixed) + rs.randint(0, min(20, n_other) + 1, n_rows - len(fixed)).tolist()
    return [np.sort(rs.choice(n_other, n, replace=False)).astype(np.int32) for n in lens]


def histories(n_items, seed, n_users=150):
    """n_users sorted, distinct item lists: lengths 0, 1, 2, 63, 64, 65, n_items - 1, n_items, then random 0..20."""
    return random_lists(n_users, n_items, seed, (0, 1, 2, 63, 64, 65, n_items - 1, n_items))


def tables(n_users, n_items, D, seed, scale=0.3):
    """(X (n_users, D), Y (n_items, D)) float32: scale * randn from a seeded generator."""
    rs = np.random.RandomState(seed)
    return ((scale * rs.randn(n_users, D)).astype(np.float32), (scale * rs.randn(n_items, D)).astype(np.float32))


EXACT_LAMBDA, EXACT_ALPHA, EXACT_BITS = 1.0, 3.0, 5


def exact_case(D, n_rows=70):
    """(X start values, Y, lists) on which every fp32 operation of the rule is exact at lambda = 1, alpha = 3.
    Y: one-hot rows of value 1; column c has 4, 12 or 28 of them (c mod 3), so G = diag(4 | 12 | 28).  Row h takes 1..3
    neighbours in distinct columns of ONE type and starts from 0 (h even) or from integers in [-1, 1] on those columns
    (h odd), so on the support of its residual A = (g + lambda + alpha) I = 8 | 16 | 32 times the identity: one step
    with a = 1 / 8 | 1 / 16 | 1 / 32 lands on the solution 0.5 | 0.25 | 0.125 and leaves r = 0.  Every intermediate is
    a multiple of 2^-5 and the largest, p . A p <= 3 * 36 * 1152, stays below 2^19 (half_sweep(exact_bits=5) asserts
    |value| * 2^5 < 2^24 for each).  Row 0 has an empty list."""
    rs = np.random.RandomState(D)
    per = (4, 12, 28)
    col_rows, rows = [], []
    for c in range(D):
        col_rows.append(list(range(len(rows), len(rows) + per[c % 3])))
        rows += [c] * per[c % 3]
    Y = np.zeros((len(rows), D), dtype=np.float32)
    Y[np.arange(len(rows)), rows] = 1.0
    X = np.zeros((n_rows, D), dtype=np.float32)
    lists = [np.zeros(0, np.int32)]
    for h in range(1, n_rows):
        cols = np.arange(h % 3, D, 3)
        cols = rs.choice(cols, min(1 + h % 3 if h % 2 else 1 + (h // 2) % 3, cols.size), replace=False)
        lists.append(np.sort([col_rows[c][rs.randint(per[c % 3])] for c in cols]).astype(np.int32))
        if h % 2:
            X[h, cols] = rs.randint(-1, 2, cols.size)
    return X, Y, lists


def csr(lists):
    """(offsets int64 (n + 1,), ids int32) of a list of id lists."""
    off = np.concatenate([[0], np.cumsum([len(h) for h in lists])]).astype(np.int64)
    ids = np.concatenate([np.asarray(h, dtype=np.int32) for h in lists] + [np.zeros(0, np.int32)])
    return off, ids


def transpose(lists, n_other):
    """The lists of the other side: entry j = the sorted rows r whose list holds j."""
    out = [[] for _ in range(n_other)]
    for r, h in enumerate(lists):
        for j in h:
            out[int(j)].append(r)
    return [np.asarray(o, dtype=np.int32) for o in out]


def _seq_sum(P, axis, dtype, order="asc"):
    """Sum of P along `axis`: float32 strictly sequential from the first element in the given order (ufunc.accumulate
    adds one element at a time), float64 numpy's own (the order is far below what the tests resolve)."""
    if dtype == np.float64:
        return P.sum(axis=axis)
    if order == "desc":
        P = np.flip(P, axis=axis)
    if P.shape[axis] == 0:
        return np.zeros(np.delete(P.shape, axis), dtype=dtype)
    return np.take(np.add.accumulate(P, axis=axis, dtype=dtype), -1, axis=axis)


def gram(Y, dtype=np.float64, order="asc"):
    """G = Y^T Y, every product rounded to dtype, the sum over the rows sequential (float32) in `order`."""
    Y = np.asarray(Y, dtype=dtype)
    G = np.empty((Y.shape[1], Y.shape[1]), dtype=dtype)
    for a in range(Y.shape[1]):
        G[a] = _seq_sum(Y[:, a:a + 1] * Y, 0, dtype, order)
    return G


class _Exact:
    """require_exact: every intermediate is a multiple of 2^-bits below 2^(24 - bits) in magnitude, so that every fp32
    product and sum of the rule is exact in every order; `bound` keeps the largest |value| * 2^bits seen."""

    def __init__(self, bits):
        self.scale, self.bound = float(2 ** bits), 0.0

    def __call__(self, v):
        v = np.asarray(v, dtype=np.float64) * self.scale
        assert np.all(v == np.round(v)), "an intermediate is not a multiple of 2^-bits"
        self.bound = max(self.bound, float(np.abs(v).max()) if v.size else 0.0)
        assert self.bound < 2 ** 24, self.bound
        return None


def solve_row(x, Yn, G, lam, alpha, cg_steps, dtype=np.float64, order="asc", exact=None):
    """One row of trs_als_solve: start value x (D,), neighbour rows Yn (|N|, D) in CSR order, Gram matrix G (D, D).
    Returns (x, steps taken)."""
    f = dtype
    x = np.asarray(x, dtype=f).copy()
    if Yn.shape[0] == 0:
        return np.zeros_like(x), 0
    Yn, G = np.asarray(Yn, dtype=f), np.asarray(G, dtype=f)
    lam, alpha = f(lam), f(alpha)
    one_alpha = f(f(1.0) + alpha)
    chk = exact if exact is not None else (lambda v: None)

    def dot(a, b):
        return _seq_sum(a * b, a.ndim - 1, f, order)

    def amul(v):
        gv = _seq_sum(G * v[:, None], 0, f, order)  # sum_e G[e][d] * v_e
        d = dot(Yn, v[None, :])  # (|N|,)
        acc = _seq_sum(d[:, None] * Yn, 0, f)  # CSR order
        chk(gv), chk(d), chk(d[:, None] * Yn), chk(acc), chk(lam * v), chk(alpha * acc)
        out = (gv + lam * v) + alpha * acc
        chk(gv + lam * v), chk(out)
        return out

    s = _seq_sum(Yn, 0, f)
    b = one_alpha * s
    ax = amul(x)
    r = b - ax
    p = r.copy()
    rho = dot(r, r)
    chk(s), chk(b), chk(r), chk(r * r), chk(rho)
    steps = 0
    if rho < RHO_STOP:
        return x, steps
    for _ in range(int(cg_steps)):
        ap = amul(p)
        pap = dot(p, ap)
        a = f(rho / pap)
        chk(p * ap), chk(pap), chk(a), chk(a * p), chk(a * ap)
        x = x + a * p
        r = r - a * ap
        rho2 = dot(r, r)
        chk(x), chk(r), chk(rho2)
        steps += 1
        if rho2 < RHO_STOP:
            break
        beta = f(rho2 / rho)
        chk(beta), chk(beta * p)
        p = r + beta * p
        chk(p)
        rho = rho2
    return x, steps


def half_sweep(X, Y, lists, lam, alpha, cg_steps, dtype=np.float64, order="asc", G=None, exact_bits=None):
    """Every row of X re-solved against the frozen Y (lists[h] = the sorted, distinct rows of Y of row h).  Returns the
    new X in `dtype` (and leaves its arguments alone).  G: the Gram matrix to use (default: gram(Y) in dtype / order).
    exact_bits: assert that every intermediate is exact in fp32 (see _Exact); the bound is left in half_sweep.bound."""
    X = np.asarray(X, dtype=dtype)
    Y = np.asarray(Y, dtype=dtype)
    if G is None:
        G = gram(Y, dtype, order)
    exact = _Exact(exact_bits) if exact_bits is not None else None
    if exact is not None:
        exact(G)
    out = np.empty_like(X)
    for h, N in enumerate(lists):
        out[h], _ = solve_row(X[h], Y[np.asarray(N, dtype=np.int64)], G, lam, alpha, cg_steps, dtype, order, exact)
    half_sweep.bound = exact.bound if exact is not None else None
    return out


def iteration(X, Y, user_lists, item_lists, lam, alpha, cg_steps, dtype=np.float64, order="asc"):
    """One fit_als iteration: the user half-sweep, then the item half-sweep.  Returns (X, Y)."""
    X = half_sweep(X, Y, user_lists, lam, alpha, cg_steps, dtype, order)
    Y = half_sweep(Y, X, item_lists, lam, alpha, cg_steps, dtype, order)
    return X, Y


def loss(X, Y, user_lists, lam, alpha):
    """The objective in float64:
    L = sum_u x_u^T G_Y x_u + sum_{(u,i) observed} [(1 + alpha)(1 - s_ui)^2 - s_ui^2] + lam (|X|^2 + |Y|^2)."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    total = float(((X.T @ X) * (Y.T @ Y)).sum()) + lam * (float((X * X).sum()) + float((Y * Y).sum()))
    for u, N in enumerate(user_lists):
        if len(N):
            s = Y[np.asarray(N, dtype=np.int64)] @ X[u]
            total += float(((1.0 + alpha) * (1.0 - s) ** 2 - s ** 2).sum())
    return total


def dense_solution(Y, N, lam, alpha):
    """The weighted least-squares row ALS converges to: (Y^T C Y + lam I)^-1 Y^T C p with confidence 1 + alpha and
    preference 1 on N, confidence 1 and preference 0 elsewhere (Hu, Koren, Volinsky 2008, eq. 4), by a dense solve."""
    Y = np.asarray(Y, dtype=np.float64)
    c = np.ones(Y.shape[0])
    pref = np.zeros(Y.shape[0])
    c[np.asarray(N, dtype=np.int64)] += alpha
    pref[np.asarray(N, dtype=np.int64)] = 1.0
    A = Y.T @ (c[:, None] * Y) + lam * np.eye(Y.shape[1])
    return np.linalg.solve(A, Y.T @ (c * pref))
