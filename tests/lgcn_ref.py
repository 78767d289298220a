# -*- coding: utf-8 -*-
"""numpy restatement of the LightGCN contract (include/trs.h "LightGCN").  Imports without a GPU.

  neighbour_sums / finish / propagate   the operator trs_lgcn_propagate: with dtype=np.float32 the float32 loop of the
                                        rule (every product and sum rounded on its own, segments of SEG neighbours,
                                        partials added in ascending segment order), with np.float64 the same in double
  horner                                the Horner forward (and, on a gradient, the backward) built from it
  pair_grads                            the pairwise loss of given triples on the propagated tables and dL/dFinal
  step                                  one training step on the base tables, SGD or Adam, in either precision
  dense_adjacency / layer_mean          the paper's definition: dense A^, layers summed then averaged (no Horner)
  autograd_step                         a float64 torch-autograd step written that standard way"""
import numpy as np
import torch

SEG = 512  # TRS_LGCN_SEG


# ------------------------------------------------------------------------------------------------ graphs
def csr_from_pairs(rows, cols, n_rows):
    """(off int64, ids int32) of the DISTINCT (row, col) pairs, ids ascending inside a row."""
    key = np.unique(np.asarray(rows, dtype=np.int64) * (1 << 32) + np.asarray(cols, dtype=np.int64))
    r, c = key >> 32, key & 0xFFFFFFFF
    off = np.zeros(n_rows + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(r, minlength=n_rows))
    return off, c.astype(np.int32)


def dinv(off):
    """float32(1 / sqrt(float64(degree))), 0 for an empty list."""
    deg = np.diff(off).astype(np.float64)
    out = np.zeros(deg.size, dtype=np.float64)
    out[deg > 0] = 1.0 / np.sqrt(deg[deg > 0])
    return out.astype(np.float32)


def make_graph(n_users, n_items, n_pairs, seed):
    """A random bipartite graph as (by_user CSR, by_item CSR, dinv_user, dinv_item)."""
    rs = np.random.RandomState(seed)
    u, i = rs.randint(0, n_users, n_pairs), rs.randint(0, n_items, n_pairs)
    by_user, by_item = csr_from_pairs(u, i, n_users), csr_from_pairs(i, u, n_items)
    return by_user, by_item, dinv(by_user[0]), dinv(by_item[0])


# ------------------------------------------------------------------------------------------------ the operator
def neighbour_sums(inp, off, ids, dinv_in, dtype=np.float32):
    """s (n_out, D): per row the sum of the segments' partials in ascending segment order, a partial being the sum over
    the segment's neighbours c in CSR order, from 0, of dinv_in[c] * inp[c].  An id outside [0, n_in) is skipped.
    Vectorised over the rows (position by position inside a segment), which leaves every row's own order untouched."""
    inp, w = np.asarray(inp, dtype=dtype), np.asarray(dinv_in, dtype=dtype)
    off, ids = np.asarray(off, dtype=np.int64), np.asarray(ids, dtype=np.int64)
    n_out, n_in, D = off.size - 1, inp.shape[0], inp.shape[1]
    lens = np.diff(off)
    s = np.zeros((n_out, D), dtype=dtype)
    for g in range(int(-(-lens.max() // SEG)) if n_out else 0):
        seg_len = np.clip(lens - g * SEG, 0, SEG)
        part = np.zeros((n_out, D), dtype=dtype)
        for j in range(int(seg_len.max())):
            rows = np.nonzero(seg_len > j)[0]
            c = ids[off[rows] + g * SEG + j]
            good = (c >= 0) & (c < n_in)
            rows, c = rows[good], c[good]
            part[rows] = part[rows] + w[c][:, None] * inp[c]
        has = seg_len > 0
        s[has] = s[has] + part[has]
    return s


def finish(s, dinv_out, add=None, scale=1.0, out=None, accumulate=False, dtype=np.float32):
    """out = [out +] scale * ([add +] dinv_out * s), each operation rounded to dtype."""
    p = np.asarray(dinv_out, dtype=dtype)[:, None] * np.asarray(s, dtype=dtype)
    if add is not None:
        p = np.asarray(add, dtype=dtype) + p
    v = dtype(scale) * p
    return (np.asarray(out, dtype=dtype) + v) if accumulate else v


def propagate(inp, nbr, dinv_out, dinv_in, add=None, scale=1.0, out=None, accumulate=False, dtype=np.float32):
    return finish(neighbour_sums(inp, nbr[0], nbr[1], dinv_in, dtype), dinv_out, add, scale, out, accumulate, dtype)


# ------------------------------------------------------------------------------------------------ Horner
def horner(U, V, graph, layers, scale, dtype=np.float32):
    """scale * F_0 with F_K = E, F_k = E + A^ F_{k+1} for E = [U; V]: the forward with E the base tables and scale =
    alpha, the backward with E the gradient.  Both sides of a step read the previous step's values."""
    by_user, by_item, du, di = graph
    U, V = np.asarray(U, dtype=dtype), np.asarray(V, dtype=dtype)
    if layers == 0:
        return dtype(scale) * U, dtype(scale) * V
    Fu, Fv = U, V
    for k in range(layers):
        sc = scale if k == layers - 1 else 1.0
        Fu, Fv = (propagate(Fv, by_user, du, di, add=U, scale=sc, dtype=dtype),
                  propagate(Fu, by_item, di, du, add=V, scale=sc, dtype=dtype))
    return Fu, Fv


def alpha(layers):
    return np.float32(1.0 / (layers + 1))


# ------------------------------------------------------------------------------------------------ the loss
def pair_rows(Fu, Fv, user, pos, neg, loss, dtype=np.float32):
    """(sum of the row losses, then per triple the gradient rows of its user, its positive and its negative) of the MEAN
    pairwise loss of the triples on the propagated tables."""
    Fu, Fv = np.asarray(Fu, dtype=dtype), np.asarray(Fv, dtype=dtype)
    B = user.size
    u, p, n = Fu[user], Fv[pos], Fv[neg]
    zp, zn = (u * p).sum(1, dtype=dtype), (u * n).sum(1, dtype=dtype)
    if loss == "bpr":
        x = zn - zp
        value = np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))
        dneg = dtype(1) / (dtype(1) + np.exp(-x))
    else:
        h = zn - zp + dtype(1)
        value = np.maximum(h, 0)
        dneg = (h >= 0).astype(dtype)
    gn = (dneg * dtype(1.0 / B)).astype(dtype)
    gp = -gn
    return float(value.sum(dtype=np.float64)), gp[:, None] * p + gn[:, None] * n, gp[:, None] * u, gn[:, None] * u


def pair_grads(Fu, Fv, user, pos, neg, loss, dtype=np.float32):
    """(sum of the row losses, dL/dFu, dL/dFv): the rows of pair_rows added into zeroed tables, one add per reference."""
    value, ru, rp, rn = pair_rows(Fu, Fv, user, pos, neg, loss, dtype)
    Gu, Gv = np.zeros(Fu.shape, dtype=dtype), np.zeros(Fv.shape, dtype=dtype)
    np.add.at(Gu, user, ru)
    np.add.at(Gv, pos, rp)
    np.add.at(Gv, neg, rn)
    return value, Gu, Gv


def l2_rows(U, V, user, pos, neg, l2, dtype=np.float32):
    """The per-reference L2 gradient on the base tables: l2 / B times the row, once per reference."""
    c = dtype(l2 / user.size)
    Lu, Lv = np.zeros_like(U), np.zeros_like(V)
    np.add.at(Lu, user, c * U[user])
    np.add.at(Lv, pos, c * V[pos])
    np.add.at(Lv, neg, c * V[neg])
    return Lu, Lv


def adam_constants(lr, beta1, beta2, t):
    """(1 - beta1, beta2, 1 - beta2, lr / (1 - beta1^t), sqrt(1 - beta2^t)) in double, as torch.optim.Adam forms them."""
    return 1.0 - beta1, beta2, 1.0 - beta2, lr / (1.0 - beta1 ** t), (1.0 - beta2 ** t) ** 0.5


def adam_update(p, g, m, v, lr, beta1, beta2, eps, t, dtype=np.float32):
    """torch.optim.Adam's rule, operation by operation, in dtype; returns (p, m, v)."""
    ob1, b2, ob2, step, bc2s = (dtype(c) for c in adam_constants(lr, beta1, beta2, t))
    p, g, m, v = (np.asarray(a, dtype=dtype) for a in (p, g, m, v))
    m = m + ob1 * (g - m)
    v = v * b2 + (ob2 * g) * g
    denom = np.sqrt(v) / bc2s + dtype(eps)
    return p + (-step * m) / denom, m, v


def step(U0, V0, graph, layers, user, pos, neg, loss, lr, l2=0.0, optimizer="sgd", state=None, t=1,
         betas=(0.9, 0.999), eps=1e-8, dtype=np.float32):
    """One training step on the base tables in dtype -> (U0', V0', sum of the row losses, state).  state = (mU, vU, mV, vV)
    for Adam (None: zeros)."""
    U0, V0 = np.asarray(U0, dtype=dtype), np.asarray(V0, dtype=dtype)
    a = alpha(layers)
    Fu, Fv = horner(U0, V0, graph, layers, a, dtype)
    value, Gu, Gv = pair_grads(Fu, Fv, user, pos, neg, loss, dtype)
    if optimizer == "sgd":
        if layers == 0:  # plain matrix factorisation: every reference is added to its base row on its own, at -lr
            _, ru, rp, rn = pair_rows(Fu, Fv, user, pos, neg, loss, dtype)
            Un, Vn = U0.copy(), V0.copy()
            np.add.at(Un, user, dtype(-lr) * ru)
            np.add.at(Vn, pos, dtype(-lr) * rp)
            np.add.at(Vn, neg, dtype(-lr) * rn)
        else:            # the last backward launches add -lr * alpha * H_0 to the base tables
            dU, dV = horner(Gu, Gv, graph, layers, np.float32(-lr * float(a)), dtype)
            Un, Vn = U0 + dU, V0 + dV
        if l2:  # l2 / B times the PRE-update row, once per reference, each added on its own at -lr
            c = dtype(l2 / user.size)
            np.add.at(Un, user, dtype(-lr) * (c * U0[user]))
            np.add.at(Vn, pos, dtype(-lr) * (c * V0[pos]))
            np.add.at(Vn, neg, dtype(-lr) * (c * V0[neg]))
        return Un, Vn, value, None
    gU, gV = horner(Gu, Gv, graph, layers, a, dtype)
    if l2:
        Lu, Lv = l2_rows(U0, V0, user, pos, neg, l2, dtype)
        gU, gV = gU + Lu, gV + Lv
    if state is None:
        state = tuple(np.zeros_like(x) for x in (U0, U0, V0, V0))
    Un, mU, vU = adam_update(U0, gU, state[0], state[1], lr, betas[0], betas[1], eps, t, dtype)
    Vn, mV, vV = adam_update(V0, gV, state[2], state[3], lr, betas[0], betas[1], eps, t, dtype)
    return Un, Vn, value, (mU, vU, mV, vV)


# ------------------------------------------------------------------------------------------------ the paper's form
def dense_adjacency(graph, n_users, n_items):
    """A^ (n_users + n_items square, float64): dinv_u * dinv_i on every pair, both triangles."""
    (off, ids), _, du, di = graph
    A = np.zeros((n_users + n_items, n_users + n_items), dtype=np.float64)
    u = np.repeat(np.arange(n_users), np.diff(off))
    w = du.astype(np.float64)[u] * di.astype(np.float64)[ids]
    A[u, n_users + ids] = w
    A[n_users + ids, u] = w
    return A


def layer_mean(U, V, graph, layers):
    """Final = 1/(K+1) * sum_k A^^k E in float64: every layer formed, then summed, then averaged."""
    n_users, n_items = U.shape[0], V.shape[0]
    A = dense_adjacency(graph, n_users, n_items)
    E = np.concatenate([U, V]).astype(np.float64)
    total, cur = E.copy(), E
    for _ in range(layers):
        cur = A @ cur
        total = total + cur
    total = total / (layers + 1)
    return total[:n_users], total[n_users:]


def autograd_step(U0, V0, graph, layers, user, pos, neg, loss, lr, l2=0.0, optimizer="sgd", steps=1):
    """`steps` float64 torch-autograd steps written the standard way (dense A^, layers summed then averaged, the mean
    pairwise loss plus l2 / (2B) times the squared norm of every referenced base row, torch.optim.SGD / Adam) ->
    (U0', V0', sum of the row losses of the last step)."""
    n_users, n_items = U0.shape[0], V0.shape[0]
    # alpha and dinv are the contract's float32 values: the comparison is about the arithmetic, not about them
    A = torch.from_numpy(dense_adjacency(graph, n_users, n_items))
    a = float(alpha(layers))
    E = torch.from_numpy(np.concatenate([U0, V0]).astype(np.float64)).requires_grad_(True)
    opt = torch.optim.SGD([E], lr=lr) if optimizer == "sgd" else torch.optim.Adam([E], lr=lr)
    u, p, n = (torch.from_numpy(np.asarray(x, dtype=np.int64)) for x in (user, pos, neg))
    B = int(u.numel())
    for _ in range(steps):
        opt.zero_grad()
        total, cur = E, E
        for _k in range(layers):
            cur = A @ cur
            total = total + cur
        F = total * a
        Fu, Fv = F[:n_users], F[n_users:]
        zp, zn = (Fu[u] * Fv[p]).sum(1), (Fu[u] * Fv[n]).sum(1)
        rows = torch.nn.functional.softplus(zn - zp) if loss == "bpr" else torch.clamp(zn - zp + 1.0, min=0.0)
        reg = (E[u] ** 2).sum() + (E[n_users + p] ** 2).sum() + (E[n_users + n] ** 2).sum()
        (rows.mean() + (l2 / (2.0 * B)) * reg).backward()
        opt.step()
    out = E.detach().numpy()
    return out[:n_users].copy(), out[n_users:].copy(), float(rows.detach().sum())
