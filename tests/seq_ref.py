# -*- coding: utf-8 -*-
"""The sequence model of include/trs.h ("sequence model") restated in numpy, with nothing of the library in it:

    q(u, k) = U[u] + sum_{l < min(L, k)} w_l C[s_u[k-1-l]]      z(u, k, i) = <q, V[i]> + b[i]

staged(): the staged gradients and the loss of one batch, in float64 or in float32 with a selectable order of the inner
product's sum; user_rows(): trs_seq_user_rows as a float32 loop; step(): one plain-SGD step; fit(): whole epochs of
sequential batches in float64; evaluate_next(): the held-out item's metrics.  The reference project has no sequence
model, so no program text of it is involved."""
import numpy as np

ORDERS = ("sequential", "pairwise", "tree")


def weights(L, decay):
    """w_l = decay^l / sum_j decay^j in float64, rounded to float32 once (ops.seq_weights)."""
    w = [float(decay) ** l for l in range(int(L))]
    return np.array([x / sum(w) for x in w], dtype=np.float32)


def make_sequences(n_users, n_items, lengths, seed):
    """Random ordered sequences: (offsets int64 (n_users + 1,), ids int32), user u's length lengths[u % len]."""
    rs = np.random.RandomState(seed)
    lens = np.array([lengths[u % len(lengths)] for u in range(n_users)], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return off, rs.randint(0, n_items, int(off[-1])).astype(np.int32)


def make_tables(n_users, n_items, D, seed, scale=0.3):
    rs = np.random.RandomState(seed)
    f = lambda *s: (scale * rs.standard_normal(s)).astype(np.float32)
    return {"U": f(n_users, D), "V": f(n_items, D), "b": f(n_items), "C": f(n_items, D)}


def _dots(A, Bm, dtype, order):
    """Row-wise <A[t], Bm[t]> with the products rounded to dtype and summed in the given order (float64: any)."""
    p = (A * Bm).astype(dtype)
    n, D = p.shape
    if dtype == np.float64:
        return p.sum(1)
    if order == "sequential":
        return np.cumsum(p, axis=1, dtype=dtype)[:, -1]
    if order == "pairwise":
        m = 1
        while m < D:
            m *= 2
        v = np.zeros((n, m), dtype=dtype)
        v[:, :D] = p
        while v.shape[1] > 1:
            v = (v[:, 0::2] + v[:, 1::2]).astype(dtype)
        return v[:, 0]
    # "tree": a lane group — lanes of 4 consecutive columns summed in order, then a butterfly over the lanes
    g = 1
    while g < -(-D // 4):
        g *= 2
    v = np.zeros((n, 4 * g), dtype=dtype)
    v[:, :D] = p
    v = np.cumsum(v.reshape(n, g, 4), axis=2, dtype=dtype)[:, :, -1]
    while v.shape[1] > 1:
        h = v.shape[1] // 2
        v = (v[:, :h] + v[:, h:]).astype(dtype)
    return v[:, 0]


def pair_loss(loss, zp, zn, dtype):
    """(values, d value / d z_n) of trs_pair_loss, element-wise."""
    zp, zn = np.asarray(zp, dtype=dtype), np.asarray(zn, dtype=dtype)
    if loss == "bpr":
        x = (zn - zp).astype(dtype)
        val = (np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)).astype(dtype)).astype(dtype)).astype(dtype)
        return val, (dtype(1) / (dtype(1) + np.exp(-x).astype(dtype)).astype(dtype)).astype(dtype)
    h = ((zn - zp).astype(dtype) + dtype(1)).astype(dtype)
    return np.maximum(h, 0).astype(dtype), (h >= 0).astype(dtype)


def query(T, off, ids, u, k, w, dtype, last=None):
    """q(u, k) (u < 0: no user row) and the present context ids, most recent first.  `last`: index of the most recent
    context item in ids (default off[u] + k - 1)."""
    D = T["C"].shape[1]
    q = T["U"][u].astype(dtype).copy() if u >= 0 else np.zeros(D, dtype=dtype)
    if last is None:
        last = int(off[u]) + k - 1
    ctx = []
    for l in range(min(len(w), k)):
        c = int(ids[last - l])
        ctx.append(c)
        q = (q + (dtype(w[l]) * T["C"][c].astype(dtype)).astype(dtype)).astype(dtype)
    return q, ctx


def staged(T, off, ids, user, entry, neg, w, loss, inv_B=None, dtype=np.float64, order="sequential"):
    """One batch: (grad_rows (3 + L, B, D), grad_lin (3, B), ctx_ids (L, B) int32, loss_sum, auc_count).  Every
    operation is rounded to dtype on its own (no fused multiply-add), as the library is built."""
    user, entry, neg = (np.asarray(a, dtype=np.int64) for a in (user, entry, neg))
    B, L, D = len(user), len(w), T["U"].shape[1]
    inv_B = dtype(1.0 / B if inv_B is None else inv_B)
    gr, gl = np.zeros((3 + L, B, D), dtype=dtype), np.zeros((3, B), dtype=dtype)
    cid = np.zeros((L, B), dtype=np.int32)
    k, p = entry - off[user], ids[entry].astype(np.int64)
    q = T["U"][user].astype(dtype)
    present = np.zeros((L, B), dtype=bool)
    for l in range(L):
        present[l] = k > l
        cid[l] = np.where(present[l], ids[np.maximum(entry - 1 - l, 0)], 0)
        s = (q + (dtype(w[l]) * T["C"][cid[l]].astype(dtype)).astype(dtype)).astype(dtype)
        q = np.where(present[l][:, None], s, q)
    vp, vn = T["V"][p].astype(dtype), T["V"][neg].astype(dtype)
    zp = (_dots(q, vp, dtype, order) + T["b"][p].astype(dtype)).astype(dtype)
    zn = (_dots(q, vn, dtype, order) + T["b"][neg].astype(dtype)).astype(dtype)
    val, dneg = pair_loss(loss, zp, zn, dtype)
    gn = (dneg * inv_B).astype(dtype)
    gp = (-gn).astype(dtype)
    gu = ((gp[:, None] * vp).astype(dtype) + (gn[:, None] * vn).astype(dtype)).astype(dtype)
    gr[0], gr[1], gr[2] = gu, (gp[:, None] * q).astype(dtype), (gn[:, None] * q).astype(dtype)
    gl[0], gl[1], gl[2] = (gp + gn).astype(dtype), gp, gn
    for l in range(L):
        gr[3 + l] = np.where(present[l][:, None], (dtype(w[l]) * gu).astype(dtype), dtype(0))
    return gr, gl, cid, float(val.astype(np.float64).sum()), int((zp > zn).sum())


def user_rows(T, off, ids, users, w, ld=None):
    """trs_seq_user_rows as a float32 loop: (n, ld) rows, columns beyond D zero."""
    n, D = len(off) - 1, T["C"].shape[1]
    out = np.zeros((n, D if ld is None else ld), dtype=np.float32)
    for r in range(n):
        u = -1 if users is None else int(users[r])
        q, _ = query(T, off, ids, u, int(off[r + 1] - off[r]), w, np.float32, last=int(off[r + 1]) - 1)
        out[r, :D] = q
    return out


def step(T, off, ids, user, entry, neg, w, loss, lr, dtype=np.float64, scatter_order=None, order="sequential"):
    """One plain-SGD step in place: every staged row times -lr (rounded), added to its table row in scatter_order (a
    permutation of the batch; None: ascending).  Returns the batch's loss sum."""
    gr, gl, cid, loss_sum, _ = staged(T, off, ids, user, entry, neg, w, loss, dtype=dtype, order=order)
    B = len(user)
    pos = ids[np.asarray(entry, dtype=np.int64)]
    alpha = dtype(-lr)
    tabs = {k: v.astype(dtype) for k, v in T.items()}
    for t in (range(B) if scatter_order is None else scatter_order):
        tabs["U"][user[t]] = (tabs["U"][user[t]] + (alpha * gr[0, t]).astype(dtype)).astype(dtype)
        for f, i in ((1, int(pos[t])), (2, int(neg[t]))):
            tabs["V"][i] = (tabs["V"][i] + (alpha * gr[f, t]).astype(dtype)).astype(dtype)
            tabs["b"][i] = dtype(tabs["b"][i] + dtype(alpha * gl[f, t]))
        for l in range(len(w)):
            c = int(cid[l, t])
            tabs["C"][c] = (tabs["C"][c] + (alpha * gr[3 + l, t]).astype(dtype)).astype(dtype)
    for k in T:
        T[k] = tabs[k]
    return loss_sum


def holdout(off):
    """(train positions, held-out users, held-out positions) of fit_sequence(holdout_last=True)."""
    lens = np.diff(off)
    users = np.nonzero(lens >= 2)[0]
    held = off[1:][users] - 1
    keep = np.ones(int(off[-1]), dtype=bool)
    keep[held] = False
    return np.nonzero(keep)[0], users, held


def fit(T, off, ids, entries, w, loss, lr, batch, epochs, seed):
    """Whole epochs in float64, sequential batches: every epoch a numpy permutation of `entries`, uniform negatives
    other than the row's positive.  Tables are updated in place (as float64)."""
    rs = np.random.RandomState(seed)
    n_items = T["V"].shape[0]
    user_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
    for k in T:
        T[k] = T[k].astype(np.float64)
    for _ in range(epochs):
        ent = entries[rs.permutation(len(entries))]
        for s in range(0, len(ent), batch):
            e = ent[s:s + batch]
            p = ids[e].astype(np.int64)
            r = rs.randint(0, n_items - 1, len(e))
            fast_step(T, off, ids, user_of[e], e, r + (r >= p), w, loss, lr)
    return T


def fast_step(T, off, ids, user, entry, neg, w, loss, lr):
    """step() in float64, vectorised over the batch (numpy scatter-adds; same mathematics)."""
    B, L = len(user), len(w)
    k = entry - off[user]
    q = T["U"][user].copy()
    ctx = np.zeros((L, B), dtype=np.int64)
    present = np.zeros((L, B), dtype=bool)
    for l in range(L):
        present[l] = k > l
        ctx[l] = np.where(present[l], ids[np.maximum(entry - 1 - l, 0)], 0)
        q += np.where(present[l][:, None], float(w[l]) * T["C"][ctx[l]], 0.0)
    p = ids[entry].astype(np.int64)
    vp, vn = T["V"][p], T["V"][neg]
    x = ((q * vn).sum(1) + T["b"][neg]) - ((q * vp).sum(1) + T["b"][p])
    if loss == "bpr":
        dneg = 1.0 / (1.0 + np.exp(-x))
    else:
        dneg = (x + 1.0 >= 0).astype(np.float64)
    gn = dneg / B
    gu = gn[:, None] * (vn - vp)
    np.add.at(T["U"], user, -lr * gu)
    np.add.at(T["V"], p, -lr * (-gn[:, None] * q))
    np.add.at(T["V"], neg, -lr * (gn[:, None] * q))
    np.add.at(T["b"], p, lr * gn)
    np.add.at(T["b"], neg, -lr * gn)
    for l in range(L):
        np.add.at(T["C"], ctx[l], -lr * np.where(present[l][:, None], float(w[l]) * gu, 0.0))


def ranks_of(scores, target, excluded):
    """0-based rank of `target`: candidates other than it ordered before it (value descending, ties by ascending id),
    the excluded ids taken out (the target itself stays a candidate)."""
    s = scores.copy()
    ex = np.array([i for i in excluded if i != target], dtype=np.int64)
    v = s[target]
    before = (s > v) | ((s == v) & (np.arange(len(s)) < target))
    before[ex] = False
    return int(before.sum())


def evaluate_next(T, off, ids, w, k, context=True):
    """hit rate, NDCG and MRR at k of every held-out last item given what precedes it (context=False: U[u] alone)."""
    _, users, held = holdout(off)
    hit = ndcg = mrr = 0.0
    for u, h in zip(users, held):
        n_prev = int(h - off[u])
        if context:
            q, _ = query(T, off, ids, int(u), n_prev, w, np.float64)
        else:
            q = T["U"][u].astype(np.float64)
        r = ranks_of(T["V"].astype(np.float64) @ q + T["b"], int(ids[h]), set(ids[off[u]:h].tolist()))
        if r < k:
            hit += 1
            ndcg += 1.0 / np.log2(r + 2.0)
            mrr += 1.0 / (r + 1.0)
    n = max(len(users), 1)
    return {"hit_rate": hit / n, "ndcg": ndcg / n, "mrr": mrr / n, "n_users": len(users)}


def planted(n_users, n_items, length, p_follow, seed):
    """Sequences in which the next item is perm[current] with probability p_follow, else uniform: (user ids, item ids)
    of the interactions in input order (user-major, each user's in sequence order), and perm."""
    rs = np.random.RandomState(seed)
    perm = rs.permutation(n_items)
    items = np.zeros((n_users, length), dtype=np.int64)
    items[:, 0] = rs.randint(0, n_items, n_users)
    for j in range(1, length):
        follow = rs.random_sample(n_users) < p_follow
        items[:, j] = np.where(follow, perm[items[:, j - 1]], rs.randint(0, n_items, n_users))
    return np.repeat(np.arange(n_users), length), items.reshape(-1), perm


# The planted-order case of tests/test_gpu_seq.py::test_learns_order (data, training arguments, and what the float64
# restatement reaches on it: tests/test_seq_host.py runs it with three seeds and holds it to both bars).
PLANTED = dict(n_users=300, n_items=200, length=30, p_follow=0.8, data_seed=11, D=16, context=1, decay=0.7, loss="bpr",
               lr=10.0, batch=128, epochs=20, k=10)
PLANTED_REF_HIT = (0.840, 0.837, 0.827)  # hit_rate@10 with context, restatement seeds 0, 1, 2 (spread 0.013)
PLANTED_REF_HIT_NO_CONTEXT = (0.100, 0.097, 0.070)


def planted_case():
    """(user ids, item ids in input order, offsets, ids int32) of PLANTED: input order is user-major, in sequence order."""
    P = PLANTED
    users, items, _ = planted(P["n_users"], P["n_items"], P["length"], P["p_follow"], P["data_seed"])
    off = np.arange(P["n_users"] + 1, dtype=np.int64) * P["length"]
    return users, items, off, items.astype(np.int32)


def planted_fit(seed):
    """The restatement's fit on PLANTED from a seeded N(0, 1/D) start (C = 0, b = 0): hit_rate@k with and without context."""
    P = PLANTED
    _, _, off, ids = planted_case()
    rs = np.random.RandomState(100 + seed)
    D = P["D"]
    T = {"U": rs.standard_normal((P["n_users"], D)) / D, "V": rs.standard_normal((P["n_items"], D)) / D,
         "b": np.zeros(P["n_items"]), "C": np.zeros((P["n_items"], D))}
    w = weights(P["context"], P["decay"])
    fit(T, off, ids, holdout(off)[0], w, P["loss"], P["lr"], P["batch"], P["epochs"], seed)
    return (evaluate_next(T, off, ids, w, P["k"])["hit_rate"],
            evaluate_next(T, off, ids, w, P["k"], context=False)["hit_rate"])
