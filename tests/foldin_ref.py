# -*- coding: utf-8 -*-
"""numpy restatement of the fold-in update rule (trs_fold_in_users, include/trs.h "fold-in").
TEST INFRASTRUCTURE.  The schedule is built only from oracle.loader's restatements of the device streams
(philox4x32_10, feistel_perm, device_negatives) and the rejection sampler (oracle.loader.device_negatives_opt or its
vectorised twin mining_ref.negatives_opt); the arithmetic is float64 unless a dtype is asked for.

For user h with sorted, distinct history `hist` (n_h items), epoch e, visit j:
  r = j (shuffle off) or feistel_perm(j, n_h, key_e), key_e = ((y << 32) | x) | 1 of Philox(counter e, key seed + KEY_STEP)
  p = hist[r];  n = the sampler's draw at counter (e << 32) | r, seed `seed`, positive p, seen = the history itself
  z = (<u, S_i> + b) + c_i;  s = z (linear) | sigmoid(z) (fm);  (value, dneg) = pair loss;  g_p = -dneg w_p, g_n = dneg w_n
  u <- u - lr ((g_p S_p + g_n S_n) + l2 u);  b <- b - lr ((g_p + g_n) + l2 b);  loss[e] += value, / n_h after the epoch
"""
import numpy as np

import mining_ref
from oracle import loader

KEY_STEP = 0xD1B54A32D192ED03
MASK64 = (1 << 64) - 1


def epoch_key(seed, e):
    x, y, _, _ = loader.philox4x32_10(np.array([e], dtype=np.uint64), (int(seed) + KEY_STEP) & MASK64)
    return ((int(y[0]) << 32) | int(x[0])) | 1


def visit_order(n_h, seed, e, shuffle):
    """(n_h,) history positions r in visit order."""
    if not shuffle:
        return np.arange(n_h, dtype=np.int64)
    key = epoch_key(seed, e)
    return np.array([loader.feistel_perm(j, n_h, key) for j in range(n_h)], dtype=np.int64)


def negatives_by_position(hist, n_items, seed, e, reject_seen, max_tries, vectorised=True):
    """(n_h,) the negative of history position r in epoch e (counter (e << 32) | r): it does not depend on the user's
    index, only on the history."""
    hist = np.asarray(hist, dtype=np.int64)
    if hist.size == 0:
        return np.zeros(0, dtype=np.int64)
    offset = int(e) << 32
    if not reject_seen:
        return loader.device_negatives(hist, n_items, seed, offset)
    seen = (np.array([0, hist.size], dtype=np.int64), hist)
    fn = mining_ref.negatives_opt if vectorised else loader.device_negatives_opt
    return fn(np.zeros(hist.size, dtype=np.int64), hist, n_items, seed, offset, seen=seen, max_tries=max_tries)


def schedule(hist, n_items, epochs, seed, shuffle, reject_seen, max_tries):
    """Per epoch (r, p, n), each (n_h,) in visit order."""
    hist = np.asarray(hist, dtype=np.int64)
    out = []
    for e in range(epochs):
        r = visit_order(hist.size, seed, e, shuffle)
        neg = negatives_by_position(hist, n_items, seed, e, reject_seen, max_tries)
        out.append((r, hist[r], neg[r]))
    return out


_SCHEDULES = {}


def schedules(hists, n_items, epochs, seed, shuffle, reject_seen, max_tries):
    """schedule() of every history, computed once per distinct argument set (it depends on neither the tables nor D)."""
    key = (tuple(np.asarray(h, dtype=np.int64).tobytes() for h in hists), n_items, epochs, seed, bool(shuffle),
           bool(reject_seen), max_tries)
    if key not in _SCHEDULES:
        _SCHEDULES[key] = [schedule(h, n_items, epochs, seed, shuffle, reject_seen, max_tries) for h in hists]
    return _SCHEDULES[key]


def _pair_loss(loss, sp, sn, one):
    """trs_pair_loss in the dtype of its arguments, element-wise: (value, dneg)."""
    if loss == "bpr":
        x = sn - sp
        return np.maximum(x, 0 * one) + np.log1p(np.exp(-np.abs(x))), one / (one + np.exp(-x))
    h = sn - sp + one
    return np.maximum(h, 0 * one), np.where(h >= 0, one, 0 * one)


def _dots(U, R, order):
    """Row-wise <U_i, R_i>: 'exact' numpy's float64 sum; 'asc' / 'desc' every product rounded to the dtype, then a
    sequential sum over the columns in that order."""
    prod = U * R
    if order == "exact":
        return prod.sum(axis=1)
    if order == "desc":
        prod = prod[:, ::-1]
    return np.add.accumulate(prod, axis=1)[:, -1]


def fold_in(S, c, hists, net, loss, epochs, lr, l2, seed=0, shuffle=True, reject_seen=True, max_tries=8, D=None,
            dtype=np.float64, order="exact", require_exact=False):
    """Every history of a call, each independently of the others (that is the rule); the users advance in lock-step,
    visit t of all users that have one at a time.  S (n_items, Dp), c (n_items,).
    Returns dict: U (n, D), b (n,), loss (epochs, n) in `dtype`; negs (per user an (epochs, n_h) array in visit order);
    active = visits with dneg != 0 (under hinge: the active ones), visits; bound = max over visits and both items of
    (sum_d |u_d S_d| + |b| + |c|) * 64.  require_exact: assert bound < 2^24 at every visit (every fp32 order of the sums
    is then exact when all values are multiples of 2^-6)."""
    f = dtype
    S, c = np.asarray(S, dtype=f), np.asarray(c, dtype=f)
    n_items, Dp = S.shape
    D = Dp if D is None else D
    hists = [np.asarray(h, dtype=np.int64) for h in hists]
    n = len(hists)
    one, lr, l2 = f(1), f(lr), f(l2)
    sched = schedules(hists, n_items, epochs, seed, shuffle, reject_seen, max_tries)
    lens = np.array([h.size for h in hists], dtype=np.int64)
    tmax = int(lens.max()) if n else 0
    U, b = np.zeros((n, Dp), dtype=f), np.zeros(n, dtype=f)
    losses = np.zeros((epochs, n), dtype=f)
    active = visits = 0
    bound = 0.0
    for e in range(epochs):
        P = np.zeros((n, tmax), dtype=np.int64)
        N = np.zeros((n, tmax), dtype=np.int64)
        for i in range(n):
            P[i, :lens[i]], N[i, :lens[i]] = sched[i][e][1], sched[i][e][2]
        tot = np.zeros(n, dtype=f)
        for t in range(tmax):
            a = np.nonzero(lens > t)[0]
            p, q = P[a, t], N[a, t]
            Ua, ba, Sp, Sn = U[a], b[a], S[p], S[q]
            for R, ci in ((Sp, c[p]), (Sn, c[q])):
                bv = 64.0 * (np.abs(Ua.astype(np.float64) * R).sum(axis=1) + np.abs(ba) + np.abs(ci)).max()
                bound = max(bound, float(bv))
            zp = (_dots(Ua, Sp, order) + ba) + c[p]
            zn = (_dots(Ua, Sn, order) + ba) + c[q]
            if net == "fm":
                sp, sn = one / (one + np.exp(-zp)), one / (one + np.exp(-zn))
                wp, wn = sp * (one - sp), sn * (one - sn)
            else:
                sp, sn, wp, wn = zp, zn, one, one
            value, dneg = _pair_loss(loss, sp, sn, one)
            gp, gn = -dneg * wp, dneg * wn
            U[a] = Ua - lr * ((gp[:, None] * Sp + gn[:, None] * Sn) + l2 * Ua)
            b[a] = ba - lr * ((gp + gn) + l2 * ba)
            tot[a] = tot[a] + value
            visits += a.size
            active += int((dneg != 0).sum())
        nz = lens > 0
        losses[e, nz] = tot[nz] / lens[nz].astype(f)
    if require_exact:
        assert bound < 2.0 ** 24, bound
    assert U.dtype == f and b.dtype == f and losses.dtype == f
    return {"U": U[:, :D].copy(), "b": b, "loss": losses,
            "negs": [np.array([s[2] for s in sc], dtype=np.int64).reshape(epochs, -1) for sc in sched],
            "active": active, "visits": visits, "bound": bound}


def fold_in_one(S, c, hist, net, loss, epochs, lr, l2, **kw):
    """fold_in of one history alone: u (D,), b, loss (epochs,) and the rest."""
    o = fold_in(S, c, [hist], net, loss, epochs, lr, l2, **kw)
    return dict(o, u=o["U"][0], b=o["b"][0], loss=o["loss"][:, 0], negs=o["negs"][0])


def clean(histories):
    """Sorted, distinct form of every history (what fold_in_users makes of its input)."""
    return [np.unique(np.asarray(h, dtype=np.int64)) for h in histories]


SPECIAL_LENGTHS = (0, 1, 2, 63, 64, 65, 150, 199, 200)


def histories(n_items, seed, n_random=300, max_random=20, special=SPECIAL_LENGTHS):
    """The test histories: one per special length (capped at n_items), then n_random of random length 0..max_random."""
    rs = np.random.RandomState(seed)
    lens = [min(s, n_items) for s in special] + rs.randint(0, max_random + 1, n_random).tolist()
    return [np.sort(rs.choice(n_items, size=n, replace=False)).astype(np.int64) for n in lens]


def planted(D, seed=0):
    """The planted case: 96 items whose folded rows are +4 e_0 (items 0..47) or -4 e_0 (items 48..95) plus noise in
    {-1, 0, 1} on the other columns, zero constants, and a history of 12 items of the first half."""
    rs = np.random.RandomState(seed)
    S = rs.randint(-1, 2, (96, D)).astype(np.float64)
    S[:48, 0], S[48:, 0] = 4.0, -4.0
    hist = np.sort(rs.choice(48, size=12, replace=False)).astype(np.int64)
    return S, np.zeros(96), hist


def make_model(net_type, n_users, n_items, D, M=0, seed=0, int_range=None, scale=1.0, **kw):
    """A TorchRecSys over every user and item id (needs no GPU), its parameters overwritten from a seeded generator:
    integers of int_range (every fp32 product and sum of the tests is then exact) or scale * randn."""
    import contextlib
    import io

    import torch
    from torchrecsys_amd.model import TorchRecSys
    rs = np.random.RandomState(seed)
    n = max(4 * n_users, 2 * n_items)
    u = np.concatenate([np.arange(n_users), rs.randint(0, n_users, n - n_users)])
    i = np.concatenate([np.arange(n_items), rs.randint(0, n_items, n - n_items)])
    meta = torch.from_numpy(rs.randint(0, 5, (n_items, M))) if M else None
    with contextlib.redirect_stdout(io.StringIO()):
        torch.manual_seed(seed)
        np.random.seed(seed)
        m = TorchRecSys.from_tensors(torch.from_numpy(u), torch.from_numpy(i), n_users=n_users, n_items=n_items,
                                     item_metadata=meta, metadata_names=[f"m{j}" for j in range(M)] if M else None,
                                     n_factors=D, net_type=net_type, **kw)
    g = torch.Generator().manual_seed(seed + 1)
    for p in m.net.parameters():
        if int_range is not None:
            p.data.copy_(torch.randint(int_range[0], int_range[1], p.shape, generator=g).float())
        else:
            p.data.copy_(scale * torch.randn(p.shape, generator=g))
    return m


def item_side(m):
    """float64 (S (n_items, D), c (n_items,)) of a Linear / FM model's parameters (include/trs.h "retrieval")."""
    P = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.net.state_dict().items()}
    tab = m.data_processor.item_meta_table
    M = 0 if tab is None else tab.shape[1]
    I = P["item.weight"]
    metas = [P[f"metadata.{j}.weight"][np.asarray(tab)[:, j]] for j in range(M)]
    S = I + sum(metas) if metas else I.copy()
    if m.net_type == "linear":
        return S, P["item_bias.weight"][:, 0].copy()
    lin = P["linear_item.weight"][:, 0].copy()
    for j in range(M):
        lin = lin + P[f"linear_metadata.{j}.weight"][np.asarray(tab)[:, j], 0]
    return S, lin + 0.5 * ((S * S).sum(1) - (I * I).sum(1) - sum((x * x).sum(1) for x in metas))


def rank(U, b, S, c, seen, k):
    """Top-k of (U @ S.T + b) + c per row in float64, ties by ascending row, `seen[r]` excluded; ids (n, k) with -1 and
    values (n, k) with -inf beyond the candidates."""
    z = (np.asarray(U, np.float64) @ np.asarray(S, np.float64)[:, :U.shape[1]].T + np.asarray(b, np.float64)[:, None]) \
        + np.asarray(c, np.float64)[None, :]
    n, n_items = z.shape
    ids = np.full((n, k), -1, dtype=np.int64)
    vals = np.full((n, k), -np.inf)
    for r in range(n):
        zr = z[r].copy()
        if seen is not None:
            zr[np.asarray(seen[r], dtype=np.int64)] = -np.inf
        o = np.argsort(-zr, kind="stable")[:k]
        o = o[np.isfinite(zr[o])]
        ids[r, :o.size] = o
        vals[r, :o.size] = zr[o]
    return ids, vals
