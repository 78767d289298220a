# -*- coding: utf-8 -*-
"""numpy restatement of the WARP loss (trs_score_warp_fwd_bwd, include/trs.h).  TEST INFRASTRUCTURE,
float64, built on tests/mining_ref.py's `scores64` (the value z) and tests/multineg_ref.py's `prepare` (the candidates).

Row i has user u, positive p and candidates c_0 .. c_{K-1} (items: (1 + K, B), slot 0 the positive).
  violation   h_j = (z(u,c_j) - z(u,p)) + margin; candidate j violates iff h_j > 0 (a NaN does not)
  choice      J = the smallest violating j; trials = J + 1, 0 when nothing violates
  weight      w = weights[J]; rank_weights(): r_N = floor((n_items - 1) / N); 'log' log(max(1, r_N)), 'harmonic' H_{r_N}
  loss        row loss = w * h_J (0 without a violator); d(mean loss)/d z(u,c_J) = w / B, d/d z(u,p) = -w / B
Gradients come out in trs_score_fwd_bwd's staged form, R = 3 + 2M fields per row, uncoalesced: user, positive, chosen
candidate, then per metadata column the positive's and the chosen candidate's.  A row without a violator stages zeros and
reports c_0 as its negative.  The user's 1-wide gradient is an exact 0.
"""
import numpy as np

import mining_ref
from multineg_ref import lin_names, table_names  # noqa: F401  (re-exported for the tests)


def rank_weights(n_items, K, kind="log"):
    """(K,) float64: entry N - 1 is the weight of a row whose first violator came at draw N."""
    out = np.zeros(K)
    for N in range(1, K + 1):
        r = (n_items - 1) // N
        if kind == "log":
            out[N - 1] = np.log(max(1, r))
        elif kind == "harmonic":
            out[N - 1] = sum(1.0 / i for i in range(1, r + 1))
        else:
            raise ValueError(kind)
    return out


def select(z, margin):
    """(h (B, K), J (B,) with -1 = no violator) from z (B, 1 + K), slot 0 the positive."""
    z = np.asarray(z, dtype=np.float64)
    h = (z[:, 1:] - z[:, :1]) + margin
    viol = h > 0  # (False for a NaN)
    J = np.where(viol.any(axis=1), viol.argmax(axis=1), -1)
    return h, J


def near_ties(z, margin, tol):
    """Rows whose choice an fp32 evaluation may make differently: some |h_j| < tol * (1 + |z_p| + |z_cj|) for j up to
    the row's J (every j when nothing violates)."""
    z = np.asarray(z, dtype=np.float64)
    h, J = select(z, margin)
    K = h.shape[1]
    close = np.abs(h) < tol * (1.0 + np.abs(z[:, :1]) + np.abs(z[:, 1:]))
    upto = np.where(J < 0, K - 1, J)
    return (close & (np.arange(K)[None, :] <= upto[:, None])).any(axis=1)


def staged(net, params, user, items, item_meta, margin, weights, J=None):
    """dict: loss (mean over the rows), row_loss (B,), trials (B,), neg (B,), neg_meta (B, M) or None, gr (R, B, D),
    gl (R, B), z (B, 1 + K), h (B, K) — float64 / int64.  J: hold the choice fixed (the autograd comparison)."""
    P = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    user, items = np.asarray(user, dtype=np.int64), np.asarray(items, dtype=np.int64)
    S1, B = items.shape
    M = len([k for k in P if k.startswith("metadata.")])
    D = P["user.weight"].shape[1]
    z = mining_ref.scores64(net, P, user, items.T, item_meta)
    h, J_own = select(z, margin)
    J = J_own if J is None else np.asarray(J)
    found = J >= 0
    Jc = np.maximum(J, 0)
    rows = np.arange(B)
    w = np.where(found, np.asarray(weights, dtype=np.float64)[Jc], 0.0)
    row_loss = np.where(found, w * h[rows, Jc], 0.0)
    pos, neg = items[0], items[1 + Jc, rows]  # (c_0 without a violator)
    gn, gp = w / B, -w / B
    U, Ip, In = P["user.weight"][user], P["item.weight"][pos], P["item.weight"][neg]
    meta = None if item_meta is None or M == 0 else np.asarray(item_meta)
    Mp = [P[f"metadata.{m}.weight"][meta[pos, m]] for m in range(M)]
    Mn = [P[f"metadata.{m}.weight"][meta[neg, m]] for m in range(M)]
    R = 3 + 2 * M
    gr, gl = np.zeros((R, B, D)), np.zeros((R, B))
    gp_, gn_ = gp[:, None], gn[:, None]
    if net == "fm":
        Sp, Sn = U + Ip + sum(Mp), U + In + sum(Mn)
        gr[0] = gp_ * (Sp - U) + gn_ * (Sn - U)
        gr[1], gr[2] = gp_ * (Sp - Ip), gn_ * (Sn - In)
        for m in range(M):
            gr[3 + 2 * m], gr[4 + 2 * m] = gp_ * (Sp - Mp[m]), gn_ * (Sn - Mn[m])
            gl[3 + 2 * m], gl[4 + 2 * m] = gp, gn
    else:
        Sp, Sn = Ip + sum(Mp), In + sum(Mn)
        gr[0] = gp_ * Sp + gn_ * Sn
        gr[1], gr[2] = gp_ * U, gn_ * U
        for m in range(M):
            gr[3 + 2 * m], gr[4 + 2 * m] = gp_ * U, gn_ * U
    gl[1], gl[2] = gp, gn  # gl[0]: the user's 1-wide term enters both z with derivative 1 — exactly 0
    return {"loss": float(row_loss.mean()), "row_loss": row_loss, "trials": J + 1, "neg": neg,
            "neg_meta": None if meta is None else meta[neg], "gr": gr, "gl": gl, "z": z, "h": h, "J": J}


def coalesce(net, params, user, pos, neg, item_meta, gr, gl):
    """Dense gradients {state_dict name: array} of the staged triples (what the row updates add up)."""
    user, pos, neg = (np.asarray(a, dtype=np.int64) for a in (user, pos, neg))
    M = len([k for k in params if k.startswith("metadata.")])
    out = {k: np.zeros(np.asarray(v).shape, dtype=np.float64) for k, v in params.items()}
    lu, li = lin_names(net)
    np.add.at(out["user.weight"], user, gr[0])
    np.add.at(out[lu][:, 0], user, gl[0])
    for f, idx in ((1, pos), (2, neg)):
        np.add.at(out["item.weight"], idx, gr[f])
        np.add.at(out[li][:, 0], idx, gl[f])
        for m in range(M):
            mids = np.asarray(item_meta)[idx, m]
            np.add.at(out[f"metadata.{m}.weight"], mids, gr[2 + 2 * m + f])
            if net == "fm":
                np.add.at(out[f"linear_metadata.{m}.weight"][:, 0], mids, gl[2 + 2 * m + f])
    return out


def touched(net, params, user, pos, neg, item_meta):
    """{state_dict name: sorted distinct rows the step's index lists name}."""
    M = len([k for k in params if k.startswith("metadata.")])
    lu, li = lin_names(net)
    u, i = np.unique(user), np.unique(np.concatenate([pos, neg]))
    rows = {"user.weight": u, "item.weight": i, lu: u, li: i}
    for m in range(M):
        r = np.unique(np.asarray(item_meta)[i, m])
        rows[f"metadata.{m}.weight"] = r
        if net == "fm":
            rows[f"linear_metadata.{m}.weight"] = r
    return rows


def loss_and_grads(net, params, user, items, item_meta, margin, weights):
    """(mean loss, dense gradients by state_dict name, staged dict)."""
    st = staged(net, params, user, items, item_meta, margin, weights)
    items = np.asarray(items)
    return st["loss"], coalesce(net, params, user, items[0], st["neg"], item_meta, st["gr"], st["gl"]), st
