# -*- coding: utf-8 -*-
"""numpy restatement of training on K sampled negatives per positive (trs_batch_prepare_multi /
trs_score_multi_fwd_bwd, include/trs.h).  TEST INFRASTRUCTURE, float64, built on tests/mining_ref.py's
`candidates` (the candidate schedule) and `scores64` (the value z the candidates are scored by).

Row i has user u, positive p and candidates c_0 .. c_{K-1}; slot 0 is the positive, slot 1 + j candidate j.
  sampled softmax   zh_s = z_s / tau; loss_i = logsumexp_s zh_s - zh_0; d loss / d zh_s = (softmax_s - [s == 0]) / B
  hinge / bpr       loss_i = (1 / K) sum_j pair(score_p, score_cj); Linear scores are z, FM scores sigmoid(z)
Gradients come out in the kernel's staged form: per (field, row), uncoalesced, field 0 the user, field 1 + s the item of
slot s, field 1 + (1 + K) + m * (1 + K) + s metadata column m of slot s.
"""
import numpy as np

import mining_ref
from oracle import loader

SAMPLED_SOFTMAX = "sampled_softmax"


def lin_names(net):
    return ("user_bias.weight", "item_bias.weight") if net == "linear" else ("linear_user.weight", "linear_item.weight")


def table_names(net, M):
    """state_dict names in table_params() order: user, item, their 1-wide tables, metadata, (FM) 1-wide metadata."""
    names = ["user.weight", "item.weight", *lin_names(net)] + [f"metadata.{m}.weight" for m in range(M)]
    if net == "fm":
        names += [f"linear_metadata.{m}.weight" for m in range(M)]
    return names


def n_fields(K, M):
    return 1 + (1 + K) * (1 + M)


def prepare(stream_user, stream_item, shuffle_key, t0, B, n_items, seed, offset, K, sampler=None, item_meta=None):
    """trs_batch_prepare_multi restated: user (B,), items (1 + K, B) slot-major, meta (1 + K, B, M) or None."""
    N = len(stream_user)
    k = (sampler or {}).get("k", 1)
    rows = np.array([loader.feistel_perm(t0 + t, N * k, shuffle_key) % N for t in range(B)], dtype=np.int64)
    u = np.asarray(stream_user)[rows].astype(np.int64)
    p = np.asarray(stream_item)[rows].astype(np.int64)
    cand = mining_ref.candidates(u, p, n_items, seed, offset, K, sampler, pop_items=np.asarray(stream_item))
    items = np.concatenate([p[None, :], cand.T], axis=0)
    meta = None if item_meta is None else np.asarray(item_meta)[items]
    return {"user": u, "items": items, "meta": meta}


def slot_weights(net, z, loss, tau):
    """(row losses (B,), d(mean loss) / d z (B, 1 + K)) from the float64 values z (B, 1 + K), slot 0 the positive."""
    z = np.asarray(z, dtype=np.float64)
    B, S1 = z.shape
    K = S1 - 1
    if loss == SAMPLED_SOFTMAX:
        zh = z / tau
        mx = zh.max(axis=1, keepdims=True)
        e = np.exp(zh - mx)
        tot = e.sum(axis=1, keepdims=True)
        row = (mx[:, 0] - zh[:, 0]) + np.log(tot[:, 0])
        P = e / tot
        P[:, 0] -= 1.0
        return row, P / B / tau
    s = z if net == "linear" else 1.0 / (1.0 + np.exp(-z))
    sp, sn = s[:, :1], s[:, 1:]
    if loss == "hinge":
        h = sn - sp + 1.0
        val, dneg = np.maximum(h, 0.0), (h >= 0).astype(np.float64)
    elif loss == "bpr":
        x = sn - sp
        val = np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))
        dneg = 1.0 / (1.0 + np.exp(-x))
    else:
        raise ValueError(loss)
    ds = np.concatenate([-dneg.sum(axis=1, keepdims=True), dneg], axis=1) / (B * K)
    if net == "fm":
        ds = ds * s * (1.0 - s)
    return val.mean(axis=1), ds


def staged(net, params, user, items, item_meta, loss, tau=1.0):
    """(mean loss, grad_rows (F, B, D), grad_lin (F, B), z (B, 1 + K)), all float64.  items: (1 + K, B)."""
    P = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    user, items = np.asarray(user, dtype=np.int64), np.asarray(items, dtype=np.int64)
    S1, B = items.shape
    K = S1 - 1
    M = len([k for k in P if k.startswith("metadata.")])
    D = P["user.weight"].shape[1]
    it = items.T  # (B, 1 + K)
    z = mining_ref.scores64(net, P, user, it, item_meta)
    row, dz = slot_weights(net, z, loss, tau)
    U = P["user.weight"][user]                                             # (B, D)
    I = P["item.weight"][it]                                               # (B, S1, D)
    metas = [P[f"metadata.{m}.weight"][np.asarray(item_meta)[it, m]] for m in range(M)]
    gr = np.zeros((n_fields(K, M), B, D))
    gl = np.zeros((n_fields(K, M), B))
    g = dz[:, :, None]
    if net == "fm":
        S = U[:, None, :] + I + (sum(metas) if metas else 0.0)
        gr[0] = (g * (S - U[:, None, :])).sum(axis=1)
        gr[1:1 + S1] = np.transpose(g * (S - I), (1, 0, 2))
        for m in range(M):
            gr[1 + S1 + m * S1:1 + S1 + (m + 1) * S1] = np.transpose(g * (S - metas[m]), (1, 0, 2))
            gl[1 + S1 + m * S1:1 + S1 + (m + 1) * S1] = dz.T
    else:
        S = I + (sum(metas) if metas else 0.0)
        gr[0] = (g * S).sum(axis=1)
        gU = np.transpose(g * U[:, None, :], (1, 0, 2))
        gr[1:1 + S1] = gU
        for m in range(M):
            gr[1 + S1 + m * S1:1 + S1 + (m + 1) * S1] = gU
    gl[1:1 + S1] = dz.T
    # the user's 1-wide term enters every z of a row with derivative 1: under the softmax the weights sum to exactly 0
    gl[0] = 0.0 if loss == SAMPLED_SOFTMAX else dz.sum(axis=1)
    return float(row.mean()), gr, gl, z


def coalesce(net, params, user, items, item_meta, gr, gl):
    """Dense gradients {state_dict name: array} of the staged blocks (what the row updates add up)."""
    user, items = np.asarray(user, dtype=np.int64), np.asarray(items, dtype=np.int64)
    S1, B = items.shape
    M = len([k for k in params if k.startswith("metadata.")])
    out = {k: np.zeros(np.asarray(v).shape, dtype=np.float64) for k, v in params.items()}
    lu, li = lin_names(net)
    flat = items.reshape(-1)
    np.add.at(out["user.weight"], user, gr[0])
    np.add.at(out["item.weight"], flat, gr[1:1 + S1].reshape(S1 * B, -1))
    np.add.at(out[lu][:, 0], user, gl[0])
    np.add.at(out[li][:, 0], flat, gl[1:1 + S1].reshape(-1))
    for m in range(M):
        mids = np.asarray(item_meta)[items, m].reshape(-1)
        sl = slice(1 + S1 + m * S1, 1 + S1 + (m + 1) * S1)
        np.add.at(out[f"metadata.{m}.weight"], mids, gr[sl].reshape(S1 * B, -1))
        if net == "fm":
            np.add.at(out[f"linear_metadata.{m}.weight"][:, 0], mids, gl[sl].reshape(-1))
    return out


def touched(net, params, user, items, item_meta):
    """{state_dict name: sorted distinct rows a batch touches}."""
    M = len([k for k in params if k.startswith("metadata.")])
    lu, li = lin_names(net)
    u, i = np.unique(user), np.unique(items)
    rows = {"user.weight": u, "item.weight": i, lu: u, li: i}
    for m in range(M):
        r = np.unique(np.asarray(item_meta)[np.asarray(items), m])
        rows[f"metadata.{m}.weight"] = r
        if net == "fm":
            rows[f"linear_metadata.{m}.weight"] = r
    return rows


def loss_and_grads(net, params, user, items, item_meta, loss, tau=1.0):
    """(mean loss, dense gradients by state_dict name)."""
    val, gr, gl, _ = staged(net, params, user, items, item_meta, loss, tau)
    return val, coalesce(net, params, user, items, item_meta, gr, gl)
