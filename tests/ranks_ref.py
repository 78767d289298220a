# -*- coding: utf-8 -*-
"""Reference helpers of the rank_items() / evaluate_ranks() tests: a small model builder, the float64 restatement of the
ranking values (as tests/test_ranking.py states them), the reference rank

    rank(u, t) = position of t in np.lexsort((ids, -vals)) over C_u + {t}

and the per-user metrics written as plain loops over a materialised ranked list."""
import contextlib
import io
import math

import numpy as np
import torch


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def build_model(net_type, n_users, n_items, D, M=0, n=None, seed=0, int_range=None, **kw):
    """Every user and every item occurs; int_range: small integer weights, so every fp32 value is exact in any
    summation order and true ties abound."""
    from torchrecsys_amd.model import TorchRecSys
    rs = np.random.RandomState(seed)
    n = n or 20 * n_users
    u = np.concatenate([np.arange(n_users), rs.randint(0, n_users, n - n_users)])
    i = np.concatenate([np.arange(n_items) % n_items, rs.randint(0, n_items, max(n - n_items, 0))])[:n]
    u = u[:len(i)]
    meta = torch.from_numpy(rs.randint(0, 5, (n_items, M))) if M else None
    with quiet():
        torch.manual_seed(seed)
        np.random.seed(seed)
        m = TorchRecSys.from_tensors(torch.from_numpy(u), torch.from_numpy(i), n_users=n_users, n_items=n_items,
                                     item_metadata=meta, metadata_names=[f"m{j}" for j in range(M)] if M else None,
                                     n_factors=D, net_type=net_type, **kw)
    if int_range is not None:
        g = torch.Generator().manual_seed(seed + 1)
        for p in m.net.parameters():
            p.data.copy_(torch.randint(int_range[0], int_range[1], p.shape, generator=g).float())
    return m


def tables(m):
    """(S, U, user constants, item constants) in float64: value(u, i) = <U_u, S_i> + ucon_u + c_i."""
    net = m.net
    f = lambda t: t.detach().cpu().double().numpy()
    M = net.n_meta_tables()
    meta_ids = m.data_processor.item_meta_table
    metas = [f(l.weight) for l in net.metadata] if M else []
    S = f(net.item.weight).copy()
    for j in range(M):
        S += metas[j][meta_ids[:, j]]
    if m.net_type == "linear":
        return S, f(net.user.weight), f(net.user_bias.weight)[:, 0], f(net.item_bias.weight)[:, 0]
    I = f(net.item.weight)
    c = f(net.linear_item.weight)[:, 0] + 0.5 * ((S * S).sum(1) - (I * I).sum(1))
    for j in range(M):
        c += f(net.linear_metadata[j].weight)[meta_ids[:, j], 0] - 0.5 * (metas[j][meta_ids[:, j]] ** 2).sum(1)
    return S, f(net.user.weight), f(net.linear_user.weight)[:, 0], c


def values(m, users):
    """(n, n_items) float64 ranking values: Linear scores / FM logits z."""
    S, U, ucon, c = tables(m)
    users = np.asarray(users)
    return U[users] @ S.T + ucon[users][:, None] + c[None, :]


def seen_sets(m):
    """(offsets, items) of the train split's distinct (user, item) pairs."""
    return tuple(t.cpu().numpy() for t in m._seen_csr())


def ranks_of(vals, targets, seen=None):
    """Reference ranks of `targets` for one user: vals (n_items,) float64, seen: the user's excluded items or None.
    A candidate target's rank is its position in the ordering of C_u; a seen target's its position among C_u + {t}."""
    n_items = vals.shape[0]
    ok = np.ones(n_items, bool)
    if seen is not None:
        ok[seen] = False
    cand = np.nonzero(ok)[0]
    order = cand[np.lexsort((cand, -vals[cand]))]
    pos = np.full(n_items, -1, np.int64)
    pos[order] = np.arange(order.size)
    out = np.empty(len(targets), np.int64)
    down = -vals[order]  # ascending
    for j, t in enumerate(targets):
        if ok[t]:
            out[j] = pos[t]
        else:  # where t goes into the ordered list: behind the larger values and the equal ones with a smaller id
            lo, hi = np.searchsorted(down, -vals[t], "left"), np.searchsorted(down, -vals[t], "right")
            out[j] = lo + np.searchsorted(order[lo:hi], t)
    return out


def ranks_of_by_sorting(vals, targets, seen=None):
    """ranks_of() by its definition, one ordering of C_u + {t} per target (small cases)."""
    ok = np.ones(vals.shape[0], bool)
    if seen is not None:
        ok[seen] = False
    out = np.empty(len(targets), np.int64)
    for j, t in enumerate(targets):
        c = ok.copy()
        c[t] = True
        ids = np.nonzero(c)[0]
        out[j] = int(np.nonzero(ids[np.lexsort((ids, -vals[ids]))] == t)[0][0])
    return out


def user_metrics(ranks, n_c, ks, n_items, brute_force_auc=False):
    """Metrics of one user from the ranks of its m relevant items among n_c candidates, over the ranked list
    `listed[p] = the item at position p is relevant`."""
    rel = set(int(r) for r in ranks)
    m = len(rel)
    assert m == len(ranks) and 0 < m < n_c and all(0 <= r < n_c for r in rel)
    listed = [p in rel for p in range(n_c)]
    if brute_force_auc:
        good = sum(1 for a in range(n_c) for b in range(n_c) if listed[a] and not listed[b] and a < b)
    else:
        flags = np.array(listed)
        good = sum(int(np.sum(~flags[a + 1:])) for a in range(n_c) if listed[a])
    out = {"auc": good / (m * (n_c - m)), "mrr": 1.0 / (min(rel) + 1), "mean_rank": sum(rel) / m}
    for k in ks:
        kk = min(k, n_items)
        top = listed[:kk]
        hits = sum(top)
        out[f"hit_rate@{k}"] = float(hits >= 1)
        out[f"precision@{k}"] = hits / kk
        out[f"recall@{k}"] = hits / m
        dcg = sum(1.0 / math.log2(p + 2) for p, hit in enumerate(top) if hit)
        out[f"ndcg@{k}"] = dcg / sum(1.0 / math.log2(p + 2) for p in range(min(kk, m)))
        found, ap = 0, 0.0
        for p, hit in enumerate(top):
            if hit:
                found += 1
                ap += found / (p + 1)  # the precision at each hit
        out[f"map@{k}"] = ap / min(kk, m)
    return out


def mean_metrics(per_user):
    """Average of a list of user_metrics() dicts, summed in list order."""
    keys = per_user[0].keys()
    return {k: sum(d[k] for d in per_user) / len(per_user) for k in keys}


def relevant_items(m, exclude_seen):
    """{user: sorted relevant items} of the test split (without the train items when exclude_seen), users ascending."""
    td = m.data_processor.test_data
    tu, ti = td["user_id"].cpu().numpy(), td["pos_item_id"].cpu().numpy()
    off, items = seen_sets(m)
    out = {}
    for u in np.unique(tu):
        T = set(ti[tu == u].tolist())
        if exclude_seen:
            T -= set(items[off[u]:off[u + 1]].tolist())
        if T:
            out[int(u)] = sorted(T)
    return out
