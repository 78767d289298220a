# -*- coding: utf-8 -*-
"""numpy restatement of score-aware hard-negative mining (trs_batch_prepare_mined, include/trs.h).
TEST INFRASTRUCTURE, built on oracle.loader's restatements of the device streams; candidate scores in float64.

For epoch position q (user u, positive p), sampler seed s and counter ctr = offset + t:
  candidates  c_j = the sampler's draw under seed s_j = (s + j * KEY_STEP) mod 2^64, j < K (c_0 = the unmined negative);
  scores      z_j = the scorer's value of (u, c_j, metadata of c_j) before the FM sigmoid;
  choice      candidates ordered by (z descending, j ascending, NaN first); rank r = 0 if top == 1 else
              mulhi64(words (y << 32 | x) of Philox(ctr, s_K), top); the mined negative is the candidate of rank r.
"""
import numpy as np

from oracle import loader

KEY_STEP = 0xD1B54A32D192ED03  # between the seeds of consecutive candidates
TRY_STEP = 0x9E3779B97F4A7C15  # between the retry keys inside one draw (trs_sample_neg_opt)
MASK64 = (1 << 64) - 1


def key_offsets(max_j=65, max_t=64):
    """Offsets (mod 2^64) of every Philox key a triple may use: candidate j (0..max_j; j = K is the rank draw), try t."""
    return [(j * KEY_STEP + t * TRY_STEP) & MASK64 for j in range(max_j + 1) for t in range(max_t + 1)]


def _mulhi64(x, n):
    return ((np.asarray(x, dtype=np.uint64).astype(object) * int(n)) >> 64).astype(np.int64)


def _seen_keys(seen, n_items):
    """user * n_items + item of every seen pair, from a dict user -> set or a CSR (offsets, items)."""
    if isinstance(seen, tuple):
        off, items = (np.asarray(a).astype(np.int64) for a in seen)
        users = np.repeat(np.arange(off.size - 1, dtype=np.int64), np.diff(off))
        return users * n_items + items
    return np.array([int(u) * n_items + int(i) for u, its in seen.items() for i in its], dtype=np.int64)


def negatives_opt(users, pos, n_items, seed, offset, popularity=False, seen=None, pop_items=None, max_tries=8):
    """oracle.loader.device_negatives_opt, every row at once per try (test_mining_host.py holds the two equal)."""
    users, pos = np.asarray(users, dtype=np.int64), np.asarray(pos, dtype=np.int64)
    ctr = np.arange(pos.size, dtype=np.uint64) + np.uint64(offset)
    keys = None if seen is None else _seen_keys(seen, n_items)
    c = np.zeros(pos.size, dtype=np.int64)
    active = np.ones(pos.size, dtype=bool)
    for k in range(max_tries):
        x, y, z, w = loader.philox4x32_10(ctr, (int(seed) + k * TRY_STEP) & MASK64)
        v = _mulhi64((y.astype(np.uint64) << np.uint64(32)) | x.astype(np.uint64), n_items - 1)
        cand = v + (v >= pos)
        skip = np.zeros(pos.size, dtype=bool)
        if popularity:
            cp = np.asarray(pop_items, dtype=np.int64)[
                _mulhi64((w.astype(np.uint64) << np.uint64(32)) | z.astype(np.uint64), len(pop_items))]
            skip = cp == pos  # the row's own positive: next try, the uniform draw stays as the fallback
            cand = np.where(skip, cand, cp)
        c = np.where(active, cand, c)
        ok = ~skip
        if keys is not None:
            ok &= ~np.isin(users * n_items + cand, keys)
        active &= ~ok
    return c


def candidates(users, pos, n_items, seed, offset, K, sampler=None, pop_items=None):
    """(B, K) int64: the K candidate negatives of every triple."""
    sampler = sampler or {}
    opt = bool(sampler.get("popularity")) or sampler.get("seen") is not None
    cols = []
    for j in range(K):
        sj = (int(seed) + j * KEY_STEP) & MASK64
        if opt:
            cols.append(negatives_opt(users, pos, n_items, sj, offset, popularity=sampler.get("popularity", False),
                                      seen=sampler.get("seen"), pop_items=pop_items,
                                      max_tries=sampler.get("max_tries", 8)))
        else:  # try 0 with every option off is the plain sampler's draw
            cols.append(loader.device_negatives(pos, n_items, sj, offset))
    return np.stack(cols, axis=1).astype(np.int64)


def scores64(net, params, users, items, item_meta=None):
    """float64 value the candidates are ranked by: Linear the score, FM the argument of the sigmoid.  users (B,),
    items (B,) or (B, K); returns the shape of items."""
    items = np.asarray(items, dtype=np.int64)
    u = np.asarray(users, dtype=np.int64).reshape((-1,) + (1,) * (items.ndim - 1))
    u = np.broadcast_to(u, items.shape)
    P = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    M = len([k for k in P if k.startswith("metadata.")])
    U, I = P["user.weight"][u], P["item.weight"][items]
    metas = [P[f"metadata.{m}.weight"][np.asarray(item_meta)[items, m]] for m in range(M)]
    if net == "linear":
        S = I + sum(metas) if metas else I
        return (U * S).sum(-1) + P["user_bias.weight"][u, 0] + P["item_bias.weight"][items, 0]
    fields = [U, I] + metas
    S = sum(fields)
    lin = P["linear_user.weight"][u, 0] + P["linear_item.weight"][items, 0]
    for m in range(M):
        lin = lin + P[f"linear_metadata.{m}.weight"][np.asarray(item_meta)[items, m], 0]
    return lin + 0.5 * (S * S - sum(f * f for f in fields)).sum(-1)


def order_desc(z):
    """(B, K) candidate indices by (score descending, index ascending), NaN first; -0.0 ties with +0.0."""
    z = np.asarray(z, dtype=np.float64)
    nan = np.isnan(z)
    o = np.argsort(-np.where(nan, np.inf, z), axis=1, kind="stable")
    o2 = np.argsort(~np.take_along_axis(nan, o, axis=1), axis=1, kind="stable")
    return np.take_along_axis(o, o2, axis=1)


def ranks(B, K, top, seed, offset):
    """(B,) rank of the candidate every triple trains on."""
    if top == 1:
        return np.zeros(B, dtype=np.int64)
    ctr = np.arange(B, dtype=np.uint64) + np.uint64(offset)
    x, y, _, _ = loader.philox4x32_10(ctr, (int(seed) + K * KEY_STEP) & MASK64)
    return _mulhi64((y.astype(np.uint64) << np.uint64(32)) | x.astype(np.uint64), top)


def mined_batch(stream_user, stream_item, shuffle_key, t0, B, n_items, seed, offset, net, params, K, top=1,
                sampler=None, item_meta=None, cand=None):
    """trs_batch_prepare_mined restated.  Returns user / pos / neg / chosen (+ pos_meta / neg_meta) and, for the
    tolerance rules of the float tests, cand (B, K) and z (B, K) float64.  cand: the candidates of an earlier call with
    the same arguments but `top` (they do not depend on it)."""
    N = len(stream_user)
    k = (sampler or {}).get("k", 1)
    rows = np.array([loader.feistel_perm(t0 + t, N * k, shuffle_key) % N for t in range(B)], dtype=np.int64)
    u = np.asarray(stream_user)[rows].astype(np.int64)
    p = np.asarray(stream_item)[rows].astype(np.int64)
    if cand is None:
        cand = candidates(u, p, n_items, seed, offset, K, sampler, pop_items=np.asarray(stream_item))
    z = scores64(net, params, u, cand, item_meta)
    chosen = np.take_along_axis(order_desc(z), ranks(B, K, top, seed, offset)[:, None], axis=1)[:, 0]
    neg = np.take_along_axis(cand, chosen[:, None], axis=1)[:, 0]
    out = {"user": u, "pos": p, "neg": neg, "chosen": chosen, "cand": cand, "z": z}
    if item_meta is not None:
        out["pos_meta"] = np.asarray(item_meta)[p]
        out["neg_meta"] = np.asarray(item_meta)[neg]
    return out
