# -*- coding: utf-8 -*-
"""numpy restatement of fit(l2=...), the per-sample L2 regularisation of the embedding rows a batch references
(trs_stage_add_l2, include/trs.h).  TEST INFRASTRUCTURE, float64.

A batch of B rows stages one gradient row per reference: field 0 the user, field 1 + s the item of slot s, field
1 + S + m * S + s metadata column m of slot s (S = 1 the in-batch softmax, 2 a pair or the WARP triple, 1 + K for K
sampled negatives).  Every reference r gains lambda_group(r) / B times its pre-update row (and the entry of the 1-wide
table with the same id, where that table exists), so per table the penalty's gradient is
    lambda_group / B * count_r * W_r,   count_r = the number of references of row r in the batch.
Composes with multineg_ref / warp_ref / oracle.nets (the data gradients) and oracle.optim (the rules), by state_dict
name.
"""
import numpy as np

import multineg_ref

GROUPS = ("user", "item", "metadata")


def id_blocks(user, items, meta):
    """user (B,), items (S, B), meta (S, B, M) or None as int64 arrays; a 1-D items is one slot."""
    user = np.asarray(user, dtype=np.int64)
    items = np.asarray(items, dtype=np.int64)
    if items.ndim == 1:
        items = items[None, :]
    if meta is not None:
        meta = np.asarray(meta, dtype=np.int64)
        if meta.ndim == 2:
            meta = meta[None, :, :]
    return user, items, meta


def counts(params, user, items, meta):
    """{state_dict name of a D-wide table: (rows,) number of references of each row in the batch}."""
    user, items, meta = id_blocks(user, items, meta)
    M = len([k for k in params if k.startswith("metadata.")])
    out = {"user.weight": np.zeros(np.asarray(params["user.weight"]).shape[0]),
           "item.weight": np.zeros(np.asarray(params["item.weight"]).shape[0])}
    np.add.at(out["user.weight"], user, 1.0)
    np.add.at(out["item.weight"], items.reshape(-1), 1.0)
    for m in range(M):
        c = np.zeros(np.asarray(params[f"metadata.{m}.weight"]).shape[0])
        np.add.at(c, meta[:, :, m].reshape(-1), 1.0)
        out[f"metadata.{m}.weight"] = c
    return out


def grads(net, params, user, items, meta, coefs, inv_B):
    """The penalty's dense gradient per table, {state_dict name: c_group * inv_B * count_r * W_r}, float64.  coefs =
    (lambda_user, lambda_item, lambda_metadata); a 1-wide table takes its group's coefficient and its group's counts."""
    P = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    M = len([k for k in P if k.startswith("metadata.")])
    n = counts(P, user, items, meta)
    lu, li = multineg_ref.lin_names(net)
    cu, ci, cm = (float(c) * float(inv_B) for c in coefs)
    out = {"user.weight": cu * n["user.weight"][:, None] * P["user.weight"],
           "item.weight": ci * n["item.weight"][:, None] * P["item.weight"],
           lu: cu * n["user.weight"][:, None] * P[lu],
           li: ci * n["item.weight"][:, None] * P[li]}
    for m in range(M):
        k = f"metadata.{m}.weight"
        out[k] = cm * n[k][:, None] * P[k]
        if net == "fm":
            out[f"linear_metadata.{m}.weight"] = cm * n[k][:, None] * P[f"linear_metadata.{m}.weight"]
    assert sorted(out) == sorted(P)
    return out


def touched(net, params, user, items, meta):
    """{state_dict name: sorted distinct rows the batch references}."""
    n = counts(params, user, items, meta)
    lu, li = multineg_ref.lin_names(net)
    rows = {k: np.flatnonzero(v) for k, v in n.items()}
    rows[lu], rows[li] = rows["user.weight"], rows["item.weight"]
    if net == "fm":
        for k in list(n):
            if k.startswith("metadata."):
                rows["linear_" + k] = rows[k]
    return rows


def field_refs(net, params, user, items, meta, coefs):
    """The staged references, one entry per field: [(coefficient, D-wide table, 1-wide table or None, ids (B,))] in
    field order; F = 1 + S * (1 + M) entries.  coefs already hold whatever 1 / B the caller wants."""
    user, items, meta = id_blocks(user, items, meta)
    M = len([k for k in params if k.startswith("metadata.")])
    S = items.shape[0]
    lu, li = multineg_ref.lin_names(net)
    cu, ci, cm = coefs
    out = [(cu, params["user.weight"], params[lu], user)]
    out += [(ci, params["item.weight"], params[li], items[s]) for s in range(S)]
    for m in range(M):
        lin = params[f"linear_metadata.{m}.weight"] if net == "fm" else None
        out += [(cm, params[f"metadata.{m}.weight"], lin, meta[s, :, m]) for s in range(S)]
    return out


def staged_add(net, params, user, items, meta, coefs, gr, gl, dtype=np.float64, skip=None):
    """The staging buffers after trs_stage_add_l2, computed in `dtype`: g + c * W[id] per reference (the product, then
    the sum).  np.float32 restates the kernel's arithmetic operation by operation; np.float64 is the exact reference.
    Also returns the magnitudes |g| + |c * w| (float64) an error bound scales with.  skip: (F, B) bool, references that
    stay as they are (an id outside its table); a group whose coefficient is 0 stays as it is too."""
    gr = np.array(gr, dtype=dtype)
    gl = np.array(gl, dtype=dtype)
    mag_r, mag_l = np.abs(gr).astype(np.float64), np.abs(gl).astype(np.float64)
    for f, (c, W, w, ids) in enumerate(field_refs(net, params, user, items, meta, coefs)):
        if not c > 0:
            continue
        keep = np.ones(len(ids), bool) if skip is None else ~skip[f]
        t = np.flatnonzero(keep)
        pr = dtype(c) * np.asarray(W, dtype=dtype)[ids[t]]
        gr[f, t] = gr[f, t] + pr
        mag_r[f, t] += np.abs(pr)
        if w is not None:
            pl = dtype(c) * np.asarray(w, dtype=dtype)[ids[t], 0]
            gl[f, t] = gl[f, t] + pl
            mag_l[f, t] += np.abs(pl)
    return gr, gl, mag_r, mag_l
