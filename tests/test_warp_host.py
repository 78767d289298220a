# -*- coding: utf-8 -*-
"""WARP loss, host side (no GPU): the numpy restatement tests/warp_ref.py against float64 torch autograd with the choice
held fixed, the rank-weight table against hand values, fit()'s argument errors before anything touches a device, and the
new C entry point's declaration, binding and host-side argument validation."""
import contextlib
import ctypes
import io
import math
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

import warp_ref
from conftest import rel_err
from torchrecsys_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000  # a non-NULL "device pointer": validation never dereferences it
META_SIZES = (13, 7)


def _err():
    return _lib.load().trs_last_error().decode()


# ------------------------------------------------------------------------------------------- 1. restatement vs autograd
def random_params(net, NU, NI, D, M, rs):
    p = {}
    for name in warp_ref.table_names(net, M):
        rows = NU if "user" in name else NI
        if "metadata" in name:
            rows = META_SIZES[int(name.split(".")[1])]
        wide = name in ("user.weight", "item.weight") or name.startswith("metadata.")
        p[name] = rs.normal(0, 0.3 if wide else 0.1, (rows, D if wide else 1))
    item_meta = np.stack([rs.randint(0, META_SIZES[m], NI) for m in range(M)], 1) if M else None
    return p, item_meta


def z_torch(net, W, user, items, item_meta):
    """z (B, 1 + K) as a float64 torch expression of dense tables, written from the formulas of fit()'s docstring."""
    M = len([k for k in W if k.startswith("metadata.")])
    u = torch.from_numpy(np.asarray(user)).long()
    it = torch.from_numpy(np.asarray(items)).long().T
    lu, li = warp_ref.lin_names(net)
    U = W["user.weight"][u][:, None, :]
    I = W["item.weight"][it]
    mids = [torch.from_numpy(np.asarray(item_meta))[it, m].long() for m in range(M)]
    metas = [W[f"metadata.{m}.weight"][mids[m]] for m in range(M)]
    if net == "linear":
        S = I
        for x in metas:
            S = S + x
        return (U * S).sum(-1) + W[lu][u, 0][:, None] + W[li][it, 0]
    fields = [U.expand_as(I), I] + metas
    S = sum(fields)
    z = W[lu][u, 0][:, None] + W[li][it, 0]
    for m in range(M):
        z = z + W[f"linear_metadata.{m}.weight"][mids[m], 0]
    return z + 0.5 * ((S * S) - sum(f * f for f in fields)).sum(-1)


def rows_with_and_without_violators(rs, NU, NI, B, K):
    """user (B,), items (1 + K, B).  Item 0 is the positive of every fourth row and carries a large 1-wide term (set by
    the caller), so those rows have no violator; it is nobody's candidate.  Users and items repeat."""
    user = rs.randint(0, NU, B)
    items = rs.randint(1, NI, (1 + K, B))
    user[1::3] = user[0]
    items[0, ::4] = 0
    clash = items[1:] == items[0][None, :]
    items[1:][clash] = items[0][None, :].repeat(K, 0)[clash] % (NI - 1) + 1
    return user, items


@pytest.mark.parametrize("K", [1, 5, 17])
@pytest.mark.parametrize("M", [0, 2])
@pytest.mark.parametrize("net", ["linear", "fm"])
def test_restatement_matches_float64_autograd_with_the_choice_held_fixed(net, M, K):
    rs = np.random.RandomState(11 + M + K)
    NU, NI, D, B, margin = 30, 40, 9, 41, 0.05
    params, item_meta = random_params(net, NU, NI, D, M, rs)
    params[warp_ref.lin_names(net)[1]][0, 0] = 50.0  # item 0 outranks everything
    user, items = rows_with_and_without_violators(rs, NU, NI, B, K)
    assert (items[1:] != items[0]).all()
    weights = warp_ref.rank_weights(NI, K, "harmonic")
    st = warp_ref.staged(net, params, user, items, item_meta, margin, weights)
    J = st["J"]
    assert (J[::4] == -1).all() and (J >= 0).sum() >= B // 4  # rows without and with a violator
    assert K == 1 or (J > 0).any()  # ... and some whose first violator is not c_0
    assert np.array_equal(st["trials"], J + 1)
    assert np.array_equal(st["neg"], items[1 + np.maximum(J, 0), np.arange(B)])
    # autograd of sum_rows w_J * h_J / B with J held fixed
    W = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in params.items()}
    z = z_torch(net, W, user, items, item_meta)
    assert np.allclose(z.detach().numpy(), st["z"], rtol=1e-12, atol=1e-12)
    found = torch.from_numpy(J >= 0)
    Jc = torch.from_numpy(np.maximum(J, 0)).long()
    hJ = (z[torch.arange(B), 1 + Jc] - z[:, 0]) + margin
    wJ = torch.from_numpy(weights)[Jc]
    val = (torch.where(found, wJ * hJ, torch.zeros_like(hJ))).sum() / B
    val.backward()
    val = float(val.detach())
    assert abs(st["loss"] - val) <= 1e-12 * abs(val) and st["loss"] > 0
    got = warp_ref.coalesce(net, params, user, items[0], st["neg"], item_meta, st["gr"], st["gl"])
    lu = warp_ref.lin_names(net)[0]
    for k, w in W.items():
        want = w.grad.numpy() if w.grad is not None else np.zeros(w.shape)
        if k == lu:  # enters both z of a row with derivative 1: autograd leaves rounding, the restatement an exact 0
            assert np.abs(want).max() < 1e-12 and not got[k].any()
            continue
        assert np.abs(want).max() > 0, k
        assert rel_err(got[k], want) <= 1e-12, k
    # a row without a violator stages zeros in every field
    assert not st["gr"][:, J < 0].any() and not st["gl"][:, J < 0].any() and not st["row_loss"][J < 0].any()
    assert not st["gl"][0].any()
    if net == "linear" and M:
        assert not st["gl"][3:].any()  # Linear has no 1-wide metadata tables


def test_a_nan_does_not_violate_and_the_first_violator_wins():
    z = np.array([[0.0, np.nan, -2.0, 0.5, 3.0], [0.0, -5.0, -5.0, -5.0, -5.0], [0.0, -1.0, -0.5, np.nan, -3.0]])
    h, J = warp_ref.select(z, 1.0)
    assert J.tolist() == [2, -1, 1]  # -2 + 1 <= 0; 0.5 + 1 > 0; h == 0 exactly does not violate, -0.5 + 1 does
    assert warp_ref.near_ties(z, 1.0, 1e-5).tolist() == [False, False, True]  # row 2: h_0 == 0 sits before its J


# ------------------------------------------------------------------------------------------- 2. rank weights
def test_rank_weights_against_hand_values():
    from torchrecsys_amd import ops
    H = lambda r: sum(1.0 / i for i in range(1, r + 1))
    r = [100, 50, 33, 25]  # floor(100 / N), N = 1..4
    for fn in (ops.warp_rank_weight_values, warp_ref.rank_weights):
        assert np.allclose(fn(101, 4, "log"), [math.log(x) for x in r], rtol=1e-15, atol=0)
        assert np.allclose(fn(101, 4, "harmonic"), [H(x) for x in r], rtol=1e-14, atol=0)
        # n_items - 1 < N: the weight is 0 (r = 2, 1, 0, 0)
        assert np.allclose(fn(3, 4, "log"), [math.log(2), 0.0, 0.0, 0.0], rtol=1e-15, atol=0)
        assert np.allclose(fn(3, 4, "harmonic"), [1.5, 1.0, 0.0, 0.0], rtol=1e-15, atol=0)
        assert fn(3, 4, "log")[2:].tolist() == [0.0, 0.0] and fn(3, 4, "harmonic")[2:].tolist() == [0.0, 0.0]
    assert np.allclose(ops.warp_rank_weight_values(1_000_000, 64, "harmonic"),
                       warp_ref.rank_weights(1_000_000, 64, "harmonic"), rtol=1e-12, atol=0)
    with pytest.raises(ValueError, match="rank_weight"):
        ops.warp_rank_weight_values(10, 2, "nope")
    # the table handed to the kernel: float64 rounded to fp32, one object per (n_items, K, kind)
    t = ops.warp_rank_weights(101, 4, "log", "cpu")
    assert t.dtype == torch.float32 and t.shape == (4,)
    assert np.array_equal(t.numpy(), np.array([math.log(x) for x in r]).astype(np.float32))
    assert ops.warp_rank_weights(101, 4, "log", "cpu") is t
    assert ops.warp_rank_weights(101, 4, "harmonic", "cpu") is not t


# ------------------------------------------------------------------------------------------- 3. fit() arguments
def _df(seed=0):
    rs = np.random.RandomState(seed)
    return pd.DataFrame({"user_id": np.concatenate([np.arange(40), rs.randint(0, 40, 360)]),
                         "item_id": np.concatenate([np.arange(30), rs.randint(0, 30, 370)])})


def _model(net_type, rng="device", dynamic=True, neg_sampling=None):
    from torchrecsys_amd.model import TorchRecSys
    with contextlib.redirect_stdout(io.StringIO()):
        return TorchRecSys(_df(), "user_id", "item_id", n_factors=8, net_type=net_type, rng=rng,
                           dynamic_neg_sampling=dynamic, neg_sampling=neg_sampling)


def test_fit_argument_errors_name_the_argument_and_come_first(monkeypatch):
    from torchrecsys_amd import model as model_mod

    def no_device(*a, **kw):
        raise AssertionError("fit() reached the device before validating its arguments")
    monkeypatch.setattr(model_mod.TorchRecSys, "make_runner", no_device)

    def fit(m, **kw):
        m.fit(torch.optim.SGD(m.parameters(), lr=0.1), epochs=1, **kw)

    for kw in (dict(loss="warp"), dict(loss="warp", n_negatives=8, margin=0.5, rank_weight="harmonic")):
        with pytest.raises(ValueError, match="net_type"):
            fit(_model("mlp"), **kw)
        with pytest.raises(ValueError, match="rng"):
            fit(_model("fm", rng="reference"), **kw)
        with pytest.raises(ValueError, match="dynamic_neg_sampling"):
            fit(_model("linear", dynamic=False), **kw)
        with pytest.raises(ValueError, match=r"neg_sampling\['mine'\]"):
            fit(_model("fm", neg_sampling={"mine": "hardest", "candidates": 4}), **kw)
    for bad in (0.0, -1.0, float("inf"), float("-inf"), float("nan"), "x", None):
        with pytest.raises(ValueError, match="margin"):
            fit(_model("fm"), loss="warp", margin=bad)
    for bad in ("nope", "", None, 1):
        with pytest.raises(ValueError, match="rank_weight"):
            fit(_model("fm"), loss="warp", rank_weight=bad)
    for bad in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match="n_negatives"):
            fit(_model("fm"), loss="warp", n_negatives=bad)
    for loss in ("hinge", "bpr", "softmax", "sampled_softmax"):
        with pytest.raises(ValueError, match="margin"):
            fit(_model("linear"), loss=loss, margin=0.5)
        with pytest.raises(ValueError, match="rank_weight"):
            fit(_model("linear"), loss=loss, rank_weight="harmonic")
    with pytest.raises(ValueError, match="temperature"):
        fit(_model("linear"), loss="warp", temperature=0.5)
    with pytest.raises(ValueError, match="logq_correction"):
        fit(_model("linear"), loss="warp", logq_correction=True)
    with pytest.raises(ValueError, match="warp"):
        fit(_model("linear"), loss="nope")
    # valid arguments get past the checks (and, here, to the stub)
    for kw in (dict(loss="warp"), dict(loss="warp", n_negatives=64, margin=0.25, rank_weight="harmonic"),
               dict(loss="warp", n_negatives=1, rank_weight="log")):
        with pytest.raises(AssertionError, match="reached the device"):
            fit(_model("fm", neg_sampling={"k": 2, "popularity": True, "reject_seen": True}), **kw)
    assert "warp" not in _lib.LOSS_ID and _lib.LOSS_WARP not in _lib.LOSS_ID.values()


# ------------------------------------------------------------------------------------------- 4. the C entry point
def test_new_symbol_declared_exported_and_bound_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "trs.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    name = "trs_score_warp_fwd_bwd"
    assert re.search(r"\b%s\s*\(" % name, hdr)
    assert name in _lib.PROTOTYPES and hasattr(raw, name) and hasattr(lib, name)
    assert len(_lib.PROTOTYPES[name][1]) == 20
    assert int(re.search(r"#define TRS_LOSS_WARP (\d+)", hdr).group(1)) == _lib.LOSS_WARP == 3
    assert int(re.search(r"#define TRS_ABI_VERSION (\d+)", hdr).group(1)) == 6 == _lib.ABI_VERSION
    assert lib.trs_abi_version() == 6
    note = text[text.index("6: batched top-k retrieval"):]
    note = note[:note.index("*/")]
    assert name in note and "TRS_LOSS_WARP" in note  # appended to the version comment's parenthesis


def _tables(D=8, M=0):
    T = _lib.TrsTables()
    T.user = T.item = T.user_lin = T.item_lin = P
    T.n_users, T.n_items, T.D, T.M = 50, 40, D, M
    for m in range(M):
        T.meta[m], T.meta_lin[m], T.n_meta[m] = P, P, 5
    return T


def test_score_warp_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()
    FM = _lib.TRS_NET_FM

    def score(T=_tables(), net=FM, user=P, items=P, meta=None, B=10, M=0, K=4, margin=1.0, rw=P, loss_sum=P, neg=P,
              neg_meta=None, gr=P, gl=P):
        return lib.trs_score_warp_fwd_bwd(net, ctypes.byref(T) if T is not None else None, user, items, meta, B, M, K,
                                          margin, rw, 0.1, loss_sum, None, neg, neg_meta, None, gr, gl, None, None)

    # the grounds of trs_score_multi_fwd_bwd
    assert score(T=None) == -1 and "tables is NULL" in _err()
    for bad in (0, -1, 65, 4096):
        assert score(K=bad) == -1 and "K=" in _err(), bad
    assert score(M=1) == -1 and "does not match" in _err()
    assert score(T=_tables(M=2), M=2, neg_meta=P) == -1 and "metadata ids are NULL" in _err()
    for D in (0, -4, 1025, 257):
        assert score(T=_tables(D=D)) == -1 and "n_factors" in _err(), D
    assert score(net=7) == -1 and "net must be" in _err()
    T0 = _tables()
    T0.item_lin = None
    assert score(T=T0) == -1 and "1-wide" in _err()
    assert score(loss_sum=None) == -1 and "loss_sum is NULL" in _err()
    assert score(gr=None) == -1 and "both" in _err()
    assert score(gl=None) == -1 and "both" in _err()
    assert score(user=None) == -1 and "ids are NULL" in _err()
    assert score(B=-1) == -1
    # ... and its own
    for bad in (float("inf"), float("-inf"), float("nan")):
        assert score(margin=bad) == -1 and "margin" in _err(), bad
    assert score(rw=None) == -1 and "rank_weight is NULL" in _err()
    assert score(neg=None) == -1 and "neg_out is NULL" in _err()
    assert score(T=_tables(M=2), M=2, meta=P) == -1 and "neg_meta_out" in _err()
    assert _err().startswith("trs_score_warp_fwd_bwd")
    assert score(B=0) == 0 and score(B=0, gr=None, gl=None) == 0  # nothing to launch
    assert score(B=0, margin=float("nan")) == -1  # ... but bad arguments are still refused
