# -*- coding: utf-8 -*-
"""Training on K sampled negatives per positive, host side (no GPU): the numpy restatement tests/multineg_ref.py against
float64 torch autograd on dense tables, fit()'s argument errors before anything touches a device, and the two new C
entry points' host-side argument validation."""
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

import multineg_ref
from conftest import rel_err
from torchrecsys_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["trs_batch_prepare_multi", "trs_score_multi_fwd_bwd"]
P = 0x1000  # a non-NULL "device pointer": validation never dereferences it
META_SIZES = (13, 7)


def _err():
    return _lib.load().trs_last_error().decode()


# ------------------------------------------------------------------------------------------- 1. restatement vs autograd
def random_params(net, NU, NI, D, M, rs):
    p = {}
    for name in multineg_ref.table_names(net, M):
        rows = NU if "user" in name else NI
        if "metadata" in name:
            rows = META_SIZES[int(name.split(".")[1])]
        wide = name in ("user.weight", "item.weight") or name.startswith("metadata.")
        p[name] = rs.normal(0, 0.3 if wide else 0.1, (rows, D if wide else 1))
    item_meta = np.stack([rs.randint(0, META_SIZES[m], NI) for m in range(M)], 1) if M else None
    return p, item_meta


def autograd(net, params, user, items, item_meta, loss, tau):
    """float64 autograd of the batch-mean loss on dense tables, written from the formulas of fit()'s docstring."""
    W = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in params.items()}
    M = len([k for k in W if k.startswith("metadata.")])
    u = torch.from_numpy(np.asarray(user)).long()
    it = torch.from_numpy(np.asarray(items)).long().T  # (B, 1 + K)
    lu, li = multineg_ref.lin_names(net)
    U = W["user.weight"][u][:, None, :]
    I = W["item.weight"][it]
    mids = [torch.from_numpy(np.asarray(item_meta))[it, m].long() for m in range(M)]
    metas = [W[f"metadata.{m}.weight"][mids[m]] for m in range(M)]
    if net == "linear":
        S = I
        for x in metas:
            S = S + x
        z = (U * S).sum(-1) + W[lu][u, 0][:, None] + W[li][it, 0]
    else:
        fields = [U.expand_as(I), I] + metas
        S = sum(fields)
        z = W[lu][u, 0][:, None] + W[li][it, 0]
        for m in range(M):
            z = z + W[f"linear_metadata.{m}.weight"][mids[m], 0]
        z = z + 0.5 * ((S * S) - sum(f * f for f in fields)).sum(-1)
    if loss == "sampled_softmax":
        zh = z / tau
        val = (torch.logsumexp(zh, 1) - zh[:, 0]).mean()
    else:
        s = z if net == "linear" else torch.sigmoid(z)
        sp, sn = s[:, :1], s[:, 1:]
        pair = torch.clamp(sn - sp + 1, min=0) if loss == "hinge" else torch.nn.functional.softplus(sn - sp)
        val = pair.mean(1).mean()
    val.backward()
    return float(val.detach()), {k: (w.grad.numpy() if w.grad is not None else np.zeros(w.shape)) for k, w in W.items()}


def forced_rows(rs, NU, NI, B, K):
    """user (B,), items (1 + K, B): a repeated candidate inside a row, one item as a candidate of many rows and the
    positive of another, repeated users; no candidate equals its row's positive."""
    user = rs.randint(0, NU, B)
    items = rs.randint(0, NI, (1 + K, B))
    if B >= 3:
        user[1::3] = user[0]
        items[1:, ::2] = 5  # item 5: a candidate of every second row ...
        items[0, 1] = 5     # ... and the positive of row 1
    if K >= 2:
        items[2] = items[1]  # the same candidate twice in every row
    clash = items[1:] == items[0][None, :]
    items[1:][clash] = (items[0][None, :].repeat(K, 0)[clash] + 1) % NI
    return user, items


@pytest.mark.parametrize("loss", ["sampled_softmax", "hinge", "bpr"])
@pytest.mark.parametrize("M", [0, 2])
@pytest.mark.parametrize("net", ["linear", "fm"])
def test_restatement_matches_float64_autograd(net, M, loss):
    rs = np.random.RandomState(7 + M)
    NU, NI, D, B, K, tau = 30, 40, 9, 23, 5, 0.2
    params, item_meta = random_params(net, NU, NI, D, M, rs)
    user, items = forced_rows(rs, NU, NI, B, K)
    assert (items[1:] != items[0]).all() and (items[1] == items[2]).all()
    want_loss, want = autograd(net, params, user, items, item_meta, loss, tau)
    got_loss, got = multineg_ref.loss_and_grads(net, params, user, items, item_meta, loss, tau)
    assert abs(got_loss - want_loss) <= 1e-12 * abs(want_loss)
    assert sorted(got) == sorted(want)
    lu = multineg_ref.lin_names(net)[0]
    for k in want:
        if k == lu and (loss == "sampled_softmax" or net == "linear"):
            # the user's 1-wide term enters every score of a row with derivative 1: it cancels in the row softmax and in
            # a Linear pair difference (autograd leaves float64 rounding); the softmax restatement writes an exact 0
            assert np.abs(want[k]).max() < 1e-12 and np.abs(got[k]).max() < 1e-12
            assert loss != "sampled_softmax" or not got[k].any()
            continue
        assert np.abs(want[k]).max() > 0, k
        assert rel_err(got[k], want[k]) <= 1e-12, k
    rows = multineg_ref.touched(net, params, user, items, item_meta)
    for k, g in got.items():
        keep = np.ones(g.shape[0], bool)
        keep[rows[k]] = False
        assert not g[keep].any(), k


def test_one_negative_pair_loss_is_the_oracles_step():
    """K = 1 with hinge / BPR is the existing step: the restatement against oracle.nets on the same triples."""
    from oracle import nets as onets
    rs = np.random.RandomState(3)
    for net in ("linear", "fm"):
        params, item_meta = random_params(net, 30, 40, 8, 2, rs)
        params = {k: v.astype(np.float32) for k, v in params.items()}
        user, items = forced_rows(rs, 30, 40, 19, 1)
        batch = {"user_id": user, "pos_item_id": items[0], "neg_item_id": items[1],
                 "pos_metadata_id": item_meta[items[0]], "neg_metadata_id": item_meta[items[1]]}
        for loss in ("hinge", "bpr"):
            _, _, oloss, ograds = onets.train_forward_backward(net, params, batch, loss=loss)
            val, grads = multineg_ref.loss_and_grads(net, params, user, items, item_meta, loss)
            assert abs(val - float(oloss)) <= 1e-5 * abs(val)
            for k in grads:
                assert rel_err(ograds[k], grads[k]) <= 1e-5, (net, loss, k)


def test_prepare_restatement_follows_the_candidate_schedule():
    """Slot 1 + j of multineg_ref.prepare is the plain loader's negative under seed + j * KEY_STEP."""
    import mining_ref
    from oracle import loader
    rs = np.random.RandomState(1)
    su, si = rs.randint(0, 50, 300), rs.randint(0, 70, 300)
    out = multineg_ref.prepare(su, si, 0xABCD, 40, 33, 70, 9, 40, 4)
    rows = np.array([loader.feistel_perm(40 + t, 300, 0xABCD) % 300 for t in range(33)])
    assert np.array_equal(out["user"], su[rows]) and np.array_equal(out["items"][0], si[rows])
    for j in range(4):
        want = loader.device_negatives(si[rows], 70, (9 + j * mining_ref.KEY_STEP) & mining_ref.MASK64, 40)
        assert np.array_equal(out["items"][1 + j], want)
    assert (out["items"][1:] != out["items"][0]).all()


# ------------------------------------------------------------------------------------------- 2. fit() arguments
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

    for bad in (0, 65, -1, 2.0, True, "4", None):
        with pytest.raises(ValueError, match="n_negatives"):
            fit(_model("fm"), n_negatives=bad)
    for kw in (dict(loss="sampled_softmax"), dict(loss="hinge", n_negatives=4), dict(loss="bpr", n_negatives=2)):
        with pytest.raises(ValueError, match="net_type"):
            fit(_model("mlp"), **kw)
        with pytest.raises(ValueError, match="rng"):
            fit(_model("fm", rng="reference"), **kw)
        with pytest.raises(ValueError, match="dynamic_neg_sampling"):
            fit(_model("linear", dynamic=False), **kw)
        with pytest.raises(ValueError, match=r"neg_sampling\['mine'\]"):
            fit(_model("fm", neg_sampling={"mine": "hardest", "candidates": 4}), **kw)
    with pytest.raises(ValueError, match="n_negatives"):
        fit(_model("fm"), loss="softmax", n_negatives=2)
    with pytest.raises(ValueError, match="logq_correction"):
        fit(_model("fm"), loss="sampled_softmax", logq_correction=True)
    for tau in (0.0, -1.0, float("inf"), float("nan"), "x"):
        with pytest.raises(ValueError, match="temperature"):
            fit(_model("linear"), loss="sampled_softmax", temperature=tau)
    with pytest.raises(ValueError, match="temperature"):
        fit(_model("linear"), loss="hinge", n_negatives=4, temperature=0.5)
    with pytest.raises(ValueError, match="sampled_softmax"):
        fit(_model("linear"), loss="nope")
    # valid arguments get past the checks (and, here, to the stub)
    for kw in (dict(loss="sampled_softmax", temperature=0.5, n_negatives=8), dict(loss="sampled_softmax"),
               dict(loss="bpr", n_negatives=64), dict(loss="hinge", n_negatives=1),
               dict(loss="sampled_softmax", n_negatives=1)):
        with pytest.raises(AssertionError, match="reached the device"):
            fit(_model("fm", neg_sampling={"k": 2, "popularity": True}), **kw)
    assert "sampled_softmax" not in _lib.LOSS_ID and _lib.LOSS_SAMPLED_SOFTMAX not in _lib.LOSS_ID.values()


# ------------------------------------------------------------------------------------------- 3. the C entry points
def test_new_symbols_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trs.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(raw, name), name
    assert lib.trs_abi_version() == _lib.ABI_VERSION
    assert int(re.search(r"#define TRS_LOSS_SAMPLED_SOFTMAX (\d+)", hdr).group(1)) == _lib.LOSS_SAMPLED_SOFTMAX


def _tables(D=8, M=0):
    T = _lib.TrsTables()
    T.user = T.item = T.user_lin = T.item_lin = P
    T.n_users, T.n_items, T.D, T.M = 50, 40, D, M
    for m in range(M):
        T.meta[m], T.meta_lin[m], T.n_meta[m] = P, P, 5
    return T


def test_prepare_multi_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()

    def prep(n_neg=4, neg_static=None, M=0, item_meta=None, meta_out=None, N=100, t0=0, B=10, n_items=40, su=P,
             items_out=P):
        return lib.trs_batch_prepare_multi(su, P, neg_static, N, 1, t0, B, n_items, 2, 0, item_meta, M, P, items_out,
                                           meta_out, None, n_neg, None)

    for bad in (0, -3, 65, 1000):
        assert prep(n_neg=bad) == -1 and "n_neg" in _err(), bad
    assert prep(neg_static=P) == -1 and "static" in _err()
    assert prep(M=9) == -1 and "M=9" in _err()
    assert prep(M=-1) == -1
    assert prep(M=2) == -1 and "item_meta" in _err()
    assert prep(M=2, item_meta=P) == -1 and "item_meta" in _err()
    assert prep(t0=95) == -1 and "slice" in _err()
    assert prep(N=0) == -1
    assert prep(n_items=1) == -1 and "n_items" in _err()
    assert prep(su=None) == -1 and "stream is NULL" in _err()
    assert prep(items_out=None) == -1 and "outputs are NULL" in _err()
    assert prep(B=0) == 0  # an empty slice launches nothing


def test_score_multi_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()
    FM = _lib.TRS_NET_FM

    def score(T=_tables(), net=FM, user=P, items=P, meta=None, B=10, M=0, K=4, loss=_lib.LOSS_SAMPLED_SOFTMAX, tau=1.0,
              loss_sum=P, gr=P, gl=P):
        return lib.trs_score_multi_fwd_bwd(net, ctypes.byref(T) if T is not None else None, user, items, meta, B, M, K,
                                           loss, tau, 0.1, loss_sum, None, gr, gl, None, None)

    assert score(T=None) == -1 and "tables is NULL" in _err()
    for bad in (0, -1, 65, 4096):
        assert score(K=bad) == -1 and "K=" in _err(), bad
    for bad in (3, -1, 99):
        assert score(loss=bad) == -1 and "unknown loss id" in _err(), bad
    assert score(M=1) == -1 and "does not match" in _err()
    assert score(T=_tables(M=2), M=0) == -1 and "does not match" in _err()
    assert score(T=_tables(M=2), M=2) == -1 and "metadata ids are NULL" in _err()
    for D in (0, -4, 1025, 2048, 257, 999):  # odd widths are instantiated up to 256 only
        assert score(T=_tables(D=D)) == -1 and "n_factors" in _err(), D
    assert score(net=7) == -1 and "net must be" in _err()
    T0 = _tables()
    T0.item_lin = None
    assert score(T=T0) == -1 and "1-wide" in _err()
    for tau in (0.0, -1.0, float("inf"), float("nan")):
        assert score(tau=tau) == -1 and "temperature" in _err(), tau
    assert score(loss_sum=None) == -1 and "loss_sum is NULL" in _err()
    assert score(gr=None) == -1 and "both" in _err()
    assert score(gl=None) == -1 and "both" in _err()
    assert score(user=None) == -1 and "ids are NULL" in _err()
    assert score(B=-1) == -1
    assert score(B=0) == 0 and score(B=0, gr=None, gl=None, loss=_lib.LOSS_ID["hinge"]) == 0  # nothing to launch
