# -*- coding: utf-8 -*-
"""fit(l2=...), host side (no GPU): the numpy restatement tests/l2_ref.py against float64 torch autograd of the penalty
as fit()'s docstring states it, fit()'s argument errors before anything touches a device, and the host-side argument
validation of trs_stage_add_l2."""
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

import l2_ref
import multineg_ref
from conftest import rel_err
from torchrecsys_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "trs_stage_add_l2"
P = 0x1000  # a non-NULL "device pointer": validation never dereferences it
META_SIZES = (13, 7)


def _err():
    return _lib.load().trs_last_error().decode()


# ------------------------------------------------------------------------------------------- 1. restatement vs autograd
@pytest.mark.parametrize("S", [1, 2, 6])
@pytest.mark.parametrize("M", [0, 2])
@pytest.mark.parametrize("net", ["linear", "fm"])
def test_restatement_matches_float64_autograd(net, M, S):
    """(1/B) sum_b 1/2 sum_{references r of row b} lambda_group (|W_r|^2 + w_r^2), differentiated by autograd on dense
    tables, against l2_ref.grads; the staged form summed per table gives the same."""
    rs = np.random.RandomState(S + M)
    NU, NI, D, B = 30, 40, 9, 23
    lam = (0.3, 0.2, 0.1)
    params = {}
    for name in multineg_ref.table_names(net, M):
        rows = META_SIZES[int(name.split(".")[1])] if "metadata" in name else (NU if "user" in name else NI)
        wide = name in ("user.weight", "item.weight") or name.startswith("metadata.")
        params[name] = rs.normal(0, 0.3, (rows, D if wide else 1))
    user = rs.randint(0, NU, B)
    user[1::3] = user[0]
    items = rs.randint(0, NI, (S, B))
    items[:, ::2] = 5  # one item in every slot of every second row
    item_meta = np.stack([rs.randint(0, META_SIZES[m], NI) for m in range(M)], 1) if M else None
    meta = item_meta[items] if M else None

    W = {k: torch.tensor(v, requires_grad=True) for k, v in params.items()}
    lu, li = multineg_ref.lin_names(net)
    u, it = torch.from_numpy(user), torch.from_numpy(items)
    pen = lam[0] * ((W["user.weight"][u] ** 2).sum() + (W[lu][u] ** 2).sum())
    pen = pen + lam[1] * ((W["item.weight"][it] ** 2).sum() + (W[li][it] ** 2).sum())
    for m in range(M):
        mid = torch.from_numpy(meta[:, :, m])
        pen = pen + lam[2] * (W[f"metadata.{m}.weight"][mid] ** 2).sum()
        if net == "fm":
            pen = pen + lam[2] * (W[f"linear_metadata.{m}.weight"][mid] ** 2).sum()
    (0.5 * pen / B).backward()
    got = l2_ref.grads(net, params, user, items, meta, lam, 1.0 / B)
    assert sorted(got) == sorted(params)
    for k in params:
        want = W[k].grad.numpy()
        assert np.abs(want).max() > 0, k
        assert rel_err(got[k], want) <= 1e-12, k
    rows = l2_ref.touched(net, params, user, items, meta)
    for k, g in got.items():
        keep = np.ones(g.shape[0], bool)
        keep[rows[k]] = False
        assert not g[keep].any(), k
        assert keep.any() or "metadata" in k, k  # (a 7-row metadata table may be referenced whole)
    # the staged form: zeros + c * W[id] per reference, coalesced per table
    F = 1 + S * (1 + M)
    gr, gl, _, _ = l2_ref.staged_add(net, params, user, items, meta, [c / B for c in lam], np.zeros((F, B, D)),
                                     np.zeros((F, B)))
    if S > 1:  # (multineg_ref.coalesce's blocks are (1 + K, B))
        summed = multineg_ref.coalesce(net, params, user, items, item_meta, gr, gl)
        for k in params:
            assert rel_err(summed[k], got[k]) <= 1e-12, k
    if net == "linear" and M:
        assert not gl[1 + S:].any()  # Linear has no 1-wide metadata tables


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


def test_fit_l2_argument_errors_name_the_argument_and_come_first(monkeypatch):
    from torchrecsys_amd import model as model_mod

    def no_device(*a, **kw):
        raise AssertionError("fit() reached the device before validating its arguments")
    monkeypatch.setattr(model_mod.TorchRecSys, "make_runner", no_device)

    def fit(m, **kw):
        m.fit(torch.optim.SGD(m.parameters(), lr=0.1), epochs=1, **kw)

    for bad in (True, False, -0.1, -1, float("inf"), float("-inf"), float("nan"), "0.1", None, [0.1], (0.1, 0.2, 0.3)):
        with pytest.raises(ValueError, match="l2"):
            fit(_model("fm"), l2=bad)
    for bad in ({"user": True}, {"item": -1e-3}, {"metadata": float("nan")}, {"user": float("inf")}, {"item": "x"},
                {"item": None}):
        with pytest.raises(ValueError, match=r"l2\["):
            fit(_model("linear"), l2=bad)
    for bad in ({"users": 0.1}, {"user": 0.1, "bias": 0.0}, {0: 0.1}):
        with pytest.raises(ValueError, match="unknown key"):
            fit(_model("fm"), l2=bad)
    # the MLP: any non-zero coefficient; the message says where its regularisation lives
    for bad in (0.01, {"item": 1e-6}, {"user": 0.0, "metadata": 0.5}):
        with pytest.raises(ValueError, match="weight_decay") as e:
            fit(_model("mlp"), l2=bad)
        assert "embedding rows are not covered" in str(e.value) and "net_type" in str(e.value)
    # valid arguments get past the checks (and, here, to the stub): zero on every net, non-zero with every option
    for kw in (dict(l2=0), dict(l2=0.0), dict(l2={}), dict(l2={"item": 0}), dict(l2={"user": 0.0, "metadata": 0})):
        with pytest.raises(AssertionError, match="reached the device"):
            fit(_model("mlp"), **kw)
    for kw in (dict(l2=0.01), dict(l2=1), dict(l2=np.float32(0.5)), dict(l2={"user": 0.05, "item": 0.02}),
               dict(l2={"metadata": 0.1}), dict(l2=0.01, loss="bpr"), dict(l2=0.01, loss="softmax", temperature=0.5),
               dict(l2=0.01, loss="sampled_softmax", n_negatives=8), dict(l2=0.01, loss="warp", n_negatives=4),
               dict(l2=0.01, loss="hinge", n_negatives=3)):
        for net in ("fm", "linear"):
            with pytest.raises(AssertionError, match="reached the device"):
                fit(_model(net), **kw)
    with pytest.raises(AssertionError, match="reached the device"):
        fit(_model("fm", neg_sampling={"mine": "hardest", "candidates": 4}), l2=0.01)
    with pytest.raises(AssertionError, match="reached the device"):
        fit(_model("fm", rng="reference"), l2={"item": 0.01})


def test_l2_reaches_the_trainer_only_when_a_coefficient_is_not_zero():
    from torchrecsys_amd.model import _check_l2
    assert _check_l2(0.0, "fm") is None and _check_l2({}, "mlp") is None and _check_l2({"item": 0}, "linear") is None
    assert _check_l2(0.03, "fm") == (0.03, 0.03, 0.03)
    assert _check_l2({"user": 0.05, "item": 0.02}, "linear") == (0.05, 0.02, 0.0)
    assert _check_l2({"metadata": 1}, "fm") == (0.0, 0.0, 1.0)
    from torchrecsys_amd.engine import SparseScorerTrainer
    assert SparseScorerTrainer.l2 is None


# ------------------------------------------------------------------------------------------- 3. the C entry point
def test_new_symbol_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "trs.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, hdr)
    assert NAME in _lib.PROTOTYPES and len(_lib.PROTOTYPES[NAME][1]) == 15
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert int(re.search(r"#define TRS_ABI_VERSION (\d+)", src).group(1)) == 6 == _lib.ABI_VERSION
    assert _lib.load().trs_abi_version() == 6
    assert "l2.hip" in open(os.path.join(ROOT, "torchrecsys_amd", "csrc", "Makefile")).read()


def _tables(D=8, M=0):
    T = _lib.TrsTables()
    T.user = T.item = T.user_lin = T.item_lin = P
    T.n_users, T.n_items, T.D, T.M = 50, 40, D, M
    for m in range(M):
        T.meta[m], T.meta_lin[m], T.n_meta[m] = P, P, 5
    return T


def test_stage_add_l2_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()
    FM, LINEAR = _lib.TRS_NET_FM, _lib.TRS_NET_LINEAR

    def add(T=_tables(), net=FM, user=P, items=P, meta=None, B=10, S=2, M=0, cu=0.1, ci=0.1, cm=0.1, gr=P, gl=P):
        return lib.trs_stage_add_l2(net, ctypes.byref(T) if T is not None else None, user, items, meta, B, S, M, cu, ci,
                                    cm, gr, gl, None, None)

    assert add(T=None) == -1 and "tables is NULL" in _err()
    assert _err().startswith(NAME)
    for net in (7, -1, 2):  # (2: the MLP has no staged rows)
        assert add(net=net) == -1 and "net must be" in _err(), net
    for bad in (0, -1, 66, 4096):
        assert add(S=bad) == -1 and "S=" in _err(), bad
    assert add(M=1) == -1 and "does not match" in _err()
    assert add(T=_tables(M=2), M=0) == -1 and "does not match" in _err()
    for D in (0, -4, 1025, 2048, 257, 999):  # odd widths are instantiated up to 256 only
        assert add(T=_tables(D=D)) == -1 and "n_factors" in _err(), D
    for member in ("user", "item", "user_lin", "item_lin"):
        T0 = _tables()
        setattr(T0, member, None)
        assert add(T=T0) == -1 and "NULL" in _err(), member
    T0 = _tables(M=2)
    T0.meta[1] = None
    assert add(T=T0, M=2, meta=P) == -1 and "metadata table 1" in _err()
    T0 = _tables(M=2)
    T0.meta_lin[0] = None
    assert add(T=T0, M=2, meta=P) == -1 and "linear_metadata" in _err()
    assert add(T=T0, M=2, meta=P, net=LINEAR, B=0) == 0  # (Linear has no 1-wide metadata tables)
    for which in ("cu", "ci", "cm"):
        for bad in (-0.1, -1e-30, float("inf"), float("-inf"), float("nan")):
            assert add(**{which: bad}) == -1 and "coefficient" in _err(), (which, bad)
    assert add(gr=None) == -1 and "grad_rows is NULL" in _err()
    assert add(gl=None) == -1 and "grad_lin is NULL" in _err()
    assert add(user=None) == -1 and "ids are NULL" in _err()
    assert add(items=None) == -1 and "ids are NULL" in _err()
    assert add(T=_tables(M=2), M=2) == -1 and "metadata ids are NULL" in _err()
    assert add(B=-1) == -1
    # nothing to launch: an empty batch (whatever the id pointers), or every coefficient 0
    assert add(B=0) == 0 and add(B=0, user=None, items=None) == 0
    assert add(T=_tables(M=2), M=2, B=0) == 0
    assert add(cu=0.0, ci=0.0, cm=0.0) == 0
    assert add(S=65, B=0) == 0 and add(S=1, B=0) == 0
