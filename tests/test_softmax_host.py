# -*- coding: utf-8 -*-
"""In-batch softmax loss without a GPU: the C-ABI entry points (include/trs.h "in-batch softmax") are declared, exported
and bound, validate their arguments on the host before any launch, and fit(loss='softmax') rejects what it does not
support before it touches the device."""
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

from torchrecsys_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("trs_softmax_workspace_bytes", "trs_softmax_stage", "trs_softmax_rows", "trs_softmax_grads")
P = 0x1000  # a non-NULL pointer that validation never dereferences


def _err():
    return _lib.load().trs_last_error().decode()


def _tables(n_users=10, n_items=20, D=8):
    T = _lib.TrsTables()
    T.user = T.item = T.user_lin = T.item_lin = P
    T.n_users, T.n_items, T.D, T.M = n_users, n_items, D, 0
    return T


def _batch(B=5):
    b = _lib.TrsBatch()
    b.user = b.pos = P
    b.B, b.idx_bytes = B, 4
    return b


def test_new_symbols_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trs.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(raw, name), name
    assert lib.trs_abi_version() == _lib.ABI_VERSION == 6


def test_workspace_bytes_follow_the_documented_layout():
    lib = _lib.load()
    assert lib.trs_softmax_workspace_bytes(0, 64) == 0 and lib.trs_softmax_workspace_bytes(10, 0) == 0
    for B, D in [(1, 1), (7, 8), (300, 64), (1000, 17), (16384, 64), (65536, 128), (5, 300)]:
        Dp = 16
        while Dp < D:
            Dp *= 2
        blk = lambda n: (n + 63) // 64 * 64  # noqa: E731
        want = 4 * (4 * blk(B * (Dp + 4)) + 3 * blk(B))
        assert lib.trs_softmax_workspace_bytes(B, D) == want, (B, D)


def _stage(lib, T, b, tau=1.0, ws=P, ws_bytes=None):
    nb = lib.trs_softmax_workspace_bytes(b.B if b is not None else 5, T.D if T is not None else 8) \
        if ws_bytes is None else ws_bytes
    return lib.trs_softmax_stage(_lib.TRS_NET_FM, ctypes.byref(T) if T is not None else None,
                                 ctypes.byref(b) if b is not None else None, tau, None, ws, nb, None)


def test_stage_rejects_bad_arguments():
    lib = _lib.load()
    T, b = _tables(), _batch()
    need = lib.trs_softmax_workspace_bytes(5, 8)
    assert _stage(lib, None, b) == -1 and "tables is NULL" in _err()
    assert _stage(lib, T, None) == -1 and "batch is NULL" in _err()
    T0 = _tables()
    T0.user = None
    assert _stage(lib, T0, b) == -1 and "user/item table" in _err()
    b0 = _batch()
    b0.pos = None
    assert _stage(lib, T, b0) == -1 and "user/pos ids are NULL" in _err()
    assert _stage(lib, T, _batch(0), ws_bytes=need) == -1 and "B=0 < 1" in _err()
    for tau in (0.0, -1.0, float("inf"), float("nan")):
        assert _stage(lib, T, b, tau=tau) == -1 and "temperature" in _err(), tau
    assert _stage(lib, T, b, ws=None) == -1 and "workspace is NULL" in _err()
    assert _stage(lib, T, b, ws_bytes=need - 4) == -1 and "workspace too small" in _err()
    assert lib.trs_softmax_stage(7, ctypes.byref(T), ctypes.byref(b), 1.0, None, P, need, None) == -1
    assert "net must be" in _err()


def test_rows_rejects_bad_arguments():
    lib = _lib.load()
    B, D = 6, 8
    need = lib.trs_softmax_workspace_bytes(B, D)
    zb = 4 * B * B

    def rows(z=P, z_bytes=zb, row0=0, n=B, B_=B, tau=1.0, ws=P, ws_bytes=need):
        return lib.trs_softmax_rows(z, z_bytes, row0, n, B_, D, tau, ws, ws_bytes, None)

    assert rows(z=None) == -1 and "logits are NULL" in _err()
    assert rows(ws=None) == -1 and "workspace is NULL" in _err()
    assert rows(B_=0, n=0, ws_bytes=0) == -1 and "B=0 < 1" in _err()
    assert rows(tau=0.0) == -1 and "temperature" in _err()
    assert rows(tau=-2.0) == -1 and "temperature" in _err()
    assert rows(ws_bytes=need - 1) == -1 and "workspace too small" in _err()
    assert rows(row0=4, n=3) == -1 and "outside [0, 6)" in _err()
    assert rows(n=0) == -1 and "outside" in _err()
    assert rows(z_bytes=zb - 4) == -1 and "logit buffer too small" in _err()


def test_grads_rejects_bad_arguments():
    lib = _lib.load()
    T, b = _tables(), _batch()
    need = lib.trs_softmax_workspace_bytes(5, 8)

    def grads(T_=T, b_=b, tau=1.0, ws=P, ws_bytes=need, gr=P, gl=P, loss=P):
        return lib.trs_softmax_grads(_lib.TRS_NET_LINEAR, ctypes.byref(T_) if T_ is not None else None,
                                     ctypes.byref(b_) if b_ is not None else None, tau, ws, ws_bytes, gr, gl, loss,
                                     None)

    assert grads(T_=None) == -1 and "tables is NULL" in _err()
    assert grads(b_=None) == -1 and "batch is NULL" in _err()
    assert grads(loss=None) == -1 and "loss_sum is NULL" in _err()
    assert grads(gl=None) == -1 and "both be given or both NULL" in _err()
    assert grads(ws=None) == -1 and "workspace is NULL" in _err()
    assert grads(b_=_batch(0)) == -1 and "B=0 < 1" in _err()
    assert grads(tau=0.0) == -1 and "temperature" in _err()
    assert grads(ws_bytes=need - 8) == -1 and "workspace too small" in _err()
    T0 = _tables()
    T0.item_lin = None
    assert grads(T_=T0) == -1 and "1-wide item table" in _err()


# ---------------------------------------------------------------------------------------------- fit() arguments
def _df(seed=0):
    rs = np.random.RandomState(seed)
    return pd.DataFrame({"user_id": np.concatenate([np.arange(40), rs.randint(0, 40, 360)]),
                         "item_id": np.concatenate([np.arange(30), rs.randint(0, 30, 370)])})


def _model(net_type):
    from torchrecsys_amd.model import TorchRecSys
    with contextlib.redirect_stdout(io.StringIO()):
        return TorchRecSys(_df(), "user_id", "item_id", n_factors=8, net_type=net_type)


def test_fit_softmax_argument_errors_come_first():
    mlp = _model("mlp")
    opt = torch.optim.SGD(mlp.parameters(), lr=0.1)
    with pytest.raises(ValueError, match=r"(?s)Linear.*FM"):
        mlp.fit(opt, epochs=1, loss="softmax")
    for net_type in ("linear", "fm"):
        m = _model(net_type)
        opt = torch.optim.SGD(m.parameters(), lr=0.1)
        for tau in (0.0, -1.0, math.inf, math.nan, "x"):
            with pytest.raises(ValueError, match="temperature"):
                m.fit(opt, epochs=1, loss="softmax", temperature=tau)
        with pytest.raises(ValueError, match="softmax"):
            m.fit(opt, epochs=1, loss="hinge", temperature=0.5)
        with pytest.raises(ValueError, match="softmax"):
            m.fit(opt, epochs=1, loss="bpr", logq_correction=True)
        with pytest.raises(ValueError, match="softmax"):
            m.fit(opt, epochs=1, loss="nope")
        m.neg_sampling = {"k": 2}
        with pytest.raises(ValueError, match="neg_sampling"):
            m.fit(opt, epochs=1, loss="softmax")
    assert "softmax" not in _lib.LOSS_ID


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_fit_softmax_with_valid_arguments_needs_the_device():
    m = _model("fm")
    with pytest.raises(RuntimeError, match="MI355X"):
        m.fit(torch.optim.SGD(m.parameters(), lr=0.1), epochs=1, loss="softmax", temperature=0.1, logq_correction=True)
