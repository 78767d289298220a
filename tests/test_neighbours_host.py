# -*- coding: utf-8 -*-
"""similar_items() / similar_users() without a GPU: the two C entry points are declared, exported and bound; their
arguments and the public methods' arguments are validated on the host before any device work; the numpy oracle
(tests/neighbours_ref.py) has the properties the GPU tests rely on."""
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pandas as pd
import pytest

import neighbours_ref as ref
from torchrecsys_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("trs_neighbour_fold", "trs_neighbours_topk")


def _err():
    return _lib.load().trs_last_error().decode()


def test_new_symbols_declared_exported_and_bound():
    lib = _lib.load()
    assert lib.trs_abi_version() == _lib.ABI_VERSION == 6
    header = open(os.path.join(ROOT, "include", "trs.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(raw, name), name
    assert len(_lib.PROTOTYPES["trs_neighbour_fold"][1]) == 8
    assert len(_lib.PROTOTYPES["trs_neighbours_topk"][1]) == 12


def test_entry_points_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    P = 0x1000  # never dereferenced
    fb = lib.trs_item_fold_bytes(300, 24)
    assert fb == 384 * 33 * 4
    fold = lambda *a: lib.trs_neighbour_fold(*a, None)
    assert fold(None, 300, 24, 24, 1, P, fb) == -1 and "NULL" in _err()
    assert fold(P, 0, 24, 24, 1, P, fb) == -1 and "n_rows" in _err()
    assert fold(P, 300, 0, 24, 1, P, fb) == -1 and "D=0" in _err()
    assert fold(P, 300, _lib.RETRIEVE_DMAX + 1, 300, 1, P, 1 << 30) == -1 and "D=" in _err()
    assert fold(P, 300, 24, 23, 1, P, fb) == -1 and "ld=" in _err()
    assert fold(P, 300, 24, 24, 2, P, fb) == -1 and "cosine" in _err()
    assert fold(P, 300, 24, 24, 1, P, fb - 4) == -1 and "fold buffer too small" in _err()
    assert fold(P, 300, 24, 24, 1, None, fb) == -1 and "fold buffer" in _err()

    ws = lib.trs_retrieve_workspace_bytes(5, 10)

    def topk(n_rows=300, D=24, k=10, n_q=5, fold_dev=P, fold_bytes=fb, queries=P, ids=P, sc=P, w=P, wb=ws):
        return lib.trs_neighbours_topk(fold_dev, fold_bytes, n_rows, D, queries, n_q, k, ids, sc, w, wb, None)
    assert topk(n_rows=0) == -1 and "n_rows" in _err()
    assert topk(k=0) == -1 and "k=0" in _err()
    K1 = _lib.RETRIEVE_KMAX + 1
    assert topk(k=K1, wb=lib.trs_retrieve_workspace_bytes(5, K1)) == -1 and f"k={K1}" in _err()
    assert topk(n_rows=5, k=6, fold_bytes=1 << 20) == -1 and "k=6 > n_items=5" in _err()
    assert topk(n_q=-1) == -1 and "n_q" in _err()
    assert topk(D=_lib.RETRIEVE_DMAX + 1) == -1 and "D=" in _err()
    assert topk(fold_bytes=fb - 4) == -1 and "fold buffer too small" in _err()
    assert topk(fold_dev=None) == -1 and "fold buffer" in _err()
    assert topk(wb=ws - 8) == -1 and "workspace too small" in _err()
    assert topk(w=None) == -1 and "workspace" in _err()
    assert topk(queries=None) == -1 and "NULL" in _err()
    assert topk(ids=None) == -1 and "NULL" in _err()
    assert topk(sc=None) == -1 and "NULL" in _err()
    assert topk(n_q=0, queries=None, w=None, wb=0) == 0  # nothing to do, nothing launched
    for msg_owner in ("trs_neighbours_topk",):
        topk(k=0)
        assert _err().startswith(msg_owner)


def _df():
    rs = np.random.RandomState(0)
    return pd.DataFrame({"user_id": np.concatenate([np.arange(40), rs.randint(0, 40, 360)]),
                         "item_id": np.concatenate([np.arange(30), rs.randint(0, 30, 370)])})


def _model(net_type, n_factors=8):
    from torchrecsys_amd.model import TorchRecSys
    with contextlib.redirect_stdout(io.StringIO()):
        return TorchRecSys(_df(), "user_id", "item_id", n_factors=n_factors, net_type=net_type)


def test_argument_errors_come_before_any_device_work(monkeypatch):
    from torchrecsys_amd import model as model_mod

    def no_device(*a, **kw):
        raise AssertionError("reached the device before validating the arguments")
    monkeypatch.setattr(model_mod, "_device", no_device)
    for fn in ("similar_items", "similar_users"):
        m = _model("fm")
        for bad in ("euclid", "", None, "Cosine", 1):
            with pytest.raises(ValueError, match="metric"):
                getattr(m, fn)([0], metric=bad)
        with pytest.raises(ValueError, match="mlp") as e:
            getattr(_model("mlp"), fn)([0])
        assert "concatenated" in str(e.value)
        with pytest.raises(ValueError, match="n_factors"):
            getattr(_model("linear", n_factors=257), fn)([0], metric="dot")
        # empty queries and top_k <= 0 need no device either; unknown ids are found on the host
        ids, sc = getattr(m, fn)([], top_k=4, return_scores=True)
        assert ids.shape == (0, 4) and sc.shape == (0, 4) and str(ids.dtype) == "torch.int64"
        assert getattr(m, fn)([1, 2], top_k=0).shape == (2, 0)
        with pytest.raises(IndexError, match="1000"):
            getattr(m, fn)([0, 1000])
        with pytest.raises(AssertionError, match="reached the device"):  # valid arguments get as far as the device
            getattr(m, fn)([0, 1], top_k=3, metric="dot")


def test_oracle_ranking_self_exclusion_tie_order_and_padding():
    rs = np.random.RandomState(3)
    X = rs.randint(-2, 3, (40, 6)).astype(np.float64)  # many ties
    X[9] = X[4]
    q = np.array([4, 9, 0, 39, 4])
    for metric in ("dot", "cosine"):
        vals = ref.similarities(X, q, metric)
        ids, v = ref.rank(vals, q, 40)
        for r, qq in enumerate(q):
            assert qq not in ids[r] and ids[r, -1] == -1 and np.isneginf(v[r, -1])
            assert sorted(ids[r, :-1].tolist()) == [x for x in range(40) if x != qq]
            assert np.all(np.diff(v[r, :-1]) <= 0)
            same = np.diff(v[r, :-1]) == 0
            assert np.all(np.diff(ids[r, :-1])[same] > 0)  # ties: ascending id
            assert np.array_equal(v[r, :-1], vals[r][ids[r, :-1]])
        if metric == "cosine":  # the identical row is returned, with cosine 1
            assert 9 in ids[0] and 4 in ids[1] and abs(v[0, 0] - 1.0) < 1e-12 and abs(v[1, 0] - 1.0) < 1e-12
    ids, v = ref.rank(ref.similarities(X, q, "dot"), q, 3)
    assert ids.shape == (5, 3) and np.all(ids >= 0)
    a = ref.neighbours(X, q, 7, "dot", block=2)
    b = ref.rank(ref.similarities(X, q, "dot"), q, 7)
    c = ref.neighbours_int(X, q, 7, block=2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(c[0], b[0]) and np.array_equal(c[1], b[1])
    ids, v = ref.neighbours_int(X[:3], [0, 1, 2], 5)
    assert np.all(ids[:, 2:] == -1) and np.all(np.isneginf(v[:, 2:])) and np.all(ids[:, :2] >= 0)


def test_oracle_normalisation_fp32_restatement():
    rs = np.random.RandomState(1)
    for D in (3, 16, 100, 256):
        X = rs.randn(50, D).astype(np.float32)
        X[7] = 0.0
        got = ref.normalise_f32(X)
        assert got.dtype == np.float32 and not got[7].any()
        want = ref.normalise(X.astype(np.float64))
        assert np.abs(got - want).max() <= 4 * 2.0 ** -24  # a few roundings of values below 1
        n = np.sqrt((got.astype(np.float64) ** 2).sum(1))
        assert np.all(np.abs(np.delete(n, 7) - 1.0) <= 1e-6)
    # rows with 4 or 16 entries of +-1: norms 2 and 4, the restatement is exact
    X = np.zeros((2, 24), np.float32)
    X[0, [0, 5, 9, 23]] = [1, -1, 1, -1]
    X[1, :16] = 1
    assert np.array_equal(ref.normalise_f32(X), ref.normalise(X.astype(np.float64)).astype(np.float32))
    assert set(np.unique(np.abs(ref.normalise_f32(X))).tolist()) == {0.0, 0.25, 0.5}
    assert ref.tol(24) == 40 * 2.0 ** -23 and ref.tol(100) == 136 * 2.0 ** -23 and ref.dp(8) == 16
