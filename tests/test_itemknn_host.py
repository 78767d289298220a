# -*- coding: utf-8 -*-
"""Item kNN without a GPU: the binding, the host-side argument checks of the trs_knn_* entry points, the numpy
restatement tests/itemknn_ref.py against a brute-force dense X^T X, the model surface that answers before any device
work, and the kernels' registers."""
import contextlib
import ctypes
import io
import math
import os
import re

import numpy as np
import pytest
import torch

import itemknn_ref as ref
from test_abi import ROOT, _shipped_kernel_registers
from torchrecsys_amd import _lib
from torchrecsys_amd.model import TorchRecSys

ENTRY_POINTS = ("trs_knn_build_workspace_bytes", "trs_knn_build", "trs_knn_scores")


# ------------------------------------------------------------------------------------------------ binding
def test_entry_points_are_declared_exported_and_bound_with_the_same_argument_counts():
    src = open(os.path.join(ROOT, "include", "trs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        proto = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, code)
        assert proto, f"{name} is not declared in include/trs.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(proto.group(1).split(",")) == len(_lib.PROTOTYPES[name][1]), name
    for name, value in (("KMAX", _lib.KNN_KMAX), ("TILE", _lib.KNN_TILE), ("TOUCHED", _lib.KNN_TOUCHED)):
        assert int(re.search(r"#define TRS_KNN_%s (\d+)" % name, src).group(1)) == value, name
    for kind, value in _lib.KNN_KIND.items():
        assert int(re.search(r"#define TRS_KNN_%s (\d+)" % kind.upper(), src).group(1)) == value, kind
    assert sorted(_lib.KNN_KIND) == sorted(ref.KINDS)
    assert _lib.KNN_KMAX == _lib.RETRIEVE_KMAX == 128
    assert _lib.KNN_TILE // 22 > _lib.KNN_TOUCHED  # the touched-list overflow case of tests/test_gpu_itemknn.py
    mk = open(os.path.join(ROOT, "torchrecsys_amd", "csrc", "Makefile")).read()
    assert len(re.findall(r"\bknn\.hip\b", mk)) == 1


def test_every_entry_point_rejects_bad_arguments_before_a_launch():
    """No GPU here: a call that got as far as a launch would fail with another code and another message."""
    lib = _lib.load()
    off = (ctypes.c_int64 * 3)(0, 1, 2)
    items = (ctypes.c_int32 * 2)(0, 1)
    ioff = (ctypes.c_int64 * 5)(0, 1, 2, 2, 2)
    good = _lib.TrsCsr(ctypes.cast(off, ctypes.c_void_p), ctypes.cast(items, ctypes.c_void_p), 2)
    good_inv = _lib.TrsCsr(ctypes.cast(ioff, ctypes.c_void_p), ctypes.cast(items, ctypes.c_void_p), 4)
    no_arrays = _lib.TrsCsr(None, None, 2)
    csr, inv, bad_csr = ctypes.byref(good), ctypes.byref(good_inv), ctypes.byref(no_arrays)
    p = ctypes.c_void_p(64)  # a non-NULL value that is never dereferenced: every call below is refused

    def refused(rc, entry, word):
        msg = lib.trs_last_error().decode()
        assert rc == -1 and msg.startswith(entry + ":") and word in msg, (rc, msg)

    assert lib.trs_knn_build_workspace_bytes(4, 10) > 0
    for n, K in ((0, 10), (2 ** 31, 10), (4, 0), (4, _lib.KNN_KMAX + 1)):
        assert lib.trs_knn_build_workspace_bytes(n, K) == 0
    ws = lib.trs_knn_build_workspace_bytes(4, 10)
    b, who = lib.trs_knn_build, "trs_knn_build"
    refused(b(csr, inv, 2, 0, 0, 0.0, 10, p, p, p, ws, None, None), who, "n=0")
    refused(b(csr, inv, -1, 4, 0, 0.0, 10, p, p, p, ws, None, None), who, "n_users")
    for K in (0, -1, _lib.KNN_KMAX + 1):
        refused(b(csr, inv, 2, 4, 0, 0.0, K, p, p, p, ws, None, None), who, "K=")
    for kind in (-1, 4):
        refused(b(csr, inv, 2, 4, kind, 0.0, 10, p, p, p, ws, None, None), who, "kind")
    for h in (-1.0, float("nan"), float("inf")):
        refused(b(csr, inv, 2, 4, 0, h, 10, p, p, p, ws, None, None), who, "shrinkage")
    refused(b(csr, inv, 2, 4, 0, 0.0, 10, None, p, p, ws, None, None), who, "NULL")
    refused(b(csr, inv, 2, 4, 0, 0.0, 10, p, None, p, ws, None, None), who, "NULL")
    refused(b(None, inv, 2, 4, 0, 0.0, 10, p, p, p, ws, None, None), who, "NULL")
    refused(b(csr, None, 2, 4, 0, 0.0, 10, p, p, p, ws, None, None), who, "NULL")
    refused(b(bad_csr, inv, 2, 4, 0, 0.0, 10, p, p, p, ws, None, None), who, "NULL")
    refused(b(csr, inv, 3, 4, 0, 0.0, 10, p, p, p, ws, None, None), who, "rows")
    refused(b(csr, inv, 2, 5, 0, 0.0, 10, p, p, p, ws, None, None), who, "rows")
    refused(b(csr, inv, 2, 4, 0, 0.0, 10, p, p, None, ws, None, None), who, "workspace")
    refused(b(csr, inv, 2, 4, 0, 0.0, 10, p, p, p, ws - 1, None, None), who, "workspace")

    s, who = lib.trs_knn_scores, "trs_knn_scores"
    refused(s(p, p, 0, 10, csr, p, 1, p, None, None), who, "n=0")
    refused(s(p, p, 4, 0, csr, p, 1, p, None, None), who, "K=")
    refused(s(p, p, 4, _lib.KNN_KMAX + 1, csr, p, 1, p, None, None), who, "K=")
    refused(s(p, p, 4, 10, csr, p, -1, p, None, None), who, "n_rows")
    refused(s(None, p, 4, 10, csr, p, 1, p, None, None), who, "NULL")
    refused(s(p, None, 4, 10, csr, p, 1, p, None, None), who, "NULL")
    refused(s(p, p, 4, 10, csr, None, 1, p, None, None), who, "NULL")
    refused(s(p, p, 4, 10, csr, p, 1, None, None, None), who, "NULL")
    refused(s(p, p, 4, 10, None, p, 1, p, None, None), who, "NULL")
    refused(s(p, p, 4, 10, bad_csr, p, 1, p, None, None), who, "NULL")
    refused(s(p, p, 8192 * 65535 + 1, 10, csr, p, 1, p, None, None), who, "tiles")
    assert s(p, p, 4, 10, csr, p, 0, p, None, None) == 0  # no rows: nothing launched


# ------------------------------------------------------------------------------------------------ the restatement
def brute_force(lists, n, kind, h, K):
    """Dense X^T X and Python scalars: (ids, w) lists of lists, independent of itemknn_ref's vectorised route."""
    X = np.zeros((len(lists), n), dtype=np.int64)
    for u, v in enumerate(lists):
        X[u, np.asarray(v, dtype=np.int64)] = 1
    Cm = X.T @ X
    ids, w = [], []
    for i in range(n):
        cand = []
        for j in range(n):
            c, ni, nj = int(Cm[i, j]), int(Cm[i, i]), int(Cm[j, j])
            if j == i or c == 0:
                continue
            if kind == "cosine":
                s = c / (math.sqrt(float(ni * nj)) + h)
            elif kind == "jaccard":
                s = c / (float(ni + nj - c) + h)
            elif kind == "conditional":
                s = c / (float(ni) + h)
            else:
                s = float(c)
            cand.append((-float(np.float32(s)), j))
        cand.sort()
        ids.append([j for _, j in cand[:K]] + [-1] * (K - len(cand[:K])))
        w.append([np.float32(-s) for s, _ in cand[:K]] + [np.float32(0)] * (K - len(cand[:K])))
    return np.array(ids, dtype=np.int32).reshape(n, K), np.array(w, dtype=np.float32).reshape(n, K)


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("n,n_users", [(1, 20), (2, 40), (65, 150), (200, 400)])
def test_restatement_against_brute_force_dense_counts(kind, n, n_users):
    lists = ref.histories(n_users, n, seed=n)
    pairs = ref.cocounts(lists, n)
    for h, K in ((0.0, 1), (10.0, 7), (0.0, 64), (2.5, 128)):
        ids, w = ref.neighbours(pairs, n, kind, h, K)
        bi, bw = brute_force(lists, n, kind, h, K)
        assert np.array_equal(ids, bi), (h, K)
        assert np.array_equal(w.view(np.int32), bw.view(np.int32)), (h, K)
    inv = ref.inverse(lists, n)
    assert [len(v) for v in inv] == pairs[3].tolist()
    assert all(i in lists[u] for i in range(n) for u in inv[i])


def test_restatement_orders_ties_by_id_pads_and_scores_in_float32():
    lists = [[0, 1], [0, 2], [0, 3], [4]]  # item 0 meets 1, 2, 3 once each; item 4 meets nobody; item 5 has no user
    pairs = ref.cocounts(lists, 6)
    ids, w = ref.neighbours(pairs, 6, "count", 0.0, 2)
    assert ids.tolist() == [[1, 2], [0, -1], [0, -1], [0, -1], [-1, -1], [-1, -1]]
    assert w.tolist() == [[1, 1], [1, 0], [1, 0], [1, 0], [0, 0], [0, 0]]
    rows = ref.score_rows(ids, w, [[], [0], [1, 2, 3], [4, 5]], 6)
    assert rows.dtype == np.float32
    assert rows.tolist() == [[0] * 6, [0, 1, 1, 0, 0, 0], [3, 0, 0, 0, 0, 0], [0] * 6]
    c = ref.similarity("cosine", np.array([1]), np.array([3]), np.array([1]), 0.0)
    assert c[0] == np.float32(1.0 / math.sqrt(3.0))
    oi, ow = ref.item_weights(ids, w, 1, 3)
    assert oi.tolist() == [0, -1, -1] and ow.tolist() == [1.0, -np.inf, -np.inf]


# ------------------------------------------------------------------------------------------------ the model on the CPU
def _model(net_type='itemknn', **kw):
    rs = np.random.RandomState(0)
    u, i = torch.from_numpy(rs.randint(0, 40, 300)), torch.from_numpy(rs.randint(0, 30, 300))
    with contextlib.redirect_stdout(io.StringIO()):
        return TorchRecSys.from_tensors(u, i, n_users=40, n_items=30, net_type=net_type, **kw)


def test_itemknn_model_constructs_without_parameters_and_refuses_what_does_not_apply():
    m = _model(n_factors=7)
    assert m.net_type == 'itemknn' and not list(m.parameters()) and not m.state_dict()
    with pytest.raises(ValueError, match="metadata"):
        _model(item_metadata=torch.zeros((30, 1), dtype=torch.int64), metadata_names=['genre'])
    refusals = [
        (NotImplementedError, "fit_itemknn", lambda: m.fit(None)),
        (ValueError, "fit_itemknn", lambda: m.fit_als()),
        (ValueError, "fit_itemknn", lambda: m.fit_lightgcn()),
        (ValueError, "net_type='ease'", lambda: m.fit_ease()),
        (NotImplementedError, "evaluate_ranking", lambda: m.evaluate()),
        (ValueError, "recommend_for_histories", lambda: m.fold_in_users([[1]])),
        (ValueError, "recommend_for_histories", lambda: m.fold_in_items([[1]])),
        (ValueError, "fit_itemknn", lambda: m.recommend_with_new_items([1], [99], torch.zeros(1, 7), torch.zeros(1))),
        (ValueError, "item_weights", lambda: m.similar_items([1])),
        (ValueError, "item_weights", lambda: m.similar_users([1])),
        (ValueError, r"recommend\(\)", lambda: m.recommend_diverse([1])),
        (ValueError, "evaluate_ranking", lambda: m.evaluate_diversity()),
        (ValueError, "fold-in options", lambda: m.recommend_for_histories([[1]], epochs=2)),
    ]
    for exc, hint, call in refusals:
        with pytest.raises(exc, match=hint) as e:
            call()
        assert "itemknn" in str(e.value) and "fit_ease()" not in str(e.value).replace("or fit_ease()", "")
    for call in (lambda: m.predict(0), lambda: m.item_weights([1]), lambda: m.recommend_for_histories([[1]]),
                 lambda: m.net.score_rows(torch.zeros(1, dtype=torch.int64)), lambda: m.net.score_all_items(0, None)):
        with pytest.raises(RuntimeError, match=r"call fit_itemknn\(\) first"):
            call()


def test_the_messages_for_ease_are_unchanged():
    m = _model('ease')
    with pytest.raises(NotImplementedError) as e:
        m.fit(None)
    assert str(e.value) == ("fit() does not apply to net_type='ease' (a closed-form item-item model without embedding "
                            "rows): call fit_ease(), which needs no optimiser")
    with pytest.raises(ValueError) as e:
        m.fold_in_users([[1]])
    assert str(e.value) == ("fold_in_users() does not apply to net_type='ease' (a closed-form item-item model without "
                            "embedding rows): call recommend_for_histories(), which needs no fitting with EASE")


def test_fit_itemknn_checks_its_arguments_before_any_device_work(monkeypatch):
    m = _model()
    for bad in (-1.0, float("nan"), float("inf"), None, "1", True):
        with pytest.raises(ValueError, match="shrinkage"):
            m.fit_itemknn(shrinkage=bad)
    for bad in (0, -1, _lib.KNN_KMAX + 1, 10.0, None, "7", True):
        with pytest.raises(ValueError, match="neighbours"):
            m.fit_itemknn(neighbours=bad)
    for bad in ("euclid", "", None, 0, "Cosine"):
        with pytest.raises(ValueError, match="similarity"):
            m.fit_itemknn(similarity=bad)
    for other in ('linear', 'ease'):
        with pytest.raises(ValueError, match="net_type='itemknn'"):
            _model(other).fit_itemknn()
    with pytest.raises(ValueError, match="item_weights needs net_type='ease'"):
        _model('linear').item_weights([1])
    from torchrecsys_amd import dist as tdist
    monkeypatch.setattr(tdist, "world_info", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="single process"):
        m.fit_itemknn()


# ------------------------------------------------------------------------------------------------ registers
def test_no_knn_kernel_uses_scratch(tmp_path):
    found = _shipped_kernel_registers(tmp_path)
    mine = {n: v for n, v in found.items() if re.search(r"\dknn_[a-z_]+_kernel", n)}
    families = {re.search(r"\d(knn_[a-z_]+_kernel)", n).group(1) for n in mine}
    assert families == {"knn_build_kernel", "knn_rows_kernel"}, sorted(families)
    for n, (vgpr, scratch) in mine.items():
        assert scratch == 0 and vgpr <= 128, (n, vgpr, scratch)  # knn_build_kernel runs 16 waves per CU
