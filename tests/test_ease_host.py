# -*- coding: utf-8 -*-
"""EASE without a GPU: the binding, the host-side argument checks of the trs_ease_* entry points, the numpy restatement
tests/ease_ref.py against the real reference's output (tests/golden/g5_ease.npz, written by make_golden_ease.py) and
against numpy.linalg.inv, the model surface that answers before any device work, and the kernels' registers."""
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

import ease_ref as ref
from conftest import load_golden
from test_abi import ROOT, _shipped_kernel_registers
from torchrecsys_amd import _lib
from torchrecsys_amd.model import TorchRecSys

ENTRY_POINTS = ("trs_ease_gram", "trs_ease_invert_workspace_bytes", "trs_ease_invert", "trs_ease_weights",
                "trs_ease_scores")


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
    assert int(re.search(r"#define TRS_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 6
    assert int(re.search(r"#define TRS_EASE_NB (\d+)", src).group(1)) == _lib.EASE_NB
    assert int(re.search(r"#define TRS_EASE_NMAX (\d+)", src).group(1)) == _lib.EASE_NMAX == 32768
    mk = open(os.path.join(ROOT, "torchrecsys_amd", "csrc", "Makefile")).read()
    assert len(re.findall(r"\bease\.hip\b", mk)) == 1


def test_workspace_bytes_is_a_fixed_function_of_n():
    lib = _lib.load()
    for n in (1, 63, 64, 65, 200, 520, 16384, 32768):
        nbar = -(-n // _lib.EASE_NB) * _lib.EASE_NB
        assert lib.trs_ease_invert_workspace_bytes(n) == nbar * nbar * 8
    assert lib.trs_ease_invert_workspace_bytes(0) == 0 and lib.trs_ease_invert_workspace_bytes(32769) == 0


# ------------------------------------------------------------------------------------------------ arguments
def test_every_entry_point_rejects_bad_arguments_before_a_launch():
    """No GPU here: a call that got as far as a launch would fail with another code and another message."""
    lib = _lib.load()
    off = (ctypes.c_int64 * 3)(0, 1, 2)
    items = (ctypes.c_int32 * 2)(0, 1)
    good = _lib.TrsCsr(ctypes.cast(off, ctypes.c_void_p), ctypes.cast(items, ctypes.c_void_p), 2)
    no_arrays = _lib.TrsCsr(None, None, 2)
    csr, bad_csr = ctypes.byref(good), ctypes.byref(no_arrays)
    p = ctypes.c_void_p(64)  # a non-NULL, 16-byte aligned value that is never dereferenced: every call below is refused

    def refused(rc, entry, word):
        msg = lib.trs_last_error().decode()
        assert rc == -1 and msg.startswith(entry + ":") and word in msg, (rc, msg)

    g = lib.trs_ease_gram
    refused(g(csr, 2, 0, 0.5, p, None, None), "trs_ease_gram", "n=0")
    refused(g(csr, 2, 32769, 0.5, p, None, None), "trs_ease_gram", "n=32769")
    for lam in (0.0, -1.0, float("inf"), float("nan")):
        refused(g(csr, 2, 4, lam, p, None, None), "trs_ease_gram", "lambda")
    refused(g(csr, 2, 4, 0.5, None, None, None), "trs_ease_gram", "NULL")
    refused(g(None, 2, 4, 0.5, p, None, None), "trs_ease_gram", "NULL")
    refused(g(bad_csr, 2, 4, 0.5, p, None, None), "trs_ease_gram", "NULL")
    refused(g(csr, 3, 4, 0.5, p, None, None), "trs_ease_gram", "rows")
    refused(g(csr, -1, 4, 0.5, p, None, None), "trs_ease_gram", "n_users")

    inv = lib.trs_ease_invert
    ws = lib.trs_ease_invert_workspace_bytes(65)
    refused(inv(p, 0, p, ws, p, None), "trs_ease_invert", "n=0")
    refused(inv(p, 32769, p, 1 << 40, p, None), "trs_ease_invert", "n=32769")
    refused(inv(None, 65, p, ws, p, None), "trs_ease_invert", "NULL")
    refused(inv(p, 65, None, ws, p, None), "trs_ease_invert", "NULL")
    refused(inv(p, 65, p, ws, None, None), "trs_ease_invert", "NULL")
    refused(inv(p, 65, p, ws - 1, p, None), "trs_ease_invert", "workspace")
    refused(inv(ctypes.c_void_p(72), 65, p, ws, p, None), "trs_ease_invert", "aligned")

    w = lib.trs_ease_weights
    refused(w(p, 0, p, None), "trs_ease_weights", "n=0")
    refused(w(p, 32769, p, None), "trs_ease_weights", "n=32769")
    refused(w(None, 4, p, None), "trs_ease_weights", "NULL")
    refused(w(p, 4, None, None), "trs_ease_weights", "NULL")

    s = lib.trs_ease_scores
    refused(s(p, 0, csr, p, 1, p, None, None), "trs_ease_scores", "n=0")
    refused(s(p, 32769, csr, p, 1, p, None, None), "trs_ease_scores", "n=32769")
    refused(s(p, 4, csr, p, -1, p, None, None), "trs_ease_scores", "n_rows")
    refused(s(None, 4, csr, p, 1, p, None, None), "trs_ease_scores", "NULL")
    refused(s(p, 4, csr, None, 1, p, None, None), "trs_ease_scores", "NULL")
    refused(s(p, 4, csr, p, 1, None, None, None), "trs_ease_scores", "NULL")
    refused(s(p, 4, None, p, 1, p, None, None), "trs_ease_scores", "NULL")
    refused(s(p, 4, bad_csr, p, 1, p, None, None), "trs_ease_scores", "NULL")
    assert s(p, 4, csr, p, 0, p, None, None) == 0  # no rows: nothing to do, nothing launched


# ------------------------------------------------------------------------------------------------ restatement
def test_restatement_equals_the_reference():
    g = load_golden("g5_ease.npz")
    nu, n, lam = int(g["n_users"]), int(g["n_items"]), float(g["lam"])
    assert (nu, n, lam) == (150, 65, 0.5)
    lists = ref.histories(nu, n, int(g["seed"]))
    users = np.repeat(np.arange(nu), [len(v) for v in lists])
    assert np.array_equal(users, g["users"]) and np.array_equal(np.concatenate(lists), g["items"])
    assert np.unique(users * n + np.concatenate(lists)).size == users.size  # duplicate-free: binary X == the reference's
    b = ref.from_byte_planes(g["b_planes"], (n, n))
    pred = ref.from_byte_planes(g["pred_planes"], (nu, n))
    X = ref.dense_x(lists, n)
    B = ref.weights(np.linalg.inv(ref.gram(X, lam)))
    assert np.abs(B - b).max() <= 1e-12 and np.abs(X @ B - pred).max() <= 1e-12
    assert not np.allclose(B, B.T)  # column j is scaled by its own diagonal entry
    top6 = -np.sort(-pred, axis=1)[:, :6]
    assert ((top6[:, :-1] - top6[:, 1:]) < 1e-6).any(axis=1).sum() <= nu // 10  # the seed's property (make_golden_ease.py)


@pytest.mark.parametrize("nb", [16, 64, 128])
def test_blocked_restatement_equals_numpy_inv(nb):
    """The yardstick of the GPU test: the residual of the blocked route within 8 x numpy's on the same matrix.  (No 1 x 1
    case here: with 150 users numpy's inverse of it is one correctly rounded division whose residual, 8.7e-19, is below
    a float64 ulp, and no route through a square root can be held to a multiple of that.)"""
    for n, lam in ((2, 0.5), (65, 0.5), (200, 0.5), (200, 0.01)):
        A = ref.gram(ref.dense_x(ref.histories(150, n, n), n), lam)
        P0, P1 = np.linalg.inv(A), ref.blocked_inverse(A, nb)
        assert ref.residual(A, P1) <= 8 * ref.residual(A, P0)
        assert np.abs(P1 - P0).max() <= 1e-12 * np.abs(P0).max() * np.linalg.cond(A)
        assert np.array_equal(P1, P1.T)


def test_restatement_score_rows_and_tie_rules():
    B = np.array([[0, 1, 1, -2], [3, 0, 0, 0], [0, 0, 0, 0], [1, 1, 1, 0]], dtype=np.float32)
    rows = ref.score_rows(B, [[], [0], [0, 1, 3]])
    assert rows.tolist() == [[0, 0, 0, 0], [0, 1, 1, -2], [4, 2, 2, -2]]
    ids, sc = ref.recommend(rows, [[], [0], [0, 1, 3]], 3, True)
    assert ids.tolist() == [[0, 1, 2], [1, 2, 3], [2, -1, -1]] and sc[2].tolist() == [2.0, -np.inf, -np.inf]
    assert ref.rank(rows[1], 2, [0], True) == 1 and ref.rank(rows[1], 0, [0], True) == 2
    assert ref.item_weights(B, 0, 4)[0].tolist() == [1, 2, 3, -1]


# ------------------------------------------------------------------------------------------------ the model on the CPU
def _model(net_type='ease', **kw):
    rs = np.random.RandomState(0)
    u, i = torch.from_numpy(rs.randint(0, 40, 300)), torch.from_numpy(rs.randint(0, 30, 300))
    with contextlib.redirect_stdout(io.StringIO()):
        return TorchRecSys.from_tensors(u, i, n_users=40, n_items=30, net_type=net_type, **kw)


def test_ease_model_constructs_without_parameters_and_refuses_what_does_not_apply():
    m = _model(n_factors=7)
    assert m.net_type == 'ease' and not list(m.parameters()) and not m.state_dict()
    with pytest.raises(ValueError, match="metadata"):
        _model(item_metadata=torch.zeros((30, 1), dtype=torch.int64), metadata_names=['genre'])
    refusals = [
        (NotImplementedError, "fit_ease", lambda: m.fit(None)),
        (ValueError, "fit_ease", lambda: m.fit_als()),
        (NotImplementedError, "evaluate_ranking", lambda: m.evaluate()),
        (ValueError, "recommend_for_histories", lambda: m.fold_in_users([[1]])),
        (ValueError, "recommend_for_histories", lambda: m.fold_in_items([[1]])),
        (ValueError, "fit_ease", lambda: m.recommend_with_new_items([1], [99], torch.zeros(1, 7), torch.zeros(1))),
        (ValueError, "item_weights", lambda: m.similar_items([1])),
        (ValueError, "item_weights", lambda: m.similar_users([1])),
        (ValueError, r"recommend\(\)", lambda: m.recommend_diverse([1])),
        (ValueError, "evaluate_ranking", lambda: m.evaluate_diversity()),
        (ValueError, "fold-in options", lambda: m.recommend_for_histories([[1]], epochs=2)),
    ]
    for exc, hint, call in refusals:
        with pytest.raises(exc, match=hint) as e:
            call()
        assert "ease" in str(e.value)
    for call in (lambda: m.predict(0), lambda: m.item_weights([1]), lambda: m.recommend_for_histories([[1]]),
                 lambda: m.net.score_rows(torch.zeros(1, dtype=torch.int64)), lambda: m.net.score_all_items(0, None)):
        with pytest.raises(RuntimeError, match=r"call fit_ease\(\) first"):
            call()


def test_fit_ease_checks_its_arguments_before_any_device_work(monkeypatch):
    m = _model()
    for bad in (0, -1.0, float("nan"), float("inf"), None, "1", True):
        with pytest.raises(ValueError, match="regularization"):
            m.fit_ease(bad)
    with pytest.raises(ValueError, match="net_type='ease'"):
        _model('linear').fit_ease()
    with pytest.raises(ValueError, match="item_weights needs net_type='ease'"):
        _model('linear').item_weights([1])
    m.n_items = _lib.EASE_NMAX + 1
    with pytest.raises(ValueError, match="GB"):
        m.fit_ease()
    m.n_items = 30
    from torchrecsys_amd import dist as tdist
    monkeypatch.setattr(tdist, "world_info", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="single process"):
        m.fit_ease()


# ------------------------------------------------------------------------------------------------ registers
def test_no_ease_kernel_uses_scratch(tmp_path):
    found = _shipped_kernel_registers(tmp_path)
    mine = {n: v for n, v in found.items() if re.search(r"\dease_[a-z_]+_kernel", n)}
    families = {re.search(r"\d(ease_[a-z_]+_kernel)", n).group(1) for n in mine}
    assert families == {"ease_gram_init_kernel", "ease_gram_pairs_kernel", "ease_gram_diag_kernel",
                        "ease_chol_block_kernel", "ease_gemm_kernel", "ease_mirror_kernel", "ease_weights_kernel",
                        "ease_rows_kernel"}, sorted(families)
    assert len(mine) == 6 + 3 + 2  # three GEMM instances (NT, NN, TN), two of the score rows (16-byte loads or not)
    for n, (vgpr, scratch) in mine.items():
        assert scratch == 0, (n, vgpr, scratch)
