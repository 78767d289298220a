# -*- coding: utf-8 -*-
"""fit_als() without a GPU: trs_als_gram / trs_als_solve are declared, exported and bound; their arguments and fit_als's
are validated on the host before any device work; and the numpy restatement of the rule (tests/als_ref.py) really is
ALS: run to convergence it gives the dense solution of the weighted normal equations, and one iteration lowers the
objective it reports."""
import ctypes
import os
import re

import numpy as np
import pytest

import als_ref as ref
import foldin_ref as base
from torchrecsys_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTO = _lib.PROTOTYPES["trs_als_solve"]  # this module is about that entry point: without its binding nothing applies


def _err():
    return _lib.load().trs_last_error().decode()


def test_symbols_declared_exported_and_bound():
    lib = _lib.load()
    assert lib.trs_abi_version() == _lib.ABI_VERSION == 6  # added without touching a signature: no bump
    header = open(os.path.join(ROOT, "include", "trs.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in (("trs_als_gram", 7), ("trs_als_solve", 12), ("trs_als_gram_workspace_bytes", 2)):
        assert re.search(r"\b%s\s*\(" % name, header)
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        assert len(_lib.PROTOTYPES[name][1]) == n_args
        decl = header[header.index(name + "("):]
        assert decl[:decl.index(")")].count(",") == n_args - 1
    assert open(os.path.join(ROOT, "torchrecsys_amd", "csrc", "Makefile")).read().count("als.hip") == 1


def test_gram_workspace_is_a_fixed_function_of_the_shape():
    lib = _lib.load()
    ws = lib.trs_als_gram_workspace_bytes
    assert ws(0, 8) == 0 and ws(1, 8) == 8 * 8 * 4 and ws(16, 8) == 8 * 8 * 4 and ws(17, 8) == 2 * 8 * 8 * 4
    assert ws(150, 24) == 10 * 24 * 24 * 4  # the GPU tests' shapes reduce several chunks
    assert ws(10_000_000, 128) <= 512 * 128 * 128 * 4 and ws(10_000_000, 256) <= 256 * 256 * 256 * 4
    assert ws(-1, 8) == 0 and ws(10, 0) == 0 and ws(10, 257) == 0


def test_entry_points_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    P = 0x1000  # never dereferenced
    inf, nan = float("inf"), float("nan")

    def csr(off=P, items=P, n_rows=5):
        c = _lib.TrsCsr()
        c.off, c.items, c.n_rows = off, items, n_rows
        return c

    def solve(other=P, n_other=100, D=24, G=P, nbr=csr(), lam=0.1, alpha=10.0, cg=3, rows=P, n_rows=5, err=None):
        return lib.trs_als_solve(other, n_other, D, G, ctypes.byref(nbr) if nbr is not None else None, lam, alpha, cg,
                                 rows, n_rows, err, None)
    for kw, word in ((dict(D=0), "D=0"), (dict(D=257), "D=257"), (dict(cg=0), "cg_steps"), (dict(cg=257), "cg_steps"),
                     (dict(lam=0.0), "lambda"), (dict(lam=-1.0), "lambda"), (dict(lam=inf), "lambda"),
                     (dict(lam=nan), "lambda"), (dict(alpha=-0.5), "alpha"), (dict(alpha=inf), "alpha"),
                     (dict(alpha=nan), "alpha"), (dict(n_rows=-1), "n_rows"), (dict(other=None), "NULL"),
                     (dict(G=None), "NULL"), (dict(rows=None), "NULL"), (dict(nbr=None), "NULL"),
                     (dict(nbr=csr(off=None)), "NULL"), (dict(nbr=csr(items=None)), "NULL"),
                     (dict(nbr=csr(n_rows=4)), "rows"), (dict(n_other=0), "n_other"), (dict(n_other=1 << 31), "n_other")):
        assert solve(**kw) == -1, kw
        assert _err().startswith("trs_als_solve:") and word in _err(), (kw, _err())
    # nothing to do, nothing launched (the arrays may then be NULL); bad arguments are still bad
    assert solve(n_rows=0) == 0
    assert solve(n_rows=0, other=None, G=None, rows=None, nbr=None) == 0
    assert solve(n_rows=0, cg=0) == -1 and "cg_steps" in _err()
    assert solve(n_rows=0, lam=0.0) == -1 and "lambda" in _err()
    assert solve(alpha=0.0, n_rows=0) == 0  # alpha == 0 is allowed

    def gram(rows=P, n=10, D=24, ld=24, G=P, ws=P):
        return lib.trs_als_gram(rows, n, D, ld, G, ws, None)
    for kw, word in ((dict(D=0), "D=0"), (dict(D=257), "D=257"), (dict(n=-1), "n="), (dict(ld=23), "ld="),
                     (dict(G=None), "NULL"), (dict(rows=None), "NULL"), (dict(ws=None), "NULL")):
        assert gram(**kw) == -1, kw
        assert _err().startswith("trs_als_gram:") and word in _err(), (kw, _err())


# ------------------------------------------------------------------------------------------------ fit_als arguments
def _model(net_type, M=0, n_factors=8, **kw):
    return base.make_model(net_type, 40, 30, n_factors, M, seed=1, scale=0.3, **kw)


def test_fit_als_refusals_come_before_any_device_work(monkeypatch):
    from torchrecsys_amd import model as model_mod

    def no_device(*a, **kw):
        raise AssertionError("reached the device before validating the arguments")
    monkeypatch.setattr(model_mod, "_device", no_device)
    with pytest.raises(ValueError, match="mlp"):
        _model("mlp").fit_als()
    with pytest.raises(ValueError, match="metadata"):
        _model("linear", M=2).fit_als()
    with pytest.raises(ValueError, match="metadata"):
        _model("fm", M=1).fit_als()
    with pytest.raises(ValueError, match="n_factors"):
        _model("linear", n_factors=257).fit_als()
    monkeypatch.setattr(model_mod.tdist, "world_info", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="world"):
        _model("fm").fit_als()
    monkeypatch.undo()
    monkeypatch.setattr(model_mod, "_device", no_device)
    m = _model("fm")
    for kw, word in ((dict(iterations=0), "iterations"), (dict(iterations=1.5), "iterations"),
                     (dict(iterations=True), "iterations"), (dict(cg_steps=0), "cg_steps"),
                     (dict(cg_steps=257), "cg_steps"), (dict(regularization=0), "regularization"),
                     (dict(regularization=-0.1), "regularization"), (dict(regularization=float("nan")), "regularization"),
                     (dict(regularization=1e-60), "regularization"), (dict(alpha=-1.0), "alpha"),
                     (dict(alpha=float("inf")), "alpha"), (dict(alpha="10"), "alpha")):
        with pytest.raises(ValueError, match=word):
            m.fit_als(**kw)
    with pytest.raises(AssertionError, match="reached the device"):  # valid arguments do go on to the device
        m.fit_als(iterations=1, alpha=0.0)


# ------------------------------------------------------------------------------------------------ the reference
def _against_dense(got, Y, lists):
    for h, N in enumerate(lists):
        if len(N) == 0:
            assert not got[h].any()
        else:
            want = ref.dense_solution(Y, N, 0.1, 10.0)
            assert np.allclose(got[h], want, rtol=1e-8, atol=1e-8 * np.abs(want).max()), h


@pytest.mark.parametrize("D", [4, 8])
def test_the_rule_run_for_D_steps_solves_the_weighted_normal_equations(D):
    """cg_steps = D in float64: conjugate gradient on a D x D positive definite system ends at its solution, the row of
    Hu / Koren / Volinsky's closed form, whatever the start value.  (The finite termination is a property of exact
    arithmetic that float64 keeps to 1e-8 only while D is small: measured 8e-15 at D = 4, 2e-13 at D = 8, 3e-7 at D = 12.
    Beyond, the convergence is the geometric one of the next test.)"""
    lists = ref.random_lists(30, 40, 3, (0, 1, 39, 40))
    X, Y = ref.tables(30, 40, D, D)
    _against_dense(ref.half_sweep(X, Y, lists, 0.1, 10.0, D), Y, lists)


def test_warm_started_sweeps_converge_to_the_same_solution():
    """D = 24: two half-sweeps of D steps over the same frozen table, the second starting where the first stopped, are
    at the dense solution too (condition number 45: 48 steps shrink the error by far more than 1e8)."""
    lists = ref.random_lists(30, 40, 3, (0, 1, 39, 40))
    X, Y = ref.tables(30, 40, 24, 24)
    got = ref.half_sweep(X, Y, lists, 0.1, 10.0, 24)
    _against_dense(ref.half_sweep(got, Y, lists, 0.1, 10.0, 24), Y, lists)


def test_float32_restatements_stay_close_to_float64_and_differ_by_order():
    lists = ref.random_lists(30, 40, 3, (0, 1, 39, 40))
    X, Y = ref.tables(30, 40, 24, 5)
    w = ref.half_sweep(X, Y, lists, 0.1, 10.0, 3)
    a = ref.half_sweep(X, Y, lists, 0.1, 10.0, 3, dtype=np.float32, order="asc")
    d = ref.half_sweep(X, Y, lists, 0.1, 10.0, 3, dtype=np.float32, order="desc")
    assert a.dtype == np.float32 and np.abs(a - w).max() < 1e-4 and np.abs(d - w).max() < 1e-4
    assert not np.array_equal(a, d)  # the order of the factor sums is visible in fp32


def test_one_iteration_lowers_the_objective():
    lists = ref.random_lists(30, 40, 3, (0, 1, 39, 40))
    items = ref.transpose(lists, 40)
    assert sum(len(h) for h in items) == sum(len(h) for h in lists)
    X, Y = ref.tables(30, 40, 8, 2)
    l0 = ref.loss(X, Y, lists, 0.1, 10.0)
    X1 = ref.half_sweep(X, Y, lists, 0.1, 10.0, 3)
    l1 = ref.loss(X1, Y, lists, 0.1, 10.0)
    Y1 = ref.half_sweep(Y, X1, items, 0.1, 10.0, 3)
    l2 = ref.loss(X1, Y1, lists, 0.1, 10.0)
    assert l1 < 0.99 * l0 and l2 < 0.99 * l1, (l0, l1, l2)
    # the objective is what the solves minimise: at the dense solution of a row its gradient vanishes
    u = 5
    x = ref.dense_solution(Y, lists[u], 0.1, 10.0)
    G = Y.astype(np.float64).T @ Y.astype(np.float64)
    Yn = Y[lists[u].astype(np.int64)].astype(np.float64)
    grad = 2 * (G @ x + 0.1 * x + 10.0 * Yn.T @ (Yn @ x) - 11.0 * Yn.sum(0))
    assert np.abs(grad).max() < 1e-9


def test_the_exact_case_is_exact_in_every_order():
    """The bit-for-bit case of the GPU tests (tests/test_gpu_als.py exact_case): every intermediate is a multiple of
    2^-5 below 2^19, asserted by the reference; float32 in both orders then equals float64."""
    for D in (8, 24):
        X, Y, lists = ref.exact_case(D)
        w = ref.half_sweep(X, Y, lists, ref.EXACT_LAMBDA, ref.EXACT_ALPHA, 3, exact_bits=ref.EXACT_BITS)
        assert 0 < ref.half_sweep.bound < 2 ** 24
        for order in ("asc", "desc"):
            g = ref.half_sweep(X, Y, lists, ref.EXACT_LAMBDA, ref.EXACT_ALPHA, 3, dtype=np.float32, order=order)
            assert np.array_equal(g.astype(np.float64), w)
        assert sorted({float(v) for v in np.abs(w).ravel()}) == [0.0, 0.125, 0.25, 0.5]
