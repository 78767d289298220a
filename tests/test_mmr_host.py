# -*- coding: utf-8 -*-
"""recommend_diverse() / evaluate_diversity() without a GPU: the two C entry points are declared, exported and bound;
their arguments and the public methods' arguments are validated on the host before any device work; the numpy oracle
(tests/mmr_ref.py) has the properties the GPU tests rely on."""
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pandas as pd
import pytest

import mmr_ref as ref
from torchrecsys_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("trs_mmr_rerank", "trs_list_ild")


def _err():
    return _lib.load().trs_last_error().decode()


def test_new_symbols_declared_exported_and_bound():
    lib = _lib.load()
    assert lib.trs_abi_version() == _lib.ABI_VERSION == 6
    header = open(os.path.join(ROOT, "include", "trs.h")).read()
    assert "diversified re-ranking" in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(raw, name), name
    assert len(_lib.PROTOTYPES["trs_mmr_rerank"][1]) == 15
    assert len(_lib.PROTOTYPES["trs_list_ild"][1]) == 9
    from torchrecsys_amd import ops
    assert callable(ops.mmr_rerank) and callable(ops.list_ild)


def test_entry_points_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    P = 0x1000  # never dereferenced
    fb = lib.trs_item_fold_bytes(300, 24)
    assert fb == 384 * 33 * 4

    def mmr(fold=P, fold_bytes=fb, n_items=300, D=24, pids=P, psc=P, n_q=5, N=32, k=10, lam=0.5, ids=P, sc=P, pos=P,
            err=P):
        return lib.trs_mmr_rerank(fold, fold_bytes, n_items, D, pids, psc, n_q, N, k, lam, ids, sc, pos, err, None)
    K1 = _lib.RETRIEVE_KMAX + 1
    assert mmr(N=0) == -1 and "N=0" in _err()
    assert mmr(N=K1, k=10) == -1 and f"N={K1}" in _err()
    assert mmr(k=0) == -1 and "k=0" in _err()
    assert mmr(N=_lib.RETRIEVE_KMAX, k=K1) == -1 and f"k={K1}" in _err()
    assert mmr(N=8, k=9) == -1 and "k=9 > N=8" in _err()
    for lam in (-0.001, 1.001, float("nan"), float("inf"), -float("inf")):
        assert mmr(lam=lam) == -1 and "lambda" in _err(), lam
    assert mmr(D=0) == -1 and "D=0" in _err()
    assert mmr(D=_lib.RETRIEVE_DMAX + 1, fold_bytes=1 << 30) == -1 and "D=" in _err()
    assert mmr(n_items=0) == -1 and "n_items" in _err()
    assert mmr(fold_bytes=fb - 4) == -1 and "fold_bytes" in _err()
    assert mmr(fold_bytes=fb + 4) == -1 and "fold_bytes" in _err()
    assert mmr(n_items=385) == -1 and "fold_bytes" in _err()  # another padded row count: another buffer
    assert mmr(n_q=-1) == -1 and "n_q" in _err()
    assert mmr(fold=None) == -1 and "NULL" in _err()
    for name in ("pids", "psc", "ids", "sc"):
        assert mmr(**{name: None}) == -1 and "NULL" in _err(), name
    assert _err().startswith("trs_mmr_rerank")
    assert mmr(n_q=0, fold=None, pids=None, psc=None, ids=None, sc=None, pos=None, err=None) == 0  # nothing launched
    for bad in (dict(N=0), dict(k=0), dict(lam=2.0), dict(fold_bytes=8)):  # ... but still validated
        assert mmr(n_q=0, **bad) == -1

    def ild(fold=P, fold_bytes=fb, n_items=300, D=24, ids=P, n_q=5, k=10, out=P):
        return lib.trs_list_ild(fold, fold_bytes, n_items, D, ids, n_q, k, out, None)
    assert ild(k=0) == -1 and "k=0" in _err()
    assert ild(k=K1) == -1 and f"k={K1}" in _err()
    assert ild(D=_lib.RETRIEVE_DMAX + 1, fold_bytes=1 << 30) == -1 and "D=" in _err()
    assert ild(fold_bytes=fb - 4) == -1 and "fold_bytes" in _err()
    assert ild(n_q=-1) == -1 and "n_q" in _err()
    assert ild(fold=None) == -1 and "NULL" in _err()
    assert ild(ids=None) == -1 and "NULL" in _err()
    assert ild(out=None) == -1 and "NULL" in _err()
    assert _err().startswith("trs_list_ild")
    assert ild(n_q=0, fold=None, ids=None, out=None) == 0


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
    m = _model("fm")
    calls = (lambda **kw: m.recommend_diverse([0], **kw), lambda **kw: m.evaluate_diversity(**kw))
    for call in calls:
        for bad in ("euclid", "", None, "Cosine", 1):
            with pytest.raises(ValueError, match="metric"):
                call(metric=bad)
        for bad in (-0.1, 1.5, True, False, None, "0.3", float("nan")):
            with pytest.raises(ValueError, match="diversity"):
                call(diversity=bad)
        for bad in (_lib.RETRIEVE_KMAX + 1, 1000):
            with pytest.raises(ValueError, match="TRS_RETRIEVE_KMAX"):
                call(pool=bad)
        for bad in (0, -3, 2.5, True):
            with pytest.raises(ValueError, match="pool"):
                call(pool=bad)
    with pytest.raises(ValueError, match="top_k=10 > pool=5"):
        m.recommend_diverse([0], top_k=10, pool=5)
    with pytest.raises(ValueError, match="> pool=5"):
        m.evaluate_diversity(k=10, pool=5)
    for fn, kw in (("recommend_diverse", {"user_ids": [0]}), ("evaluate_diversity", {})):
        with pytest.raises(ValueError, match="mlp") as e:
            getattr(_model("mlp"), fn)(**kw)
        assert "concatenated" in str(e.value)
        with pytest.raises(ValueError, match="n_factors"):
            getattr(_model("linear", n_factors=257), fn)(**kw)
    # empty queries and top_k <= 0 need no device either; unknown ids are found on the host
    ids, sc = m.recommend_diverse([], top_k=4, return_scores=True)
    assert ids.shape == (0, 4) and sc.shape == (0, 4) and str(ids.dtype) == "torch.int64" and str(sc.dtype) == "torch.float32"
    assert m.recommend_diverse([1, 2], top_k=0).shape == (2, 0)
    with pytest.raises(IndexError, match="1000"):
        m.recommend_diverse([0, 1000])
    with pytest.raises(AssertionError, match="reached the device"):  # valid arguments get as far as the device
        m.recommend_diverse([0, 1], top_k=3, metric="dot", diversity=1)
    with pytest.raises(AssertionError, match="reached the device"):
        m.evaluate_diversity(k=3, diversity=0.5)


def test_default_pool_and_clamping():
    from torchrecsys_amd.evaluate import diversity as dv
    chk = lambda top_k, pool, n_items: dv.check("x", "fm", 8, n_items, top_k, 0.3, pool, "cosine", 128, 256)
    assert chk(10, None, 10_000) == (10, 40)
    assert chk(5, None, 10_000) == (5, 32)
    assert chk(50, None, 10_000) == (50, 128)
    assert chk(10, None, 20) == (10, 20)
    assert chk(30, None, 20) == (20, 20)  # k = min(top_k, n_items), the pool is the whole catalogue
    assert chk(10, 128, 40) == (10, 40)
    assert chk(0, None, 40) == (0, 32)
    with pytest.raises(ValueError, match="pool"):
        chk(129, None, 10_000)  # the default pool stops at 128


def test_evaluate_diversity_refuses_data_parallel_runs(monkeypatch):
    from torchrecsys_amd import model as model_mod
    monkeypatch.setattr(model_mod, "_device", lambda: (_ for _ in ()).throw(AssertionError("reached the device")))
    monkeypatch.setattr(model_mod.tdist, "world_info", lambda: (0, 2))
    with pytest.raises(ValueError, match="coverage"):
        _model("fm").evaluate_diversity(k=3)


# ------------------------------------------------------------------------------------------------ the oracle itself
def _pool(rs, n, N, n_items, short=0):
    ids = np.stack([rs.permutation(n_items)[:N] for _ in range(n)]).astype(np.int64)
    sc = -np.sort(-rs.rand(n, N).astype(np.float32), axis=1)
    for q in range(min(short, n)):
        ids[q, N - 1 - q:] = -1
        sc[q, N - 1 - q:] = -np.inf
    return ids, sc


def test_oracle_lambda_zero_keeps_the_pool_order():
    rs = np.random.RandomState(0)
    ids, sc = _pool(rs, 6, 20, 50, short=3)
    sc[4, 3:9] = sc[4, 3]  # ties in relevance: still the pool order
    X = rs.randn(50, 50)
    for k in (1, 7, 20):
        got, gsc, pos = ref.rerank(ids, sc, X, k, 0.0)
        assert np.array_equal(got, ids[:, :k]) and np.array_equal(gsc, sc[:, :k])
        want_pos = np.where(ids[:, :k] >= 0, np.arange(k)[None, :], -1)
        assert np.array_equal(pos, want_pos)


def test_oracle_identical_rows_at_lambda_one_give_the_pool_order():
    rs = np.random.RandomState(1)
    ids, sc = _pool(rs, 4, 16, 30)
    X = np.ones((30, 30))  # every row the same unit vector: every penalty equal, ties go to the lowest position
    got, _, pos = ref.rerank(ids, sc, X, 16, 1.0)
    assert np.array_equal(got, ids) and np.array_equal(pos, np.tile(np.arange(16), (4, 1)))


def test_oracle_never_selects_the_padding_suffix_or_an_id_outside_the_catalogue():
    rs = np.random.RandomState(2)
    ids, sc = _pool(rs, 8, 12, 40, short=8)
    ids[7, 2] = 40  # an id >= n_items in the middle of a pool: invalid, skipped
    X = rs.randn(40, 40)
    X = X + X.T
    for lam in (0.0, 0.5, 1.0):
        got, gsc, pos = ref.rerank(ids, sc, X, 12, lam)
        for q in range(8):
            valid = (ids[q] >= 0) & (ids[q] < 40)
            nv = int(valid.sum())
            assert np.all(got[q, nv:] == -1) and np.all(np.isneginf(gsc[q, nv:])) and np.all(pos[q, nv:] == -1)
            assert sorted(pos[q, :nv].tolist()) == np.nonzero(valid)[0].tolist()
            assert np.array_equal(got[q, :nv], ids[q][pos[q, :nv]]) and np.array_equal(gsc[q, :nv], sc[q][pos[q, :nv]])
        assert 40 not in got
    none = np.full((2, 5), -1, np.int64)
    got, gsc, pos = ref.rerank(none, np.full((2, 5), -np.inf, np.float32), X, 3, 0.5)
    assert np.all(got == -1) and np.all(np.isneginf(gsc)) and np.all(pos == -1)


def test_oracle_relevance_is_scaled_and_non_increasing():
    v = np.array([0.9, 0.9000001, 0.5, 0.7, 0.1, -np.inf], np.float32)
    valid = np.array([1, 1, 1, 1, 1, 0], bool)
    rel = ref.relevance(v, valid)
    assert rel.dtype == np.float32 and rel[5] == 0 and np.all(np.diff(rel[:5]) <= 0)
    assert rel[0] < 1 and rel[1] == rel[0] and rel[3] == rel[2] and rel[4] == 0  # clamped to the entry before
    assert not ref.relevance(np.full(4, 0.3, np.float32), np.ones(4, bool)).any()  # v_max == v_min
    assert not ref.relevance(v, np.zeros(6, bool)).any()


def test_oracle_picks_the_other_cluster_first_and_breaks_ties_by_position():
    # items 0, 1 identical, item 2 orthogonal; pool order 0, 1, 2 with falling scores
    E = np.array([[1, 0], [1, 0], [0, 1]], np.float64)
    X = E @ E.T
    ids = np.array([[0, 1, 2]])
    sc = np.array([[0.9, 0.8, 0.1]], np.float32)
    assert ref.rerank(ids, sc, X, 3, 0.0)[0].tolist() == [[0, 1, 2]]
    assert ref.rerank(ids, sc, X, 3, 1.0)[0].tolist() == [[0, 2, 1]]
    # a * rel_1 - b * 1 against a * rel_2 - b * 0 with rel = (1, 0.875, 0): item 2 overtakes item 1 from lambda = 7/15 on
    assert ref.rerank(ids, sc, X, 3, 0.45)[0].tolist() == [[0, 1, 2]]
    assert ref.rerank(ids, sc, X, 3, 0.5)[0].tolist() == [[0, 2, 1]]
    # NaN ranks below every number; among equals the lowest position
    m = np.array([np.nan, 0.5, 0.5, -0.0, 0.0], np.float32)
    assert ref._pick(m, np.zeros(5, bool)) == 1
    assert ref._pick(m, np.array([0, 1, 1, 0, 0], bool)) == 3
    assert ref._pick(m, np.array([0, 1, 1, 1, 1], bool)) == 0


def test_oracle_metrics():
    rows = np.array([[1, 0], [1, 0], [0, 1], [0.6, 0.8]])
    got = ref.ild(np.array([[0, 1, -1], [0, 2, -1], [0, 2, 3], [3, -1, -1], [-1, -1, -1]]), rows)
    np.testing.assert_allclose(got, [0.0, 1.0, (1.0 + 0.4 + 0.2) / 3.0, 0.0, 0.0], rtol=0, atol=1e-15)
    lists = np.array([[0, 1, -1], [1, 2, 3], [-1, -1, -1]])
    assert ref.coverage(lists, 8) == 0.5
    c = np.array([0, 1, 3, 7, 0, 0, 0, 0])
    want = np.mean([np.mean([3.0, 2.0]), np.mean([2.0, 1.0, 0.0]), 0.0])
    np.testing.assert_allclose(ref.novelty(lists, c, 7), want, rtol=0, atol=1e-15)
    from torchrecsys_amd.evaluate import diversity as dv
    assert dv.coverage(lists, 8) == 0.5
    np.testing.assert_allclose(dv.novelty_per_user(lists, c, 7).mean(), want, rtol=0, atol=1e-15)
    assert ref.eps(0.5, 24) == 2 * (0.5 * 34 + 3) * 2.0 ** -24 and ref.ild_tol(100) == 130 * 2.0 ** -24 + 1e-12


def test_oracle_check_greedy_accepts_the_oracle_and_rejects_a_wrong_pick():
    rs = np.random.RandomState(5)
    D = 24
    rows = rs.randn(60, ref.dp(D))
    rows[:, D:] = 0
    rows /= np.sqrt((rows * rows).sum(1))[:, None]
    rows = rows.astype(np.float32)
    ids, sc = _pool(rs, 5, 32, 60, short=2)
    X = rows.astype(np.float64) @ rows.astype(np.float64).T
    for lam in (0.3, 1.0):
        got = ref.rerank(ids, sc, X, 10, lam)
        assert ref.check_greedy(ids, sc, rows, 10, lam, D, *got) <= ref.eps(lam, D)
        bad = [g.copy() for g in got]
        p = [x for x in range(32) if x not in got[2][0][:3].tolist()][-1]  # swap pick 2 of list 0 for a late entry
        bad[2][0, 2], bad[0][0, 2], bad[1][0, 2] = p, ids[0, p], sc[0, p]
        with pytest.raises(AssertionError):
            ref.check_greedy(ids, sc, rows, 10, lam, D, *bad)


def test_shipped_rerank_kernels_use_no_scratch(tmp_path):
    """Register guard on the shipped code objects (no GPU, no recompilation; the reader is tests/test_abi.py's): the five
    row widths of both kernels are there, none uses scratch, and the widest instances stay at three waves per SIMD."""
    from test_abi import _shipped_kernel_registers
    found = _shipped_kernel_registers(tmp_path)
    for kernel in ("mmr_rerank_kernel", "list_ild_kernel"):
        inst = {n: v for n, v in found.items() if kernel in n}
        widths = sorted(int(re.search(r"kernelILi(\d+)ELi[24]E", n).group(1)) for n in inst)
        assert widths == [16, 32, 64, 128, 256], sorted(inst)
        for n, (vgpr, scratch) in inst.items():
            assert scratch == 0 and vgpr <= 168, (n, vgpr, scratch)
