# -*- coding: utf-8 -*-
"""fold_in_users() / recommend_for_histories() without a GPU: trs_fold_in_users is declared, exported and bound; its
arguments and the public methods' arguments are validated on the host before any device work; the numpy restatement
(tests/foldin_ref.py) has the properties the GPU tests rely on."""
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pandas as pd
import pytest

import foldin_ref as ref
import mining_ref
from oracle import loader
from torchrecsys_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "trs_fold_in_users"
PROTO = _lib.PROTOTYPES[NAME]  # this module is about that entry point: without its binding nothing here applies


def _err():
    return _lib.load().trs_last_error().decode()


def test_symbol_declared_exported_and_bound():
    lib = _lib.load()
    assert lib.trs_abi_version() == _lib.ABI_VERSION == 6  # added without touching a signature: no bump
    header = open(os.path.join(ROOT, "include", "trs.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint %s\s*\(" % NAME, header)
    assert NAME in _lib.PROTOTYPES and hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert len(PROTO[1]) == 19
    decl = header[header.index("int " + NAME):]
    assert decl[:decl.index(")")].count(",") == 18
    assert "foldin.hip" in open(os.path.join(ROOT, "torchrecsys_amd", "csrc", "Makefile")).read()
    assert lib.trs_tuning_set(b"FOLDIN_DEPTH", 1, 0) == 0 and lib.trs_tuning_set(b"FOLDIN_DEPTH", 0, 1) == 0


def test_entry_point_rejects_bad_arguments_before_any_launch():
    lib = _lib.load()
    P = 0x1000  # never dereferenced
    fb = lib.trs_item_fold_bytes(300, 24)
    hist = _lib.TrsCsr()
    hist.off, hist.items, hist.n_rows = P, P, 5
    empty = _lib.TrsCsr()
    empty.off, empty.items, empty.n_rows = P, P, 0
    inf, nan = float("inf"), float("nan")

    def call(net=0, fold=P, fold_bytes=fb, n_items=300, D=24, h=hist, loss=0, epochs=4, lr=0.05, l2=0.0, seed=1,
             shuffle=1, reject=1, tries=8, U=P, b=P, ls=None, err=None):
        return lib.trs_fold_in_users(net, fold, fold_bytes, n_items, D, ctypes.byref(h) if h is not None else None, loss,
                                     epochs, lr, l2, seed, shuffle, reject, tries, U, b, ls, err, None)
    for kw, word in ((dict(net=2), "net"), (dict(net=-1), "net"), (dict(fold=None), "fold buffer"),
                     (dict(fold_bytes=fb - 4), "fold buffer too small"), (dict(D=0), "D=0"),
                     (dict(D=_lib.RETRIEVE_DMAX + 1, fold_bytes=1 << 30), "D="), (dict(n_items=1), "n_items"),
                     (dict(n_items=0), "n_items"), (dict(epochs=0), "epochs"), (dict(epochs=1025), "epochs"),
                     (dict(lr=0.0), "lr"), (dict(lr=-1.0), "lr"), (dict(lr=inf), "lr"), (dict(lr=nan), "lr"),
                     (dict(l2=-0.5), "l2"), (dict(l2=inf), "l2"), (dict(l2=nan), "l2"), (dict(loss=2), "loss"),
                     (dict(loss=3), "loss"), (dict(loss=-1), "loss"), (dict(tries=-1), "max_tries"),
                     (dict(tries=65), "max_tries"), (dict(reject=1, tries=0), "reject_seen"), (dict(h=None), "NULL"),
                     (dict(U=None), "NULL"), (dict(b=None), "NULL")):
        assert call(**kw) == -1, kw
        assert _err().startswith(NAME + ":") and word in _err(), (kw, _err())
    for arr in ("off", "items"):
        bad = _lib.TrsCsr()
        bad.off, bad.items, bad.n_rows = P, P, 5
        setattr(bad, arr, None)
        assert call(h=bad) == -1 and "NULL" in _err()
    # nothing to do, nothing launched: no new user (outputs may then be NULL); bad arguments are still bad
    assert call(h=empty) == 0
    assert call(h=empty, U=None, b=None) == 0
    assert call(h=empty, reject=0, tries=0) == 0
    assert call(h=empty, epochs=0) == -1 and "epochs" in _err()
    with _lib.tuning(FOLDIN_DEPTH=3):
        assert call() == -1 and "FOLDIN_DEPTH" in _err()


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
    for fn in ("fold_in_users", "recommend_for_histories"):
        f = getattr(m, fn)
        with pytest.raises(ValueError, match="mlp"):
            getattr(_model("mlp"), fn)([[0]])
        with pytest.raises(ValueError, match="n_factors"):
            getattr(_model("linear", n_factors=257), fn)([[0]])
        for bad in (dict(epochs=0), dict(epochs=1025), dict(epochs=2.5), dict(lr=0), dict(lr=-1.0),
                    dict(lr=float("inf")), dict(lr=float("nan")), dict(lr="fast"), dict(l2=-1e-3),
                    dict(l2=float("nan")), dict(loss="warp"), dict(loss=None), dict(max_tries=-1), dict(max_tries=65),
                    dict(max_tries=1.5), dict(reject_seen=True, max_tries=0), dict(seed=1.5)):
            with pytest.raises(ValueError, match=list(bad)[0] if "reject_seen" not in bad else "reject_seen"):
                f([[0, 1]], **bad)
        with pytest.raises(IndexError, match="1000"):
            f([[0, 1], [2, 1000]])
        with pytest.raises(IndexError, match="-1"):
            f([[-1]])
        with pytest.raises(AssertionError, match="reached the device"):  # valid arguments get as far as the device
            f([[0, 1], [], [5, 5, 3]])
        with pytest.raises(AssertionError, match="reached the device"):
            f([np.array([0, 1]), (2,)], reject_seen=False, max_tries=0, loss="bpr", l2=0.25, seed=-3, shuffle=False)
    # empty calls need no device
    U, b = m.fold_in_users([])
    assert U.shape == (0, 8) and b.shape == (0,) and str(U.dtype) == str(b.dtype) == "torch.float32"
    U, b, ls = m.fold_in_users([], epochs=3, return_loss=True)
    assert ls.shape == (3, 0) and str(ls.dtype) == "torch.float32"
    ids, sc = m.recommend_for_histories([], top_k=4, return_scores=True)
    assert ids.shape == (0, 4) and sc.shape == (0, 4) and str(ids.dtype) == "torch.int64"
    assert m.recommend_for_histories([[1], [2]], top_k=0).shape == (2, 0)
    with pytest.raises(ValueError, match="top_k"):
        m.recommend_for_histories([[0]], top_k=_lib.RETRIEVE_KMAX + 1)
    with pytest.raises(ValueError, match="unknown fold-in options"):
        m.recommend_for_histories([[0]], epoch=3)


def test_history_csr_is_sorted_distinct_and_longest_first():
    m = _model("linear")
    hs = [[5, 3, 5, 9], [], [7], [2, 1, 0, 1, 29, 4], [4, 4]]
    off, items, rank = m._history_csr(hs)
    assert off.dtype == np.int64 and items.dtype == np.int32 and off[0] == 0 and off[-1] == items.size
    lens = np.diff(off)
    assert np.all(lens[:-1] >= lens[1:])  # longest first
    for r, h in enumerate(ref.clean(hs)):
        k = rank[r]
        assert np.array_equal(items[off[k]:off[k + 1]], h)
    assert sorted(rank.tolist()) == list(range(5))
    off, items, rank = m._history_csr([[], []])
    assert off.tolist() == [0, 0, 0] and items.size == 0


# ------------------------------------------------------------------------------------------------ the reference
N_ITEMS = 50


def _hists():
    rs = np.random.RandomState(4)
    lens = [0, 1, 2, 7, 33, 48, 49, 50]
    return [np.sort(rs.choice(N_ITEMS, size=n, replace=False)).astype(np.int64) for n in lens]


def test_schedule_is_a_permutation_and_rejects_seen_items():
    for shuffle in (False, True):
        for h in _hists():
            sched = ref.schedule(h, N_ITEMS, 3, 9, shuffle, True, 8)
            orders = []
            for e, (r, p, n) in enumerate(sched):
                assert sorted(r.tolist()) == list(range(h.size))  # every visit once per epoch
                assert np.array_equal(p, h[r]) and np.all(n != p) and np.all((n >= 0) & (n < N_ITEMS))
                if not shuffle:
                    assert np.array_equal(r, np.arange(h.size))
                orders.append(tuple(r.tolist()))
            if shuffle and h.size >= 7:
                assert len(set(orders)) == 3  # another order every epoch
    # with reject_seen the negatives are outside the history.  The tries are bounded, so "never" can only be asked where
    # a run of max_tries seen candidates is out of reach: at most 33 of the 49 other items seen and 64 tries, a miss has
    # probability (32/49)^64 < 2e-12 per draw.  (n_h >= n_items - 1 leaves no unseen item at all: below.)
    for h in _hists():
        if h.size <= 33:
            for (r, p, n) in ref.schedule(h, N_ITEMS, 3, 9, True, True, 64):
                assert not np.isin(n, h).any()
    # a history of all items (or all but one) cannot be avoided: the last candidate is kept, still never the positive
    full = np.arange(N_ITEMS, dtype=np.int64)
    for (r, p, n) in ref.schedule(full, N_ITEMS, 2, 9, True, True, 8):
        assert np.isin(n, full).all() and np.all(n != p)
    # without rejection every max_tries gives the plain draw
    h = _hists()[4]
    plain = ref.negatives_by_position(h, N_ITEMS, 9, 2, False, 0)
    opt = loader.device_negatives_opt(np.zeros(h.size, dtype=np.int64), h, N_ITEMS, 9, 2 << 32, seen=None, max_tries=5)
    assert np.array_equal(plain, opt)


def test_the_two_sampler_restatements_agree_on_the_fold_in_schedule():
    for h in _hists()[1:]:
        for e in (0, 3):
            a = ref.negatives_by_position(h, N_ITEMS, 21, e, True, 8, vectorised=True)
            b = ref.negatives_by_position(h, N_ITEMS, 21, e, True, 8, vectorised=False)
            assert np.array_equal(a, b)
    x, y, _, _ = loader.philox4x32_10(np.array([2], dtype=np.uint64), (21 + mining_ref.KEY_STEP) & mining_ref.MASK64)
    assert ref.epoch_key(21, 2) == ((int(y[0]) << 32) | int(x[0])) | 1 and ref.epoch_key(21, 2) & 1


def test_a_history_folds_in_the_same_alone_or_among_others():
    rs = np.random.RandomState(2)
    S, c = rs.randint(-3, 4, (N_ITEMS, 16)).astype(np.float64), rs.randint(-3, 4, N_ITEMS).astype(np.float64)
    hs = _hists()
    for net, loss in (("linear", "hinge"), ("fm", "bpr")):
        kw = dict(seed=5, shuffle=True, reject_seen=True, max_tries=8)
        both = ref.fold_in(S, c, hs, net, loss, 3, 2.0 ** -6, 0.0, **kw)
        other = ref.fold_in(S, c, hs[::-1] + hs[3:5], net, loss, 3, 2.0 ** -6, 0.0, **kw)
        for i, h in enumerate(hs):
            one = ref.fold_in_one(S, c, h, net, loss, 3, 2.0 ** -6, 0.0, **kw)
            assert np.array_equal(one["u"], both["U"][i]) and one["b"] == both["b"][i]
            assert np.array_equal(one["loss"], both["loss"][:, i])
            j = len(hs) - 1 - i
            assert np.array_equal(other["U"][j], both["U"][i]) and np.array_equal(other["negs"][j], both["negs"][i])
        assert np.array_equal(other["U"][len(hs)], both["U"][3])
        assert not both["U"][0].any() and both["b"][0] == 0 and not both["loss"][:, 0].any()  # the empty history
    lin = ref.fold_in(S, c, hs, "linear", "hinge", 3, 2.0 ** -6, 0.0, seed=5, require_exact=True)
    assert not lin["b"].any()  # Linear, l2 = 0: g_p + g_n = 0 keeps the bias at exactly 0
    assert lin["bound"] < 2.0 ** 24 and 0 < lin["active"] < lin["visits"]
    # fp32 restatements in two summation orders stay close to float64 (the GPU test's tolerance is measured this way)
    S3, c3 = (0.3 * rs.randn(N_ITEMS, 24)).astype(np.float32), (0.3 * rs.randn(N_ITEMS)).astype(np.float32)
    a = ref.fold_in(S3.astype(np.float64), c3.astype(np.float64), hs, "fm", "bpr", 3, 0.05, 0.125, seed=1)
    for order in ("asc", "desc"):
        g = ref.fold_in(S3, c3, hs, "fm", "bpr", 3, 0.05, 0.125, seed=1, dtype=np.float32, order=order)
        assert g["U"].dtype == np.float32 and np.abs(g["U"] - a["U"]).max() < 1e-5 and np.abs(g["loss"] - a["loss"]).max() < 1e-5


def test_planted_case_learns_the_planted_direction():
    for D in (8, 64):
        S, c, hist = ref.planted(D, seed=D)
        for net in ("linear", "fm"):
            o = ref.fold_in_one(S, c, hist, net, "hinge", 8, 0.05, 0.0, seed=0)
            assert o["loss"][-1] < o["loss"][0], (net, D, o["loss"])
            ids, _ = ref.rank(o["u"][None, :], np.array([o["b"]]), S, c, [hist], 10)
            assert np.all(ids[0] < 48) and not np.isin(ids[0], hist).any(), (net, D, ids)
