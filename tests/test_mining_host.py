# -*- coding: utf-8 -*-
"""Score-aware hard-negative mining without a GPU: the neg_sampling keys are validated on the host, the C entry point
trs_batch_prepare_mined refuses bad arguments before any launch, the Philox keys of a triple never collide, the numpy
restatement (tests/mining_ref.py) with one candidate is the unmined loader, and evaluate() never mines."""
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pandas as pd
import pytest

import mining_ref
from oracle import loader
from torchrecsys_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000  # a non-NULL pointer that validation never dereferences


def _df(seed=0):
    rs = np.random.RandomState(seed)
    return pd.DataFrame({"user_id": np.concatenate([np.arange(40), rs.randint(0, 40, 360)]),
                         "item_id": np.concatenate([np.arange(30), rs.randint(0, 30, 370)])})


def _model(neg_sampling, net_type="fm", rng="device", dynamic=True):
    from torchrecsys_amd.model import TorchRecSys
    with contextlib.redirect_stdout(io.StringIO()):
        return TorchRecSys(_df(), "user_id", "item_id", n_factors=8, net_type=net_type, rng=rng,
                           dynamic_neg_sampling=dynamic, neg_sampling=neg_sampling)


# ------------------------------------------------------------------------------------------------ 1. constructor
def test_mining_keys_construct_and_refusals_name_the_key():
    for net_type in ("linear", "fm"):
        m = _model({"mine": "hardest", "candidates": 8}, net_type)
        assert m.neg_sampling["mine"] == "hardest"
    _model({"mine": "hardest"})  # defaults: candidates 8, top 1
    _model({"mine": "hardest", "candidates": 64, "top": 64, "k": 2, "reject_seen": True, "popularity": True})
    _model({"mine": "hardest", "candidates": np.int64(4), "top": 2})
    with pytest.raises(ValueError, match="mine"):
        _model({"mine": "warp"})
    with pytest.raises(ValueError, match="mine"):
        _model({"mine": None, "k": 2})
    with pytest.raises(ValueError, match=r"(?s)mine.*mlp.*out of scope"):
        _model({"mine": "hardest"}, net_type="mlp")
    with pytest.raises(ValueError, match="candidates"):
        _model({"candidates": 8})
    with pytest.raises(ValueError, match="top"):
        _model({"top": 2})
    for bad in (0, 65, -1, 2.0, "8", True, None):
        with pytest.raises(ValueError, match="candidates"):
            _model({"mine": "hardest", "candidates": bad})
    for bad in (0, 5, -1, 1.0, "1", True, None):
        with pytest.raises(ValueError, match="top"):
            _model({"mine": "hardest", "candidates": 4, "top": bad})
    with pytest.raises(ValueError, match="top"):
        _model({"mine": "hardest", "top": 9})  # candidates defaults to 8
    # already refused, and still: the reference RNG, static negatives, the in-batch softmax
    with pytest.raises(ValueError, match="neg_sampling"):
        _model({"mine": "hardest"}, rng="reference")
    with pytest.raises(ValueError, match="neg_sampling"):
        _model({"mine": "hardest"}, dynamic=False)
    import torch
    m = _model({"mine": "hardest"})
    with pytest.raises(ValueError, match="neg_sampling"):
        m.fit(torch.optim.SGD(m.parameters(), lr=0.1), epochs=1, loss="softmax")


# ------------------------------------------------------------------------------------------------ 2. C entry point
def _err():
    return _lib.load().trs_last_error().decode()


def _tables(D=8, M=0):
    T = _lib.TrsTables()
    T.user = T.item = T.user_lin = T.item_lin = P
    T.n_users, T.n_items, T.D, T.M = 10, 20, D, M
    for m in range(M):
        T.meta[m], T.meta_lin[m], T.n_meta[m] = P, P, 3
    return T


def _mined(T="default", net=_lib.TRS_NET_FM, K=8, top=1, neg_static=None, M=0, item_meta=None, pm=None, nm=None,
           n_items=20):
    T = _tables(M=M) if T == "default" else T
    return _lib.load().trs_batch_prepare_mined(P, P, neg_static, 100, 1, 0, 10, n_items, 1, 0, item_meta, M, P, P, P, pm,
                                               nm, None, net, ctypes.byref(T) if T is not None else None, K, top, None,
                                               None)


def test_entry_point_is_declared_exported_bound_and_validates_on_the_host():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trs.h")).read(), flags=re.S)
    assert re.search(r"\btrs_batch_prepare_mined\s*\(", hdr)
    assert "trs_batch_prepare_mined" in _lib.PROTOTYPES and hasattr(ctypes.CDLL(_lib.LIB_PATH), "trs_batch_prepare_mined")
    assert _mined(T=None) == -1 and "tables is NULL" in _err()
    for net in (2, -1, 7):
        assert _mined(net=net) == -1 and "net must be" in _err()
    for K in (0, 65, -3):
        assert _mined(K=K) == -1 and "candidates" in _err()
    for K, top in ((8, 0), (8, 9), (1, 2), (64, 65)):
        assert _mined(K=K, top=top) == -1 and "top" in _err()
    assert _mined(neg_static=P) == -1 and "static negatives" in _err()
    assert _mined(M=2) == -1 and "item_meta" in _err()
    assert _mined(M=2, item_meta=P, pm=P) == -1 and "metadata outputs" in _err()
    assert _mined(M=1) == -1 and "item_meta" in _err()
    assert _mined(T=_tables(M=1), M=0) == -1 and "does not match" in _err()
    for D in (0, -4, 1028, 301):
        assert _mined(T=_tables(D=D)) == -1 and "n_factors" in _err(), D
    T0 = _tables()
    T0.item_lin = None
    assert _mined(T=T0) == -1 and "NULL" in _err()
    assert _mined(n_items=21) == -1 and "n_items" in _err()


# ------------------------------------------------------------------------------------------------ 3. restatement
def test_philox_keys_of_one_triple_are_distinct():
    offs = mining_ref.key_offsets(65, 64)
    assert len(offs) == 66 * 65 and len(set(offs)) == len(offs)


@pytest.mark.parametrize("opts", [None, {"popularity": True}, {"seen": True}, {"popularity": True, "seen": True, "k": 2}])
def test_one_candidate_is_the_unmined_loader(opts):
    rs = np.random.RandomState(5)
    NU, NI, N, D, B = 30, 40, 300, 8, 128
    su, si = rs.randint(0, NU, N), rs.randint(0, NI, N)
    item_meta = rs.randint(0, 4, (NI, 2))
    params = {"user.weight": rs.normal(size=(NU, D)), "item.weight": rs.normal(size=(NI, D)),
              "linear_user.weight": rs.normal(size=(NU, 1)), "linear_item.weight": rs.normal(size=(NI, 1))}
    for m in range(2):
        params[f"metadata.{m}.weight"] = rs.normal(size=(4, D))
        params[f"linear_metadata.{m}.weight"] = rs.normal(size=(4, 1))
    sampler = None
    if opts:
        sampler = {"max_tries": 6, "k": opts.get("k", 1), "popularity": opts.get("popularity", False)}
        if opts.get("seen"):
            sampler["seen"] = {int(u): set(si[su == u].tolist()) for u in np.unique(su)}
    k = (sampler or {}).get("k", 1)
    t0 = N * k - B - 3
    want = loader.device_batch(su, si, None, 0xABCDEF12345, t0, B, NI, 77, t0, item_meta, sampler)
    got = mining_ref.mined_batch(su, si, 0xABCDEF12345, t0, B, NI, 77, t0, "fm", params, 1, 1, sampler, item_meta)
    for key in ("user", "pos", "neg", "pos_meta", "neg_meta"):
        assert np.array_equal(got[key], want[key]), key
    assert not got["chosen"].any()
    # more candidates: candidate 0 stays the unmined negative, the choice is the float64 arg-max, first index on ties
    got = mining_ref.mined_batch(su, si, 0xABCDEF12345, t0, B, NI, 77, t0, "fm", params, 5, 1, sampler, item_meta)
    assert np.array_equal(got["cand"][:, 0], want["neg"])
    assert np.array_equal(got["chosen"], got["z"].argmax(axis=1)) and (got["neg"] != got["pos"]).all()
    got3 = mining_ref.mined_batch(su, si, 0xABCDEF12345, t0, B, NI, 77, t0, "fm", params, 5, 3, sampler, item_meta)
    rank = (got3["z"] > np.take_along_axis(got3["z"], got3["chosen"][:, None], 1)).sum(1)
    assert rank.max() <= 2 and len(set(rank.tolist())) == 3  # uniform over the three best


def test_order_is_score_descending_index_ascending_nan_first():
    z = np.array([[1.0, 3.0, 3.0, -0.0, 0.0, np.nan, np.inf, np.nan]])
    assert mining_ref.order_desc(z)[0].tolist() == [5, 7, 6, 1, 2, 0, 3, 4]


# ------------------------------------------------------------------------------------------------ 4. evaluate()
def test_eval_sampler_never_mines_and_plain_samplers_are_unchanged():
    from torchrecsys_amd import ops
    m = _model({"mine": "hardest", "candidates": 16, "top": 2, "max_tries": 5})
    m._dev_cache["sampler"] = ops.Sampler(k=1, max_tries=5, mine="hardest", candidates=16, top=2)
    tr, ev = m._sampler(), m._eval_sampler()
    assert tr.mine == "hardest" and (tr.candidates, tr.top) == (16, 2)
    assert ev is not tr and ev.mine is None and ev.k == 1 and ev.c.max_tries == 5
    m2 = _model({"mine": "hardest", "k": 3})
    m2._dev_cache["sampler"] = ops.Sampler(k=3, mine="hardest")
    ev2 = m2._eval_sampler()
    assert ev2.mine is None and ev2.k == 1 and ev2.c.k_neg == 1
    # without mining keys: the sampler the model always built, and evaluate() shares it when k == 1
    plain = ops.Sampler(k=1, max_tries=7)
    assert plain.mine is None and (plain.c.k_neg, plain.c.popularity, plain.c.max_tries) == (1, 0, 7)
    m3 = _model({"max_tries": 7})
    m3._dev_cache["sampler"] = plain
    assert m3._eval_sampler() is plain
    assert _model(None)._sampler() is None
    with pytest.raises(ValueError, match="mine"):
        ops.Sampler(mine="softest")
    for K, top in ((0, 1), (65, 1), (4, 5), (4, 0)):
        with pytest.raises(ValueError, match="candidates"):
            ops.Sampler(mine="hardest", candidates=K, top=top)
