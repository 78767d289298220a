# -*- coding: utf-8 -*-
"""rank_items() / evaluate_ranks() without a GPU: the two entry points are declared, exported and bound; trs_item_ranks
validates its arguments on the host before any device work; the metric arithmetic (evaluate/ranks.py) equals the
brute-force definitions of tests/ranks_ref.py; rank_items() groups its pairs and scatters the answers back."""
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

import ranks_ref as ref
from torchrecsys_amd import _lib
from torchrecsys_amd.evaluate import ranks as rank_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("trs_item_ranks_workspace_bytes", "trs_item_ranks")
PROTO = _lib.PROTOTYPES["trs_item_ranks"]  # this module is about that entry point


def _err():
    return _lib.load().trs_last_error().decode()


def test_symbols_declared_exported_and_bound():
    lib = _lib.load()
    assert lib.trs_abi_version() == _lib.ABI_VERSION == 6  # added without touching a signature: no bump
    header = open(os.path.join(ROOT, "include", "trs.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in _lib.PROTOTYPES and hasattr(so, name)
    assert len(PROTO[1]) == 13
    decl = header[header.index("int trs_item_ranks("):]
    assert decl[:decl.index(")")].count(",") == 12
    assert header.index("trs_item_ranks") > header.index("trs_fold_in_users")  # after the fold-in block
    # the workspace: n_q + 1 words that are no longer used (the size is ABI) and a key per target, monotone in both
    ws = lib.trs_item_ranks_workspace_bytes
    assert ws(0, 5) == 0 and ws(3, 0) == 32 and ws(3, 10) == 32 + 80 and ws(4, 10) > ws(3, 10) and ws(3, -1) == 0


def test_entry_point_rejects_bad_arguments_before_any_device_work():
    lib = _lib.load()
    P = 0x1000  # never dereferenced
    n_items, D, n_q = 300, 24, 5

    def tables(D=D, user=P, user_lin=P):
        T = _lib.TrsTables()
        T.user, T.item, T.user_lin, T.item_lin = user, P, user_lin, P
        T.n_users, T.n_items, T.D, T.M = 40, n_items, D, 0
        return T

    def csr(rows=n_q, off=P, items=P):
        c = _lib.TrsCsr()
        c.off, c.items, c.n_rows = off, items, rows
        return c
    fb = lib.trs_item_fold_bytes(n_items, D)
    wb = lib.trs_item_ranks_workspace_bytes(n_q, 0)

    def call(net=0, T=None, fold=P, fold_bytes=fb, users=P, n_q=n_q, targets="default", seen=None, ranks=P, values=None,
             ws=P, ws_bytes=wb):
        T = tables() if T is None else T
        targets = csr() if targets == "default" else targets
        return lib.trs_item_ranks(net, ctypes.byref(T), fold, fold_bytes, users, n_q,
                                  ctypes.byref(targets) if targets is not None else None,
                                  ctypes.byref(seen) if seen is not None else None, ranks, values, ws, ws_bytes, None)
    for kw, word in ((dict(net=2), "net"), (dict(net=-1), "net"), (dict(T=tables(user=None)), "user table"),
                     (dict(T=tables(user_lin=None)), "user table"), (dict(n_q=-1, targets=csr(rows=-1)), "n_q"),
                     (dict(T=tables(D=_lib.RETRIEVE_DMAX + 1), fold_bytes=1 << 30), "D=257"),
                     (dict(T=tables(D=0)), "D=0"), (dict(fold=None), "fold buffer"),
                     (dict(fold_bytes=fb - 4), "fold buffer too small"), (dict(targets=None), "targets CSR is NULL"),
                     (dict(targets=csr(off=None)), "NULL"), (dict(targets=csr(items=None)), "NULL"),
                     (dict(targets=csr(rows=n_q + 1)), "rows"), (dict(targets=csr(rows=n_q - 1)), "rows"),
                     (dict(seen=csr(rows=40, off=None)), "seen"), (dict(ranks=None), "ranks_out"),
                     (dict(users=None), "users"), (dict(ws=None), "workspace"), (dict(ws_bytes=wb - 8), "workspace"),
                     (dict(ws_bytes=0), "workspace")):
        assert call(**kw) == -1, kw
        assert _err().startswith("trs_item_ranks:") and word in _err(), (kw, _err())
    assert lib.trs_item_ranks(0, None, P, fb, P, n_q, ctypes.byref(csr()), None, P, None, P, wb, None) == -1
    assert "tables is NULL" in _err()
    # no query: nothing to do, nothing launched (outputs and workspace may be NULL); bad arguments are still bad
    assert call(n_q=0, targets=csr(rows=0), users=None, ranks=None, ws=None, ws_bytes=0) == 0
    assert call(n_q=0, targets=csr(rows=0), fold=None) == -1 and "fold buffer" in _err()


# ------------------------------------------------------------------------------------------------ metric arithmetic
KS = (1, 3, 10, 50)
ALL = ("auc", "mrr", "mean_rank", "hit_rate", "precision", "recall", "ndcg", "map")


def _cases():
    """(ranks per user, n_c per user, n_items): hand-made users, among them m = 1, ranks at both ends, a user whose
    relevant items fill the top of the list and one whose fill the bottom."""
    n_items = 12
    users = [([0], 12), ([11], 12), ([4], 9), ([0, 1, 2], 12), ([9, 10, 11], 12), ([7, 2, 5, 0], 10), ([0, 2], 3),
             ([6, 0, 3, 9, 2], 11), ([1], 2)]
    return users, n_items


def _run(users, n_items, ks=KS, metrics=ALL, shuffle_seed=None):
    rs = np.random.RandomState(shuffle_seed or 0)
    ranks, off = [], [0]
    for r, _ in users:
        r = list(r)
        if shuffle_seed is not None:
            rs.shuffle(r)
        ranks += r
        off.append(len(ranks))
    return rank_eval.per_user(np.array(ranks, np.int64), np.array(off), np.array([c for _, c in users]), ks, metrics,
                              n_items)


def test_metrics_equal_the_brute_force_definitions():
    users, n_items = _cases()
    for seed in (None, 3):  # the order of a user's ranks in the input does not matter
        keep, got = _run(users, n_items, shuffle_seed=seed)
        assert keep.all() and set(got) == set(rank_eval.entries(ALL, KS))
        for j, (r, n_c) in enumerate(users):
            want = ref.user_metrics(r, n_c, KS, n_items, brute_force_auc=True)
            for name, v in want.items():
                assert abs(got[name][j] - v) <= 1e-15, (j, name, got[name][j], v)
    # AUC by explicit pair counting, spelled out once: relevant at positions {0, 5} of 6 -> pairs in order: 4 + 0 of 8
    _, got = _run([([0, 5], 6)], 6, metrics=("auc", "map", "ndcg"), ks=(6,))
    assert got["auc"][0] == 0.5
    assert got["map@6"][0] == (1 / 1 + 2 / 6) / 2
    assert abs(got["ndcg@6"][0] - (1 + 1 / np.log2(7)) / (1 + 1 / np.log2(3))) <= 1e-15


def test_k_above_the_catalogue_behaves_as_n_items_and_m_equal_one():
    users, n_items = _cases()
    _, big = _run(users, n_items, ks=(n_items + 30,))
    _, full = _run(users, n_items, ks=(n_items,))
    for name in ("hit_rate", "precision", "recall", "ndcg", "map"):
        assert np.array_equal(big[f"{name}@{n_items + 30}"], full[f"{name}@{n_items}"]), name
    assert np.all(full[f"recall@{n_items}"] == 1.0) and np.all(full[f"hit_rate@{n_items}"] == 1.0)
    # m = 1 at rank r among n_c: auc = 1 - r / (n_c - 1), mrr = map = 1 / (r + 1), ndcg = 1 / log2(r + 2)
    _, one = _run([([4], 9)], n_items, ks=(10,))
    assert one["auc"][0] == 1 - 4 / 8 and one["mrr"][0] == 1 / 5 and one["map@10"][0] == 1 / 5
    assert one["mean_rank"][0] == 4.0 and abs(one["ndcg@10"][0] - 1 / np.log2(6)) <= 1e-15
    assert one["precision@10"][0] == 1 / 10 and one["recall@10"][0] == 1.0


def test_skipped_users_and_argument_errors():
    # no relevant item, or every candidate relevant: no value for any metric of the call
    users = [([], 7), ([0, 1, 2], 3), ([1], 5), ([0], 1), ([], 0), ([3, 0], 6)]
    keep, got = _run(users, 8)
    assert keep.tolist() == [False, False, True, False, False, True]
    for name, v in got.items():
        assert v.shape == (2,), name
    for j, idx in enumerate((2, 5)):
        want = ref.user_metrics(users[idx][0], users[idx][1], KS, 8, brute_force_auc=True)
        for name, v in want.items():
            assert abs(got[name][j] - v) <= 1e-15
    keep, got = _run([([], 4)], 8)
    assert not keep.any() and all(v.size == 0 for v in got.values())
    with pytest.raises(ValueError, match="unknown ranking metrics"):
        rank_eval.check(("auc", "median"), (1,))
    with pytest.raises(ValueError, match="k must be"):
        rank_eval.check(("auc",), (10, 0))
    assert rank_eval.entries(("auc", "recall", "mrr"), (5, 200)) == ["auc", "recall@5", "recall@200", "mrr"]


def test_the_reference_rank_is_the_position_in_the_ordering_of_the_candidates_and_the_target():
    rs = np.random.RandomState(7)
    for n_items in (1, 2, 40):
        vals = rs.randint(-2, 3, n_items).astype(np.float64)  # ties abound
        for seen in (None, np.array([], np.int64), np.unique(rs.randint(0, n_items, n_items // 2 + 1)),
                     np.arange(n_items)):
            t = np.arange(n_items)
            assert np.array_equal(ref.ranks_of(vals, t, seen), ref.ranks_of_by_sorting(vals, t, seen))
    # value descending, ties by ascending id; a seen target is placed among the candidates
    vals = np.array([1.0, 3.0, 1.0, 3.0, 0.0])
    assert ref.ranks_of(vals, np.arange(5)).tolist() == [2, 0, 3, 1, 4]
    assert ref.ranks_of(vals, np.arange(5), np.array([1, 2])).tolist() == [1, 0, 2, 0, 2]


# ------------------------------------------------------------------------------------------------ pair grouping
def _df():
    rs = np.random.RandomState(0)
    return pd.DataFrame({"user_id": np.concatenate([np.arange(40), rs.randint(0, 40, 360)]),
                         "item_id": np.concatenate([np.arange(30), rs.randint(0, 30, 370)])})


def _model(net_type="fm"):
    from torchrecsys_amd.model import TorchRecSys
    with contextlib.redirect_stdout(io.StringIO()):
        return TorchRecSys(_df(), "user_id", "item_id", n_factors=8, net_type=net_type)


def test_rank_items_groups_pairs_and_scatters_back(monkeypatch):
    m = _model()
    calls = []

    def stub(qusers, off, items, exclude_seen, want_values=False):
        # the contract of _ranks_dense: distinct ascending query users, per row sorted distinct items
        calls.append(exclude_seen)
        assert qusers.dtype == off.dtype == items.dtype == torch.int64
        assert torch.all(qusers[1:] > qusers[:-1]) and off[0] == 0 and off[-1] == items.numel()
        assert off.numel() == qusers.numel() + 1 and torch.all(off[1:] > off[:-1])
        for q in range(qusers.numel()):
            seg = items[off[q]:off[q + 1]]
            assert torch.all(seg[1:] > seg[:-1])
        users = torch.repeat_interleave(qusers, off[1:] - off[:-1])
        ranks = users * 1000 + items  # a known answer per pair
        return ranks, (ranks.float() / 8 if want_values else None)
    monkeypatch.setattr(m, "_ranks_dense", stub)
    u = [7, 3, 7, 39, 3, 7, 0, 3, 7]   # unsorted, users in non-adjacent positions
    i = [5, 29, 5, 0, 1, 2, 11, 29, 9]  # duplicates: (7, 5) twice, (3, 29) twice
    got = m.rank_items(u, i)
    assert got.dtype == torch.int64 and got.tolist() == [a * 1000 + b for a, b in zip(u, i)]
    got, sc = m.rank_items(torch.tensor(u), np.array(i), exclude_seen=False, return_scores=True)
    assert got.tolist() == [a * 1000 + b for a, b in zip(u, i)] and sc.dtype == torch.float32
    assert sc.tolist() == [(a * 1000 + b) / 8 for a, b in zip(u, i)]
    assert calls == [True, False]
    qusers, off, items, inv = m._group_pairs(torch.tensor(u), torch.tensor(i), m.n_items)
    assert qusers.tolist() == [0, 3, 7, 39] and off.tolist() == [0, 1, 3, 6, 7]
    assert items.tolist() == [11, 1, 29, 2, 5, 9, 0] and inv.tolist() == [4, 2, 4, 6, 1, 3, 0, 2, 5]


def test_rank_items_argument_errors_come_before_any_device_work(monkeypatch):
    from torchrecsys_amd import model as model_mod

    def no_device(*a, **kw):
        raise AssertionError("reached the device before validating the arguments")
    monkeypatch.setattr(model_mod, "_device", no_device)
    m = _model()
    with pytest.raises(ValueError, match="as many"):
        m.rank_items([1, 2], [3])
    with pytest.raises(IndexError, match="user id 40"):
        m.rank_items([1, 40], [3, 3])
    with pytest.raises(IndexError, match="item id 30"):
        m.rank_items([1, 2], [3, 30])
    with pytest.raises(IndexError, match="-1"):
        m.rank_items([1], [-1])
    e = m.rank_items([], [])
    assert e.shape == (0,) and e.dtype == torch.int64
    e, s = m.rank_items([], [], return_scores=True)
    assert e.shape == s.shape == (0,) and s.dtype == torch.float32
    with pytest.raises(ValueError, match="unknown ranking metrics"):
        m.evaluate_ranks(metrics=("auc", "hitrate"))
    with pytest.raises(ValueError, match="k must be"):
        m.evaluate_ranks(k=0)
    with pytest.raises(AssertionError, match="reached the device"):  # valid arguments get as far as the device
        m.rank_items([1, 2], [3, 4])
