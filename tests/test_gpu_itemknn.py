# -*- coding: utf-8 -*-
"""fit_itemknn() / ops.knn_build / ops.knn_scores on the GPU against the numpy restatement tests/itemknn_ref.py, which
tests/test_itemknn_host.py ties to a brute-force dense X^T X.

Every comparison is exact: array_equal on the ids and on the weights' bits.  The counts are integers, the similarity is
one float64 expression rounded to float32 once and the scores are a sequential float32 loop, so a last-bit difference is
a bug in the kernel's arithmetic, not a reason for a tolerance.

Shapes: n_items in {1, 2, 63, 64, 65, 1000, TILE - 1, TILE, TILE + 1, 2 TILE + 3} (TILE = TRS_KNN_TILE, the columns
whose counters one LDS tile holds; it is also a multiple of the 8 192 columns of a score-row tile).  Histories:
itemknn_ref.histories: lengths 0, 1, 2, 63, 64, 65, then random 0..20, ids drawn over the whole range.  The three ways
the build kernel finds a user's tile segment are all met: one tile (n <= TILE), a cursor per user (more tiles, an item
with at most 512 users: the random shapes beyond TILE), two binary searches (more tiles, more users: the counter-width
case)."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

import ease_ref
import itemknn_ref as ref
from torchrecsys_amd import _lib, ops
from torchrecsys_amd.model import TorchRecSys

pytestmark = pytest.mark.gpu

TILE, KMAX, TOUCHED = _lib.KNN_TILE, _lib.KNN_KMAX, _lib.KNN_TOUCHED
BOUNDARY = (TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
COMBOS = [(1, "cosine", 0.0), (7, "jaccard", 10.0), (64, "conditional", 0.0), (KMAX, "count", 10.0)]
MORE = [(KMAX, "cosine", 10.0), (64, "jaccard", 0.0), (7, "conditional", 10.0), (1, "count", 0.0)]
# every K, kind and h at every tile-boundary shape and at 1 000; the small shapes take the combinations in turn
BUILD_CASES = [(n, *c) for n in BOUNDARY + (1000,) for c in COMBOS] + [(1000, *c) for c in MORE] + \
              [(n, *c) for k, n in enumerate((1, 2, 63, 64, 65)) for c in (COMBOS[k % 4], MORE[(k + 1) % 4])]


def n_users_for(n):
    return 40 if n <= 2 else 150 if n <= 65 else 2000 if n == 1000 else 3000


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _csrs(lists, n):
    """(user -> items, item -> users) on the GPU."""
    off, ids = ref.csr(lists)
    ioff, users = ref.csr(ref.inverse(lists, n))
    return (_gpu(off), _gpu(ids)), (_gpu(ioff), _gpu(users))


@functools.lru_cache(maxsize=None)
def lists_of(n):
    return ref.histories(n_users_for(n), n, n)


@functools.lru_cache(maxsize=None)
def pairs_of(n):
    """The co-counts of one shape, computed once and shared by its cases."""
    return ref.cocounts(lists_of(n), n)


@functools.lru_cache(maxsize=None)
def csrs_of(n):
    return _csrs(lists_of(n), n)


def build(lists, n, kind, h, K, csrs=None):
    err = torch.zeros(1, dtype=torch.int32, device=_dev())
    by_user, by_item = csrs or _csrs(lists, n)
    ids, w = ops.knn_build(by_user, by_item, n, kind, h, K, err)
    assert int(err.item()) == 0
    assert ids.shape == w.shape == (n, K) and ids.dtype == torch.int32 and w.dtype == torch.float32
    return ids, w


def same(got, want):
    (gi, gw), (wi, ww) = got, want
    gi, gw = gi.cpu().numpy(), gw.cpu().numpy()
    bad = np.nonzero((gi != wi).any(axis=1) | (gw.view(np.int32) != ww.view(np.int32)).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], gi[bad[:1]], wi[bad[:1]], gw[bad[:1]], ww[bad[:1]])


def _model(lists, n_items, seed=0, net_type='itemknn', **kw):
    """A model whose train split is exactly `lists` (split_ratio 1), the pairs in a shuffled order."""
    users = np.repeat(np.arange(len(lists)), [len(v) for v in lists])
    items = np.concatenate(lists)
    p = np.random.RandomState(seed).permutation(users.size)
    with contextlib.redirect_stdout(io.StringIO()):
        return TorchRecSys.from_tensors(torch.from_numpy(users[p]), torch.from_numpy(items[p]), n_users=len(lists),
                                        n_items=n_items, net_type=net_type, split_ratio=1.0, **kw)


# ------------------------------------------------------------------------------------------------ 1. build
@pytest.mark.parametrize("n,K,kind,h", BUILD_CASES, ids=["n%d_K%d_%s_h%g" % c for c in BUILD_CASES])
def test_build_against_the_restatement(n, K, kind, h):
    want = ref.neighbours(pairs_of(n), n, kind, h, K)
    same(build(lists_of(n), n, kind, h, K, csrs_of(n)), want)


# ------------------------------------------------------------------------------------------------ 2. edge cases
def test_a_count_beyond_16_bits_comes_back_exact():
    """Two items in different tiles are held together by 70 000 users: c = 70 000 > 65 535.  600 of them hold a third
    item in the last tile, ten more users hold the first item and 100 others spread over the tiles: an item with more
    users than the build kernel has threads finds the tile segments by binary search, long segments included."""
    n, a, b, c3 = 2 * TILE + 3, 5, TILE + 9, 2 * TILE + 1
    rs = np.random.RandomState(0)
    lists = [np.array([a, b, c3] if u < 600 else [a, b], dtype=np.int64) for u in range(70000)]
    rest = np.setdiff1d(np.arange(n), [a, b, c3])
    lists += [np.unique(np.concatenate([[a], rs.choice(rest, 100, replace=False)])).astype(np.int64) for _ in range(10)]
    pairs = ref.cocounts(lists, n)
    csrs = _csrs(lists, n)
    got = {kind: build(lists, n, kind, 0.0, 7, csrs) for kind in ("count", "cosine")}
    for kind in got:
        same(got[kind], ref.neighbours(pairs, n, kind, 0.0, 7))
    ids, w = (t.cpu().numpy() for t in got["count"])
    assert ids[a, 0] == b and ids[b, 0] == a and w[a, 0] == 70000.0 and w[b, 0] == 70000.0 and w[c3, 0] == 600.0


def test_padding_an_item_nobody_holds_and_items_with_fewer_than_K_candidates():
    n, gone = 65, 7
    lists = [v[v != gone] for v in ref.histories(150, n, 3)]
    for K in (64, KMAX):
        got = build(lists, n, "cosine", 0.0, K)
        same(got, ref.neighbours(ref.cocounts(lists, n), n, "cosine", 0.0, K))
        ids, w = got[0].cpu().numpy(), got[1].cpu().numpy()
        assert (ids[gone] == -1).all() and not w[gone].any() and not (ids == gone).any()
        assert ((ids == -1) == (w == 0)).all() and (ids[:, -1] == -1).all()  # at most 63 candidates for K >= 64


@pytest.mark.parametrize("K", [7, KMAX])
def test_ties_across_tiles_keep_the_lowest_ids_in_order(K):
    """Item 0 co-occurs exactly once with each of 3 K items of degree 1, spread over three tiles: every key has the same
    similarity, so the K lowest ids come back, in order, whichever tile they were met in."""
    n = 2 * TILE + 3
    third = [2 * TILE, 2 * TILE + 1, 2 * TILE + 2]
    first = [3 + 5 * m for m in range((3 * K - 3) // 2)]
    second = [TILE + 3 * m for m in range(3 * K - 3 - len(first))]
    others = first + second + third
    assert len(others) == 3 * K and len(set(others)) == 3 * K
    order = np.random.RandomState(K).permutation(3 * K)
    lists = [np.array([0, others[m]], dtype=np.int64) for m in order]
    for kind in ref.KINDS:
        ids, w = build(lists, n, kind, 0.0, K)
        assert ids[0].cpu().tolist() == sorted(others)[:K], kind
        assert len(set(w[0].cpu().tolist())) == 1
        same((ids, w), ref.neighbours(ref.cocounts(lists, n), n, kind, 0.0, K))


@pytest.mark.parametrize("n", [TILE, 2 * TILE + 3])
def test_touched_list_overflow_falls_back_to_the_sweep(n):
    """One user holds every 22nd id: more columns per tile than the touched list has entries, so each of those items'
    tiles is swept; every one of them still gets its exact top K.  300 random users make the similarities differ."""
    every = np.arange(0, n, 22, dtype=np.int64)
    assert min(np.sum(every // TILE == t) for t in range(min(2, -(-n // TILE)))) > TOUCHED
    lists = [every] + ref.histories(300, n, 5)
    pairs = ref.cocounts(lists, n)
    csrs = _csrs(lists, n)
    for K, kind, h in ((KMAX, "cosine", 0.0), (7, "jaccard", 10.0)):
        same(build(lists, n, kind, h, K, csrs), ref.neighbours(pairs, n, kind, h, K))


def test_two_builds_are_equal_bit_for_bit():
    n = 2 * TILE + 3
    a = build(lists_of(n), n, "cosine", 10.0, 64, csrs_of(n))
    b = build(lists_of(n), n, "cosine", 10.0, 64, csrs_of(n))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    m = 1000
    a = build(lists_of(m), m, "jaccard", 0.0, KMAX, csrs_of(m))
    b = build(lists_of(m), m, "jaccard", 0.0, KMAX, csrs_of(m))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


# ------------------------------------------------------------------------------------------------ 3. score rows
def _scores(ids, w, lists, rows):
    hist = (_gpu(ref.csr(lists)[0]), _gpu(ref.csr(lists)[1]))
    err = torch.zeros(1, dtype=torch.int32, device=_dev())
    out = ops.knn_scores(ids, w, hist, torch.tensor(rows, dtype=torch.int64, device=_dev()), err)
    assert int(err.item()) == 0
    return out.cpu().numpy()


@pytest.mark.parametrize("n,K", [(1, 1), (2, 7), (63, 64), (64, KMAX), (65, 64), (1000, KMAX), (1000, 7)])
def test_score_rows_bit_for_bit(n, K):
    """At 63..65 items with K >= 63 every list holds nearly every column: the same j from many i."""
    lists = lists_of(n)  # lengths 0, 1, 2, 63, 64, 65 first
    ids, w = build(lists, n, "cosine", 0.0, K, csrs_of(n))
    want = ref.score_rows(ids.cpu().numpy(), w.cpu().numpy(), lists, n)
    got = _scores(ids, w, lists, list(range(len(lists))))
    assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert not got[0].any()  # the empty history
    for rows in ([5], list(range(17)), [5, 3, 5, 0, 5]):  # a row listed three times
        assert np.array_equal(_scores(ids, w, lists, rows).view(np.int32), want[rows].view(np.int32)), rows
    assert ops.knn_scores(ids, w, csrs_of(n)[0], torch.zeros(0, dtype=torch.int64, device=_dev())).shape == (0, n)


@pytest.mark.parametrize("n", BOUNDARY)
def test_score_rows_at_the_tile_boundaries(n):
    lists = lists_of(n)
    ids, w = build(lists, n, "conditional", 10.0, KMAX, csrs_of(n))
    rows = [0, 1, 2, 3, 4, 5, 3, 100, 2999]
    want = ref.score_rows(ids.cpu().numpy(), w.cpu().numpy(), [lists[r] for r in rows], n)
    got = _scores(ids, w, lists, rows)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert got[5].any() and not got[0].any()


def test_score_rows_reach_the_first_and_last_column_of_every_tile():
    n = 2 * TILE + 3
    held = np.array([0, 8191, 8192, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, 2 * TILE + 2], dtype=np.int64)
    lists = [held, held[::2].copy(), np.array([0], dtype=np.int64), np.zeros(0, dtype=np.int64)]
    ids, w = build(lists, n, "count", 0.0, 7)
    same((ids, w), ref.neighbours(ref.cocounts(lists, n), n, "count", 0.0, 7))
    want = ref.score_rows(ids.cpu().numpy(), w.cpu().numpy(), lists, n)
    got = _scores(ids, w, lists, [0, 1, 2, 3])
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert set(np.nonzero(got[2])[0].tolist()) == set(held[1:].tolist()) and got[0, 2 * TILE + 2] > 0


# ------------------------------------------------------------------------------------------------ 4. the surface
@functools.lru_cache(maxsize=None)
def fitted(n, K, kind, h):
    m = _model(lists_of(n), n)
    m.fit_itemknn(neighbours=K, similarity=kind, shrinkage=h)
    ids, w = m.net.nbr_ids.cpu().numpy(), m.net.nbr_w.cpu().numpy()
    return m, ids, w, ref.score_rows(ids, w, lists_of(n), n)


@pytest.mark.parametrize("n,K,kind,h", [(65, 10, "cosine", 0.0), (1000, 100, "jaccard", 10.0)])
def test_recommend_predict_and_rank_items_position_for_position(n, K, kind, h):
    m, ids, w, rows = fitted(n, K, kind, h)
    lists = lists_of(n)
    want = ref.neighbours(pairs_of(n), n, kind, h, K)  # fit_itemknn is the launcher over the model's own CSRs
    assert np.array_equal(ids, want[0]) and np.array_equal(w.view(np.int32), want[1].view(np.int32))
    users = list(range(0, len(lists), 1 if n == 65 else 40))
    for exclude in (True, False):
        for k in (1, 10, 200):
            kk = min(k, n)
            got_i, got_s = m.recommend(users, top_k=k, exclude_seen=exclude, return_scores=True)
            wi, ws = ease_ref.recommend(rows[users], [lists[u] for u in users], kk, exclude)
            assert np.array_equal(got_i.numpy(), wi), (exclude, k)
            assert np.array_equal(got_s.numpy(), ws), (exclude, k)
    for u in (0, 1, 5):
        assert np.array_equal(m.predict(u, top_k=7).numpy(), ease_ref.recommend(rows[u:u + 1], lists, 7, False)[0][0])
    assert np.array_equal(m.predict_many([3, 9], top_k=4).numpy(), ease_ref.recommend(rows[[3, 9]], lists, 4, False)[0])
    # rank_items() is consistent with recommend(): the item recommend() puts at position r has rank r
    qu = [u for u in users if len(lists[u])][:12]
    for exclude in (True, False):
        top = m.recommend(qu, top_k=5, exclude_seen=exclude).numpy()
        us = np.repeat(qu, 5)
        keep = top.reshape(-1) >= 0
        got, val = m.rank_items(us[keep], top.reshape(-1)[keep], exclude_seen=exclude, return_scores=True)
        assert got.tolist() == np.tile(np.arange(5), len(qu))[keep].tolist(), exclude
        assert np.array_equal(val.numpy(), rows[us[keep], top.reshape(-1)[keep]])


def test_evaluate_ranking_and_evaluate_ranks_agree_on_hit_rate():
    n, nu = 200, 400
    lists = ref.histories(nu, n, 5)
    users = np.repeat(np.arange(nu), [len(v) for v in lists])
    items = np.concatenate(lists)
    p = np.random.RandomState(0).permutation(users.size)
    with contextlib.redirect_stdout(io.StringIO()):
        m = TorchRecSys.from_tensors(torch.from_numpy(users[p]), torch.from_numpy(items[p]), n_users=nu, n_items=n,
                                     net_type='itemknn', split_ratio=0.8)
        m.fit_itemknn(neighbours=20, similarity='cosine', shrinkage=1.0)
        got_k = m.evaluate_ranking(k=10)
        got_r = m.evaluate_ranks(k=(10,), metrics=('hit_rate', 'mrr'))
    assert got_k['n_users'] == got_r['n_users'] > 50  # every user has candidates: the two average over the same users
    assert 0.0 < got_k['hit_rate@10'] <= 1.0 and 0.0 < got_r['mrr'] <= 1.0
    assert got_r['hit_rate@10'] == pytest.approx(got_k['hit_rate@10'], rel=1e-12)


def test_recommend_for_histories_item_weights_and_the_state_dict_round_trip():
    n, K = 65, 10
    m, ids, w, rows = fitted(n, K, "cosine", 0.0)
    lists = lists_of(n)
    # cold start: a history identical to a train user's gives that user's recommendations
    users = [1, 2, 3, 5, 20, 0]
    for exclude in (True, False):
        a, sa = m.recommend(users, top_k=10, exclude_seen=exclude, return_scores=True)
        b, sb = m.recommend_for_histories([lists[u] for u in users], top_k=10, exclude_seen=exclude, return_scores=True)
        assert torch.equal(a, b) and torch.equal(sa, sb), exclude
    hists = [[], [4], [9, 2, 9, 30]]  # unsorted, repeated: cleaned up first
    clean = [np.unique(np.asarray(v, dtype=np.int64)) for v in hists]
    wi, ws = ease_ref.recommend(ref.score_rows(ids, w, clean, n), clean, 6, True)
    gi, gs = m.recommend_for_histories(hists, top_k=6, return_scores=True)
    assert np.array_equal(gi.numpy(), wi) and np.array_equal(gs.numpy(), ws)
    with pytest.raises(ValueError, match="fold-in options"):
        m.recommend_for_histories(hists, epochs=3)
    # item_weights reads the stored lists; beyond K: -1 / -inf
    items = [0, 7, 64, 7]
    for k in (1, K, K + 5):
        gi, gs = m.item_weights(items, top_k=k, return_scores=True)
        for r, i in enumerate(items):
            wi, ws = ref.item_weights(ids, w, i, k)
            assert np.array_equal(gi[r].numpy(), wi) and np.array_equal(gs[r].numpy(), ws), (k, i)
    assert (gi[:, K:] == -1).all() and torch.isinf(gs[:, K:]).all()
    with pytest.raises(IndexError):
        m.item_weights([n])
    # state_dict carries the lists into a fresh model
    fresh = _model(lists, n, seed=4)
    assert not fresh.state_dict()
    fresh.load_state_dict(m.state_dict())
    assert fresh.net.knn_meta.tolist() == [float(_lib.KNN_KIND["cosine"]), 0.0, float(K)]
    every = list(range(len(lists)))
    a, sa = m.recommend(every, top_k=10, return_scores=True)
    b, sb = fresh.recommend(every, top_k=10, return_scores=True)
    assert torch.equal(a, b) and torch.equal(sa, sb)


def test_fit_itemknn_twice_and_from_another_pair_order_gives_the_same_bits():
    n = 1000
    m, ids, w, _ = fitted(n, 100, "jaccard", 10.0)
    m2 = _model(lists_of(n), n, seed=9)  # the same pairs in another order
    m2.fit_itemknn(neighbours=100, similarity='jaccard', shrinkage=10.0)
    assert torch.equal(m2.net.nbr_ids, m.net.nbr_ids) and torch.equal(m2.net.nbr_w, m.net.nbr_w)
    m2.fit_itemknn(neighbours=100, similarity='jaccard', shrinkage=10.0)
    assert torch.equal(m2.net.nbr_ids, m.net.nbr_ids) and torch.equal(m2.net.nbr_w, m.net.nbr_w)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_what_does_not_apply_refuses():
    n = 65
    m, _, _, _ = fitted(n, 10, "cosine", 0.0)
    for exc, call in ((NotImplementedError, lambda: m.fit(None)), (ValueError, lambda: m.fit_als()),
                      (ValueError, lambda: m.fit_ease()), (NotImplementedError, lambda: m.evaluate()),
                      (ValueError, lambda: m.fold_in_users([[1]])), (ValueError, lambda: m.fold_in_items([[1]])),
                      (ValueError, lambda: m.similar_items([1])), (ValueError, lambda: m.recommend_diverse([1]))):
        with pytest.raises(exc, match="itemknn"):
            call()
    with pytest.raises(ValueError, match="net_type='itemknn'"):
        _model(lists_of(n), n, net_type='linear').fit_itemknn()
    unfitted = _model(lists_of(n), n)
    for call in (lambda: unfitted.recommend([0]), lambda: unfitted.predict(0), lambda: unfitted.rank_items([0], [1]),
                 lambda: unfitted.recommend_for_histories([[1]]), lambda: unfitted.item_weights([1])):
        with pytest.raises(RuntimeError, match=r"call fit_itemknn\(\) first"):
            call()
