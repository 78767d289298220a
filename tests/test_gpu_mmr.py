# -*- coding: utf-8 -*-
"""recommend_diverse() / evaluate_diversity(): greedy MMR re-ranking of the fused top-k's pool and the diversity
metrics (csrc/rerank.hip) against the numpy oracle tests/mmr_ref.py."""
import contextlib
import io

import numpy as np
import pytest
import torch

import mmr_ref as ref
import neighbours_ref as nref

pytestmark = pytest.mark.gpu

KMAX = ref.KMAX
DEV = "cuda:0"
NK = [(1, 1), (2, 2), (33, 10), (64, 64), (128, 10), (128, 128)]


def _quiet():
    return contextlib.redirect_stdout(io.StringIO())


def _model(net_type, n_users, n_items, D, M=0, seed=0, int_range=None, n=None, **kw):
    """As _model() of tests/test_gpu_neighbours.py: every user and item occurs, tables random floats or small integers."""
    from torchrecsys_amd.model import TorchRecSys
    rs = np.random.RandomState(seed)
    n = n or max(4 * n_users, 2 * n_items)
    u = np.concatenate([np.arange(n_users), rs.randint(0, n_users, n - n_users)])
    i = np.concatenate([np.arange(n_items), rs.randint(0, n_items, n - n_items)])
    meta = torch.from_numpy(rs.randint(0, 5, (n_items, M))) if M else None
    with _quiet():
        torch.manual_seed(seed)
        np.random.seed(seed)
        m = TorchRecSys.from_tensors(torch.from_numpy(u), torch.from_numpy(i), n_users=n_users, n_items=n_items,
                                     item_metadata=meta, metadata_names=[f"m{j}" for j in range(M)] if M else None,
                                     n_factors=D, net_type=net_type, **kw)
    g = torch.Generator().manual_seed(seed + 1)
    for p in m.net.parameters():
        if int_range is not None:  # small integers: every fp32 inner product is exact in any summation order
            p.data.copy_(torch.randint(int_range[0], int_range[1], p.shape, generator=g).float())
        else:
            p.data.copy_(torch.randn(p.shape, generator=g))
    return m


def _sparse_unit_rows(n, D, seed):
    """Rows with entries in {0, +-1} and exactly 4 or 16 non-zeros: norms 2 or 4, every normalised product exact."""
    rs = np.random.RandomState(seed)
    X = np.zeros((n, D), np.float32)
    for r in range(n):
        nz = rs.choice(D, 4 if rs.rand() < 0.5 else 16, replace=False)
        X[r, nz] = rs.choice([-1.0, 1.0], len(nz))
    return X


def _set_seen(m, lists):
    """Replace the model's train-split CSR (what exclude_seen masks) by the given per-user item lists."""
    off = np.zeros(m.n_users + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    items = np.concatenate([np.sort(np.asarray(x, np.int32)) for x in lists]).astype(np.int32)
    m._dev_cache["seen_csr"] = (torch.from_numpy(off).to(DEV), torch.from_numpy(items).to(DEV))


def _user_sets(n_users, seed):
    """One query, 33, and 300 with repeated users."""
    rs = np.random.RandomState(seed)
    return [np.array([n_users // 2]), rs.randint(0, n_users, 33), rs.randint(0, n_users, 300)]


def _diverse(m, users, **kw):
    ids, sc = m.recommend_diverse(users, return_scores=True, **kw)
    assert ids.dtype == torch.int64 and sc.dtype == torch.float32 and not ids.is_cuda and not sc.is_cuda
    return ids.numpy(), sc.numpy()


def _pool(m, users, N, **kw):
    ids, sc = m.recommend(users, top_k=N, return_scores=True, **kw)
    return ids.numpy(), sc.numpy()


def _check_exact(m, X, metric, lams, users_of, nk=NK):
    """recommend_diverse == the oracle's re-ranking of recommend(top_k=N)'s pool, ids and scores bit for bit.  X: the
    exact similarity matrix.  users_of(N, k): the query sets of that shape."""
    pools = {}
    for N, k in nk:
        for users in users_of(N, k):
            key = (N, len(users))
            if key not in pools:
                pools[key] = _pool(m, users, N)
            pids, psc = pools[key]
            for lam in lams:
                want_ids, want_sc, _ = ref.rerank(pids, psc, X, min(k, pids.shape[1]), lam, n_items=m.n_items)
                ids, sc = _diverse(m, users, top_k=k, diversity=lam, pool=N, metric=metric)
                assert ids.shape == want_ids.shape
                np.testing.assert_array_equal(ids, want_ids, err_msg=f"N={N} k={k} lam={lam} n_q={len(users)}")
                assert np.array_equal(sc, want_sc)


# ------------------------------------------------------------------------------------------------ 1. diversity = 0
@pytest.mark.parametrize("net_type", ["linear", "fm"])
@pytest.mark.parametrize("M", [0, 2])
def test_diversity_zero_is_recommend_bit_for_bit(net_type, M):
    k = 10
    for n_items, D in ((300, 24), (40, 100)):
        m = _model(net_type, 60, n_items, D, M, seed=3 + M + D)
        for users in _user_sets(60, seed=D):
            want_ids, want_sc = m.recommend(users, top_k=k, return_scores=True)
            for pool in (k, 33, KMAX):
                for metric in ("cosine", "dot"):
                    ids, sc = m.recommend_diverse(users, top_k=k, diversity=0, pool=pool, metric=metric,
                                                  return_scores=True)
                    assert torch.equal(ids, want_ids) and torch.equal(sc, want_sc), (n_items, pool, metric)
        ex = m.recommend([1, 2, 1], top_k=k, exclude_seen=False)
        assert torch.equal(m.recommend_diverse([1, 2, 1], top_k=k, diversity=0.0, exclude_seen=False), ex)


# ------------------------------------------------------------------------------------------------ 2. bit-exact
@pytest.mark.parametrize("net_type", ["linear", "fm"])
@pytest.mark.parametrize("M", [0, 2])
@pytest.mark.parametrize("D", [8, 24, 64, 100, 256])
def test_dot_on_integer_tables_is_bit_exact(net_type, M, D):
    n_users = 50
    sets = _user_sets(n_users, seed=D + M)
    for n_items in (40, 300):
        m = _model(net_type, n_users, n_items, D, M, seed=D + M + n_items, int_range=(-3, 4))
        S = nref.item_rows(m)
        X = S @ S.T  # integers below 2^24: exact in fp32 in any order
        assert np.abs(X).max() < 2 ** 24
        # every (N, k) on 33 users; one and 300 users where the pool is cut out of a larger catalogue
        users_of = lambda N, k: sets if (N, k) in ((33, 10), (128, 10)) else sets[1:2]
        _check_exact(m, X, "dot", (0.25, 0.5, 1.0), users_of)


@pytest.mark.parametrize("net_type,D,n_items", [("linear", 24, 300), ("fm", 100, 300), ("fm", 256, 300),
                                                ("linear", 64, 40)])
def test_cosine_on_rows_with_exact_norms_is_bit_exact(net_type, D, n_items):
    m = _model(net_type, 50, n_items, D, 0, seed=D, int_range=(-3, 4))
    R = _sparse_unit_rows(n_items, D, seed=D + 1)
    m.net.item.weight.data.copy_(torch.from_numpy(R))
    Xn = nref.normalise(R.astype(np.float64))
    assert np.array_equal(nref.normalise_f32(R).astype(np.float64), Xn)
    sets = _user_sets(50, seed=D)
    users_of = lambda N, k: sets if (N, k) == (33, 10) else sets[1:2]
    _check_exact(m, Xn @ Xn.T, "cosine", (0.25, 0.5, 1.0), users_of)


# ------------------------------------------------------------------------------------------------ 3. random floats
def _ops_rerank(m, users, N, k, lam, cosine=True, exclude_seen=True):
    """The pieces recommend_diverse is made of, with the pool and the pool positions kept: (pool ids, pool scores, fold
    rows (n_items, Dp) as stored, ids, scores, positions), numpy."""
    from torchrecsys_amd import ops
    du = torch.as_tensor(np.asarray(users), dtype=torch.int64, device=DEV)
    pids, psc, _ = m._rank_dense(du, N, exclude_seen)
    assert m.net.n_meta_tables() == 0
    nf = ops.neighbour_fold(m.net.item.weight.data, m.n_items, m.n_factors, cosine)
    rows, zero = ops.fold_views(nf, m.n_items, m.n_factors)
    assert not zero.any()
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ids, sc, pos = ops.mmr_rerank(nf, m.n_items, m.n_factors, pids, psc, k, lam, want_pos=True, err_flag=err)
    assert int(err) == 0
    return tuple(t.cpu().numpy() for t in (pids, psc, rows, ids, sc, pos))


@pytest.mark.parametrize("net_type,D", [("linear", 24), ("fm", 100), ("fm", 256)])
def test_gaussian_tables_give_greedy_lists_within_rounding(net_type, D):
    N, k, n_items = 128, 20, 300
    m = _model(net_type, 50, n_items, D, 0, seed=21 + D)
    users = _user_sets(50, seed=D)[2]
    for lam in (0.3, 0.7, 1.0):
        pids, psc, rows, ids, sc, pos = _ops_rerank(m, users, N, k, lam)
        worst = ref.check_greedy(pids, psc, rows, k, lam, D, ids, sc, pos)
        print(f"{net_type} D={D} lam={lam}: largest shortfall of a pick {worst:.3e} (eps {ref.eps(lam, D):.3e})")
        assert np.array_equal(sc, np.take_along_axis(psc, pos.astype(np.int64), 1))  # (k <= n_valid everywhere)
        got_ids, got_sc = _diverse(m, users, top_k=k, diversity=lam, pool=N)
        assert np.array_equal(got_ids, ids) and np.array_equal(got_sc, sc)  # the public method is that launch
        assert (ids != pids[:, :k]).any()  # ... and it does re-rank


# ------------------------------------------------------------------------------------------------ 4. short pools
def test_short_pools_pad_with_minus_one_and_a_user_without_candidates():
    n_users, n_items, D, k = 12, 40, 24, 10
    m = _model("fm", n_users, n_items, D, 2, seed=9, int_range=(-3, 4))
    rs = np.random.RandomState(4)
    left = [0, 1, 3, 9, 10, 11, 25, 40, 40, 40, 40, 40]  # candidates left to user u
    _set_seen(m, [rs.permutation(n_items)[:n_items - c] for c in left])
    S = nref.item_rows(m)
    X = S @ S.T
    users = np.array([0, 1, 2, 3, 4, 5, 6, 7, 0, 3])
    for N in (k, 33, KMAX):
        pids, psc = _pool(m, users, N)
        assert pids.shape[1] == min(N, n_items)
        for lam in (0.0, 0.5, 1.0):
            want_ids, want_sc, _ = ref.rerank(pids, psc, X, k, lam)
            ids, sc = _diverse(m, users, top_k=k, diversity=lam, pool=N, metric="dot")
            np.testing.assert_array_equal(ids, want_ids)
            assert np.array_equal(sc, want_sc)
            for r, u in enumerate(users):
                nv = min(k, left[u])
                assert np.all(ids[r, :nv] >= 0) and np.all(ids[r, nv:] == -1) and np.all(np.isneginf(sc[r, nv:]))
            assert np.all(ids[0] == -1) and np.all(ids[8] == -1)  # user 0 has seen the whole catalogue
    # an id outside the catalogue in a pool: never an address, reported, and skipped by the selection
    from torchrecsys_amd import ops
    nf = ops.neighbour_fold(torch.from_numpy(S.astype(np.float32)).to(DEV), n_items, D, False)
    pids = np.array([[5, n_items, 7, -1], [3, 2, 1, 0]], np.int64)
    psc = np.array([[0.9, 0.8, 0.7, -np.inf], [0.4, 0.3, 0.2, 0.1]], np.float32)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ids, sc, pos = ops.mmr_rerank(nf, n_items, D, torch.from_numpy(pids).to(DEV), torch.from_numpy(psc).to(DEV), 3, 0.5,
                                  want_pos=True, err_flag=err)
    want = ref.rerank(pids, psc, X, 3, 0.5, n_items=n_items)
    assert int(err) == 1
    for got, w in zip((ids, sc, pos), want):
        assert np.array_equal(got.cpu().numpy(), w)
    assert ids[0].tolist()[2] == -1 and sorted(ids[0].tolist()[:2]) == [5, 7]


# ------------------------------------------------------------------------------------------------ 5. structure
def _clustered(n_items, D=24, clusters=4):
    """Unit rows e_c: item i belongs to cluster i % clusters, clusters orthogonal."""
    R = np.zeros((n_items, D), np.float32)
    R[np.arange(n_items), np.arange(n_items) % clusters] = 1.0
    return R


def test_clusters_are_visited_before_any_is_repeated():
    n_items, D = 16, 24
    m = _model("linear", 20, n_items, D, 0, seed=2)
    m.net.item.weight.data.copy_(torch.from_numpy(_clustered(n_items, D)))
    users = np.arange(20)
    pids, _ = _pool(m, users, 16, exclude_seen=False)
    ids, _ = _diverse(m, users, top_k=16, diversity=1.0, pool=16, exclude_seen=False)
    for r in range(len(users)):
        first = [int(pids[r][np.nonzero(pids[r] % 4 == c)[0][0]]) for c in range(4)]
        first.sort(key=lambda x: pids[r].tolist().index(x))  # the first pool entry of each cluster, in pool order
        assert ids[r, :4].tolist() == first
        assert sorted(ids[r].tolist()) == list(range(16))
        # once every cluster is visited all penalties are 1: the rest follows in pool order
        assert ids[r, 4:].tolist() == [x for x in pids[r].tolist() if x not in first]
    # a zero row under cosine is similar to nothing (penalty 0 throughout): at diversity 1 it ties with the items of
    # clusters not yet visited and beats every item of a visited cluster
    R = _clustered(n_items, D)
    R[5] = 0.0
    m.net.item.weight.data.copy_(torch.from_numpy(R))
    pids, psc = _pool(m, users, 16, exclude_seen=False)
    ids, sc = _diverse(m, users, top_k=16, diversity=1.0, pool=16, exclude_seen=False)
    want_ids, want_sc, _ = ref.rerank(pids, psc, R.astype(np.float64) @ R.astype(np.float64).T, 16, 1.0)
    np.testing.assert_array_equal(ids, want_ids)
    assert np.array_equal(sc, want_sc)
    for r in range(len(users)):
        assert ids[r].tolist().index(5) <= 4


# ------------------------------------------------------------------------------------------------ 6. independence
def test_a_list_does_not_depend_on_the_rest_of_the_call():
    m = _model("fm", 50, 300, 100, 2, seed=13)
    users = _user_sets(50, seed=1)[2]
    kw = dict(top_k=20, diversity=0.6, pool=KMAX)
    ids, sc = _diverse(m, users, **kw)
    for u in (int(users[0]), int(users[17]), int(users[299])):
        one_ids, one_sc = _diverse(m, [u], **kw)
        at = np.nonzero(users == u)[0]
        assert len(at) >= 1
        for r in at:  # every position of the 300-query call, repeats included
            assert np.array_equal(ids[r], one_ids[0]) and np.array_equal(sc[r], one_sc[0])
    same_ids, same_sc = _diverse(m, [7] * 300, **kw)
    assert np.all(same_ids == same_ids[0]) and np.all(same_sc == same_sc[0])
    again_ids, again_sc = _diverse(m, users, **kw)
    assert np.array_equal(again_ids, ids) and np.array_equal(again_sc, sc)


# ------------------------------------------------------------------------------------------------ 7. trs_list_ild
@pytest.mark.parametrize("D", [8, 24, 64, 100, 256])
def test_list_ild_against_the_oracle(D):
    from torchrecsys_amd import ops
    n_items = 300
    rs = np.random.RandomState(D)
    W = torch.from_numpy(rs.randn(n_items, D).astype(np.float32)).to(DEV)
    nf = ops.neighbour_fold(W, n_items, D, True)
    rows = ops.fold_views(nf, n_items, D)[0].cpu().numpy()
    for k in (1, 2, 10, KMAX):
        lists = np.stack([rs.permutation(n_items)[:k] for _ in range(33)]).astype(np.int64)
        lists[1, k // 2:] = -1  # a -1 tail
        lists[2, :] = -1        # an empty list
        lists[3, k - 1] = -1
        if k >= 10:
            lists[4, 3] = lists[4, 0]  # a repeated id: a pair of similarity 1
            lists[5, 2] = n_items      # outside the catalogue: not an entry
        got = ops.list_ild(nf, n_items, D, torch.from_numpy(lists).to(DEV)).cpu().numpy()
        want = ref.ild(lists, rows, n_items=n_items)
        assert got.dtype == np.float64 and got.shape == (33,)
        print(f"D={D} k={k}: max |ild - oracle| = {np.abs(got - want).max():.3e} (tol {ref.ild_tol(D):.3e})")
        assert np.all(np.abs(got - want) <= ref.ild_tol(D))
        assert got[2] == 0.0 and (k > 2 or got[1] == 0.0)
        if k == 1:
            assert not got.any()


# ------------------------------------------------------------------------------------------------ 8. evaluate_diversity
def _eval_users(m, exclude_seen):
    """The users evaluate_ranking() evaluates and their relevant items: distinct test users with a non-empty T_u."""
    td = m.data_processor.test_data
    tu, ti = td["user_id"].cpu().numpy(), td["pos_item_id"].cpu().numpy()
    off, items = (t.cpu().numpy() for t in m._seen_csr())
    users, rel = [], []
    for u in np.unique(tu):
        t = set(ti[tu == u].tolist())
        if exclude_seen:
            t -= set(items[off[u]:off[u + 1]].tolist())
        if t:
            users.append(int(u))
            rel.append(t)
    return np.array(users), rel


def _accuracy(lists, rel, k):
    out = []
    for R, T in zip(lists, rel):
        hits = sum(1 for x in R if x in T)
        dcg = sum(1.0 / np.log2(j + 2) for j, x in enumerate(R) if x in T)
        idcg = sum(1.0 / np.log2(j + 2) for j in range(min(k, len(T))))
        out.append((float(hits >= 1), hits / len(T), dcg / idcg))
    return np.array(out)


def NDCG_ULPS(k):
    """Relative bound, in units of 2**-52, between ndcg@k from trs_rank_metrics and from the host formula.  They cannot
    be equal to the last bit: the device's log2(3.0) is one ulp away from the correctly rounded value numpy returns
    (measured: 1 / log2(r + 2) agrees for every r < 16 but r = 1; ndcg@10 0.0593134779896982 on the device against
    0.059313477989698195 on the host), and evaluate_ranking(), which this method must agree with exactly at diversity 0,
    has the device's.  Per discount: one ulp of log2 and half an ulp of the division, < 2 units; dcg and idcg are sums of
    at most k such terms with k - 1 additions of half a unit each, so each is within 2 + k / 2 units and their quotient
    within 2 (2 + k / 2) + 1/2; the mean over users adds less than k more.  4 (k + 3) covers it."""
    return 4 * (k + 3)


@pytest.mark.parametrize("net_type,M,D", [("fm", 2, 24), ("linear", 0, 100)])
def test_evaluate_diversity_matches_host_computation(net_type, M, D):
    """Coverage, hit rate and recall equal the host computation exactly, ndcg within NDCG_ULPS (see there) and exactly
    evaluate_ranking()'s at diversity 0; novelty within 1e-9 and ild within 1e-9 plus the inner-product bound."""
    from torchrecsys_amd import ops
    k = 10
    m = _model(net_type, 80, 200, D, M, seed=6, n=4000)
    off, items = (t.cpu().numpy() for t in m._seen_csr())
    item_users = np.bincount(items, minlength=m.n_items)
    # the unit-length rows ild@k is defined on, as stored: the cosine fold of the item side
    src = m.net.item.weight.data if M == 0 else \
        ops.fold_rows(ops.item_fold(m.net.NET, m.net.tables(), m.n_items, D, DEV, m._item_meta_dev()), m.n_items)
    rows = ops.fold_views(ops.neighbour_fold(src, m.n_items, D, True), m.n_items, D)[0].cpu().numpy()
    for ex in (True, False):
        users, rel = _eval_users(m, ex)
        for lam, metric in ((0.0, "cosine"), (0.5, "cosine"), (0.7, "dot")):
            with _quiet() as buf:
                res = m.evaluate_diversity(k=k, diversity=lam, metric=metric, exclude_seen=ex)
            assert set(res) == {f"{x}@{k}" for x in ("ild", "coverage", "novelty", "hit_rate", "recall", "ndcg")} | \
                {"n_users"}
            for name in ("ild", "coverage", "novelty", "hit_rate", "recall", "ndcg"):
                assert f"|--- Testing {name}@{k}: {res[f'{name}@{k}']:.4f}" in buf.getvalue()
            lists = m.recommend_diverse(users, top_k=k, diversity=lam, metric=metric, exclude_seen=ex).numpy()
            assert res["n_users"] == len(users) > 0
            assert res[f"coverage@{k}"] == ref.coverage(lists, m.n_items)
            acc = _accuracy(lists, rel, k)
            for j, name in enumerate(("hit_rate", "recall", "ndcg")):
                print(f"{name}@{k} ex={ex} lam={lam}: {res[f'{name}@{k}']!r} (host {acc[:, j].mean()!r})")
            assert res[f"hit_rate@{k}"] == acc[:, 0].mean() and res[f"recall@{k}"] == acc[:, 1].mean()
            assert abs(res[f"ndcg@{k}"] - acc[:, 2].mean()) <= NDCG_ULPS(k) * 2.0 ** -52 * acc[:, 2].mean()
            nov, want_ild = ref.novelty(lists, item_users, m.n_users), ref.ild(lists, rows).mean()
            print(f"novelty {res[f'novelty@{k}']!r} (host {nov!r}); ild {res[f'ild@{k}']!r} (host {want_ild!r})")
            assert abs(res[f"novelty@{k}"] - nov) <= 1e-9
            assert abs(res[f"ild@{k}"] - want_ild) <= 1e-9 + ref.ild_tol(D)
            if lam == 0.0:  # plain recommend(): the accuracy columns are evaluate_ranking()'s
                with _quiet():
                    base = m.evaluate_ranking(k=k, exclude_seen=ex)
                assert base["n_users"] == res["n_users"]
                for name in ("hit_rate", "recall", "ndcg"):
                    assert base[f"{name}@{k}"] == res[f"{name}@{k}"], name
        some = users[::3]
        with _quiet():
            part = m.evaluate_diversity(k=k, diversity=0.5, exclude_seen=ex, users=some)
        lists = m.recommend_diverse(some, top_k=k, diversity=0.5, exclude_seen=ex).numpy()
        assert part["n_users"] == len(some) and part[f"coverage@{k}"] == ref.coverage(lists, m.n_items)


def test_diversity_raises_intra_list_diversity_on_a_clustered_catalogue():
    n_items, D, k = 64, 24, 10
    m = _model("linear", 60, n_items, D, 0, seed=8, n=1500)
    m.net.item.weight.data.copy_(torch.from_numpy(_clustered(n_items, D)))
    m.net.item_bias.weight.data.copy_(torch.from_numpy(
        (np.arange(n_items) % 4 == 0).astype(np.float32)[:, None] * 5))  # one cluster is everybody's favourite
    with _quiet():
        plain = m.evaluate_diversity(k=k, diversity=0.0, pool=n_items)
        mixed = m.evaluate_diversity(k=k, diversity=0.7, pool=n_items)
    assert plain["n_users"] == mixed["n_users"] > 0
    print(f"ild@{k}: {plain[f'ild@{k}']:.4f} at diversity 0, {mixed[f'ild@{k}']:.4f} at 0.7")
    assert mixed[f"ild@{k}"] >= plain[f"ild@{k}"]
    assert mixed[f"ild@{k}"] > 0.5 > plain[f"ild@{k}"]  # four clusters in every list against mostly one
