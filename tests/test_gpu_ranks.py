# -*- coding: utf-8 -*-
"""rank_items() / evaluate_ranks() on the GPU (csrc/retrieve.hip rank_values_kernel / rank_count_kernel) against the
float64 reference of tests/ranks_ref.py: rank(u, t) = position of t in np.lexsort((ids, -vals)) over C_u + {t}."""
import os
import socket

import numpy as np
import pandas as pd
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ranks_ref as ref

pytestmark = pytest.mark.gpu

KMAX = 128


def _users(n_users, n, seed):
    rs = np.random.RandomState(seed)
    us = rs.randint(0, n_users, n)
    us[: n // 4] = us[n // 4: 2 * (n // 4)]  # repeats
    return us


def _want(m, vals, users, targets, exclude_seen):
    """Reference ranks of targets[r] (an array per queried user) — vals: ref.values(m, users)."""
    off, items = ref.seen_sets(m)
    return [ref.ranks_of(vals[r], targets[r], items[off[u]:off[u + 1]] if exclude_seen else None)
            for r, u in enumerate(users)]


def _rank(m, users, targets, exclude_seen, **kw):
    """rank_items over (users[r], every entry of targets[r]), split back per user."""
    uu = np.concatenate([np.full(len(t), u) for u, t in zip(users, targets)])
    got = m.rank_items(uu, np.concatenate(targets), exclude_seen=exclude_seen, **kw)
    cuts = np.cumsum([len(t) for t in targets])[:-1]
    if isinstance(got, tuple):
        return np.split(got[0].numpy(), cuts), np.split(got[1].numpy(), cuts)
    assert got.dtype == torch.int64 and got.shape == (len(uu),)
    return np.split(got.numpy(), cuts)


CASES = [(1, 0, 333), (7, 0, 333), (16, 2, 333), (24, 0, 333), (64, 0, 333), (100, 0, 333), (256, 0, 333), (7, 1, 1),
         (7, 1, 127), (7, 1, 128), (7, 1, 129), (7, 1, 100_003)]


@pytest.mark.parametrize("net_type", ["linear", "fm"])
@pytest.mark.parametrize("D,M,n_items", CASES)
def test_exact_arithmetic_ranks_are_bit_exact(net_type, D, M, n_items):
    n_users = 70
    m = ref.build_model(net_type, n_users, n_items, D, M,
                        n=max(40 * n_users, 3 * n_items) if n_items < 1000 else 60_000, seed=D + M + n_items,
                        int_range=(-3, 4))
    users = _users(n_users, 45, D)
    vals = ref.values(m, users)
    off, items = ref.seen_sets(m)
    if n_items <= 333:
        # every item a target of every queried user: many rows per user, seen items among the targets
        targets = [np.arange(n_items)] * len(users)
        for ex in (True, False):
            got = _rank(m, users, targets, ex)
            want = _want(m, vals, users, targets, ex)
            for r, u in enumerate(users):
                np.testing.assert_array_equal(got[r], want[r])
                cand = np.ones(n_items, bool)
                if ex:
                    cand[items[off[u]:off[u + 1]]] = False
                assert np.array_equal(np.sort(got[r][cand]), np.arange(cand.sum()))  # a permutation over C_u
        return
    # few rows against many tiles (several item splits): 2 000 sampled targets per user plus the user's top-128
    rs = np.random.RandomState(5)
    for ex in (True, False):
        top = m.recommend(users, top_k=KMAX, exclude_seen=ex).numpy()
        targets = [np.unique(np.concatenate([rs.choice(n_items, 2000, replace=False), top[r]]))
                   for r in range(len(users))]
        got = _rank(m, users, targets, ex)
        want = _want(m, vals, users, targets, ex)
        for r in range(len(users)):
            np.testing.assert_array_equal(got[r], want[r])
    # many user tiles, a single split: 2 000 users (with repeats) x 2 targets
    many = rs.randint(0, n_users, 2000)
    pair_t = rs.randint(0, n_items, (2000, 2))
    got = m.rank_items(np.repeat(many, 2), pair_t.reshape(-1)).numpy().reshape(2000, 2)
    all_vals = ref.values(m, np.arange(n_users))
    want = {}
    for u in np.unique(many):
        ts = np.unique(pair_t[many == u])
        want[u] = dict(zip(ts.tolist(), ref.ranks_of(all_vals[u], ts, items[off[u]:off[u + 1]]).tolist()))
    for j, u in enumerate(many):
        assert got[j].tolist() == [want[u][int(t)] for t in pair_t[j]]


RANDOM = [("linear", 0), ("fm", 0), ("fm", 2)]
_models = {}


def _random_model(net_type, M):
    """Default-initialised weights, D = 64, 300 users x 5 000 items; built once per scorer, never changed."""
    if (net_type, M) not in _models:
        m = ref.build_model(net_type, 300, 5000, 64, M, n=60_000, seed=9)
        _models[net_type, M] = (m, ref.values(m, np.arange(300)))
    return _models[net_type, M]


@pytest.mark.parametrize("net_type,M", RANDOM)
def test_ranks_are_consistent_with_recommend_on_random_weights(net_type, M):
    m, _ = _random_model(net_type, M)
    off, items = ref.seen_sets(m)
    rs = np.random.RandomState(2)
    for users in (np.arange(300), np.arange(5, 38), np.array([299])):  # 33 and 1: a partial user tile
        for ex in (True, False):
            ids, sc = m.recommend(users, top_k=KMAX, exclude_seen=ex, return_scores=True)
            ids, sc = ids.numpy(), sc.numpy()
            assert np.all(ids >= 0)
            got, val = _rank(m, users, list(ids), ex, return_scores=True)
            for r in range(len(users)):
                assert np.array_equal(got[r], np.arange(KMAX)), (users[r], ex)
                assert val[r].dtype == np.float32 and np.array_equal(val[r], sc[r])  # bit-equal to recommend()'s
            others = []  # 200 other candidates per user
            for r, u in enumerate(users):
                rest = np.setdiff1d(np.arange(5000), ids[r])
                if ex:
                    rest = np.setdiff1d(rest, items[off[u]:off[u + 1]])
                others.append(rs.choice(rest, 200, replace=False))
            for r, g in enumerate(_rank(m, users, others, ex)):
                assert np.all(g >= KMAX)


@pytest.mark.parametrize("net_type,M", RANDOM)
def test_every_rank_lies_in_the_float64_interval(net_type, M):
    """tau = 1e-5 max(1, max|v|): rank in [#{v_i > v_t + 2 tau}, #{v_i >= v_t - 2 tau}] over C_u without t, every pair."""
    m, vals = _random_model(net_type, M)
    off, items = ref.seen_sets(m)
    users = np.arange(0, 300, 3)
    tau = 1e-5 * max(1.0, np.abs(vals).max())
    rs = np.random.RandomState(4)
    for ex in (True, False):
        targets = [np.sort(rs.choice(5000, 60, replace=False)) for _ in users]
        if ex:  # among them a few seen items
            targets = [np.unique(np.concatenate([t, items[off[u]:off[u + 1]][:3]])) for t, u in zip(targets, users)]
        got = _rank(m, users, targets, ex)
        for r, u in enumerate(users):
            v = vals[u]
            cand = np.ones(5000, bool)
            if ex:
                cand[items[off[u]:off[u + 1]]] = False
            for t, g in zip(targets[r], got[r]):
                c = cand.copy()
                c[t] = False
                lo, hi = np.sum(v[c] > v[t] + 2 * tau), np.sum(v[c] >= v[t] - 2 * tau)
                assert lo <= g <= hi, (u, t, g, lo, hi)


def test_edges_seen_everything_empty_unknown_remap_determinism_and_untouched_parameters():
    from torchrecsys_amd.model import TorchRecSys
    n_items = 50
    rs = np.random.RandomState(1)
    # user 0 has every item but item 17 in train (10 times each: they stay in train under an 80/20 split)
    u = [0] * (10 * (n_items - 1)) + rs.randint(1, 40, 3000).tolist()
    i = [x for x in range(n_items) if x != 17] * 10 + rs.randint(0, n_items, 3000).tolist()
    with ref.quiet():
        torch.manual_seed(0)
        m = TorchRecSys.from_tensors(torch.tensor(u), torch.tensor(i), n_users=40, n_items=n_items, n_factors=16,
                                     net_type="fm")
    off, items = ref.seen_sets(m)
    assert off[1] - off[0] == n_items - 1
    before = [p.detach().clone() for p in m.net.parameters()]
    assert m.rank_items([0], [17]).tolist() == [0]  # its only candidate
    got = m.rank_items([0] * n_items, list(range(n_items)))
    assert set(got.tolist()) <= {0, 1} and got[17] == 0  # a seen target competes with item 17 alone
    vals = ref.values(m, [0])[0]
    assert got.tolist() == ref.ranks_of(vals, np.arange(n_items), items[off[0]:off[1]]).tolist()
    e = m.rank_items([], [])
    assert e.shape == (0,) and e.dtype == torch.int64
    for bad in (([0, 40], [1, 1]), ([0, 1], [1, n_items]), ([-1], [0])):
        with pytest.raises(IndexError):
            m.rank_items(*bad)
    with pytest.raises(ValueError):
        m.rank_items([0, 1], [1])
    uu, ii = rs.randint(0, 40, 500), rs.randint(0, n_items, 500)
    a = m.rank_items(uu, ii, return_scores=True)
    b = m.rank_items(uu, ii, return_scores=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for p, q in zip(m.net.parameters(), before):
        assert torch.equal(p.detach(), q)

    # remapped ingest with sparse original ids: original ids in
    raw_u = torch.arange(300) * 7 + 3
    raw_i = torch.arange(120) * 5 + 11
    du = np.concatenate([np.arange(300), rs.randint(0, 300, 3000)])
    di = np.concatenate([np.arange(120), rs.randint(0, 120, 3180)])[:len(du)]
    with ref.quiet():
        torch.manual_seed(2)
        r = TorchRecSys.from_tensors(raw_u[du], raw_i[di], n_factors=16, net_type="linear", remap_ids=True)
    g = torch.Generator().manual_seed(3)
    for p in r.net.parameters():  # exact arithmetic: the reference order is the kernel's
        p.data.copy_(torch.randint(-3, 4, p.shape, generator=g).float())
    q_u, q_i = np.array([0, 1, 10, 299, 10]), np.array([5, 119, 0, 64, 7])
    got = r.rank_items(raw_u[q_u], raw_i[q_i])
    off, items = ref.seen_sets(r)
    vals = ref.values(r, q_u)
    want = [int(ref.ranks_of(vals[j], [q_i[j]], items[off[a]:off[a + 1]])[0]) for j, a in enumerate(q_u)]
    assert got.tolist() == want
    rec = r.recommend(raw_u[q_u], top_k=120).numpy()
    for j in range(len(q_u)):
        if q_i[j] not in items[off[q_u[j]]:off[q_u[j] + 1]]:
            assert rec[j][int(got[j])] == int(raw_i[q_i[j]])  # consistent with recommend() in original ids
    with pytest.raises(IndexError):
        r.rank_items([4], [11])
    with pytest.raises(IndexError):
        r.rank_items([3], [12])


def test_mlp_generic_path_equals_the_position_in_recommend():
    m = ref.build_model("mlp", 40, 200, 16, 1, seed=3, hidden_layers=[32, 16])
    users = _users(40, 17, 5)
    off, items = ref.seen_sets(m)
    for ex in (True, False):
        rec = m.recommend(users, top_k=200, exclude_seen=ex).numpy()
        targets = [np.arange(200)] * len(users)
        got, val = _rank(m, users, targets, ex, return_scores=True)
        for r, u in enumerate(users):
            listed = rec[r][rec[r] >= 0]
            assert np.array_equal(got[r][listed], np.arange(len(listed)))
            row = m.net.score_all_items(int(u), m._item_meta_dev()).cpu().numpy()
            assert np.array_equal(val[r], row)
            seen = np.setdiff1d(np.arange(200), listed)  # a seen target: its position among C_u + {t}
            want = ref.ranks_of(row.astype(np.float64), seen, items[off[u]:off[u + 1]] if ex else None)
            assert np.array_equal(got[r][seen], want)


def test_wide_tables_take_the_generic_path():
    m = ref.build_model("linear", 30, 150, 260, 0, seed=8, int_range=(-3, 4))  # n_factors > TRS_RETRIEVE_DMAX
    users = np.arange(0, 30, 2)
    vals = ref.values(m, users)
    for ex in (True, False):
        targets = [np.arange(150)] * len(users)
        got = _rank(m, users, targets, ex)
        want = _want(m, vals, users, targets, ex)
        for r in range(len(users)):
            np.testing.assert_array_equal(got[r], want[r])


ALL = ("auc", "mrr", "mean_rank", "hit_rate", "precision", "recall", "ndcg", "map")


def _reference_metrics(m, ks, exclude_seen):
    rel = ref.relevant_items(m, exclude_seen)
    users = np.array(sorted(rel))
    vals = ref.values(m, users)
    off, items = ref.seen_sets(m)
    per = []
    for r, u in enumerate(users):
        seen = items[off[u]:off[u + 1]] if exclude_seen else None
        n_c = m.n_items - (len(seen) if exclude_seen else 0)
        if n_c == len(rel[u]):
            continue
        per.append(ref.user_metrics(ref.ranks_of(vals[r], rel[u], seen), n_c, ks, m.n_items))
    return ref.mean_metrics(per), len(per)


@pytest.mark.parametrize("net_type", ["linear", "fm"])
def test_evaluate_ranks_equals_the_reference_and_evaluate_ranking(net_type):
    m = ref.build_model(net_type, 300, 500, 8, 0, n=20_000, seed=6, int_range=(-3, 4))
    ks = (1, 10, KMAX, 200, 700)  # 200: above the fused top-k's limit; 700 > n_items
    for ex in (True, False):
        with ref.quiet() as buf:
            res = m.evaluate_ranks(k=ks, metrics=ALL, exclude_seen=ex)
        want, n = _reference_metrics(m, ks, ex)
        assert res["n_users"] == n > 250
        assert set(res) == set(want) | {"n_users"}
        for name, v in want.items():
            assert abs(res[name] - v) <= 1e-12, (name, res[name], v)
            assert f"|--- Testing {name}: {res[name]:.4f}" in buf.getvalue()
        for k in (10, KMAX):
            with ref.quiet():
                old = m.evaluate_ranking(k=k, exclude_seen=ex)
            assert old["n_users"] == n
            for name in ("hit_rate", "recall", "ndcg"):
                assert abs(res[f"{name}@{k}"] - old[f"{name}@{k}"]) <= 1e-12, (name, k)
    with ref.quiet():
        one = m.evaluate_ranks(k=10, metrics=("recall",), users=[3, 5, 3, 8])
    assert set(one) == {"recall@10", "n_users"} and one["n_users"] <= 3
    with pytest.raises(ValueError):
        m.evaluate_ranks(metrics=("auc", "nope"))


def test_evaluate_ranks_mlp_matches_evaluate_ranking():
    m = ref.build_model("mlp", 80, 200, 8, 0, n=4000, seed=6, hidden_layers=[16])
    for ex in (True, False):
        with ref.quiet():
            res = m.evaluate_ranks(k=10, metrics=("hit_rate", "recall", "ndcg"), exclude_seen=ex)
            old = m.evaluate_ranking(k=10, exclude_seen=ex)
        assert res["n_users"] == old["n_users"] > 0
        for name in ("hit_rate", "recall", "ndcg"):
            assert abs(res[f"{name}@10"] - old[f"{name}@10"]) <= 1e-12, name


# ------------------------------------------------------------------------------------------------ two ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _df():
    rs = np.random.RandomState(0)
    n_u, n_i, n = 200, 60, 6000
    return pd.DataFrame({"user": np.concatenate([np.arange(n_u), rs.randint(0, n_u, n - n_u)]),
                         "item": np.concatenate([np.arange(n_i), rs.randint(0, n_i, n - n_i)])})


def _rank_worker(rank, world, port, ret):
    os.environ["TRS_FLAG_ONE_LAUNCH"] = "0"
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from torchrecsys_amd.model import TorchRecSys
        torch.manual_seed(100)
        np.random.seed(5)
        with ref.quiet():
            model = TorchRecSys(_df(), "user", "item", n_factors=16, net_type="fm", dynamic_neg_sampling=True,
                                rng="device", seed=3)
            ret[rank] = model.evaluate_ranks(k=(1, 10), metrics=ALL)
            model.dp_partition = "contiguous"
            try:
                model.evaluate_ranks(k=10)
                ret[f"err{rank}"] = False
            except ValueError:
                ret[f"err{rank}"] = True
    finally:
        dist.destroy_process_group()


def test_two_ranks_evaluate_ranks_equals_single_process():
    from torchrecsys_amd.model import TorchRecSys
    torch.manual_seed(100)
    np.random.seed(5)
    with ref.quiet():
        single = TorchRecSys(_df(), "user", "item", n_factors=16, net_type="fm", dynamic_neg_sampling=True,
                             rng="device", seed=3)
        want = single.evaluate_ranks(k=(1, 10), metrics=ALL)
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_rank_worker, args=(2, _free_port(), ret), nprocs=2, join=True)  # fresh child processes
    for r in (0, 1):
        got = ret[r]
        assert got["n_users"] == want["n_users"] > 0
        for key, v in want.items():
            np.testing.assert_allclose(got[key], v, rtol=1e-12, atol=0)
        assert ret[f"err{r}"]
