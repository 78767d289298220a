# -*- coding: utf-8 -*-
"""recommend() / evaluate_ranking(): batched top-k over the whole catalogue with seen-item masking (csrc/retrieve.hip)
against the test's own float64 numpy restatement of the scorers:
  Linear  score = <U_u, S_i> + user_bias_u + item_bias_i,               S_i = item_i + sum_m meta_m(i)
  FM      z     = <U_u, S_i> + linear_user_u + c_i,  c_i = linear_item_i + sum_m linear_meta_m(i)
                  + 1/2 (|S_i|^2 - |item_i|^2 - sum_m |meta_m(i)|^2),  score = sigmoid(z), ranked by z."""
import contextlib
import io
import os
import socket

import numpy as np
import pandas as pd
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KMAX = 128


def _quiet():
    return contextlib.redirect_stdout(io.StringIO())


def _model(net_type, n_users, n_items, D, M=0, n=None, seed=0, int_range=None, **kw):
    from torchrecsys_amd.model import TorchRecSys
    rs = np.random.RandomState(seed)
    n = n or 20 * n_users
    u = np.concatenate([np.arange(n_users), rs.randint(0, n_users, n - n_users)])
    i = np.concatenate([np.arange(n_items) % n_items, rs.randint(0, n_items, max(n - n_items, 0))])[:n]
    u = u[:len(i)]
    meta = torch.from_numpy(rs.randint(0, 5, (n_items, M))) if M else None
    with _quiet():
        torch.manual_seed(seed)
        np.random.seed(seed)
        m = TorchRecSys.from_tensors(torch.from_numpy(u), torch.from_numpy(i), n_users=n_users, n_items=n_items,
                                     item_metadata=meta, metadata_names=[f"m{j}" for j in range(M)] if M else None,
                                     n_factors=D, net_type=net_type, **kw)
    if int_range is not None:  # small integers: every fp32 score is exact in any summation order
        g = torch.Generator().manual_seed(seed + 1)
        for p in m.net.parameters():
            p.data.copy_(torch.randint(int_range[0], int_range[1], p.shape, generator=g).float())
    return m


def _tabs(m):
    net = m.net
    f = lambda t: t.detach().cpu().double().numpy()
    M = net.n_meta_tables()
    meta_ids = m.data_processor.item_meta_table
    metas = [f(l.weight) for l in net.metadata] if M else []
    S = f(net.item.weight).copy()
    for j in range(M):
        S += metas[j][meta_ids[:, j]]
    if m.net_type == "linear":
        return S, f(net.user.weight), f(net.user_bias.weight)[:, 0], f(net.item_bias.weight)[:, 0]
    I = f(net.item.weight)
    c = f(net.linear_item.weight)[:, 0] + 0.5 * ((S * S).sum(1) - (I * I).sum(1))
    for j in range(M):
        c += f(net.linear_metadata[j].weight)[meta_ids[:, j], 0] - 0.5 * (metas[j][meta_ids[:, j]] ** 2).sum(1)
    return S, f(net.user.weight), f(net.linear_user.weight)[:, 0], c


def oracle_values(m, users):
    """(n, n_items) float64 ranking values: Linear scores / FM logits z."""
    S, U, ucon, c = _tabs(m)
    return U[users] @ S.T + ucon[users][:, None] + c[None, :]


def seen_sets(m):
    off, items = (t.cpu().numpy() for t in m._seen_csr())
    return off, items


def oracle_rank(vals, users, k, off=None, items=None):
    """numpy stable descending ranking (ties by ascending id), seen items excluded, -1 padding."""
    n_items = vals.shape[1]
    out = np.full((len(users), k), -1, np.int64)
    for r, u in enumerate(users):
        v = vals[r].copy()
        ok = np.ones(n_items, bool)
        if off is not None:
            ok[items[off[u]:off[u + 1]]] = False
        cand = np.nonzero(ok)[0]
        order = cand[np.lexsort((cand, -v[cand]))][:k]
        out[r, :len(order)] = order
    return out


def _check_exact(m, users, k, exclude_seen):
    ids, sc = m.recommend(users, top_k=k, exclude_seen=exclude_seen, return_scores=True)
    kk = min(k, m.n_items)
    assert ids.shape == (len(users), kk) and ids.dtype == torch.int64 and sc.dtype == torch.float32
    vals = oracle_values(m, users)
    off, items = seen_sets(m) if exclude_seen else (None, None)
    want = oracle_rank(vals, users, kk, off, items)
    np.testing.assert_array_equal(ids.numpy(), want)
    sc = sc.numpy()
    pad = want < 0
    assert np.all(np.isneginf(sc[pad]))
    if m.net_type == "linear":
        got_v = np.take_along_axis(vals, np.where(pad, 0, want), 1).astype(np.float32)
        assert np.array_equal(sc[~pad], got_v[~pad])
    else:  # FM: the sigmoid of the exact z, as the scoring kernels compute it
        for r, u in enumerate(users):
            row = m.net.score_all_items(int(u), m._item_meta_dev()).cpu().numpy()
            sel = want[r][want[r] >= 0]
            assert np.array_equal(sc[r][:len(sel)], row[sel])


def _users(n_users, n, seed):
    rs = np.random.RandomState(seed)
    us = rs.randint(0, n_users, n)
    us[: n // 4] = us[n // 4: 2 * (n // 4)]  # duplicates
    return us


CASES = ([(D, 0, 333) for D in (1, 7, 16, 24, 64, 100, 128, 256)] + [(16, M, 333) for M in (1, 3)] +
         [(7, 1, n) for n in (1, 127, 128, 129, 100_003)])


@pytest.mark.parametrize("net_type", ["linear", "fm"])
@pytest.mark.parametrize("D,M,n_items", CASES)
def test_exact_arithmetic_ranking_is_bit_exact(net_type, D, M, n_items):
    n_users = 70
    m = _model(net_type, n_users, n_items, D, M, n=max(40 * n_users, 3 * n_items) if n_items < 1000 else 60_000,
               seed=D + M + n_items, int_range=(-3, 4))
    users = _users(n_users, 45, D)
    for k in sorted({1, 10, 64, KMAX, KMAX + 1, n_items}):
        for ex in (True, False):
            if k > KMAX and n_items > 1000 and not ex:
                continue  # the generic path is the same code with and without masking
            _check_exact(m, users, k, ex)


@pytest.mark.parametrize("net_type", ["linear", "fm"])
def test_recommend_equals_predict_many_without_masking(net_type):
    m = _model(net_type, 60, 300, 2, 0, seed=4, int_range=(-1, 2))  # |logit| <= 6: no sigmoid ties
    users = _users(60, 37, 2)
    for k in (1, 10, 100, 300):
        got = m.recommend(users, top_k=k, exclude_seen=False)
        assert torch.equal(got, m.predict_many(users, top_k=k))


@pytest.mark.parametrize("net_type,M", [("linear", 0), ("fm", 0), ("fm", 2)])
def test_random_weights_tolerance_contract(net_type, M):
    n_users, n_items = 300, 5000
    m = _model(net_type, n_users, n_items, 64, M, n=60_000, seed=9)
    users = np.arange(0, n_users, 3)
    vals = oracle_values(m, users)
    off, items = seen_sets(m)
    out_units = (lambda z: 1.0 / (1.0 + np.exp(-z))) if net_type == "fm" else (lambda z: z)
    tau = 1e-5 * max(1.0, np.abs(out_units(vals)).max())
    for k in (10, 100):
        ids, sc = m.recommend(users, top_k=k, return_scores=True)
        ids, sc = ids.numpy(), sc.numpy().astype(np.float64)
        for r, u in enumerate(users):
            seen = set(items[off[u]:off[u + 1]].tolist())
            n_cand = n_items - len(seen)
            row = ids[r]
            got = row[row >= 0]
            assert len(got) == min(k, n_cand) and np.all(row[len(got):] == -1)
            assert len(set(got.tolist())) == len(got) and not (set(got.tolist()) & seen)
            assert np.all((got >= 0) & (got < n_items))
            s = sc[r][:len(got)]
            assert np.all(np.diff(s) <= 0)
            ov = out_units(vals[r])
            assert np.all(np.abs(s - ov[got]) <= tau)
            mask = np.ones(n_items, bool)
            mask[list(seen)] = False
            unseen = ov[mask]
            kth = np.sort(unseen)[::-1][len(got) - 1]
            assert np.all(ov[got] >= kth - 2 * tau)
            rest = mask.copy()
            rest[got] = False
            if rest.any():
                assert ov[rest].max() <= s.min() + 2 * tau


def test_edge_cases_seen_everything_remap_unknown_and_determinism():
    from torchrecsys_amd.model import TorchRecSys
    n_items = 50
    rs = np.random.RandomState(1)
    # user 0 has every item 10 times, user 1 all but items {3, 17, 40}: with an 80/20 split they stay seen in train
    u = [0] * (10 * n_items) + [1] * (10 * (n_items - 3))
    i = list(range(n_items)) * 10 + [x for x in range(n_items) if x not in (3, 17, 40)] * 10
    u += rs.randint(2, 40, 3000).tolist()
    i += rs.randint(0, n_items, 3000).tolist()
    with _quiet():
        torch.manual_seed(0)
        m = TorchRecSys.from_tensors(torch.tensor(u), torch.tensor(i), n_users=40, n_items=n_items, n_factors=16,
                                     net_type="fm")
    off, items = seen_sets(m)
    assert off[1] - off[0] == n_items and off[2] - off[1] == n_items - 3
    for k in (10, KMAX + 1):
        ids = m.recommend([0, 1, 5], top_k=k)
        kk = min(k, n_items)
        assert ids.shape == (3, kk)
        assert torch.all(ids[0] == -1)
        assert sorted(ids[1, :3].tolist()) == [3, 17, 40] and torch.all(ids[1, 3:] == -1)
    a = m.recommend(list(range(40)), top_k=20, return_scores=True)
    b = m.recommend(list(range(40)), top_k=20, return_scores=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(IndexError):
        m.recommend([0, 40], top_k=5)
    assert m.recommend([], top_k=5).shape == (0, 5) and m.recommend([1], top_k=0).shape == (1, 0)

    # remapped ingest: original ids in, original ids out
    raw_u = torch.arange(300) * 7 + 3
    raw_i = torch.arange(120) * 5 + 11
    uu = np.concatenate([np.arange(300), rs.randint(0, 300, 3000)])
    ii = np.concatenate([np.arange(120), rs.randint(0, 120, 3180)])[:len(uu)]
    with _quiet():
        torch.manual_seed(2)
        r = TorchRecSys.from_tensors(raw_u[uu], raw_i[ii], n_factors=16, net_type="linear", remap_ids=True)
    q = [3, 10, 73, 2096]
    dense = [(x - 3) // 7 for x in q]
    got = r.recommend(torch.tensor(q), top_k=15)
    off, items = seen_sets(r)
    want = oracle_rank(oracle_values(r, dense), dense, 15, off, items)
    assert torch.equal(got, torch.from_numpy(np.where(want >= 0, raw_i.numpy()[np.maximum(want, 0)], -1)))
    with pytest.raises(IndexError):
        r.recommend([4], top_k=5)


def test_mlp_generic_path_equals_masked_score_rows():
    m = _model("mlp", 50, 400, 16, 1, seed=3, hidden_layers=[32, 16])
    users = _users(50, 21, 5)
    off, items = seen_sets(m)
    meta = m._item_meta_dev()
    for ex in (True, False):
        ids, sc = m.recommend(users, top_k=25, exclude_seen=ex, return_scores=True)
        for r, u in enumerate(users):
            row = m.net.score_all_items(int(u), meta).cpu().numpy()
            v = row.astype(np.float64)
            want = oracle_rank(v[None], [u], 25, off if ex else None, items)[0]
            np.testing.assert_array_equal(ids[r].numpy(), want)
            sel = want >= 0
            assert np.array_equal(sc[r].numpy()[sel], row[want[sel]])


def _host_metrics(m, rec_ids, users, k, exclude_seen):
    """float64 per-user (hit, recall, ndcg) from the test split, the train seen sets and a top-k list."""
    td = m.data_processor.test_data
    tu, ti = td["user_id"].cpu().numpy(), td["pos_item_id"].cpu().numpy()
    off, items = seen_sets(m)
    out = []
    for r, u in enumerate(users):
        T = set(ti[tu == u].tolist())
        if exclude_seen:
            T -= set(items[off[u]:off[u + 1]].tolist())
        if not T:
            continue
        R = rec_ids[r]
        hits = sum(1 for x in R if x in T)
        dcg = sum(1.0 / np.log2(j + 2) for j, x in enumerate(R) if x in T)
        idcg = sum(1.0 / np.log2(j + 2) for j in range(min(k, len(T))))
        out.append((float(hits >= 1), hits / len(T), dcg / idcg))
    return np.array(out)


@pytest.mark.parametrize("net_type,k", [("linear", 10), ("fm", 5), ("fm", KMAX + 2), ("mlp", 10)])
def test_evaluate_ranking_matches_host_computation(net_type, k):
    kw = {"hidden_layers": [16]} if net_type == "mlp" else {}
    ir = None if net_type == "mlp" else (-3, 4)
    m = _model(net_type, 80, 200, 8, 0, n=4000, seed=6, int_range=ir, **kw)
    for ex in (True, False):
        with _quiet() as buf:
            res = m.evaluate_ranking(k=k, exclude_seen=ex)
        users = np.unique(m.data_processor.test_data["user_id"].cpu().numpy())
        rec = m.recommend(users, top_k=k, exclude_seen=ex).numpy()
        host = _host_metrics(m, rec, users, k, ex)
        assert res["n_users"] == len(host) > 0
        for j, name in enumerate(("hit_rate", "recall", "ndcg")):
            np.testing.assert_allclose(res[f"{name}@{k}"], host[:, j].mean(), rtol=1e-12, atol=0)
        if ir is not None:  # exact tables: the oracle ranking's metrics
            off, items = seen_sets(m)
            orc = oracle_rank(oracle_values(m, users), users, min(k, m.n_items), off if ex else None, items)
            np.testing.assert_allclose(_host_metrics(m, orc, users, k, ex).mean(0), host.mean(0), rtol=1e-12, atol=0)
        # hit rate as a per-row definition over targets padded with -1
        td = m.data_processor.test_data
        tu, ti = td["user_id"].cpu().numpy(), td["pos_item_id"].cpu().numpy()
        off, items = seen_sets(m)
        rows = []
        for u in users:
            t = set(ti[tu == u].tolist()) - (set(items[off[u]:off[u + 1]].tolist()) if ex else set())
            rows.append(sorted(t))
        width = max(len(t) for t in rows)
        targets = np.full((len(users), width), -1)
        for r, t in enumerate(rows):
            targets[r, :len(t)] = t
        keep = np.array([len(t) > 0 for t in rows])
        hr = np.mean([np.isin(rec[r][rec[r] >= 0], targets[r][targets[r] >= 0]).any() for r in np.nonzero(keep)[0]])
        np.testing.assert_allclose(res[f"hit_rate@{k}"], hr, rtol=1e-12, atol=0)
        assert f"|--- Testing hit_rate@{k}:" in buf.getvalue()


def test_fullsize_c2_sampled_users_tolerance():
    """c2 shape (FM, 1M users x 100K items, D = 64) with seen masking: 512 sampled users against the float64 oracle."""
    from torchrecsys_amd.model import TorchRecSys
    n_users, n_items, D, n = 1_000_000, 100_000, 64, 10_000_000
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    users = torch.randint(0, n_users, (n,), device=DEV, dtype=torch.int32, generator=g)
    items = torch.randint(0, n_items, (n,), device=DEV, dtype=torch.int32, generator=g)
    users[0], items[0] = n_users - 1, n_items - 1
    with _quiet():
        torch.manual_seed(11)
        m = TorchRecSys.from_tensors(users, items, n_users=n_users, n_items=n_items, n_factors=D, net_type="fm",
                                     rng="device", split="device", seed=5)
    del users, items
    q = np.sort(np.random.RandomState(0).choice(n_users, 512, replace=False))
    vals = oracle_values(m, q)
    off, its = seen_sets(m)
    z_tau = 1e-5 * np.abs(vals).max()
    for k in (10, 100):
        ids, sc = m.recommend(q, top_k=k, return_scores=True)
        ids, sc = ids.numpy(), sc.numpy().astype(np.float64)
        assert np.all(ids >= 0)
        for r, u in enumerate(q):
            seen = its[off[u]:off[u + 1]]
            got = ids[r]
            assert len(set(got.tolist())) == k and not np.isin(got, seen).any()
            assert np.all(np.diff(sc[r]) <= 0)
            z = vals[r]
            assert np.all(np.abs(sc[r] - 1.0 / (1.0 + np.exp(-z[got]))) <= 1e-6)
            mask = np.ones(n_items, bool)
            mask[seen] = False
            kth = np.partition(z[mask], -k)[-k]
            assert np.all(z[got] >= kth - 2 * z_tau)
            mask[got] = False
            assert z[mask].max() <= z[got].min() + 2 * z_tau


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
        with _quiet():
            model = TorchRecSys(_df(), "user", "item", n_factors=16, net_type="fm", dynamic_neg_sampling=True,
                                rng="device", seed=3)
            ret[rank] = model.evaluate_ranking(k=10)
            model.dp_partition = "contiguous"
            try:
                model.evaluate_ranking(k=10)
                ret[f"err{rank}"] = False
            except ValueError:
                ret[f"err{rank}"] = True
    finally:
        dist.destroy_process_group()


def test_two_ranks_evaluate_ranking_equals_single_process():
    from torchrecsys_amd.model import TorchRecSys
    torch.manual_seed(100)
    np.random.seed(5)
    with _quiet():
        single = TorchRecSys(_df(), "user", "item", n_factors=16, net_type="fm", dynamic_neg_sampling=True,
                             rng="device", seed=3)
        want = single.evaluate_ranking(k=10)
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_rank_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
    for r in (0, 1):
        got = ret[r]
        assert got["n_users"] == want["n_users"]
        for key in ("hit_rate@10", "recall@10", "ndcg@10"):
            np.testing.assert_allclose(got[key], want[key], rtol=1e-12, atol=0)
        assert ret[f"err{r}"]
