# -*- coding: utf-8 -*-
"""fit_ease() / ops.ease_gram / ease_invert / ease_weights / ease_scores on the GPU against the numpy restatement
tests/ease_ref.py, which tests/test_ease_host.py ties to the real reference's output (tests/golden/g5_ease.npz).

Shapes: n_items in {1, 2, 63, 64, 65, 200, 520} (the solver's block is 64: one block with padding, exactly one, one item
more than one, four blocks with padding, nine blocks); n_users 40 / 150 / 300 / 600; lambda 0.5, at 520 also 0.01 and 500.
Inputs: ease_ref.histories(n_users, n_items, seed=n_items): lengths 0, 1, 2, 63, 64, 65, n_items, then random 0..20.

1. Gram matrix exact; 2. inverse by its residual; 3. weights; 4. score rows bit for bit; 5. the model surface position
for position, and against the reference's own scores; 6. determinism and persistence; 7. refusals.

Tolerances, measured on the CPU restatement, never on the kernel (ease_ref.blocked_inverse with block sizes 16, 64, 128
against numpy.linalg.inv on exactly these inputs):

    n_items lambda  cond(A)  max|A P - I| numpy   blocked (16 / 64 / 128)        blocked / numpy   max|B_blk - B_inv|
    1       0.5     1        6.4e-17              1.9e-16                        3.0               0
    2       0.5     50       1.6e-15              1.8e-15                        1.1               1.1e-16
    63      0.5     279      1.0e-15              2.1e-15 / 1.7e-15 / 1.8e-15    1.7 .. 2.0        1.5e-15
    64      0.5     251      1.2e-15              2.2e-15 / 2.0e-15 / 1.9e-15    1.6 .. 1.8        1.1e-15
    65      0.5     254      1.2e-15              2.1e-15 / 2.1e-15 / 1.9e-15    1.5 .. 1.7        1.2e-15
    200     0.5     652      2.1e-15              3.8e-15 / 3.9e-15 / 4.6e-15    1.8 .. 2.2        2.5e-15
    520     0.5     1.4e3    4.7e-15              1.1e-14 / 7.0e-15 / 6.4e-15    1.4 .. 2.4        4.4e-15
    520     0.01    2.7e4    2.8e-14              1.9e-14 / 2.3e-14 / 3.2e-14    0.7 .. 1.1        6.7e-14
    520     500     2.4      1.1e-15              2.2e-15 / 2.3e-15 / 2.6e-15    2.0 .. 2.3        3.5e-17

Residual bar (test 2): 8 x numpy's residual on the same matrix.  The blocked route stays within 3.1 x; the kernel's GEMM
sums in yet another order (MFMA K slices) and the explicit L^-1 carries cond(A) with other constants than LU.
TOL_B (test 3): 8 x the largest |B_blocked - B_inv| over the three block sizes on the same input, computed by the test
from the restatement; the fp32 rounding term 2^-23 |B| covers the rest (|B| <= 1.1; float32(B_blocked) was within 1 ulp
of float32(B_inv) everywhere).
The kernel, on one MI355X: residual 1.07 .. 3.03 x numpy's over the nine cases (3.03 at n = 1, 2.93 at n = 520 with
lambda = 500); B equal to float32(B64) in eight cases and 4.7e-10 off (inside the fp32 rounding term) at lambda = 0.01."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

import ease_ref as ref
from conftest import load_golden
from torchrecsys_amd import ops
from torchrecsys_amd.evaluate import ranks as rank_eval
from torchrecsys_amd.model import TorchRecSys

pytestmark = pytest.mark.gpu

NB = 64
CASES = [(1, 0.5), (2, 0.5), (63, 0.5), (64, 0.5), (65, 0.5), (200, 0.5), (520, 0.5), (520, 0.01), (520, 500.0)]
IDS = ["n%d_l%g" % c for c in CASES]
RESIDUAL_BAR = 8.0


def n_users_for(n):
    return 40 if n <= 2 else 150 if n <= 65 else 300 if n == 200 else 600


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _csr(lists):
    off, ids = ref.csr(lists)
    return _gpu(off), _gpu(ids)


@functools.lru_cache(maxsize=None)
def lists_of(n):
    return ref.histories(n_users_for(n), n, n)


@functools.lru_cache(maxsize=None)
def host(n, lam):
    """The float64 reference of one case, computed once: A, numpy's inverse and its residual, B, TOL_B."""
    A = ref.gram(ref.dense_x(lists_of(n), n), lam)
    P = np.linalg.inv(A)
    B = ref.weights(P)
    tol_b = 8.0 * max(np.abs(ref.weights(ref.blocked_inverse(A, nb)) - B).max() for nb in (16, 64, 128))
    return dict(A=A, P=P, res=ref.residual(A, P), B=B, tol_b=tol_b)


@functools.lru_cache(maxsize=None)
def device(n, lam):
    """The three launchers on one case, run once: padded A and P as numpy, B on the GPU and as numpy."""
    err = torch.zeros(1, dtype=torch.int32, device=_dev())
    A = ops.ease_gram(_csr(lists_of(n)), n, lam, err)
    A_np = A.cpu().numpy().copy()
    P = ops.ease_invert(A, err)
    B = ops.ease_weights(P, n)
    assert int(err.item()) == 0
    return dict(A=A_np, P=P.cpu().numpy(), B=B, B_np=B.cpu().numpy())


def _model(lists, n_items, seed=0, **kw):
    """A model whose train split is exactly `lists` (split_ratio 1), the pairs in a shuffled order."""
    users = np.repeat(np.arange(len(lists)), [len(v) for v in lists])
    items = np.concatenate(lists)
    p = np.random.RandomState(seed).permutation(users.size)
    with contextlib.redirect_stdout(io.StringIO()):
        return TorchRecSys.from_tensors(torch.from_numpy(users[p]), torch.from_numpy(items[p]), n_users=len(lists),
                                        n_items=n_items, net_type='ease', split_ratio=1.0, **kw)


# ------------------------------------------------------------------------------------------------ 1. Gram matrix
@pytest.mark.parametrize("n,lam", CASES, ids=IDS)
def test_gram_matrix_is_exact_padding_included(n, lam):
    got = device(n, lam)["A"]
    nbar = -(-n // NB) * NB
    assert got.shape == (nbar, nbar)
    assert np.array_equal(got, ref.padded(host(n, lam)["A"], NB))
    again = ops.ease_gram(_csr(lists_of(n)), n, lam).cpu().numpy()
    assert np.array_equal(again, got)  # independent of the order of the atomic adds


def test_gram_matrix_with_an_item_nobody_holds():
    n, gone = 65, 7
    lists = [v[v != gone] for v in ref.histories(150, n, 3)]
    A = ops.ease_gram(_csr(lists), n, 0.5).cpu().numpy()
    assert np.array_equal(A, ref.padded(ref.gram(ref.dense_x(lists, n), 0.5), NB))
    assert A[gone, gone] == 0.5 and np.count_nonzero(A[gone]) == 1 and np.count_nonzero(A[:, gone]) == 1


# ------------------------------------------------------------------------------------------------ 2. inverse
@pytest.mark.parametrize("n,lam", CASES, ids=IDS)
def test_inverse_residual_against_numpy(n, lam):
    h, P = host(n, lam), device(n, lam)["P"]
    nbar = P.shape[0]
    assert np.array_equal(P[n:, n:], np.eye(nbar - n)) and not P[:n, n:].any() and not P[n:, :n].any()
    P = P[:n, :n]
    res = ref.residual(h["A"], P)
    print("n=%d lambda=%g: max|A P - I| = %.3g, numpy %.3g, ratio %.2f (bar %g)"
          % (n, lam, res, h["res"], res / h["res"], RESIDUAL_BAR))
    assert res <= RESIDUAL_BAR * h["res"]
    assert np.abs(P - P.T).max() <= RESIDUAL_BAR * h["res"]


def test_inverse_flags_a_matrix_that_is_not_positive_definite():
    A = torch.eye(128, dtype=torch.float64, device=_dev())
    A[70, 70] = -1.0
    err = torch.zeros(1, dtype=torch.int32, device=_dev())
    P = ops.ease_invert(A, err)
    assert int(err.item()) == 1 and bool(torch.isfinite(P).all())


# ------------------------------------------------------------------------------------------------ 3. weights
@pytest.mark.parametrize("n,lam", CASES, ids=IDS)
def test_weights_against_float64(n, lam):
    h, B = host(n, lam), device(n, lam)["B_np"]
    assert B.dtype == np.float32 and B.shape == (n, n)
    want = h["B"]
    dev = np.abs(B.astype(np.float64) - want.astype(np.float32).astype(np.float64))
    print("n=%d lambda=%g: max |B - float32(B64)| = %.3g, TOL_B %.3g, max|B| %.3g"
          % (n, lam, dev.max(), h["tol_b"], np.abs(want).max()))
    assert np.all(dev <= 2.0 ** -23 * np.abs(want) + h["tol_b"])
    assert not np.diag(B).any()


# ------------------------------------------------------------------------------------------------ 4. score rows
@pytest.mark.parametrize("n,lam", CASES[:7], ids=IDS[:7])
def test_score_rows_bit_for_bit(n, lam):
    d = device(n, lam)
    lists = lists_of(n)  # lengths 0, 1, 2, 63, 64, 65, n first
    hist = _csr(lists)
    want = ref.score_rows(d["B_np"], lists)
    every = torch.arange(len(lists), dtype=torch.int64, device=_dev())
    got = ops.ease_scores(d["B"], hist, every).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert not got[0].any()  # the empty history
    for rows in ([6], list(range(16)), list(range(17)), [5, 3, 5, 0, 5]):  # 1, 16, 17 rows; a row listed three times
        r = ops.ease_scores(d["B"], hist, torch.tensor(rows, dtype=torch.int64, device=_dev())).cpu().numpy()
        assert np.array_equal(r.view(np.int32), want[rows].view(np.int32)), rows
    assert ops.ease_scores(d["B"], hist, every[:0]).shape == (0, n)


def test_score_rows_skip_ids_outside_the_catalogue_and_rows_outside_the_csr():
    n = 65
    d = device(n, 0.5)
    lists = [np.array([3, 64, 65, 1000]), np.array([5])]
    err = torch.zeros(1, dtype=torch.int32, device=_dev())
    got = ops.ease_scores(d["B"], _csr(lists), torch.tensor([0, 1, 2, -1], dtype=torch.int64, device=_dev()), err)
    want = ref.score_rows(d["B_np"], [[3, 64], [5], [], []])
    assert np.array_equal(got.cpu().numpy(), want) and int(err.item()) == 1


# ------------------------------------------------------------------------------------------------ 5. the surface
@functools.lru_cache(maxsize=None)
def fitted(n):
    m = _model(lists_of(n), n)
    m.fit_ease(0.5)
    B = m.net.B.cpu().numpy()
    return m, B, ref.score_rows(B, lists_of(n))


@pytest.mark.parametrize("n", [65, 200])
def test_recommend_predict_and_rank_items_position_for_position(n):
    m, B, rows = fitted(n)
    lists = lists_of(n)
    assert np.array_equal(B, device(n, 0.5)["B_np"])  # fit_ease is the three launchers
    users = list(range(len(lists)))
    for exclude in (True, False):
        for k in (1, 10, n):
            ids, sc = m.recommend(users, top_k=k, exclude_seen=exclude, return_scores=True)
            wi, ws = ref.recommend(rows, lists, k, exclude)
            assert np.array_equal(ids.numpy(), wi), (exclude, k)
            assert np.array_equal(sc.numpy(), ws), (exclude, k)
    ids = m.recommend(users, top_k=n, exclude_seen=True).numpy()
    assert (ids[6] == -1).all() and (ids[0] >= 0).all()  # the user who holds every item; the one who holds none
    for u in (0, 1, 5, 6, 20):
        assert np.array_equal(m.predict(u, top_k=7).numpy(), ref.recommend(rows[u:u + 1], lists, min(7, n), False)[0][0])
    assert np.array_equal(m.predict_many([3, 9], top_k=4).numpy(), ref.recommend(rows[[3, 9]], lists, 4, False)[0])
    rs = np.random.RandomState(1)
    qu = rs.randint(0, len(lists), size=60)
    qt = rs.randint(0, n, size=60)
    qu[:3], qt[:3] = [5, 5, 6], [lists[5][0], lists[5][-1], 0]  # targets that are train items
    for exclude in (True, False):
        got, val = m.rank_items(qu, qt, exclude_seen=exclude, return_scores=True)
        want = [ref.rank(rows[u], t, lists[u], exclude) for u, t in zip(qu, qt)]
        assert got.tolist() == want, exclude
        assert np.array_equal(val.numpy(), rows[qu, qt])


def test_recommend_for_histories_and_item_weights():
    n = 65
    m, B, _ = fitted(n)
    rs = np.random.RandomState(2)
    hists = [[], list(range(n)), [4], [9, 2, 9, 30], list(rs.choice(n, 20, replace=False))]
    clean = [np.unique(np.asarray(h, dtype=np.int64)) for h in hists]
    rows = ref.score_rows(B, clean)
    for exclude in (True, False):
        for k in (1, 10, n):
            ids, sc = m.recommend_for_histories(hists, top_k=k, exclude_seen=exclude, return_scores=True)
            wi, ws = ref.recommend(rows, clean, k, exclude)
            assert np.array_equal(ids.numpy(), wi) and np.array_equal(sc.numpy(), ws), (exclude, k)
    with pytest.raises(ValueError, match="fold-in options"):
        m.recommend_for_histories(hists, epochs=3)
    items = [0, 7, 64, 7]
    for k in (1, 10, n):
        ids, sc = m.item_weights(items, top_k=k, return_scores=True)
        for r, i in enumerate(items):
            wi, ws = ref.item_weights(B, i, k)
            assert np.array_equal(ids[r].numpy(), wi) and np.array_equal(sc[r].numpy(), ws), (k, i)
    assert i not in ids[r].tolist()
    with pytest.raises(IndexError):
        m.item_weights([n])


def test_evaluate_ranking_and_evaluate_ranks_against_the_restatement():
    n, nu = 65, 150
    lists = ref.histories(nu, n, 5)
    users = np.repeat(np.arange(nu), [len(v) for v in lists])
    items = np.concatenate(lists)
    p = np.random.RandomState(0).permutation(users.size)
    with contextlib.redirect_stdout(io.StringIO()):
        m = TorchRecSys.from_tensors(torch.from_numpy(users[p]), torch.from_numpy(items[p]), n_users=nu, n_items=n,
                                     net_type='ease', split_ratio=0.8)
        m.fit_ease(0.5)
        got_k = m.evaluate_ranking(k=10)
        got_r = m.evaluate_ranks(k=(1, 10), metrics=('auc', 'mrr', 'recall', 'ndcg', 'map'))
    tr, te = m.data_processor.train_data, m.data_processor.test_data
    train = [np.unique(tr['pos_item_id'].numpy()[tr['user_id'].numpy() == u]) for u in range(nu)]
    test = [np.setdiff1d(np.unique(te['pos_item_id'].numpy()[te['user_id'].numpy() == u]), train[u]) for u in range(nu)]
    rows = ref.score_rows(m.net.B.cpu().numpy(), train)
    ev = [u for u in range(nu) if test[u].size]
    ranks = [[ref.rank(rows[u], t, train[u], True) for t in test[u]] for u in ev]
    off = np.concatenate([[0], np.cumsum([len(r) for r in ranks])])
    n_c = np.array([n - train[u].size for u in ev])
    keep, per = rank_eval.per_user(np.concatenate(ranks), off, n_c, [1, 10], ['auc', 'mrr', 'recall', 'ndcg', 'map'], n)
    assert got_r['n_users'] == int(keep.sum()) > 20
    for name, v in per.items():
        assert got_r[name] == pytest.approx(float(np.sum(v)) / keep.sum(), rel=1e-12, abs=1e-15), name
    hit = rec = ndcg = 0.0
    for u, r in zip(ev, ranks):
        r = np.sort(np.asarray(r))
        top = r[r < 10]
        hit += float(top.size >= 1)
        rec += top.size / r.size
        ndcg += np.sum(1.0 / np.log2(top + 2.0)) / np.sum(1.0 / np.log2(np.arange(min(10, r.size)) + 2.0))
    assert got_k['n_users'] == len(ev)
    for name, v in (('hit_rate@10', hit), ('recall@10', rec), ('ndcg@10', ndcg)):
        assert got_k[name] == pytest.approx(v / len(ev), rel=1e-12), name


def test_recommend_orders_items_as_the_reference_does():
    g = load_golden("g5_ease.npz")
    nu, n = int(g["n_users"]), int(g["n_items"])
    pred = ref.from_byte_planes(g["pred_planes"], (nu, n))
    users, items = g["users"].astype(np.int64), g["items"].astype(np.int64)
    with contextlib.redirect_stdout(io.StringIO()):
        m = TorchRecSys.from_tensors(torch.from_numpy(users), torch.from_numpy(items), n_users=nu, n_items=n,
                                     net_type='ease', split_ratio=1.0)
    m.fit_ease(float(g["lam"]))
    got = m.recommend(list(range(nu)), top_k=5, exclude_seen=False).numpy()
    top6 = -np.sort(-pred, axis=1)[:, :6]
    clear = ~((top6[:, :-1] - top6[:, 1:]) < 1e-6).any(axis=1)
    assert (~clear).sum() <= nu // 10
    want = np.argsort(-pred, axis=1, kind='stable')[:, :5]
    assert np.array_equal(got[clear], want[clear])
    b = ref.from_byte_planes(g["b_planes"], (n, n))
    assert np.abs(m.net.B.cpu().numpy() - b).max() <= 2.0 ** -23 * np.abs(b).max() + 1e-12


# ------------------------------------------------------------------------------------------------ 6. determinism
def test_fit_ease_twice_gives_the_same_bits_and_state_dict_carries_the_weights():
    n = 200
    m, B, _ = fitted(n)
    m2 = _model(lists_of(n), n, seed=9)  # the same pairs in another order
    assert 'net.B' not in m2.state_dict()
    m2.fit_ease(0.5)
    assert torch.equal(m2.net.B, m.net.B)
    m2.fit_ease(0.5)
    assert torch.equal(m2.net.B, m.net.B)
    fresh = _model(lists_of(n), n)
    fresh.load_state_dict(m.state_dict())
    users = list(range(0, n_users_for(n), 7))
    a, sa = m.recommend(users, top_k=10, return_scores=True)
    b, sb = fresh.recommend(users, top_k=10, return_scores=True)
    assert torch.equal(a, b) and torch.equal(sa, sb)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_unfitted_model_and_too_little_memory_refuse(monkeypatch):
    n = 65
    m = _model(lists_of(n), n)
    for call in (lambda: m.recommend([0]), lambda: m.predict(0), lambda: m.rank_items([0], [1]),
                 lambda: m.recommend_for_histories([[1]]), lambda: m.item_weights([1])):
        with pytest.raises(RuntimeError, match=r"call fit_ease\(\) first"):
            call()
    launched = []
    for name in ("ease_gram", "ease_invert", "ease_weights"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: launched.append(_n))
    total = torch.cuda.mem_get_info()[1]
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (20 * 128 * 128 - 1, total))
    with pytest.raises(RuntimeError, match="free device memory"):
        m.fit_ease(0.5)
    assert not launched and m.net.B is None
