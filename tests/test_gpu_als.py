# -*- coding: utf-8 -*-
"""fit_als() / ops.als_gram / ops.als_solve on the GPU against the numpy restatement tests/als_ref.py.

1. one half-sweep against float64, both directions, D in {8, 24, 64, 100, 256} (every lane-group width; D = 256 reads G
   from L2, the others from LDS; 24 and 100 are not powers of two, 100 also takes the 16-byte loads' path with padding
   lanes), (alpha, lambda, cg_steps) in {(10, 0.1, 3), (40, 0.01, 3), (10, 0.1, D)};
2. exact cases, bit for bit; 3. independence of the launch; 4. determinism and warm start; 5. descent and the reported
   objective; 6. the retrieval surface after fit_als; 7. refusals.

TOL (test 1), measured on the CPU, not on the kernel: the fp32 restatement (als_ref.half_sweep(dtype=float32), factor
sums in ascending and in descending column order, its own fp32 Gram matrix) against the float64 one on exactly these
inputs (HISTS and its transpose, als_ref.tables(150, 120, D, seed=D)), as max |x32 - x64| / (1 + |x64|) over both orders,
both directions and the five D, per parameter set:
    (alpha, lambda, cg_steps) = (10, 0.1, 3)    1.82e-6   (per case 3.4e-7 .. 1.8e-6)
                                (40, 0.01, 3)   5.81e-5   (4.9e-7 .. 5.8e-5; the user side at D = 256 is the largest)
                                (10, 0.1, D)    1.14e-3   (5.1e-7 .. 1.1e-3: D = 100, user side.  D fp32 CG steps lose the
                                                          conjugacy of the directions; the float64 run itself is not at
                                                          the solution after D steps, tests/test_als_host.py)
D = 10 and D = 130 (no 16-byte loads: the scalar-load instances of the kernel) were measured too, with the first parameter
set: 1.0e-6, inside its figure.
atol = rtol = 8 x that: two fp32 orders may differ from each other by twice the deviation of one from float64, and the
kernel's butterfly (and the fmaf chains of its Gram matrix) is a third order.

LOSS_TOL (test 5): fit_als(return_loss=True) takes the Gram matrices and the scores of the train pairs in fp32 and sums
in float64.  Measured on the CPU on the model of test 5 (its init and its tables after each of three float64 reference
iterations): the objective with fp32 Gram matrices (als_ref.gram(dtype=float32), both orders) and fp32 scores (sequential
fp32 dot products, both orders) deviates from the float64 objective by at most 7.4e-8 relative.  Bound 8 x that, for
the same reason as above."""
import contextlib
import io

import numpy as np
import pytest
import torch

import als_ref as ref
from torchrecsys_amd import ops
from torchrecsys_amd.model import TorchRecSys
from torchrecsys_amd.ops import als_solve as ops_als_solve  # noqa: F401  (the subject of this module)

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS = 150, 120
HISTS = ref.histories(N_ITEMS, 11, N_USERS)  # lengths 0, 1, 2, 63, 64, 65, 119, 120, then 142 of random length 0..20
HISTS_T = ref.transpose(HISTS, N_ITEMS)
DS = [8, 24, 64, 100, 256]
CASES = {"a10_l0.1_cg3": (10.0, 0.1, 3, 8 * 1.82e-6), "a40_l0.01_cg3": (40.0, 0.01, 3, 8 * 5.81e-5),
         "a10_l0.1_cgD": (10.0, 0.1, None, 8 * 1.14e-3)}
LOSS_TOL = 8 * 7.4e-8


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _csr(lists):
    off, ids = ref.csr(lists)
    return _gpu(off), _gpu(ids)


def _solve(X, Y, lists, lam, alpha, cg, err=None):
    """ops.als_gram + ops.als_solve on copies: the new X as a float32 numpy array."""
    Yd, Xd = _gpu(Y), _gpu(X.copy())
    ops.als_solve(Yd, ops.als_gram(Yd), _csr(lists), lam, alpha, cg, Xd, err)
    return Xd.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("D", DS)
def test_one_half_sweep_against_float64(D, case):
    alpha, lam, cg, tol = CASES[case]
    cg = D if cg is None else cg
    X, Y = ref.tables(N_USERS, N_ITEMS, D, D)
    for name, A, B, lists in (("user", X, Y, HISTS), ("item", Y, X, HISTS_T)):
        want = ref.half_sweep(A, B, lists, lam, alpha, cg)
        got = _solve(A, B, lists, lam, alpha, cg).astype(np.float64)
        err = np.abs(got - want)
        print("%s side D=%d %s: max |got - float64| / (1 + |float64|) = %.3g (TOL %.3g)"
              % (name, D, case, (err / (1 + np.abs(want))).max(), tol))
        assert np.all(err <= tol + tol * np.abs(want)), (name, err.max())
        assert np.abs(want - A).max() > 0.05  # the rows moved


@pytest.mark.parametrize("D", [10, 130])
def test_one_half_sweep_against_float64_at_widths_without_16_byte_rows(D):
    test_one_half_sweep_against_float64(D, "a10_l0.1_cg3")


def test_gram_matrix_is_symmetric_repeatable_and_close_to_float64():
    for D in DS:
        Y = ref.tables(N_USERS, N_ITEMS, D, D)[0]  # 150 rows: ten chunks of 16 are reduced
        Yd = _gpu(Y)
        G = ops.als_gram(Yd)
        assert torch.equal(G, G.t()) and torch.equal(G, ops.als_gram(Yd))
        want = Y.astype(np.float64).T @ Y.astype(np.float64)
        # 150 products of magnitude <= |y_a| |y_b| summed in fp32: plus ten chunk sums: error <= 200 eps sum |y_a y_b|
        bound = 200 * 2.0 ** -24 * (np.abs(Y).astype(np.float64).T @ np.abs(Y).astype(np.float64))
        assert np.all(np.abs(G.cpu().numpy() - want) <= bound)
        wide = torch.cat([Yd, torch.full((N_USERS, 3), 7.0, device=Yd.device)], 1).contiguous()  # ld > D
        assert torch.equal(ops.als_gram(wide, D=D), G)
        assert torch.equal(ops.als_gram(Yd, n=0), torch.zeros_like(G))


# ------------------------------------------------------------------------------------------------ 2. exact cases
def test_empty_lists_give_zero_rows_and_alpha_zero_with_a_zero_table_drives_rows_to_zero():
    for D in DS:
        X, Y = ref.tables(N_USERS, N_ITEMS, D, D)
        got = _solve(X, Y, [[] for _ in range(N_USERS)], 0.1, 10.0, 3)
        assert got.shape == X.shape and not got.any()
        got = _solve(X, Y, HISTS, 0.1, 10.0, 3)
        assert not got[0].any() and got[1:8].any(axis=1).all()  # the empty list among others
        # Y = 0, alpha = 0: A = lambda I, b = 0, r = -lambda x, a = 1 / lambda: x - x = 0 exactly (lambda a power of two)
        got = _solve(X, np.zeros_like(Y), HISTS, 0.25, 0.0, 3)
        assert not got.any()


@pytest.mark.parametrize("D", DS + [10, 130])
def test_the_integer_case_is_bit_exact(D):
    """als_ref.exact_case: every intermediate is a multiple of 2^-5 below 2^19 (the reference asserts |v| 2^5 < 2^24), so
    every fp32 product and sum is exact in every order, the kernel's included.  Values are compared, not bits: a sum of
    exact zeros may carry either sign."""
    X, Y, lists = ref.exact_case(D)
    want = ref.half_sweep(X, Y, lists, ref.EXACT_LAMBDA, ref.EXACT_ALPHA, 3, exact_bits=ref.EXACT_BITS)
    print("bound %.0f" % ref.half_sweep.bound)
    got = _solve(X, Y, lists, ref.EXACT_LAMBDA, ref.EXACT_ALPHA, 3)
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)
    assert sorted({float(v) for v in np.abs(want).ravel()}) == [0.0, 0.125, 0.25, 0.5]
    G = ops.als_gram(_gpu(Y)).cpu().numpy()  # integers: the Gram matrix is exact too
    assert np.array_equal(G.astype(np.float64), Y.astype(np.float64).T @ Y.astype(np.float64))


# ------------------------------------------------------------------------------------------------ 3. independence
@pytest.mark.parametrize("D", [24, 100])
def test_a_row_does_not_depend_on_the_rest_of_the_launch(D):
    G_LANES = {24: 8, 100: 32}[D]
    X, Y = ref.tables(N_USERS, N_ITEMS, D, D)
    Yd = _gpu(Y)
    G = ops.als_gram(Yd)
    full = _gpu(X.copy())
    ops.als_solve(Yd, G, _csr(HISTS), 0.1, 10.0, 3, full)
    full = full.cpu()
    per_wave = 64 // G_LANES
    picks = [3, 4, 5, 6, 7] + list(range(40, 40 + per_wave))  # the long lists, then one row per lane position
    assert {p % per_wave for p in picks} == set(range(per_wave))
    for p in picks:
        one = _gpu(X[p:p + 1].copy())
        ops.als_solve(Yd, G, _csr([HISTS[p]]), 0.1, 10.0, 3, one)
        assert torch.equal(one.cpu()[0], full[p]), p
    # ... nor on its position: the same rows in reversed order
    rev = _gpu(X[::-1].copy())
    ops.als_solve(Yd, G, _csr(HISTS[::-1]), 0.1, 10.0, 3, rev)
    assert torch.equal(rev.cpu().flip(0), full)


# ------------------------------------------------------------------------------------------------ models
def _interactions(lists):
    u = np.concatenate([np.full(len(h), r, dtype=np.int64) for r, h in enumerate(lists)])
    i = np.concatenate([np.asarray(h, dtype=np.int64) for h in lists])
    return u, i


def _model(net_type, lists=HISTS, n_users=N_USERS, n_items=N_ITEMS, D=24, seed=0, **kw):
    u, i = _interactions(lists)
    with contextlib.redirect_stdout(io.StringIO()):
        torch.manual_seed(seed)
        np.random.seed(seed)
        return TorchRecSys.from_tensors(torch.from_numpy(u), torch.from_numpy(i), n_users=n_users, n_items=n_items,
                                        n_factors=D, net_type=net_type, **kw)


def _tables(m):
    return m.net.user.weight.data.cpu().numpy().copy(), m.net.item.weight.data.cpu().numpy().copy()


def _train_lists(m):
    off, items = (t.cpu().numpy() for t in m._seen_csr())
    return [items[off[u]:off[u + 1]] for u in range(m.n_users)]


# ------------------------------------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("net_type", ["linear", "fm"])
def test_fit_als_is_deterministic_and_warm_starts(net_type):
    a, b, c = (_model(net_type, seed=3) for _ in range(3))
    assert a.fit_als(iterations=3) is None
    b.fit_als(iterations=3)
    for _ in range(3):
        c.fit_als(iterations=1)
    for other in (b, c):
        assert torch.equal(a.net.user.weight.data, other.net.user.weight.data)
        assert torch.equal(a.net.item.weight.data, other.net.item.weight.data)
    assert a.net.user.weight.data.abs().max() > 0.05


# ------------------------------------------------------------------------------------------------ 5. descent
def test_every_iteration_lowers_the_objective_and_the_reported_losses_are_its_values():
    lam, alpha = 0.1, 10.0
    m = _model("linear", seed=5)
    lists = _train_lists(m)
    items = ref.transpose(lists, N_ITEMS)
    X0, Y0 = _tables(m)
    # the condition on the inputs, on the CPU reference: its own objective falls by at least 1 % per half-sweep
    Xr, Yr = X0.astype(np.float64), Y0.astype(np.float64)
    prev = ref.loss(Xr, Yr, lists, lam, alpha)
    for _ in range(3):
        Xr = ref.half_sweep(Xr, Yr, lists, lam, alpha, 3)
        mid = ref.loss(Xr, Yr, lists, lam, alpha)
        Yr = ref.half_sweep(Yr, Xr, items, lam, alpha, 3)
        end = ref.loss(Xr, Yr, lists, lam, alpha)
        assert mid < 0.99 * prev and end < 0.99 * mid, (prev, mid, end)
        prev = end
    values = [ref.loss(X0, Y0, lists, lam, alpha)]
    for _ in range(3):
        m.fit_als(iterations=1, regularization=lam, alpha=alpha)
        values.append(ref.loss(*_tables(m), lists, lam, alpha))
    print("objective per iteration:", values)
    assert all(values[k + 1] < values[k] for k in range(3)), values
    m2 = _model("linear", seed=5)
    got = m2.fit_als(iterations=3, regularization=lam, alpha=alpha, return_loss=True)
    assert got.dtype == torch.float64 and got.device.type == "cpu" and got.shape == (4,)
    rel = np.abs(got.numpy() - np.array(values)) / np.abs(values)
    print("reported vs float64 objective, relative:", rel, "LOSS_TOL %.3g" % LOSS_TOL)
    assert np.all(rel <= LOSS_TOL), rel
    assert torch.equal(m2.net.user.weight.data, m.net.user.weight.data)  # return_loss does not change the fit


# ------------------------------------------------------------------------------------------------ 6. surface
def _two_blocks(seed=0):
    """Users 0..74 interact with items 0..59 only, users 75..149 with items 60..119: 24 distinct items each."""
    rs = np.random.RandomState(seed)
    return [np.sort(rs.choice(60, 24, replace=False) + (60 if u >= 75 else 0)).astype(np.int32) for u in range(N_USERS)]


def test_the_retrieval_surface_ranks_by_the_als_score():
    lists = _two_blocks()
    lin, fm = _model("linear", lists, seed=1), _model("fm", lists, seed=1)
    fm.net.user.weight.data.copy_(lin.net.user.weight.data)
    fm.net.item.weight.data.copy_(lin.net.item.weight.data)
    lin.net.user_bias.weight.data.normal_()  # whatever fit() may have left there
    lin.net.item_bias.weight.data.normal_()
    with contextlib.redirect_stdout(io.StringIO()):
        before = lin.evaluate_ranking(k=10)["hit_rate@10"]
    frozen = {}
    for m in (lin, fm):
        m._seen_csr()
        frozen[m] = [t.clone() for t in m._seen_csr()] + \
                    [m.data_processor.train_data[k].clone() for k in ("user_id", "pos_item_id")] + \
                    [m.data_processor.test_data[k].clone() for k in ("user_id", "pos_item_id")]
        m.fit_als(iterations=5)
    for m in (lin, fm):
        now = list(m._seen_csr()) + [m.data_processor.train_data[k] for k in ("user_id", "pos_item_id")] + \
              [m.data_processor.test_data[k] for k in ("user_id", "pos_item_id")]
        assert all(torch.equal(x, y) for x, y in zip(frozen[m], now))  # the split and the cached CSR are not written
        for name, p in m.net.state_dict().items():
            if p.dim() == 2 and p.shape[1] == 1:
                assert not p.any(), name  # every 1-wide table is zero
    assert torch.equal(lin.net.user.weight.data, fm.net.user.weight.data)
    assert torch.equal(lin.net.item.weight.data, fm.net.item.weight.data)
    users = list(range(0, N_USERS, 7))
    ids, sc = lin.recommend(users, top_k=10, return_scores=True)
    assert torch.equal(ids, fm.recommend(users, top_k=10))  # FM's logit is the same inner product
    X, Y = _tables(lin)
    s64 = X.astype(np.float64)[users] @ Y.astype(np.float64).T
    assert np.allclose(sc.numpy(), np.take_along_axis(s64, ids.numpy(), 1), atol=1e-5)  # ... the ALS score
    for m in (lin, fm):
        uu = np.repeat(users, 10)
        ranks = m.rank_items(uu, ids.reshape(-1))
        assert torch.equal(ranks.reshape(len(users), 10), torch.arange(10).expand(len(users), 10))
    with contextlib.redirect_stdout(io.StringIO()):
        after = lin.evaluate_ranking(k=10)["hit_rate@10"]
    print("hit_rate@10: %.3f before, %.3f after fit_als(5)" % (before, after))
    assert after > before


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals():
    with pytest.raises(ValueError, match="mlp"):
        _model("mlp").fit_als()
    with pytest.raises(ValueError, match="n_factors"):
        _model("linear", D=257).fit_als()
    u, i = _interactions(HISTS)
    with contextlib.redirect_stdout(io.StringIO()):
        meta = TorchRecSys.from_tensors(torch.from_numpy(u), torch.from_numpy(i), n_users=N_USERS, n_items=N_ITEMS,
                                        item_metadata=torch.randint(0, 5, (N_ITEMS, 1)), metadata_names=["m0"],
                                        n_factors=8, net_type="fm")
    with pytest.raises(ValueError, match="metadata"):
        meta.fit_als()
    m = _model("fm")
    before = _tables(m)
    for kw in (dict(iterations=0), dict(cg_steps=0), dict(regularization=0), dict(alpha=-1.0)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            m.fit_als(**kw)
    assert all(np.array_equal(x, y) for x, y in zip(before, _tables(m)))


def test_an_id_outside_the_table_sets_the_flag_and_is_skipped():
    D = 24
    X, Y = ref.tables(N_USERS, N_ITEMS, D, D)
    lists = [list(h) for h in HISTS[:70]]
    bad = [list(h) for h in lists]
    bad[5] = bad[5] + [N_ITEMS]  # one past the table
    bad[9] = [-1] + bad[9]
    bad[40] = bad[40] + [2 ** 31 - 1]
    err = torch.zeros(1, dtype=torch.int32, device=_dev())
    guard = np.full((4, D), 123.0, dtype=np.float32)  # rows behind the ones to solve: never written
    Xd = _gpu(np.concatenate([X[:70], guard]))
    Yd = _gpu(np.concatenate([Y, np.full((4, D), np.nan, dtype=np.float32)]))  # what an id one past the table would read
    G = ops.als_gram(Yd, n=N_ITEMS)
    ops.als_solve(Yd[:N_ITEMS], G, _csr(bad), 0.1, 10.0, 3, Xd[:70], err)
    assert int(err.item()) == 1
    got = Xd.cpu().numpy()
    assert np.array_equal(got[70:], guard) and np.isfinite(got).all()
    clean = torch.zeros(1, dtype=torch.int32, device=_dev())
    want = _solve(X[:70], Y, lists, 0.1, 10.0, 3, clean)
    assert int(clean.item()) == 0 and np.array_equal(got[:70], want)  # the bad ids are skipped, nothing else changes
