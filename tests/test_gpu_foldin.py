# -*- coding: utf-8 -*-
"""fold_in_users() / recommend_for_histories() on the GPU against the numpy restatement tests/foldin_ref.py.

1. bit-exact: Linear + hinge on integer tables with lr = 2^-6 — every value is a multiple of 2^-6 and the reference
   asserts (sum_d |u_d S_d| + |b| + |c|) * 64 < 2^24 at every visit, so every summation order is exact;
2. batch independence: a row of a large call equals the row of a one-user call, bit for bit, at every lane position,
   and at every prefetch depth;
3. smooth losses (FM hinge, FM BPR, Linear BPR; l2 = 2^-3, tables 0.3 randn) against float64 within TOL;
4. degenerate inputs; 5. end to end through recommend_for_histories(); 6. the model is not written.

TOL (test 3), measured on the CPU, not on the kernel: an fp32 numpy restatement of the rule that sums the factors in
DESCENDING column order (foldin_ref.fold_in(dtype=float32, order='desc')) against the float64 reference on exactly these
inputs (the six cases below, the histories of HISTS, E = 4, lr = 0.05, l2 = 2^-3) deviates by at most 3.37e-7 over U, b and
the epoch losses (per case 2.2e-7 .. 3.4e-7; ascending order: the same to two digits).  atol = rtol = 8 x that = 2.7e-6:
two fp32 orders may differ from each other by twice the deviation of one from float64, and the kernel's butterfly is a
third order.
"""
import numpy as np
import pytest
import torch

import foldin_ref as ref
from torchrecsys_amd.ops import fold_in_users as ops_fold_in_users  # noqa: F401  (the subject of this module)

pytestmark = pytest.mark.gpu

N_ITEMS = 200
E = 4
LR_EXACT = 2.0 ** -6
TOL = 8 * 3.37e-7
HISTS = ref.histories(N_ITEMS, 11)  # lengths 0, 1, 2, 63, 64, 65, 150, 199, 200, then 300 of random length 0..20


def _fold(m):
    """(S (n_items, Dp), c (n_items,)) float64 copies of the model's item fold as the device wrote it."""
    from torchrecsys_amd import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    m.net.eval()
    fold = ops.item_fold(m.net.NET, m.net.tables(), m.n_items, m.n_factors, dev, m._item_meta_dev())
    S, c = ops.fold_views(fold, m.n_items, m.n_factors)
    return fold, S.cpu().numpy().astype(np.float64), c.cpu().numpy().astype(np.float64)


def _same_bits(got, want64, what):
    got = got.numpy() if hasattr(got, "numpy") else np.asarray(got)
    want = np.asarray(want64).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    # -0.0 never arises from u = 0 minus a product here, but compare values too so a sign of zero reads clearly
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])


# ------------------------------------------------------------------------------------------------ 1. bit-exact
@pytest.mark.parametrize("flags", [True, False], ids=["shuffle+reject", "plain"])
@pytest.mark.parametrize("D", [8, 24, 64, 100, 256])
@pytest.mark.parametrize("M", [0, 2])
def test_linear_hinge_on_integer_tables_is_bit_exact(M, D, flags):
    m = ref.make_model("linear", 10, N_ITEMS, D, M, seed=D + M, int_range=(-3, 4))
    _, S, c = _fold(m)
    kw = dict(seed=5, shuffle=flags, reject_seen=flags, max_tries=8 if flags else 0)
    want = ref.fold_in(S, c, HISTS, "linear", "hinge", E, LR_EXACT, 0.0, D=D, require_exact=True, **kw)
    frac = want["active"] / want["visits"]
    print("hinge-active fraction %.3f, bound %.0f" % (frac, want["bound"]))
    assert 0.10 <= frac <= 0.90, frac  # a condition on the inputs: both branches of the hinge are exercised
    U, b, ls = m.fold_in_users(HISTS, epochs=E, lr=LR_EXACT, loss="hinge", l2=0.0, return_loss=True, **kw)
    _same_bits(U, want["U"], "U")
    _same_bits(b, want["b"], "b")
    _same_bits(ls, want["loss"], "loss")
    assert not b.numpy().any()  # Linear with l2 = 0: the bias stays exactly 0


# ------------------------------------------------------------------------------------------------ 2. independence
def _csr(hists, dev):
    off = np.concatenate([[0], np.cumsum([len(h) for h in hists])]).astype(np.int64)
    items = np.concatenate([np.asarray(h, dtype=np.int32) for h in hists] + [np.zeros(0, np.int32)])
    return torch.from_numpy(off).to(dev), torch.from_numpy(items).to(dev)


def test_a_row_does_not_depend_on_the_rest_of_the_call_or_the_prefetch_depth(tune):
    from torchrecsys_amd import ops
    D = 24  # lane groups of 8: eight positions in a wave
    m = ref.make_model("fm", 10, N_ITEMS, D, 2, seed=3, scale=0.3)
    fold, _, _ = _fold(m)
    dev = fold.device
    args = ("bpr", E, 0.05, 0.125, 7, True, True, 8)
    U, b, ls = ops.fold_in_users("fm", fold, N_ITEMS, D, _csr(HISTS, dev), *args, want_loss=True)
    U, b, ls = U.cpu(), b.cpu(), ls.cpu()
    assert U.abs().max() > 0.01
    picks = [3, 4, 5, 6, 7, 8] + list(range(40, 48))  # the long histories, then one user per lane position (40..47)
    assert {p % 8 for p in picks} == set(range(8))
    for p in picks:
        u1, b1, l1 = ops.fold_in_users("fm", fold, N_ITEMS, D, _csr([HISTS[p]], dev), *args, want_loss=True)
        assert torch.equal(u1.cpu()[0], U[p]) and torch.equal(b1.cpu()[0], b[p]) and torch.equal(l1.cpu()[:, 0], ls[:, p]), p
    for depth in (1, 2, 8):
        tune(FOLDIN_DEPTH=depth)
        u2, b2, l2 = ops.fold_in_users("fm", fold, N_ITEMS, D, _csr(HISTS, dev), *args, want_loss=True)
        assert torch.equal(u2.cpu(), U) and torch.equal(b2.cpu(), b) and torch.equal(l2.cpu(), ls), depth


# ------------------------------------------------------------------------------------------------ 3. smooth losses
@pytest.mark.parametrize("D,M", [(24, 0), (128, 2)])
@pytest.mark.parametrize("net,loss", [("fm", "hinge"), ("fm", "bpr"), ("linear", "bpr")])
def test_smooth_losses_against_float64(net, loss, D, M):
    m = ref.make_model(net, 10, N_ITEMS, D, M, seed=D + M, scale=0.3)
    _, S, c = _fold(m)
    kw = dict(seed=7, shuffle=True, reject_seen=True, max_tries=8)
    want = ref.fold_in(S, c, HISTS, net, loss, E, 0.05, 2.0 ** -3, D=D, **kw)
    U, b, ls = m.fold_in_users(HISTS, epochs=E, lr=0.05, loss=loss, l2=2.0 ** -3, return_loss=True, **kw)
    for name, got, w in (("U", U, want["U"]), ("b", b, want["b"]), ("loss", ls, want["loss"])):
        err = np.abs(got.numpy().astype(np.float64) - w)
        print("%s: max |got - float64| = %.3g (TOL %.3g)" % (name, err.max(), TOL))
        assert np.all(err <= TOL + TOL * np.abs(w)), (name, err.max())
    assert np.abs(want["U"]).max() > 0.05  # the rows moved


# ------------------------------------------------------------------------------------------------ 4. degenerate
def test_two_items_one_user_and_empty_histories():
    m = ref.make_model("linear", 5, 2, 8, 0, seed=1, int_range=(-3, 4))
    _, S, c = _fold(m)
    hs = [[0], [1], [0, 1], []]
    kw = dict(seed=3, shuffle=True, reject_seen=True, max_tries=8)
    want = ref.fold_in(S, c, ref.clean(hs), "linear", "hinge", E, LR_EXACT, 0.0, D=8, require_exact=True, **kw)
    U, b, ls = m.fold_in_users(hs, epochs=E, lr=LR_EXACT, l2=0.0, return_loss=True, **kw)
    _same_bits(U, want["U"], "U")
    _same_bits(ls, want["loss"], "loss")
    for r in range(3):  # a call of one user
        u1, b1 = m.fold_in_users([hs[r]], epochs=E, lr=LR_EXACT, l2=0.0, **kw)
        assert torch.equal(u1[0], U[r]) and torch.equal(b1[0], b[r])
    U0, b0, l0 = m.fold_in_users([[], [], []], epochs=3, return_loss=True)
    assert U0.shape == (3, 8) and not U0.any() and not b0.any() and l0.shape == (3, 3) and not l0.any()
    ids, sc = m.recommend_for_histories([[], [0], [0, 1]], top_k=5, return_scores=True)
    assert ids.shape == (3, 2)  # k = min(top_k, n_items)
    order = np.argsort(-c, kind="stable")  # the empty history: the ranking by c
    assert ids[0].tolist() == order.tolist() and np.array_equal(sc[0].numpy(), c[order].astype(np.float32))
    assert ids[1].tolist() == [1, -1] and ids[2].tolist() == [-1, -1] and np.isneginf(sc[2].numpy()).all()


def test_duplicate_and_unsorted_histories_fold_in_as_their_sorted_distinct_form():
    m = ref.make_model("fm", 10, N_ITEMS, 24, 0, seed=2, scale=0.3)
    rs = np.random.RandomState(0)
    raw = [rs.randint(0, N_ITEMS, n).tolist() for n in (1, 5, 40, 300)] + [[7, 7, 7], [9, 3, 9, 3, 1]]
    a = m.fold_in_users(raw, epochs=3, loss="bpr", return_loss=True)
    b = m.fold_in_users(ref.clean(raw), epochs=3, loss="bpr", return_loss=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    i1 = m.recommend_for_histories(raw, top_k=7, loss="bpr", epochs=3)
    i2 = m.recommend_for_histories([np.asarray(h) for h in ref.clean(raw)], top_k=7, loss="bpr", epochs=3)
    assert torch.equal(i1, i2)
    for r, h in enumerate(raw):
        assert not np.isin(i1[r].numpy(), h).any()


def test_remapped_ids_go_in_and_come_out_as_original_ids():
    from torchrecsys_amd.model import TorchRecSys
    import contextlib
    import io
    rs = np.random.RandomState(1)
    raw_u = torch.arange(300) * 7 + 3
    raw_i = torch.arange(120) * 5 + 11
    uu = np.concatenate([np.arange(300), rs.randint(0, 300, 3000)])
    ii = np.concatenate([np.arange(120), rs.randint(0, 120, 3180)])[:len(uu)]
    with contextlib.redirect_stdout(io.StringIO()):
        torch.manual_seed(2)
        m = TorchRecSys.from_tensors(raw_u[uu], raw_i[ii], n_factors=16, net_type="linear", remap_ids=True)
    g = torch.Generator().manual_seed(3)
    for p in m.net.parameters():
        p.data.copy_(torch.randint(-3, 4, p.shape, generator=g).float())
    _, S, c = _fold(m)
    dense = [[0, 5, 119], [64], list(range(10, 40))]
    raw = [[11 + 5 * x for x in h] for h in dense]
    kw = dict(seed=1, shuffle=True, reject_seen=True, max_tries=8)
    want = ref.fold_in(S, c, dense, "linear", "hinge", E, LR_EXACT, 0.0, D=16, require_exact=True, **kw)
    U, b = m.fold_in_users(raw, epochs=E, lr=LR_EXACT, **kw)
    _same_bits(U, want["U"], "U")
    ids, sc = m.recommend_for_histories(raw, top_k=15, return_scores=True, epochs=E, lr=LR_EXACT, **kw)
    wi, wv = ref.rank(want["U"], want["b"], S, c, dense, 15)
    assert np.array_equal(ids.numpy(), raw_i.numpy()[wi]) and np.array_equal(sc.numpy(), wv.astype(np.float32))
    with pytest.raises(IndexError, match="12"):
        m.fold_in_users([[11, 12]])
    with pytest.raises(IndexError, match="12"):
        m.recommend_for_histories([[11], [12]])


def test_an_item_id_outside_the_catalogue_is_skipped_and_flagged():
    from torchrecsys_amd import ops
    m = ref.make_model("linear", 10, N_ITEMS, 24, 0, seed=4, int_range=(-3, 4))
    fold, _, _ = _fold(m)
    dev = fold.device
    args = ("hinge", E, LR_EXACT, 0.0, 5, True, False, 0)
    good = [HISTS[3], HISTS[12], HISTS[20]]
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    U0, b0, l0 = ops.fold_in_users("linear", fold, N_ITEMS, 24, _csr(good, dev), *args, want_loss=True, err_flag=err)
    assert int(err.item()) == 0
    U1, b1, l1 = ops.fold_in_users("linear", fold, N_ITEMS, 24, _csr(good[:1] + [[-5, N_ITEMS, 1 << 30]] + good[1:], dev),
                                   *args, want_loss=True, err_flag=err)
    assert int(err.item()) & 1
    keep = [0, 2, 3]
    assert torch.equal(U1[keep], U0) and torch.equal(b1[keep], b0) and torch.equal(l1[:, keep], l0)
    assert not U1[1].any() and float(b1[1]) == 0 and not l1[:, 1].any()  # every visit skipped: nothing learned


# ------------------------------------------------------------------------------------------------ 5. + 6. end to end
@pytest.mark.parametrize("D,M", [(8, 0), (64, 2), (8, 2), (64, 0)])
@pytest.mark.parametrize("net", ["linear", "fm"])
def test_recommend_for_histories_ranks_the_folded_in_rows(net, D, M):
    m = ref.make_model(net, 10, N_ITEMS, D, M, seed=D + M + 1, int_range=(-3, 4))
    before = {k: v.detach().cpu().clone() for k, v in m.net.state_dict().items()}
    _, S, c = _fold(m)
    hs = HISTS[:60]  # every special length (199 and 200 leave 1 and 0 candidates) and 51 short ones
    opts = dict(epochs=E, lr=LR_EXACT, loss="hinge", seed=2)
    U, b = m.fold_in_users(hs, **opts)
    Un, bn = U.numpy().astype(np.float64), b.numpy().astype(np.float64)
    z = (Un @ S[:, :D].T + bn[:, None]) + c[None, :]
    for k in (1, 10, 128):
        for exclude in (True, False):
            ids, sc = m.recommend_for_histories(hs, top_k=k, exclude_seen=exclude, return_scores=True, **opts)
            ids, sc = ids.numpy(), sc.numpy()
            wi, wv = ref.rank(Un, bn, S, c, hs if exclude else None, k)
            assert ids.shape == (len(hs), k) and ids.dtype == np.int64 and sc.dtype == np.float32
            pad = wi < 0
            assert np.array_equal(ids < 0, pad) and np.all(ids[pad] == -1) and np.isneginf(sc[pad]).all()
            if exclude:  # -1 / -inf exactly beyond n_items - n_h
                n_cand = np.array([N_ITEMS - len(h) for h in hs])
                assert np.array_equal((~pad).sum(1), np.minimum(n_cand, k))
                for r, h in enumerate(hs):
                    assert not np.isin(ids[r], h).any()
            if net == "linear":  # every value a multiple of 2^-6: the ranking, its ties and the scores are exact
                assert np.array_equal(ids, wi)
                assert np.array_equal(sc, wv.astype(np.float32))
            else:  # FM rows are not dyadic: the same ranking up to swaps of scores closer than fp32 resolves
                for r in range(len(hs)):
                    live = ~pad[r]
                    assert len(set(ids[r][live].tolist())) == int(live.sum())
                    zg, zw = z[r][ids[r][live]], wv[r][live]
                    assert np.all(np.abs(zg - zw) <= 1e-5 * np.maximum(1.0, np.abs(zw))), r
                    want_s = 1.0 / (1.0 + np.exp(-zg))
                    assert np.all(np.abs(sc[r][live] - want_s) <= 2e-6), r
    after = m.net.state_dict()
    assert set(after) == set(before)
    for k_, v in before.items():
        assert torch.equal(after[k_].detach().cpu(), v), k_  # the model's parameters are never written


@pytest.mark.parametrize("D", [8, 64])
def test_planted_direction_is_recommended(D):
    S, c, hist = ref.planted(D, seed=D)
    m = ref.make_model("linear", 10, 96, D, 0, seed=D, int_range=(-3, 4))
    sd = m.net.state_dict()
    sd["item.weight"].copy_(torch.from_numpy(S).float())
    sd["item_bias.weight"].zero_()
    ids = m.recommend_for_histories([hist.tolist()], top_k=10)
    assert ids.shape == (1, 10) and bool((ids < 48).all()) and bool((ids >= 0).all())
    assert not np.isin(ids.numpy(), hist).any()
    U, b, ls = m.fold_in_users([hist], return_loss=True)
    assert float(ls[-1, 0]) < float(ls[0, 0])
    assert float(U[0, 0]) > 0  # towards the first half's +4 e_0
