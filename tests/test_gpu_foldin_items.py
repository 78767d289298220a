# -*- coding: utf-8 -*-
"""fold_in_items() / recommend_with_new_items() on the GPU against the numpy restatement tests/foldin_items_ref.py.

1. bit-exact: Linear + hinge on integer tables with lr = 2^-6 and nu = 0, 1, 3 — every value is a multiple of 2^-6 and
   the reference asserts (sum_d |U_d x_d| + |a| + |c|) * 64 < 2^24 at every visit, so every summation order is exact;
2. purity: a row of a large call equals the row of a one-item call, bit for bit, at every lane position of a wave, and
   at every prefetch depth;
3. smooth losses (FM hinge, FM BPR, Linear BPR; l2 = 2^-3, tables 0.3 randn) against float64 within TOL;
4. degenerate inputs; 5. the metadata-only item; 6. the extended catalogue against a second, larger model; 7. the planted
   direction; 8. the model is not written.

TOL (test 3), measured on the CPU, not on the kernel: an fp32 numpy restatement of the rule that sums the factors in
DESCENDING column order (foldin_items_ref.fold_in(dtype=float32, order='desc')) against the float64 reference on the
inputs of the six cases below (smooth_inputs(): the histories of HISTS, E = 4, nu = 1, lr = 0.05, l2 = 2^-3; the item
side folded in numpy and rounded to fp32 where the GPU test reads the fold the device wrote, which differs in last bits
only) deviates by at most 6.70e-7 over V, b and the epoch losses (per case 2.6e-7 .. 6.7e-7; ascending order 2.6e-7 ..
7.7e-7).  atol = rtol = 8 x 6.70e-7 = 5.4e-6: two fp32 orders may differ from each other by twice the deviation
of one from float64, and the kernel's butterfly is a third order.
"""
import contextlib
import io

import numpy as np
import pytest
import torch

import foldin_items_ref as ref
import foldin_ref as base
from torchrecsys_amd.ops import fold_in_items as ops_fold_in_items  # noqa: F401  (the subject of this module)

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS = 200, 120
E = 4
LR_EXACT = 2.0 ** -6
TOL = 8 * 6.70e-7
HISTS = base.histories(N_USERS, 11, n_random=100)  # lengths 0, 1, 2, 63, 64, 65, 150, 199, 200, then 100 of 0..20
META = np.random.RandomState(5).randint(0, 5, (len(HISTS), 2))  # the new items' metadata ids
SMOOTH = [(net, loss, D, M) for net, loss in (("fm", "hinge"), ("fm", "bpr"), ("linear", "bpr"))
          for D, M in ((24, 0), (100, 2))]  # D = 24: 16-byte user-row loads, D = 100 likewise; scalar loads: test 1, 2


def _meta(M, rows=slice(None)):
    return META[rows, :M] if M else None


def _views(fold, n, D):
    from torchrecsys_amd import ops
    S, c = ops.fold_views(fold, n, D)
    return S.cpu().numpy().astype(np.float64), c.cpu().numpy().astype(np.float64)


def _frozen(m, meta, n):
    """What the kernel reads, as float64 copies: (U, a, S, c, T, kappa, su, si, seen) — S, c, T and kappa as the device
    folded them."""
    from torchrecsys_amd import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    m.net.eval()
    fold = ops.item_fold(m.net.NET, m.net.tables(), m.n_items, m.n_factors, dev, m._item_meta_dev())
    S, c = _views(fold, m.n_items, m.n_factors)
    T, kappa = _views(m._new_item_fold(meta, n, dev), n, m.n_factors)
    U, a = ref.user_side(m)
    su, si = ref.train_stream(m)
    return U, a, S, c, T, kappa, su, si, ref.seen_csr(su, si, m.n_users)


def smooth_inputs(net, D, M):
    """The model of a smooth-loss case (needs no GPU: the tolerance is measured on the same tables)."""
    return ref.make_model(net, N_USERS, N_ITEMS, D, M, seed=D + M, scale=0.3)


def _same_bits(got, want64, what):
    got = got.numpy() if hasattr(got, "numpy") else np.asarray(got)
    want = np.asarray(want64).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])


# ------------------------------------------------------------------------------------------------ 1. bit-exact
@pytest.mark.parametrize("flags", [True, False], ids=["shuffle+reject", "plain"])
@pytest.mark.parametrize("D", [6, 24, 64, 100, 250])
@pytest.mark.parametrize("M", [0, 2])
def test_linear_hinge_on_integer_tables_is_bit_exact(M, D, flags):
    m = ref.make_model("linear", N_USERS, N_ITEMS, D, M, seed=D + M, int_range=(-3, 4))
    U, a, S, c, T, kappa, su, si, seen = _frozen(m, _meta(M), len(HISTS))
    kw = dict(seed=5, shuffle=flags, reject_seen=flags, max_tries=8 if flags else 0)
    for nu in (0, 1, 3):
        want = ref.fold_in(U, a, S, c, T, kappa, HISTS, su, si, seen, "linear", "hinge", E, LR_EXACT, 0.0, nu=nu,
                           require_exact=True, **kw)
        frac = want["active"] / want["visits"]
        print("nu %d: hinge-active fraction %.3f, bound %.0f" % (nu, frac, want["bound"]))
        assert 0.10 <= frac <= 0.90, frac  # a condition on the inputs: both branches of the hinge are exercised
        V, b, ls = m.fold_in_items(HISTS, metadata=_meta(M), epochs=E, lr=LR_EXACT, loss="hinge", l2=0.0,
                                   negative_visits=nu, return_loss=True, **kw)
        _same_bits(V, want["V"], "V")
        _same_bits(b, want["b"], "b")
        _same_bits(ls, want["loss"], "loss")
        assert b.numpy().any()  # unlike the user side, the two gradients of a visit do not cancel in beta


# ------------------------------------------------------------------------------------------------ 2. purity
def _csr(hists, dev):
    off = np.concatenate([[0], np.cumsum([len(h) for h in hists])]).astype(np.int64)
    users = np.concatenate([np.asarray(h, dtype=np.int32) for h in hists] + [np.zeros(0, np.int32)])
    return torch.from_numpy(off).to(dev), torch.from_numpy(users).to(dev)


def _ops_call(m, hists, meta, args, err=None):
    """ops.fold_in_items of a CSR in the given order (no sorting by length: row r sits in lane group r of its wave)."""
    from torchrecsys_amd import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    m.net.eval()
    T = m.net.tables()
    fold = ops.item_fold(m.net.NET, T, m.n_items, m.n_factors, dev, m._item_meta_dev())
    st = m._device_stream("train")
    out = ops.fold_in_items(m.net.NET, T, fold, m.n_items, m._new_item_fold(meta, len(hists), dev), _csr(hists, dev),
                            st["user"], st["pos"], m._seen_csr(), *args, want_loss=True, err_flag=err)
    return [t.cpu() for t in out]


@pytest.mark.parametrize("D", [24, 22])  # 16-byte and 4-byte user-row loads; lane groups of 8
def test_a_row_does_not_depend_on_the_rest_of_the_call_or_the_prefetch_depth(tune, D):
    m = ref.make_model("fm", N_USERS, N_ITEMS, D, 2, seed=3, scale=0.3)
    args = ("bpr", E, 0.05, 0.125, 2, 7, True, True, 8)  # nu = 2
    hists = base.histories(N_USERS, 11)  # no reference is computed here: the 9 special lengths and 300 short ones
    meta = np.random.RandomState(6).randint(0, 5, (len(hists), 2))
    tune(FOLDIN_DEPTH=4)
    V, b, ls = _ops_call(m, hists, meta, args)
    assert V.abs().max() > 0.01 and b.abs().max() > 0.01
    picks = [3, 4, 5, 6, 7, 8] + list(range(40, 48))  # the long histories, then one item per lane position (40..47)
    assert {p % 8 for p in picks} == set(range(8))
    for p in picks:
        v1, b1, l1 = _ops_call(m, [hists[p]], meta[p:p + 1], args)
        assert torch.equal(v1[0], V[p]) and torch.equal(b1[0], b[p]) and torch.equal(l1[:, 0], ls[:, p]), p
    for depth in (1, 2, 8):
        tune(FOLDIN_DEPTH=depth)
        v2, b2, l2 = _ops_call(m, hists, meta, args)
        assert torch.equal(v2, V) and torch.equal(b2, b) and torch.equal(l2, ls), depth


# ------------------------------------------------------------------------------------------------ 3. smooth losses
@pytest.mark.parametrize("net,loss,D,M", SMOOTH)
def test_smooth_losses_against_float64(net, loss, D, M):
    m = smooth_inputs(net, D, M)
    frozen = _frozen(m, _meta(M), len(HISTS))
    kw = dict(seed=7, shuffle=True, reject_seen=True, max_tries=8)
    want = ref.fold_in(*frozen[:6], HISTS, *frozen[6:], net, loss, E, 0.05, 2.0 ** -3, nu=1, **kw)
    V, b, ls = m.fold_in_items(HISTS, metadata=_meta(M), epochs=E, lr=0.05, loss=loss, l2=2.0 ** -3,
                               negative_visits=1, return_loss=True, **kw)
    for name, got, w in (("V", V, want["V"]), ("b", b, want["b"]), ("loss", ls, want["loss"])):
        err = np.abs(got.numpy().astype(np.float64) - w)
        print("%s: max |got - float64| = %.3g (TOL %.3g)" % (name, err.max(), TOL))
        assert np.all(err <= TOL + TOL * np.abs(w)), (name, err.max())
    assert np.abs(want["V"]).max() > 0.05 and np.abs(want["b"]).max() > 0.01  # the rows moved


# ------------------------------------------------------------------------------------------------ 4. degenerate
def test_empty_histories_one_user_and_no_negative_visits():
    m = ref.make_model("linear", N_USERS, N_ITEMS, 8, 0, seed=1, int_range=(-3, 4))
    V0, b0, l0 = m.fold_in_items([[], [], []], epochs=3, return_loss=True)
    assert V0.shape == (3, 8) and not V0.any() and not b0.any() and l0.shape == (3, 3) and not l0.any()
    hs = [[0], [199], [5, 17], []]
    frozen = _frozen(m, None, len(hs))
    kw = dict(seed=3, shuffle=True, reject_seen=True, max_tries=8)
    for nu in (0, 1):
        want = ref.fold_in(*frozen[:6], base.clean(hs), *frozen[6:], "linear", "hinge", E, LR_EXACT, 0.0, nu=nu,
                           require_exact=True, **kw)
        V, b, ls = m.fold_in_items(hs, epochs=E, lr=LR_EXACT, l2=0.0, negative_visits=nu, return_loss=True, **kw)
        _same_bits(V, want["V"], "V")
        _same_bits(b, want["b"], "b")
        _same_bits(ls, want["loss"], "loss")
        assert V[:3].any() and not V[3].any() and float(b[3]) == 0
        for r in range(3):  # a call of one item
            v1, b1 = m.fold_in_items([hs[r]], epochs=E, lr=LR_EXACT, l2=0.0, negative_visits=nu, **kw)
            assert torch.equal(v1[0], V[r]) and torch.equal(b1[0], b[r])


def test_duplicate_and_unsorted_histories_fold_in_as_their_sorted_distinct_form():
    m = ref.make_model("fm", N_USERS, N_ITEMS, 24, 2, seed=2, scale=0.3)
    rs = np.random.RandomState(0)
    raw = [rs.randint(0, N_USERS, n).tolist() for n in (1, 5, 40, 300)] + [[7, 7, 7], [9, 3, 9, 3, 1]]
    a = m.fold_in_items(raw, metadata=META[:6], epochs=3, loss="bpr", return_loss=True)
    b = m.fold_in_items(base.clean(raw), metadata=torch.from_numpy(META[:6]), epochs=3, loss="bpr", return_loss=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert a[0].abs().max() > 0.01


def test_remapped_ids_go_in_and_come_out_as_original_ids():
    from torchrecsys_amd.model import TorchRecSys
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
    dense = [[0, 5, 299], [64], list(range(10, 40))]
    raw = [[3 + 7 * x for x in h] for h in dense]
    frozen = _frozen(m, None, 3)
    kw = dict(seed=1, shuffle=True, reject_seen=True, max_tries=8)
    want = ref.fold_in(*frozen[:6], dense, *frozen[6:], "linear", "hinge", E, LR_EXACT, 0.0, nu=1, require_exact=True,
                       **kw)
    V, b = m.fold_in_items(raw, epochs=E, lr=LR_EXACT, **kw)
    _same_bits(V, want["V"], "V")
    _same_bits(b, want["b"], "b")
    new_ids = [4, 1000, 12]  # none of 5 k + 11
    users = [3, 3 + 7 * 64, 3 + 7 * 150]
    ids, sc = m.recommend_with_new_items(users, new_ids, V, b, histories=raw, top_k=123, return_scores=True)
    S, c = frozen[2], frozen[3]
    Sx = np.concatenate([S[:, :16], want["V"]])
    cx = np.concatenate([c, want["b"]])
    seen = frozen[8]
    rows = [0, 64, 150]
    excl = [seen[1][seen[0][u]:seen[0][u + 1]].tolist() + [120 + j for j, h in enumerate(dense) if u in h] for u in rows]
    wi, wv = base.rank(frozen[0][rows], frozen[1][rows], Sx, cx, excl, 123)
    names = np.concatenate([raw_i.numpy(), np.array(new_ids), [-1]])
    assert np.array_equal(ids.numpy(), names[wi]) and np.array_equal(sc.numpy(), wv.astype(np.float32))
    assert 4 not in ids[0].tolist() and 1000 not in ids[1].tolist() and 4 in ids[1].tolist()
    with pytest.raises(IndexError, match="4"):
        m.fold_in_items([[3, 4]])
    with pytest.raises(ValueError, match="item id 16 is an item"):
        m.recommend_with_new_items(users, [16], V[:1], b[:1])


def test_a_user_or_stream_id_outside_its_table_is_skipped_and_flagged():
    m = ref.make_model("linear", N_USERS, N_ITEMS, 24, 0, seed=4, int_range=(-3, 4))
    dev = torch.device("cuda", torch.cuda.current_device())
    args = ("hinge", E, LR_EXACT, 0.0, 0, 5, True, False, 0)  # nu = 0: every visit of the bad row is one of its users
    good = [HISTS[3], HISTS[12], HISTS[20]]
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    V0, b0, l0 = _ops_call(m, good, None, args, err=err)
    assert int(err.item()) == 0 and V0.any()
    V1, b1, l1 = _ops_call(m, good[:1] + [[-5, N_USERS, 1 << 30]] + good[1:], None, args, err=err)
    assert int(err.item()) & 1
    keep = [0, 2, 3]
    assert torch.equal(V1[keep], V0) and torch.equal(b1[keep], b0) and torch.equal(l1[:, keep], l0)
    assert not V1[1].any() and float(b1[1]) == 0 and not l1[:, 1].any()  # every visit skipped: nothing learned


# ------------------------------------------------------------------------------------------------ 5. metadata only
@pytest.mark.parametrize("net", ["linear", "fm"])
def test_an_item_without_history_scores_as_a_zero_row_with_the_same_metadata(net):
    m = ref.make_model(net, N_USERS, N_ITEMS, 24, 2, seed=6, scale=0.3)
    twin = 17  # an existing item whose own row and 1-wide entry are zero
    sd = m.net.state_dict()
    sd["item.weight"][twin].zero_()
    sd["item_bias.weight" if net == "linear" else "linear_item.weight"][twin].zero_()
    meta = m.data_processor.item_meta_table[twin:twin + 1]
    V, b = m.fold_in_items([[]], metadata=meta)
    assert not V.any() and not b.any()
    users = list(range(0, N_USERS, 7))
    old_ids, old_sc = m.recommend(users, top_k=N_ITEMS, exclude_seen=False, return_scores=True)
    ids, sc = m.recommend_with_new_items(users, [5000], V, b, metadata=meta, top_k=N_ITEMS + 1, exclude_seen=False,
                                         return_scores=True)
    assert ids.shape == (len(users), N_ITEMS + 1)
    for r in range(len(users)):
        at, twin_at = ids[r].tolist().index(5000), old_ids[r].tolist().index(twin)
        assert torch.equal(sc[r, at], old_sc[r, twin_at])  # the same bits
        assert at == ids[r].tolist().index(twin) + 1  # a tie: the catalogue's row comes first
        keep = torch.arange(N_ITEMS + 1) != at
        assert torch.equal(ids[r][keep], old_ids[r]) and torch.equal(sc[r][keep], old_sc[r])


# ------------------------------------------------------------------------------------------------ 6. extension
def _two_models(net, D, M, n_new, hists):
    """A model of N_ITEMS items, and a second one of N_ITEMS + n_new items with the same interactions plus (u, new item
    j) for every user u of hists[j] (split_ratio = 1: every row is a train row, so the seen sets differ by exactly
    those pairs), the same user and metadata tables, and the first model's item rows followed by integer rows V, b."""
    from torchrecsys_amd.model import TorchRecSys
    rs = np.random.RandomState(D + M)
    u = np.concatenate([np.arange(N_USERS), rs.randint(0, N_USERS, 2800)])
    i = np.concatenate([np.arange(N_ITEMS), rs.randint(0, N_ITEMS, 2880)])
    tab = rs.randint(0, 5, (N_ITEMS + n_new, M))
    tab[:5] = np.arange(5)[:, None]  # both models see every metadata id: tables of the same size
    eu = np.concatenate([np.asarray(h, dtype=np.int64) for h in hists] + [np.zeros(0, dtype=np.int64)])
    ei = np.concatenate([np.full(len(h), N_ITEMS + j, dtype=np.int64) for j, h in enumerate(hists)])
    names = [f"m{j}" for j in range(M)] if M else None
    with contextlib.redirect_stdout(io.StringIO()):
        torch.manual_seed(0)
        a = TorchRecSys.from_tensors(torch.from_numpy(u), torch.from_numpy(i), n_users=N_USERS, n_items=N_ITEMS,
                                     item_metadata=torch.from_numpy(tab[:N_ITEMS]) if M else None, metadata_names=names,
                                     n_factors=D, net_type=net, split_ratio=1.0)
        b = TorchRecSys.from_tensors(torch.from_numpy(np.concatenate([u, eu])), torch.from_numpy(np.concatenate([i, ei])),
                                     n_users=N_USERS, n_items=N_ITEMS + n_new,
                                     item_metadata=torch.from_numpy(tab) if M else None, metadata_names=names,
                                     n_factors=D, net_type=net, split_ratio=1.0)
    g = torch.Generator().manual_seed(1)
    for p in a.net.parameters():
        p.data.copy_(0.3 * torch.randn(p.shape, generator=g))
    V = torch.randint(-2, 3, (n_new, D), generator=g).float() * 0.25
    beta = torch.randint(-2, 3, (n_new,), generator=g).float() * 0.25
    sa, sb = a.net.state_dict(), b.net.state_dict()
    lin = "item_bias.weight" if net == "linear" else "linear_item.weight"
    for k in sa:
        if k == "item.weight":
            sb[k].copy_(torch.cat([sa[k].cpu(), V]))
        elif k == lin:
            sb[k].copy_(torch.cat([sa[k].cpu(), beta[:, None]]))
        else:
            assert sa[k].shape == sb[k].shape, k
            sb[k].copy_(sa[k])
    return a, b, V, beta, tab[N_ITEMS:] if M else None


@pytest.mark.parametrize("M", [0, 2])
@pytest.mark.parametrize("net,D", [("linear", 24), ("fm", 50)])
def test_recommend_with_new_items_equals_recommend_of_a_larger_model(net, D, M):
    hists = [HISTS[3], [], HISTS[12], HISTS[8], [7]]  # 63 users, none, a few, all 200, one
    a, b, V, beta, meta = _two_models(net, D, M, len(hists), hists)
    new_ids = [900, 700, 800, 1000, 600]  # not in row order: the ids are names only
    names = torch.cat([torch.arange(N_ITEMS), torch.tensor(new_ids), torch.tensor([-1])])
    users = list(range(0, N_USERS, 3)) + [7, 7]
    before = {k: v.detach().cpu().clone() for k, v in a.net.state_dict().items()}
    for k in (1, 10, 125):
        for exclude in (True, False):
            want_ids, want_sc = b.recommend(users, top_k=k, exclude_seen=exclude, return_scores=True)
            ids, sc = a.recommend_with_new_items(users, new_ids, V, beta, metadata=meta, histories=hists, top_k=k,
                                                 exclude_seen=exclude, return_scores=True)
            assert torch.equal(ids, names[want_ids]) and torch.equal(sc, want_sc), (k, exclude)
            assert torch.equal(a.recommend_with_new_items(users, new_ids, V, beta, metadata=meta, histories=hists,
                                                          top_k=k, exclude_seen=exclude), ids)
    ids = a.recommend_with_new_items(users, new_ids, V, beta, metadata=meta, histories=hists, top_k=125)
    assert not (ids == 1000).any() and (ids == 700).any()  # everyone is in item 1000's history, nobody in item 700's
    assert (ids[users.index(7)] == 600).sum() == 0 and (ids[0] == 600).sum() == 1
    # without histories only the train items are dropped: the larger model without the added pairs' exclusions
    loose = a.recommend_with_new_items(users, new_ids, V, beta, metadata=meta, top_k=125)
    assert (loose == 1000).sum() == len(users)
    # no new item: recommend() itself
    e_meta = None if meta is None else meta[:0]
    for exclude in (True, False):
        i0, s0 = a.recommend_with_new_items(users, [], V[:0], beta[:0], metadata=e_meta, top_k=10, exclude_seen=exclude,
                                            return_scores=True)
        i1, s1 = a.recommend(users, top_k=10, exclude_seen=exclude, return_scores=True)
        assert torch.equal(i0, i1) and torch.equal(s0, s1)
    after = a.net.state_dict()
    for k_, v in before.items():
        assert torch.equal(after[k_].detach().cpu(), v), k_


# ------------------------------------------------------------------------------------------------ 7. planted
@pytest.mark.parametrize("net", ["linear", "fm"])
def test_planted_direction_is_recommended_and_negative_visits_hold_the_bias_down(net):
    D = 8
    U, S, hist, plus, minus = ref.planted(N_ITEMS, D, seed=D)
    m = ref.make_model(net, N_USERS, N_ITEMS, D, 0, seed=D, scale=0.0)  # every parameter zero, then the planted rows
    sd = m.net.state_dict()
    sd["user.weight"].copy_(torch.from_numpy(U).float())
    sd["item.weight"].copy_(torch.from_numpy(S).float())
    frozen = _frozen(m, None, 1)
    beta = {}
    for nu in (0, 1):
        want = ref.fold_in(*frozen[:6], [hist], *frozen[6:], net, "hinge", 8, 0.05, 0.0, nu=nu, seed=0)
        Vr, br = want["V"][0], want["b"][0]
        zc, zn = U @ S.T, U @ Vr + br  # FM: z_new = <U_u, v> + beta too (no metadata), and the order is z's
        tenth = np.sort(zc, axis=1)[:, -10]
        assert Vr[0] > 0 and np.all(zn[plus] > tenth[plus]) and np.all(zn[minus] < tenth[minus]), (nu, "reference")
        V, b = m.fold_in_items([hist], epochs=8, lr=0.05, negative_visits=nu, seed=0)
        assert float(V[0, 0]) > 0
        ids = m.recommend_with_new_items(np.concatenate([plus, minus]), [777], V, b, histories=[hist], top_k=10)
        assert bool((ids[:plus.size] == 777).any(dim=1).all()), nu  # held-out users of the factor: in their top 10
        assert not bool((ids[plus.size:] == 777).any()), nu  # users of the opposite sign: not
        assert not bool((m.recommend_with_new_items(hist, [777], V, b, histories=[hist], top_k=10) == 777).any())
        beta[nu] = (br, float(b[0]))
    assert beta[1][0] < beta[0][0] and beta[1][1] < beta[0][1]  # what the negative visits are there for


# ------------------------------------------------------------------------------------------------ 8. not written
def test_the_model_is_never_written():
    m = ref.make_model("fm", N_USERS, N_ITEMS, 24, 2, seed=9, scale=0.3)
    before = {k: v.detach().cpu().clone() for k, v in m.net.state_dict().items()}
    V, b, ls = m.fold_in_items(HISTS[:40], metadata=META[:40], return_loss=True)
    assert V.abs().max() > 0.01 and ls.shape == (8, 40)
    m.recommend_with_new_items([0, 1, 2], list(range(500, 540)), V, b, metadata=META[:40], histories=HISTS[:40])
    after = m.net.state_dict()
    assert set(after) == set(before)
    for k, v in before.items():
        assert torch.equal(after[k].detach().cpu(), v), k
    assert m.n_items == N_ITEMS and m.net.item.weight.shape[0] == N_ITEMS
