# -*- coding: utf-8 -*-
"""The sequence model on the MI355X (trs_seq_fwd_bwd, trs_seq_user_rows, csrc/seq.hip; fit_sequence, recommend_next,
recommend_for_sequences, evaluate_next) against the numpy restatement tests/seq_ref.py: the staged
gradients of every row shape, the anchor to trs_score_fwd_bwd, out-of-range ids, the query rows bit for bit, one SGD
step, retrieval against a brute-force ranking, the planted order, and what is deterministic."""
import contextlib
import io

import numpy as np
import pytest
import torch

import seq_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NU, NI = 40, 30
LENGTHS = tuple(range(1, 13))  # sequence lengths 1..12
SHAPE_D = (8, 16, 32, 64, 128, 256, 512, 1024, 3, 10, 50, 130)  # one D per entry of TRS_ROW_SHAPES


def _ops():
    from torchrecsys_amd import ops
    return ops


def _loss_id(loss):
    from torchrecsys_amd import _lib
    return _lib.LOSS_ID[loss]


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


def build_net(T):
    """A Linear scorer on the device holding the restatement's U, V, b (user_bias = 0) and C beside it."""
    from torchrecsys_amd.collaborative.linear import Linear
    nu, D = T["U"].shape
    with contextlib.redirect_stdout(io.StringIO()):
        net = Linear(nu, T["V"].shape[0], {}, D, use_metadata=False).to(DEV)
    with torch.no_grad():
        ps = net.table_params()
        ps[0].copy_(torch.from_numpy(T["U"]))
        ps[1].copy_(torch.from_numpy(T["V"]))
        ps[2].zero_()
        ps[3].copy_(torch.from_numpy(T["b"]).view(-1, 1))
    return net, torch.from_numpy(T["C"]).to(DEV).contiguous()


def sequences(seed=1):
    """40 users x 30 items, lengths 1..12; user 5's sequence repeats one item, so a positive sits in its own context."""
    off, ids = ref.make_sequences(NU, NI, LENGTHS, seed)
    ids[off[5]:off[6]] = 7
    return off, ids


def batch(off, ids, B, seed, L=16):
    """B triples: entries drawn over the whole CSR, forced to hold (from B = 63 on) a first entry, an entry with fewer
    than L predecessors, a positive that is also in its own context, and repeated users and items."""
    rs = np.random.RandomState(seed)
    entry = rs.randint(0, int(off[-1]), B).astype(np.int64)
    if B >= 4:
        entry[0] = off[3]          # a first entry: no context
        entry[1] = off[5] + 2      # user 5: the positive 7 is also both context items
        entry[2] = off[11] + 1     # one predecessor
        entry[3] = off[11] + 1     # the same triple's user and items again
    user = np.searchsorted(off, entry, side="right") - 1
    pos = ids[entry]
    neg = rs.randint(0, NI - 1, B)
    neg = neg + (neg >= pos)
    if B >= 63:
        k = entry - off[user]
        assert (k == 0).any() and ((k > 0) & (k < L)).any() and (k >= 8).any()
        assert any(pos[t] in ids[entry[t] - min(k[t], L):entry[t]] for t in range(B) if k[t])
        assert len(set(user.tolist())) < B and len(set(pos.tolist() + neg.tolist())) < 2 * B
    return user.astype(np.int32), entry, neg.astype(np.int32)


def run_stage(net, C, off, ids, user, entry, neg, w, loss, forward_only=False, err=None, inv_B=None):
    ops = _ops()
    loss_sum = torch.zeros(1, device=DEV)
    auc = torch.zeros(1, dtype=torch.int32, device=DEV)
    gr, gl, cid = ops.seq_fwd_bwd(net.tables(), C, (dev(off, np.int64), dev(ids, np.int32)), dev(user, np.int32),
                                  dev(entry, np.int64), dev(neg, np.int32), dev(w, np.float32), _loss_id(loss), loss_sum,
                                  auc, err_flag=err, forward_only=forward_only, inv_B=inv_B)
    torch.cuda.synchronize()
    return gr, gl, cid, float(loss_sum.item()), int(auc.item())


def measured_tolerance(T, off, ids, user, entry, neg, w, loss):
    """(float64 staged values, 4 x the largest deviation of the float32 restatement from them over its three summation
    orders) — measured on the restatement, on the case's own inputs."""
    want = ref.staged(T, off, ids, user, entry, neg, w, loss)
    dev_rows = dev_lin = dev_loss = 0.0
    for order in ref.ORDERS:
        g = ref.staged(T, off, ids, user, entry, neg, w, loss, dtype=np.float32, order=order)
        dev_rows = max(dev_rows, float(np.abs(g[0] - want[0]).max()))
        dev_lin = max(dev_lin, float(np.abs(g[1] - want[1]).max()))
        dev_loss = max(dev_loss, abs(g[3] - want[3]))
    return want, 4 * dev_rows, 4 * dev_lin, 4 * dev_loss


@pytest.mark.parametrize("loss", ["bpr", "hinge"])
@pytest.mark.parametrize("L", [0, 1, 3, 8, 16])
@pytest.mark.parametrize("B", [1, 63, 257])
@pytest.mark.parametrize("D", SHAPE_D)
def test_staged_gradients_against_float64(D, B, L, loss):
    """Every row shape x batch size x context length x loss.  Tolerance per element: 4 x the largest deviation of the
    float32 restatement from the float64 one over its summation orders (sequential, pairwise, lane-group tree) on the
    same inputs, measured per case on the CPU.  Over the grid the largest deviation is 1.05e-6 and the largest tolerance
    4.2e-6 (grad_rows at D = 1024, B = 1, L = 16, bpr; staged values up to 1.5); a one-row batch on which the hinge is
    inactive stages exact zeros in every precision, and its tolerance is 0.  Absent slots are exactly 0 with id 0; the
    forward-only mode gives the same loss (to the order of the blocks' atomic adds) and the same count."""
    off, ids = sequences()
    T = ref.make_tables(NU, NI, D, seed=D + 1)
    user, entry, neg = batch(off, ids, B, seed=B + L)
    w = ref.weights(L, 0.7)
    net, C = build_net(T)
    (wr, wl, wc, wloss, _), tol_r, tol_l, tol_loss = measured_tolerance(T, off, ids, user, entry, neg, w, loss)
    gr, gl, cid, loss_sum, auc = run_stage(net, C, off, ids, user, entry, neg, w, loss)
    gr, gl = gr.cpu().numpy().astype(np.float64), gl.cpu().numpy().astype(np.float64)
    err_r, err_l = float(np.abs(gr - wr).max()), float(np.abs(gl - wl).max())
    print(f"D={D} B={B} L={L} {loss}: rows {err_r:.3g} (tol {tol_r:.3g}), lin {err_l:.3g} (tol {tol_l:.3g}), "
          f"loss {abs(loss_sum - wloss):.3g} (tol {tol_loss:.3g})")
    assert gr.shape == (3 + L, B, D) and gl.shape == (3, B)
    assert err_r <= tol_r and err_l <= tol_l and abs(loss_sum - wloss) <= max(tol_loss, 1e-6 * abs(wloss))
    if L:
        assert np.array_equal(cid.cpu().numpy(), wc)
        k = entry - off[user]
        for l in range(L):
            absent = k <= l
            assert not gr[3 + l][absent].any() and not wc[l][absent].any()
    _, _, _, loss_fwd, auc_fwd = run_stage(net, C, off, ids, user, entry, neg, w, loss, forward_only=True)
    # (the blocks' partial sums meet in one float atomic: their order, and so the last bits, vary between launches)
    assert abs(loss_fwd - loss_sum) <= 1e-6 * abs(loss_sum) and auc_fwd == auc


@pytest.mark.parametrize("loss", ["bpr", "hinge"])
@pytest.mark.parametrize("D", [64, 130])
@pytest.mark.parametrize("L,first_only", [(0, False), (4, True)])
@pytest.mark.parametrize("B", [4, 257])
def test_anchor_to_the_pair_kernel(D, B, L, first_only, loss):
    """L = 0, and L = 4 on first entries only (no slot present): user / positive / negative fields, grad_lin, the loss
    sum and the AUC count are trs_score_fwd_bwd(TRS_NET_LINEAR)'s on the same (user, positive, negative), bit for bit.
    B = 4 is one workgroup at both widths: the loss sum is one atomic add and so bit-identical.  At B = 257 both kernels
    add their workgroups' partial sums with float atomics in whatever order they finish, so the two sums (like two
    launches of either kernel) agree to that order only, 1e-6 relative; everything else stays bit for bit."""
    ops = _ops()
    off, ids = sequences()
    T = ref.make_tables(NU, NI, D, seed=D + 2)
    user, entry, neg = batch(off, ids, B, seed=9)
    if first_only:
        entry = off[user.astype(np.int64)]
        pos = ids[entry]
        neg = np.where(neg == pos, (neg + 1) % NI, neg).astype(np.int32)
    net, C = build_net(T)
    gr, gl, cid, loss_sum, auc = run_stage(net, C, off, ids, user, entry, neg, ref.weights(L, 0.7), loss)
    Bt, keep = ops.make_batch(dev(user, np.int32), dev(ids[entry], np.int32), dev(neg, np.int32))
    ls = torch.zeros(1, device=DEV)
    ac = torch.zeros(1, dtype=torch.int32, device=DEV)
    _, _, wr, wl = ops.score_fwd_bwd("linear", net.tables(), Bt, B, D, 0, DEV, ls, ac, want_scores=False,
                                     loss=_loss_id(loss))
    torch.cuda.synchronize()
    assert torch.equal(gr[:3], wr) and torch.equal(gl, wl)
    assert int(ac.item()) == auc and loss_sum > 0
    assert float(ls.item()) == loss_sum if B == 4 else abs(float(ls.item()) - loss_sum) <= 1e-6 * loss_sum
    if L:
        assert not gr[3:].any() and not cid.any()


def test_out_of_range_ids_zero_exactly_their_rows():
    off, ids = sequences()
    D, L, B = 50, 3, 63
    T = ref.make_tables(NU, NI, D, seed=3)
    user, entry, neg = batch(off, ids, B, seed=4)
    w = ref.weights(L, 0.7)
    net, C = build_net(T)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    good = run_stage(net, C, off, ids, user, entry, neg, w, "bpr", err=err)
    assert err.item() == 0
    bu, be, bn = user.copy(), entry.copy(), neg.copy()
    bu[10], bu[11] = NU, -1                       # a user outside the table
    bn[20], bn[21] = NI, -5                       # a negative outside the table
    be[30], be[31], be[32] = off[user[30] + 1], off[user[31]] - 1, int(off[-1]) + 1000  # entries outside the user's range
    bad_rows = [10, 11, 20, 21, 30, 31, 32]
    got = run_stage(net, C, off, ids, bu, be, bn, w, "bpr", err=err)
    assert err.item() == 1
    keep = np.ones(B, dtype=bool)
    keep[bad_rows] = False
    gr, gl = got[0].cpu().numpy(), got[1].cpu().numpy()
    wr, wl = good[0].cpu().numpy(), good[1].cpu().numpy()
    assert not gr[:, bad_rows].any() and not gl[:, bad_rows].any()
    assert np.array_equal(gr[:, keep].view(np.int32), wr[:, keep].view(np.int32))
    assert np.array_equal(gl[:, keep].view(np.int32), wl[:, keep].view(np.int32))
    assert np.array_equal(got[2].cpu().numpy()[:, keep], good[2].cpu().numpy()[:, keep])
    want_loss = ref.staged(T, off, ids, user[keep], entry[keep], neg[keep], w, "bpr", inv_B=1.0 / B)[3]
    assert abs(got[3] - want_loss) < 1e-5 * want_loss


@pytest.mark.parametrize("D,ld", [(8, 8), (16, 32), (64, 64), (130, 256), (10, 16), (3, 3), (1024, 1024)])
def test_query_rows_bit_for_bit(D, ld):
    """trs_seq_user_rows against the float32 loop: users -1 (no user row), empty sequences, sequences shorter and longer
    than L, and a padded output stride whose padding is left alone."""
    ops = _ops()
    L = 4
    off, ids = ref.make_sequences(17, NI, (0, 1, 2, 4, 5, 9, 0, 3), seed=D)
    users = np.arange(17, dtype=np.int64) * 2 % NU
    users[[2, 6, 9]] = -1
    T = ref.make_tables(NU, NI, D, seed=D + 5)
    w = ref.weights(L, 0.7)
    net, C = build_net(T)
    seq = (dev(off, np.int64), dev(ids, np.int32))
    out = torch.full((17, ld), 7.0, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.seq_user_rows(net.tables(), C, seq, dev(users, np.int64), dev(w, np.float32), ld=ld, out=out, err_flag=err)
    got = out.cpu().numpy()
    want = ref.user_rows(T, off, ids, users, w)
    assert err.item() == 0
    assert np.array_equal(got[:, :D].view(np.int32), want.view(np.int32))
    assert (got[:, D:] == 7.0).all()
    # no users at all: the anonymous form; an empty sequence is an all-zero row
    anon = ops.seq_user_rows(net.tables(), C, seq, None, dev(w, np.float32)).cpu().numpy()
    assert np.array_equal(anon.view(np.int32), ref.user_rows(T, off, ids, None, w).view(np.int32))
    assert not anon[0].any() and not anon[6].any()
    # a user beyond the table: bit 0, a zero row, the neighbours unchanged
    users[4] = NU
    bad = ops.seq_user_rows(net.tables(), C, seq, dev(users, np.int64), dev(w, np.float32), err_flag=err).cpu().numpy()
    assert err.item() == 1 and not bad[4].any()
    assert np.array_equal(np.delete(bad, 4, 0).view(np.int32), np.delete(want, 4, 0).view(np.int32))


def _trainer(net, C, off, ids, w, cap, lr, loss):
    from torchrecsys_amd.engine import SequenceTrainer
    return SequenceTrainer(net, C, dev(w, np.float32), (dev(off, np.int64), dev(ids, np.int32)), cap, lr, _loss_id(loss))


def _tables_of(net, C):
    ps = net.table_params()
    return {"U": ps[0].detach().cpu().numpy(), "V": ps[1].detach().cpu().numpy(),
            "b": ps[3].detach().cpu().numpy()[:, 0], "C": C.cpu().numpy()}


def _ulps(got, want, before):
    """|got - want| in units of the last place of the larger of the result and the update that was added to `before`
    (float32): one rounding of the update is at most one such unit."""
    want, before = want.astype(np.float32), before.astype(np.float32)
    unit = np.spacing(np.maximum(np.abs(want), np.abs(want - before))).astype(np.float64)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / unit


def _disjoint_step(loss, lr=0.5, D=64, L=2, n_users=12, n_items=60):
    """One seq_step on a batch in which no table row is referenced twice (asserted): the tables before and after, the
    inputs, and the rows each table's update touches."""
    # user u's sequence is (5u, 5u+1, 5u+2): entry 2 has context 5u+1, 5u and positive 5u+2; negatives 5u+3
    off = np.arange(n_users + 1, dtype=np.int64) * 3
    ids = (np.repeat(np.arange(n_users), 3) * 5 + np.tile(np.arange(3), n_users)).astype(np.int32)
    user = np.arange(n_users, dtype=np.int32)
    entry = off[:-1] + 2
    neg = (user * 5 + 3).astype(np.int32)
    refs_v = np.concatenate([ids[entry], neg])
    refs_c = np.concatenate([ids[entry - 1], ids[entry - 2]])
    assert len(set(user.tolist())) == n_users and len(set(refs_v.tolist())) == 2 * n_users
    assert len(set(refs_c.tolist())) == 2 * n_users
    T = ref.make_tables(n_users, n_items, D, seed=8)
    w = ref.weights(L, 0.7)
    net, C = build_net(T)
    before = _tables_of(net, C)
    loss_slot = torch.zeros(1, device=DEV)
    tr = _trainer(net, C, off, ids, w, n_users, lr, loss)
    tr.seq_step(dev(user, np.int32), dev(entry, np.int64), loss_slot, 0, 0, neg=dev(neg, np.int32))
    tr.check_errors()
    got = _tables_of(net, C)
    touched = {"U": user, "V": refs_v, "b": refs_v, "C": refs_c}
    for k in got:  # untouched rows are bit-identical, touched ones moved
        rows = np.unique(touched[k])
        rest = np.setdiff1d(np.arange(got[k].shape[0]), rows)
        assert np.array_equal(got[k][rest].view(np.int32), before[k][rest].view(np.int32)), k
        assert (got[k][rows] != before[k][rows]).any(), k
    return T, before, got, (off, ids, user, entry, neg, w), touched, float(loss_slot.item())


def test_one_step_without_a_shared_row():
    """After seq_step on a batch that references no table row twice, every table equals the float32 restatement's to
    one rounding of the update (<= 1 ulp per element), untouched rows bit-identical.  The loss is the hinge: its
    coefficient is exactly +-1/B in the kernel and in the restatement, so the rounding of the update is the only place
    where the two can part.  (Under bpr the coefficient goes through expf, whose device and host implementations differ
    in the last bit; V[p] and V[n] cancel in the user's gradient, so that bit is not bounded in units of the result —
    2 units were measured on U.  bpr is held to the float64 step below.)"""
    lr = 0.5
    T, before, got, (off, ids, user, entry, neg, w), touched, loss_sum = _disjoint_step("hinge", lr)
    want = {k: v.copy() for k, v in T.items()}
    want_loss = ref.step(want, off, ids, user, entry, neg, w, "hinge", lr, dtype=np.float32)
    for k in got:
        rows = np.unique(touched[k])
        assert _ulps(got[k][rows], want[k][rows], before[k][rows]).max() <= 1.0, k
    assert abs(loss_sum - want_loss) < 1e-5 * want_loss


def test_one_bpr_step_without_a_shared_row_against_float64():
    """The same batch under bpr against the float64 step, per table within 4 x the largest deviation the float32
    restatement's step shows from it over its three summation orders (measured here on the CPU: 2.9e-8 for b to 5.1e-8 for V, at
    values up to 1.2)."""
    lr = 0.5
    T, before, got, (off, ids, user, entry, neg, w), touched, loss_sum = _disjoint_step("bpr", lr)
    want = {k: v.copy() for k, v in T.items()}
    want_loss = ref.step(want, off, ids, user, entry, neg, w, "bpr", lr)
    for k in got:
        dev32 = 0.0
        for order in ref.ORDERS:
            t32 = {kk: v.copy() for kk, v in T.items()}
            ref.step(t32, off, ids, user, entry, neg, w, "bpr", lr, dtype=np.float32, order=order)
            dev32 = max(dev32, float(np.abs(t32[k] - want[k]).max()))
        err = float(np.abs(got[k] - want[k]).max())
        print(f"{k}: max |got - float64| = {err:.3g} (tol {4 * dev32:.3g})")
        assert err <= 4 * dev32, k
    assert abs(loss_sum - want_loss) < 1e-5 * want_loss


def test_one_step_with_heavy_repetition():
    """B = 257 triples over 5 items and 3 users: every row collects dozens of atomic adds.  Against the float64 step,
    per table, within 4 x the largest deviation the float32 restatement shows from it when its scatter order is
    permuted (8 permutations, measured in the test on the CPU: U 3.9e-7, V 2.7e-7, b 1.2e-7, C 2.6e-7 at values up to
    1.0, so the tolerances are 1.6e-6, 1.1e-6, 5.0e-7 and 1.0e-6; the step moves the tables by 0.02 to 0.07)."""
    D, L, lr, B = 16, 2, 0.5, 257
    n_users, n_items = 3, 5
    rs = np.random.RandomState(12)
    off = np.array([0, 40, 80, 120], dtype=np.int64)
    ids = rs.randint(0, n_items, 120).astype(np.int32)
    entry = rs.randint(0, 120, B).astype(np.int64)
    user = (entry // 40).astype(np.int32)
    neg = rs.randint(0, n_items - 1, B)
    neg = (neg + (neg >= ids[entry])).astype(np.int32)
    T = ref.make_tables(n_users, n_items, D, seed=13)
    w = ref.weights(L, 0.7)
    want = {k: v.copy() for k, v in T.items()}
    ref.step(want, off, ids, user, entry, neg, w, "bpr", lr)
    tol = {k: 0.0 for k in T}
    for p in range(8):
        t32 = {k: v.copy() for k, v in T.items()}
        ref.step(t32, off, ids, user, entry, neg, w, "bpr", lr, dtype=np.float32,
                 scatter_order=np.random.RandomState(p).permutation(B))
        for k in T:
            tol[k] = max(tol[k], 4 * float(np.abs(t32[k] - want[k]).max()))
    net, C = build_net(T)
    tr = _trainer(net, C, off, ids, w, B, lr, "bpr")
    tr.seq_step(dev(user, np.int32), dev(entry, np.int64), torch.zeros(1, device=DEV), 0, 0, neg=dev(neg, np.int32))
    tr.check_errors()
    got = _tables_of(net, C)
    for k in T:
        err = float(np.abs(got[k] - want[k]).max())
        print(f"{k}: max |got - float64| = {err:.3g} (tol {tol[k]:.3g})")
        assert err <= tol[k] and np.abs(want[k] - T[k]).max() > 1e-3, k


def test_sampled_negatives_are_the_existing_samplers():
    """seq_step draws its negatives with trs_sample_neg under (seed, offset + t): given the same draw explicitly, the
    tables end equal to 1e-6 absolute (values up to 1.5) — not bit for bit, because the batch shares rows and the float
    atomics of the two runs may meet on them in another order; a different draw would move rows by 1e-3 and more.  No
    negative equals its row's positive."""
    ops = _ops()
    off, ids = sequences()
    T = ref.make_tables(NU, NI, 16, seed=2)
    user, entry, _ = batch(off, ids, 63, seed=5)
    w = ref.weights(3, 0.7)
    neg = ops.sample_neg(dev(ids[entry], np.int32), NI, 77, 5)
    assert not bool((neg.cpu().numpy() == ids[entry]).any())
    outs = []
    for given in (None, neg):
        net, C = build_net(T)
        tr = _trainer(net, C, off, ids, w, 63, 0.3, "bpr")
        tr.seq_step(dev(user, np.int32), dev(entry, np.int64), torch.zeros(1, device=DEV), 77, 5, neg=given)
        outs.append({k: torch.from_numpy(v) for k, v in _tables_of(net, C).items()})
    # (float atomics: the order of the adds into a shared row may differ between the two runs)
    for k in outs[0]:
        assert torch.allclose(outs[0][k], outs[1][k], rtol=0, atol=1e-6), k


# ------------------------------------------------------------------------------------------------ through the model
def make_model(n_users, n_items, D, users, items, **kw):
    from torchrecsys_amd.model import TorchRecSys
    with contextlib.redirect_stdout(io.StringIO()):
        torch.manual_seed(0)
        return TorchRecSys.from_tensors(torch.from_numpy(users), torch.from_numpy(items), n_users=n_users,
                                        n_items=n_items, n_factors=D, net_type="linear", split_ratio=1.0,
                                        dynamic_neg_sampling=True, rng="device", **kw)


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def retrieval_model():
    """60 users x 50 items, D = 16, fitted for two epochs so that C is not zero; b and C perturbed so that nothing ties
    by accident.  User 7 has two interactions, user 8 one, and a 61st user (60) none at all."""
    rs = np.random.RandomState(21)
    lens = rs.randint(3, 15, 60)
    lens[7], lens[8] = 2, 1
    users = np.repeat(np.arange(60), lens)
    items = rs.randint(0, 50, users.size)
    m = make_model(61, 50, 16, users, items)
    quiet(m.fit_sequence, epochs=2, lr=2.0, batch_size=64, context=3)
    with torch.no_grad():
        g = torch.Generator().manual_seed(3)
        m.net.seq_context.add_(0.3 * torch.randn(50, 16, generator=g).to(DEV))
        m.net.item_bias.weight.add_(0.1 * torch.randn(50, 1, generator=g).to(DEV))
    off = np.concatenate([[0], np.cumsum(lens), [lens.sum()]]).astype(np.int64)
    return m, off, items.astype(np.int32)


def brute_force(rows, V, b, k, seen_lists):
    """Position-for-position top-k of rows @ V.T + b in float64 (value descending, ties by ascending id, seen excluded,
    -1 / -inf padding), from the kernel's own composed rows."""
    S = rows.astype(np.float64) @ V.astype(np.float64).T + b.astype(np.float64)[None, :]
    ids = np.full((rows.shape[0], k), -1, dtype=np.int64)
    sc = np.full((rows.shape[0], k), -np.inf)
    for r in range(rows.shape[0]):
        cand = np.setdiff1d(np.arange(S.shape[1]), np.asarray(sorted(seen_lists[r]), dtype=np.int64))
        order = cand[np.lexsort((cand, -S[r, cand]))][:k]
        ids[r, :order.size], sc[r, :order.size] = order, S[r, order]
    return ids, sc


def assert_ranking(got_ids, got_sc, want_ids, want_sc):
    """Same ids position for position wherever the float64 scores of neighbouring positions differ by more than the
    fp32 inner product's rounding (1e-5); the scores agree to 1e-5 everywhere; the padding is identical.  The float64
    brute force cannot order a nearer tie the way an fp32 matrix-core sum does, so such positions are held by their
    scores alone; 50 scores spread over about 2 leave a neighbour within 1e-5 at about 5e-4 of the positions, and at
    least 99 % of them must be clear."""
    got_ids, got_sc = got_ids.numpy(), got_sc.numpy().astype(np.float64)
    assert np.array_equal(got_ids == -1, want_ids == -1) and np.array_equal(np.isneginf(got_sc), np.isneginf(want_sc))
    real = want_ids >= 0
    assert np.abs(got_sc[real] - want_sc[real]).max() < 1e-5
    gap = np.full(want_sc.shape, np.inf)
    d = np.abs(np.diff(np.where(real, want_sc, np.nan), axis=1))
    gap[:, 1:] = np.fmin(gap[:, 1:], np.nan_to_num(d, nan=np.inf))
    gap[:, :-1] = np.fmin(gap[:, :-1], np.nan_to_num(d, nan=np.inf))
    clear = real & (gap > 1e-5)
    assert clear[real].mean() >= 0.99 and np.array_equal(got_ids[clear], want_ids[clear])


@pytest.fixture(scope="module")
def fitted():
    return retrieval_model()


@pytest.mark.parametrize("exclude_seen", [True, False])
def test_recommend_next_against_brute_force(fitted, exclude_seen):
    ops = _ops()
    m, off, ids = fitted
    q = np.array([0, 7, 8, 8, 59, 31, 60, 12], dtype=np.int64)
    C, w = m.net.seq_context, m.net.seq_weights
    T = _tables_of(m.net, C)
    sub_off = np.concatenate([[0], np.cumsum(off[q + 1] - off[q])]).astype(np.int64)
    sub_ids = np.concatenate([ids[off[u]:off[u + 1]] for u in q]).astype(np.int32)
    rows = ops.seq_user_rows(m.net.tables(), C, (dev(sub_off, np.int64), dev(sub_ids, np.int32)), dev(q, np.int64), w)
    rows = rows.cpu().numpy()
    assert np.array_equal(rows.view(np.int32), ref.user_rows(T, sub_off, sub_ids, q, w.cpu().numpy()).view(np.int32))
    seen = [set(ids[off[u]:off[u + 1]].tolist()) if exclude_seen else set() for u in q]
    for k in (10, 50):  # 50 = the catalogue: more than the candidates when the seen items are excluded
        got_ids, got_sc = quiet(m.recommend_next, q, top_k=k, exclude_seen=exclude_seen, return_scores=True)
        want_ids, want_sc = brute_force(rows, T["V"], T["b"], k, seen)
        assert got_ids.shape == (len(q), k) and got_ids.dtype == torch.int64
        assert (np.delete(want_ids, 6, 0)[:, -1] == -1).all() == (k == 50 and exclude_seen)  # (row 6 has seen nothing)
        assert_ranking(got_ids, got_sc, want_ids, want_sc)
    assert torch.equal(quiet(m.recommend_next, q, top_k=10, exclude_seen=exclude_seen), got_ids[:, :10])


@pytest.mark.parametrize("exclude_seen", [True, False])
def test_recommend_for_sequences_against_brute_force(fitted, exclude_seen):
    m, off, ids = fitted
    sessions = [[3, 9, 9, 4], [], [11], [1, 2, 3, 4, 5, 6, 7, 8], np.array([49, 0])]
    C, w = m.net.seq_context, m.net.seq_weights
    T = _tables_of(m.net, C)
    s_off = np.concatenate([[0], np.cumsum([len(s) for s in sessions])]).astype(np.int64)
    s_ids = np.concatenate([np.asarray(s, dtype=np.int32) for s in sessions])
    rows = ref.user_rows(T, s_off, s_ids, None, w.cpu().numpy())
    seen = [set(np.asarray(s).tolist()) if exclude_seen else set() for s in sessions]
    for k in (10, 50):
        got_ids, got_sc = quiet(m.recommend_for_sequences, sessions, top_k=k, exclude_seen=exclude_seen,
                                return_scores=True)
        want_ids, want_sc = brute_force(rows, T["V"], T["b"], k, seen)
        assert_ranking(got_ids, got_sc, want_ids, want_sc)
    # the empty session ranks by b alone
    by_b = np.lexsort((np.arange(50), -T["b"].astype(np.float64)))[:10]
    assert np.array_equal(got_ids.numpy()[1, :10], by_b)
    assert np.array_equal(got_sc.numpy()[1, :10], T["b"][by_b])


@pytest.mark.parametrize("exclude_seen", [True, False])
def test_queries_without_any_item(fitted, exclude_seen):
    """Batches in which NO sequence holds an item (the id array is empty): an empty session, two of them, and a single
    user without train rows.  The sessions rank by b alone, the user by <U[u], V[i]> + b[i]."""
    m, off, ids = fitted
    T = _tables_of(m.net, m.net.seq_context)
    by_b = np.lexsort((np.arange(50), -T["b"].astype(np.float64)))[:10]
    for sessions in ([[]], [[], []], [np.zeros(0, dtype=np.int64)]):
        got_ids, got_sc = quiet(m.recommend_for_sequences, sessions, top_k=10, exclude_seen=exclude_seen,
                                return_scores=True)
        assert got_ids.shape == (len(sessions), 10)
        for r in range(len(sessions)):
            assert np.array_equal(got_ids.numpy()[r], by_b) and np.array_equal(got_sc.numpy()[r], T["b"][by_b])
    got_ids, got_sc = quiet(m.recommend_next, [60], top_k=10, exclude_seen=exclude_seen, return_scores=True)
    want_ids, want_sc = brute_force(T["U"][60:61], T["V"], T["b"], 10, [set()])
    assert_ranking(got_ids, got_sc, want_ids, want_sc)
    assert torch.equal(quiet(m.recommend_next, [60, 60], top_k=10, exclude_seen=exclude_seen), got_ids.repeat(2, 1))


@pytest.mark.parametrize("split,on_gpu", [("reference", False), ("reference", True), ("device", True)])
def test_ordered_csr_of_a_real_split(split, on_gpu):
    """split_ratio < 1 through the model, both ways of drawing the split: train_rows() names the input position of
    every train row, and _sequences() — on the device — is the groupby of those rows by input position, then by
    timestamp with ties by position (set_sequence_order)."""
    import pandas as pd
    from torchrecsys_amd.model import TorchRecSys
    rs = np.random.RandomState(31)
    n = 500
    df = pd.DataFrame({"u": rs.randint(0, 23, n), "i": rs.randint(0, 17, n), "pos": np.arange(n), "ts": rs.randint(0, 25, n)})
    u, i = torch.from_numpy(df["u"].to_numpy()), torch.from_numpy(df["i"].to_numpy())
    if on_gpu:
        u, i = u.to(DEV), i.to(DEV)
    with contextlib.redirect_stdout(io.StringIO()):
        m = TorchRecSys.from_tensors(u, i, n_users=23, n_items=17, n_factors=8, net_type="linear", split_ratio=0.8,
                                     dynamic_neg_sampling=True, rng="device", split=split)
    rows = m.data_processor.train_rows().cpu().numpy()
    assert rows.size == 400 and np.unique(rows).size == 400 and not (np.diff(rows) > 0).all()
    assert np.array_equal(m.data_processor.train_data["user_id"].cpu().numpy(), df["u"].to_numpy()[rows])
    assert np.array_equal(m.data_processor.train_data["pos_item_id"].cpu().numpy(), df["i"].to_numpy()[rows])
    tr = df.iloc[rows]

    def groupby(by):
        g = tr.sort_values(by, kind="stable").groupby("u")["i"].apply(list)
        return [g.get(k, []) for k in range(23)]

    def current():
        off, ids = m._sequences()
        assert off.is_cuda and ids.is_cuda and ids.dtype == torch.int32
        off, ids = off.cpu().numpy(), ids.cpu().numpy()
        return [ids[off[k]:off[k + 1]].tolist() for k in range(23)]

    assert current() == groupby(["pos"])
    m.set_sequence_order(df["ts"].to_numpy())
    by_ts = groupby(["ts", "pos"])
    assert current() == by_ts and by_ts != groupby(["pos"])
    quiet(m.fit_sequence, epochs=1, context=2, batch_size=64)  # without timestamps: the order stays
    assert current() == by_ts
    m.set_sequence_order()
    assert current() == groupby(["pos"])


def test_learns_order():
    """The planted order (seq_ref.PLANTED: 300 users x 200 items, sequences of 30, next = perm[current] with probability
    0.8; context 1, D = 16, bpr, lr 10, batches of 128, 20 epochs).  The float64 restatement reaches hit_rate@10 =
    0.840, 0.837, 0.827 over three seeds (spread 0.013; 0.100, 0.097, 0.070 without context), checked on the CPU by
    tests/test_seq_host.py.  Bars: at least 0.8 x the lowest of the three (0.661), and at least twice the same model's
    context-free value."""
    P = ref.PLANTED
    users, items, off, ids = ref.planted_case()
    m = make_model(P["n_users"], P["n_items"], P["D"], users, items, seed=0)
    losses = quiet(m.fit_sequence, epochs=P["epochs"], lr=P["lr"], batch_size=P["batch"], context=P["context"],
                   decay=P["decay"], loss=P["loss"], holdout_last=True, return_loss=True)
    out = quiet(m.evaluate_next, P["k"])
    print(out, losses.tolist())
    assert out["n_users"] == P["n_users"] and losses[-1] < losses[0]
    hit, plain = out["hit_rate@10"], out["hit_rate@10_no_context"]
    assert hit >= 0.8 * min(ref.PLANTED_REF_HIT)
    assert hit >= 2 * plain
    assert 0 < out["mrr@10"] <= out["ndcg@10"] <= hit
    # the same numbers from the restatement's evaluation of the fitted tables
    T = {k: v.astype(np.float64) for k, v in _tables_of(m.net, m.net.seq_context).items()}
    w = m.net.seq_weights.cpu().numpy()
    for sfx, ctx in (("", True), ("_no_context", False)):
        want = ref.evaluate_next(T, off, ids, w, P["k"], context=ctx)
        for name in ("hit_rate", "ndcg", "mrr"):
            assert abs(out[f"{name}@10{sfx}"] - want[name]) < 0.01, (name, sfx)  # (fp32 near-ties may swap a rank)


def test_what_is_deterministic_is():
    """Batches that repeat no row (one triple per batch, every interaction its own item, so that a step's float
    atomics never meet on a row): two fits from the same start give identical tables.  A state_dict round trip into a fresh model gives the same recommend_next."""
    n_users, n_items, length = 32, 32 * 6, 4
    users = np.repeat(np.arange(n_users), length)
    items = np.arange(n_users * length, dtype=np.int64)  # every interaction its own item: no row is shared in a step
    fits = []
    for _ in range(2):
        m = make_model(n_users, n_items, 16, users, items, seed=3)
        quiet(m.fit_sequence, epochs=3, lr=1.0, batch_size=1, context=2, seed=5)
        fits.append(m)
    a, b = (_tables_of(m.net, m.net.seq_context) for m in fits)
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    assert np.abs(a["C"]).max() > 0
    sd = {k: v.clone() for k, v in fits[0].net.state_dict().items()}
    assert {"seq_context", "seq_weights"} <= set(sd)
    fresh = make_model(n_users, n_items, 16, users, items, seed=9)
    fresh.net.load_state_dict(sd)
    q = np.arange(n_users)
    want = quiet(fits[0].recommend_next, q, top_k=7, return_scores=True)
    got = quiet(fresh.recommend_next, q, top_k=7, return_scores=True)
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    with pytest.raises(ValueError, match="slot weights"):
        fresh.fit_sequence(context=3)
    quiet(fresh.fit_sequence, epochs=1, context=2)  # the same weights: continues
