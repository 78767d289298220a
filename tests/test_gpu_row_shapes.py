# -*- coding: utf-8 -*-
"""Every row shape on every path that dispatches on it.  csrc/score_kernels.h instantiates each Linear / FM row kernel
for the twelve (VEC, G, K) shapes of TRS_ROW_SHAPES, and most launchers split once more on FULL = (VEC*G*K == D).  This
module runs each such launcher at the smallest (ragged) and the largest (full where one exists) width of every shape
(tests/row_shapes.py), against the oracle in oracle/ and with the assertion of the launcher's own test in
test_gpu_kernels.py / test_gpu_mining.py / test_gpu_multineg.py / test_gpu_warp.py.  Two checks ride on top, which a
norm-wise criterion cannot see:

  guard rows   every table and optimiser-state table is rows [1:-1] of a buffer with one more row at each end (for odd
               D the table then starts off 16-byte alignment), staging outputs have one row after their last; the guard
               rows keep their bit pattern, and every row no id of the run names keeps its initial bits;
  which branch the one-launch step either ran as one launch or fell back to two (defer_resident_cap): both are accepted,
               the result must match the oracle either way, and the branch is printed per shape.

Tables are small (300 users, 57 items); B = 131 (prime: a partial last wave for every G) with the grid capped at two
workgroups for the direct kernels, B = 192 and 3 batches with one hot item for the presorted and flag-mode steps."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mining_ref
import multineg_ref
import row_shapes
import step_sensitivity as sens
import test_gpu_mining as t_mine
import test_gpu_multineg as t_multi
import test_gpu_warp as t_warp
import warp_ref
from conftest import rel_err
from oracle import nets as onets
from oracle import optim as ooptim
from row_shapes import ALL, FULL, RAGGED
from step_sensitivity import batch_of, float64_oracle
from test_gpu_kernels import DEV, TOL, dense_from_staging, make_case

pytestmark = pytest.mark.gpu

NU, NI = 300, 57
PATTERN = 0x4B5A5A5A  # the guard rows' bits (as a float: about 1.4e7, so a guard row that is read shows in the result)
SM = multineg_ref.SAMPLED_SOFTMAX

# linear and fm alternate so that both nets meet every shape across its two widths
NET_OF = {}
for _r, (_small, _large) in enumerate(row_shapes.WIDTHS.values()):
    NET_OF[_small], NET_OF[_large] = ("linear", "fm")[_r % 2], ("fm", "linear")[_r % 2]

COVERAGE = {}  # path -> {(VEC, G, K, FULL)} over the module's own parametrisation
BRANCH = {}    # (VEC, G, K, FULL) -> {mode: "one launch" | "fell back to two launches"}


def cells(path, widths):
    COVERAGE.setdefault(path, set()).update(row_shapes.variant(D) for D in widths)
    return [(NET_OF[D], D) for D in widths]


def _ops():
    from torchrecsys_amd import ops
    return ops


def lin_names(net):
    return ("user_bias.weight", "item_bias.weight") if net == "linear" else ("linear_user.weight", "linear_item.weight")


# ------------------------------------------------------------------------------------------------- guard rows
class Guards:
    """Tables with a guard row at each end, staging buffers with one after their last; check() after the run."""

    def __init__(self):
        self.tabs, self.stages = [], []

    @staticmethod
    def _filled(n):
        buf = torch.empty(n, dtype=torch.float32, device=DEV)
        buf.view(torch.int32).fill_(PATTERN)
        return buf

    def table(self, name, init, rows_of=None):
        """init (n, w) float32 -> the (n, w) device view [1:-1] of a guarded buffer.  rows_of: the table whose
        referenced rows are this one's (an optimiser state of that table)."""
        init = np.ascontiguousarray(init, dtype=np.float32)
        n, w = init.shape
        buf = self._filled((n + 2) * w).view(n + 2, w)
        view = buf[1:-1]
        view.copy_(torch.from_numpy(init))
        assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4 * w
        self.tabs.append((name, rows_of or name, buf, init.copy()))
        return view

    def staging(self, name, *shape):
        n, w = int(np.prod(shape)), shape[-1]
        buf = self._filled(n + w)
        self.stages.append((name, buf, n))
        return buf[:n].view(*shape)

    def check(self, referenced=None):
        """referenced: {table name: rows some id of the run names}; None: nothing may have been written at all."""
        torch.cuda.synchronize()
        for name, rows_of, buf, init in self.tabs:
            bits = buf.cpu().numpy().view(np.int32)
            assert (bits[0] == PATTERN).all(), f"{name}: the guard row before the table was written"
            assert (bits[-1] == PATTERN).all(), f"{name}: the guard row after the table was written"
            keep = np.ones(init.shape[0], bool)
            if referenced is not None:
                keep[referenced[rows_of]] = False
            same = (bits[1:-1] == init.view(np.int32)).all(axis=1)
            assert same[keep].all(), f"{name}: rows {np.nonzero(keep & ~same)[0][:8].tolist()} changed, no id names them"
        for name, buf, n in self.stages:
            tail = buf[n:].cpu().numpy().view(np.int32)
            assert (tail == PATTERN).all(), f"{name}: written beyond its last row"


def guarded_tables(net, p, g):
    """{name: guarded device view}, trs_tables over them."""
    ops = _ops()
    t = {k: g.table(k, v) for k, v in p.items()}
    M = sum(1 for k in p if k.startswith("metadata."))
    lin = lin_names(net)
    metas = [t[f"metadata.{m}.weight"] for m in range(M)]
    meta_lins = [t[f"linear_metadata.{m}.weight"] for m in range(M)] if net == "fm" else []
    T, keep = ops.make_tables(t["user.weight"], t["item.weight"], t[lin[0]], t[lin[1]], metas, meta_lins)
    return t, T, keep


# ------------------------------------------------------------------------------------------------- cases
def make_params(net, D, M):
    p, _, _ = make_case(net, D, M, 8, NU=NU, NI=NI, seed=2)
    return p


def make_ids(rs, n, skew=False, split=False):
    """n triples; the first and the last row of both tables occur; skew: one hot item takes 40 % of the references.
    split: positives from the lower half of the items, negatives from the upper half (adaptive_ids below)."""
    u, i, j = rs.randint(0, NU, n), rs.randint(0, NI, n), rs.randint(0, NI, n)
    if split:
        i, j = rs.randint(0, NI // 2, n), rs.randint(NI // 2, NI, n)
    if skew:
        i[rs.rand(n) < 0.4] = 7
        j[rs.rand(n) < 0.4] = 7
    u[0], u[1], i[0], j[1] = 0, NU - 1, 0, NI - 1
    return u, i, j


def make_item_meta(rs, p, M):
    sizes = [p[f"metadata.{m}.weight"].shape[0] for m in range(M)]
    im = np.stack([rs.randint(0, sizes[m], NI) for m in range(M)], axis=1).astype(np.int32)
    im[0], im[NI - 1] = 0, np.array(sizes) - 1  # items 0 and NI - 1 occur: so do the first and last category
    return im, sizes


def referenced_rows(p, u, i, j, item_meta=None):
    items = np.union1d(i, j)
    out = {}
    for k in p:
        if k.startswith(("metadata.", "linear_metadata.")):
            out[k] = np.unique(item_meta[items, int(k.split(".")[1])])
        else:
            out[k] = np.unique(u) if "user" in k else items
    return out


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def device_batch(u, i, j, item_meta, err):
    ops = _ops()
    M = 0 if item_meta is None else item_meta.shape[1]
    ids = [dev_i32(u), dev_i32(i), dev_i32(j)] + ([dev_i32(item_meta[i]), dev_i32(item_meta[j])] if M else [None, None])
    Bt, keep = ops.make_batch(*ids, err)
    return ids, Bt, keep


def step_case(net, D, M, B, nb, ids_seed, repeat=False, skew=False, hot=False, lr=None, per_row=False):
    """The input of the SGD-step cells (no GPU), conditioned (tests/step_sensitivity.py).  repeat: one batch, nb steps on
    it; otherwise nb consecutive batches.  hot: 90 % of the items in category 0 of the first metadata column."""
    def build(bump):
        rs = np.random.RandomState(ids_seed + 1000 * bump)
        p = sens.condition_tables(net, make_params(net, D, M))
        item_meta, sizes = make_item_meta(rs, p, M) if M else (None, None)
        if hot:
            item_meta[1:NI - 1][rs.rand(NI - 2) < 0.9, 0] = 0
        u, i, j = make_ids(rs, B if repeat else nb * B, skew=skew)
        batches = [batch_of(u, i, j, item_meta)] * nb if repeat else sens.batches_of(u, i, j, B, nb, item_meta)
        step = 0.05 if per_row else sens.step_lr(B, 0.5 if hot else 0.05, hot, D)
        return sens.StepCase(net, p, batches, step if lr is None else lr, D=D, u=u, i=i, j=j, item_meta=item_meta, sizes=sizes,
                             per_row=per_row and lr is None)
    return sens.conditioned(build, first=lr is not None)


@functools.lru_cache(maxsize=4)
def generic_step_case(net, D, lr=None):
    """test_generic_sgd_step: one batch of 131, two steps"""
    return step_case(net, D, 0, 131, 2, D, repeat=True, lr=lr)


@functools.lru_cache(maxsize=4)
def three_kernel_step_case(net, D, lr=None):
    """test_three_kernel_sgd_step: one batch of 131, three steps"""
    return step_case(net, D, 0, 131, 3, D, repeat=True, lr=lr)


@functools.lru_cache(maxsize=4)
def two_launch_step_case(net, D, lr=None):
    """test_presorted_two_launch_step and test_flag_mode_step: 3 batches of 192, one hot item"""
    return step_case(net, D, 0, 192, 3, D, skew=True, lr=lr)


@functools.lru_cache(maxsize=4)
def metadata_step_case(net, D, M, hot, lr=None):
    """test_presorted_step_with_metadata: 3 batches of 192, one hot item, M metadata columns.
    FM without the hot category keeps lr = 0.05 and is judged per row as well (a quarter of the row's smallest single
    reference: step_sensitivity.RowChangeCriterion).  Its runs subtract sum(c) * w, and a run that a
    64-reference chunk boundary cuts in two does so with a w the other piece may already have added to — second order in
    the step size, and timing dependent.  At the step size the value criterion needs (lr / B = 5.9e-3) that term was
    measured at 0.7e-5 ... 1.8e-5 of max|item.weight| on exactly the rows that straddle a boundary, at the widths whose
    rows take a whole wave (D = 132, 512, 516; below 1.2e-6 at D <= 64): a tenth of the smallest single reference, but
    past the 1e-5 of the value criterion.  At lr = 0.05 it is 500 times smaller and the per-row criterion sees every
    reference."""
    return step_case(net, D, M, 192, 3, D + M, skew=True, hot=bool(hot), lr=lr, per_row=net == "fm" and not hot)


def assert_step(case, t, losses, run=None):
    """the criterion of the SGD-step cells: every step's loss, then the tables (got, ref, before)"""
    run = run or case.oracle()
    sens.assert_losses(case, losses.cpu().numpy(), run)
    sens.criterion_for(case)({k: t[k].cpu().numpy() for k in run.after}, run.after, case.p)


def zero_err():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------- scoring
SCORE_CELLS = [(n, D, 0) for n, D in cells("score_forward / fwd_bwd / backward", ALL)] + \
              [(n, D, 2) for n, D in cells("score_forward / fwd_bwd / backward", RAGGED)]


@pytest.mark.parametrize("net,D,M", SCORE_CELLS)
def test_score_forward_fwd_bwd_backward(net, D, M, tune):
    """trs_score_forward (int32 ids without metadata: pair_scores_kernel where the shape is a whole-row one, score_kernel
    otherwise), trs_score_fwd_bwd under hinge and BPR, trs_score_backward: the assertions of test_forward_and_fwd_bwd."""
    from torchrecsys_amd import _lib
    ops = _ops()
    tune(GRID_CAP=2, PASS_GRID_CAP=2)
    B = 131
    rs = np.random.RandomState(D + M)
    p = make_params(net, D, M)
    item_meta, _ = make_item_meta(rs, p, M) if M else (None, None)
    u, i, j = make_ids(rs, B)
    batch = batch_of(u, i, j, item_meta)
    g = Guards()
    t, T, keep = guarded_tables(net, p, g)
    err = zero_err()
    ids, Bt, keepb = device_batch(u, i, j, item_meta, err)
    pos, neg = ops.score_forward(net, T, Bt, B, DEV)
    R = 3 + 2 * M
    staged = {}
    for loss in ("hinge", "bpr"):
        sp, sn, want_loss, grads = onets.train_forward_backward(net, {k: v.copy() for k, v in p.items()}, batch, loss=loss)
        loss_sum = torch.zeros(1, dtype=torch.float32, device=DEV)
        auc = torch.zeros(1, dtype=torch.int32, device=DEV)
        gr, gl = g.staging(f"grad_rows[{loss}]", R, B, D), g.staging(f"grad_lin[{loss}]", R, B)
        pos2, neg2, _, _ = ops.score_fwd_bwd(net, T, Bt, B, D, M, DEV, loss_sum, auc, grad_rows=gr, grad_lin=gl,
                                             loss=_lib.LOSS_ID[loss])
        torch.cuda.synchronize()
        assert rel_err(pos.cpu().numpy(), sp.reshape(-1)) < TOL and rel_err(neg.cpu().numpy(), sn.reshape(-1)) < TOL
        assert torch.equal(pos2, pos) and torch.equal(neg2, neg)
        assert abs(loss_sum.item() / B - float(want_loss)) <= TOL * max(abs(float(want_loss)), 1e-3)
        assert auc.item() == int((pos > neg).sum().item())
        dense = dense_from_staging(net, p, batch, gr, gl)
        for k, v in grads.items():
            e = rel_err(dense[k], v)
            print(f"{loss} {k}: {e:.2e}")
            assert e < TOL, (loss, k)
        staged[loss] = (gr, gl)
    gp, gn = ops.hinge_backward(pos, neg)
    gr2, gl2 = ops.score_backward(net, T, Bt, B, D, M, DEV, gp, gn)
    assert torch.equal(gr2, staged["hinge"][0]) and torch.equal(gl2, staged["hinge"][1])
    assert err.item() == 0
    g.check()


ALL_ITEMS_CELLS = [(n, D, 0) for n, D in cells("score_all_items", ALL)] + \
                  [(n, D, 1) for n, D in cells("score_all_items", RAGGED)]


@pytest.mark.parametrize("net,D,M", ALL_ITEMS_CELLS)
def test_score_all_items(net, D, M, tune):
    ops = _ops()
    tune(GRID_CAP=2)
    rs = np.random.RandomState(D + M)
    p = make_params(net, D, M)
    item_meta, _ = make_item_meta(rs, p, M) if M else (None, None)
    g = Guards()
    t, T, keep = guarded_tables(net, p, g)
    tim = None if item_meta is None else dev_i32(item_meta)
    fwd = onets.fm_forward if net == "fm" else onets.linear_forward
    for user in (0, NU - 1):
        sc = ops.score_all_items(net, T, user, NI, DEV, tim)
        ref = fwd(p, np.full(NI, user), np.arange(NI), None if item_meta is None else item_meta.astype(np.int64))
        assert rel_err(sc.cpu().numpy(), ref.reshape(-1)) < TOL, user
        parts = [ops.score_all_items(net, T, user, NI, DEV, tim, item0=a, n=min(20, NI - a)) for a in range(0, NI, 20)]
        assert torch.equal(torch.cat(parts), sc)
    g.check()


# ------------------------------------------------------------------------------------------------- SGD steps
@pytest.mark.parametrize("net,D", cells("generic step: score_fwd_bwd + score_sgd_update", ALL))
def test_generic_sgd_step(net, D, tune):
    ops = _ops()
    tune(GRID_CAP=2)
    case = generic_step_case(net, D)
    p, u, i, j, B, lr, steps = case.p, case.u, case.i, case.j, case.B, case.lr, case.nb
    g = Guards()
    t, T, keep = guarded_tables(net, p, g)
    err = zero_err()
    ids, Bt, keepb = device_batch(u, i, j, None, err)
    gr, gl = g.staging("grad_rows", 3, B, D), g.staging("grad_lin", 3, B)
    losses = torch.zeros(steps, device=DEV)
    for s in range(steps):
        ops.score_fwd_bwd(net, T, Bt, B, D, 0, DEV, losses[s:s + 1], want_scores=False, grad_rows=gr, grad_lin=gl)
        ops.score_sgd_update(net, T, Bt, gr, gl, lr)
    torch.cuda.synchronize()
    assert_step(case, t, losses)
    assert err.item() == 0
    g.check(referenced_rows(p, u, i, j))


FAST_CELLS = [(n, D, True) for n, D in cells("3-kernel step", ALL)] + \
             [(n, D, False) for n, D in cells("3-kernel step", RAGGED)]


@pytest.mark.parametrize("net,D,with_scratch", FAST_CELLS)
def test_three_kernel_sgd_step(net, D, with_scratch, tune):
    """trs_train_steps_sgd with the ids given (fwd_stage_kernel INL 0, item_owner / user_plain updates; without scratch
    the all-atomic item_update / user_update kernels): 3 steps == oracle steps, as
    test_fast_sgd_step_matches_oracle_and_generic_path."""
    ops = _ops()
    tune(GRID_CAP=2)
    case = three_kernel_step_case(net, D)
    p, u, i, j, B, lr, steps = case.p, case.u, case.i, case.j, case.B, case.lr, case.nb
    g = Guards()
    t, T, keep = guarded_tables(net, p, g)
    err = zero_err()
    ids = [dev_i32(a) for a in (u, i, j)]
    gz, du = torch.empty((2, B), device=DEV), g.staging("du", B, D)
    losses = torch.zeros(steps, device=DEV)
    scratch = ops.train_scratch(NU, NI, B, D, DEV) if with_scratch else None
    for s in range(steps):
        ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, 1, lr, *ids, gz, du, losses[s:s + 1], err, scratch, 1 + s)
    torch.cuda.synchronize()
    assert_step(case, t, losses)
    assert err.item() == 0
    g.check(referenced_rows(p, u, i, j))


PRESORTED_CELLS = [(n, D, True) for n, D in cells("presorted two-launch step", ALL)] + \
                  [(n, D, v) for v in (False, "items", "userflags") for n, D in cells("presorted two-launch step", RAGGED)]


@pytest.mark.parametrize("net,D,inline_user", PRESORTED_CELLS)
def test_presorted_two_launch_step(net, D, inline_user):
    """trs_epoch_presort + the sorted-run updates (trs_launch_sorted_item_update, trs_launch_sorted_updates_fused), one hot
    item: 3 batches in one C call == oracle steps, as test_presorted_item_update_matches_oracle."""
    ops = _ops()
    case = two_launch_step_case(net, D)
    p, u, i, j, B, nb, lr = case.p, case.u, case.i, case.j, case.B, case.nb, case.lr
    g = Guards()
    t, T, keep = guarded_tables(net, p, g)
    err = zero_err()
    ps = ops.EpochPresort(nb, B, NU, NI, DEV, user_sort=inline_user != "userflags")
    ps.run(None, None, 0, 0, 0, err, given_ids=[dev_i32(a) for a in (u, i, j)])
    ids, sk, sv, udup, usorted, idup = ps.step_args(0)
    gz, du, ustage = torch.empty((2, B), device=DEV), g.staging("du", B, D), g.staging("ustage", B, D)
    losses = torch.zeros(nb, device=DEV)
    scratch = ops.train_scratch(NU, NI, B, D, DEV)
    if inline_user:
        ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, nb, lr, *ids, gz, du, losses, err, scratch, 1, None, sk, sv,
                            ps.key_bytes, udup, ustage, usorted, item_dup=idup if inline_user == "items" else None)
    else:
        ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, nb, lr, *ids, gz, du, losses, err, scratch, 1, None, sk, sv,
                            ps.key_bytes)
    torch.cuda.synchronize()
    assert_step(case, t, losses)
    assert err.item() == 0
    g.check(referenced_rows(p, u, i, j))


FLAG_CELLS = [(n, D, mode) for mode in ("two", "one", "ordered") for n, D in cells("flag mode", ALL)] + \
             [(n, D, mode) for mode in ("one-nt1", "one-nt3") for n, D in cells("flag mode", RAGGED)]


@pytest.mark.parametrize("net,D,mode", FLAG_CELLS)
def test_flag_mode_step(net, D, mode, tune):
    """trs_epoch_flags + fwd_stage_kernel INL 2 / 3 + flagged_update_kernel<KD> (KD = ceil(D / 64) -> 1, 2, 4, 8, 16), one
    hot item, 300 users: two calls of 2 + 1 steps == oracle steps, as test_flag_mode_matches_oracle.  one / ordered /
    one-nt*: the one-launch form was asked for; whether the library ran it (arrivals counted: the counter identities of
    that test) or fell back to two launches (no arrivals) is recorded and printed, and either must match the oracle."""
    ops = _ops()
    one_launch, ordered = mode != "two", mode == "ordered"
    if mode.startswith("one-nt"):
        tune(K1_NT=int(mode[-1]))
    case = two_launch_step_case(net, D)
    p, u, i, j, B, nb, lr = case.p, case.u, case.i, case.j, case.B, case.nb, case.lr
    run = None
    g = Guards()
    t, T, keep = guarded_tables(net, p, g)
    err = zero_err()
    ef = ops.EpochFlags(nb, B, NU, NI, DEV, ordered=ordered)
    ef.run(None, None, 0, 0, 0, err, given_ids=[dev_i32(a) for a in (u, i, j)])
    ids, udup, idup = ef.step_args(0)
    if ordered:  # every batch: a permutation of its triples (the steps and the oracle see the presort's order)
        uo, io, jo = (x[:nb * B].cpu().numpy().astype(np.int64) for x in ids)
        for b in range(nb):
            sl = slice(b * B, (b + 1) * B)
            a_, b_ = np.stack([u[sl], i[sl], j[sl]], 1), np.stack([uo[sl], io[sl], jo[sl]], 1)
            assert np.array_equal(a_[np.lexsort(a_.T)], b_[np.lexsort(b_.T)])
        u, i, j = uo, io, jo
        run = case.oracle_on(sens.batches_of(u, i, j, B, nb))
    gz, du, ustage = torch.empty((2, B), device=DEV), g.staging("du", B, D), g.staging("ustage", B, D)
    losses = torch.zeros(nb, device=DEV)
    sync = (torch.zeros(288, dtype=torch.int32, device=DEV), ctypes.c_uint32(0)) if one_launch else None
    scratch = ops.train_scratch(NU, NI, B, D, DEV)
    ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, 2, lr, *ids, gz, du, losses, err, scratch, 1, None,
                        user_dup=udup, item_dup=idup, ustage=ustage, sync=sync, n_flagged=ef.n_flagged_from(0))
    ids2, udup2, idup2 = ef.step_args(2)
    ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, 1, lr, *ids2, gz, du, losses[2:], err, scratch, 3, None,
                        user_dup=udup2, item_dup=idup2, ustage=ustage, sync=sync, n_flagged=ef.n_flagged_from(2))
    torch.cuda.synchronize()
    if one_launch:
        arrivals = sync[1].value
        if arrivals > 0:  # every launch counted all its workgroups in, and the library knows how many it scheduled
            assert arrivals % 3 == 0 and int(sync[0][0].item()) == arrivals
            branch = "one launch"
        else:
            branch = "fell back to two launches"
        BRANCH.setdefault(row_shapes.variant(D), {})[mode] = branch
        print(f"one-launch step, shape {row_shapes.variant(D)}, {mode}: {branch}")
    assert err.item() == 0, f"err {err.item()} (bit 2 = 4: the bounded grid wait ran out)"
    assert_step(case, t, losses, run)
    g.check(referenced_rows(p, u, i, j))


# ------------------------------------------------------------------------------------------------- adaptive rules
def opt_struct(kind, hp):
    from torchrecsys_amd import _lib
    o = _lib.TrsOpt()
    o.kind, o.lr, o.beta1, o.beta2, o.eps, o.lr_decay, o.step0 = (1 if kind == "sparse_adam" else 2), *hp, 0
    return o


def hyper(kind):
    """(lr, beta1, beta2, eps, lr_decay) of test_presorted_adaptive_rules_match_the_oracle"""
    return (0.01, 0.9, 0.999, 1e-8, 0.0) if kind == "sparse_adam" else (0.05, 0.0, 0.0, 1e-10, 0.02)


def adaptive_ids(rs, n):
    """Ids for SparseAdam / Adagrad.  Both rules divide by a norm of the row's own gradient history, so a coalesced
    gradient that cancels to rounding noise becomes a +-lr step of random sign (in torch too: the docstring of
    test_presorted_adaptive_rules_match_the_oracle).  Linear's hinge makes that the common case for random ids: the
    gradient of an item's bias is (negative references - positive references) / B over the active triples, an exact 0
    whenever the two counts agree — a sixth of 57 items per batch of 192.  That is a property of the input, so the
    input avoids it: an item is a positive or a negative, never both, and every term of a row's sum has one sign."""
    return make_ids(rs, n, split=True)


def oracle_adaptive(net, kind, hp, p, u, i, j, B, nb, item_meta=None):
    """nb oracle steps of the rule on consecutive batches -> tables, first and second state, the batches' losses"""
    lr, b1, b2, eps, lr_decay = hp
    ref = {k: v.copy() for k, v in p.items()}
    r1 = {k: np.zeros_like(v) for k, v in p.items()}
    r2 = {k: np.zeros_like(v) for k, v in p.items()}
    losses = []
    for b in range(nb):
        batch = batch_of(u, i, j, item_meta, slice(b * B, (b + 1) * B))
        _, _, loss, grads = onets.train_forward_backward(net, ref, batch)
        rows = onets.touched_rows(net, ref, batch)
        for k in ref:
            if kind == "sparse_adam":
                ooptim.sparse_adam_rows(ref[k], grads[k], rows[k], r1[k], r2[k], b + 1, lr, b1, b2, eps)
            else:
                ooptim.adagrad_rows(ref[k], grads[k], rows[k], r1[k], b + 1, lr, lr_decay, eps)
        losses.append(float(loss))
    return ref, r1, r2, losses


def worst_row(got, want):
    """largest deviation of a row relative to max|want|: rows_within(got, want, tol) == 1.0 <=> worst_row <= tol"""
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def conditioned_adaptive_case(net, kind, hp, p, D, B, nb, item_meta=None):
    """(u, i, j, oracle_adaptive's result) for the first seed D, D + 1000, ... that passes a condition on the INPUT,
    computed from the oracle alone: the oracle's own fp32 run and its float64 run agree on every row of every table to
    TOL, a third of the bar below.  Without it a cell can fail on rounding alone: a row's gradient entry that is the
    remainder of a cancellation enters g / sqrt(sum g^2) with a large relative error under any fp32 evaluation (seed
    1024 for Linear, D = 1024, Adagrad: the two oracle runs differ by 2.1e-3 on one user row of 300, the kernels by
    8.1e-4 from the fp32 one)."""
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    for seed in range(D, D + 8000, 1000):
        u, i, j = adaptive_ids(np.random.RandomState(seed), nb * B)
        oracle = oracle_adaptive(net, kind, hp, p, u, i, j, B, nb, item_meta)
        with float64_oracle():
            ref64 = oracle_adaptive(net, kind, hp, p64, u, i, j, B, nb, item_meta)[0]
        moved = max(worst_row(oracle[0][k], ref64[k]) for k in p)
        print(f"ids of seed {seed}: fp32 and float64 oracle differ by {moved:.2e} on their worst row")
        if moved <= TOL:
            return u, i, j, oracle
    raise AssertionError("no seed gives a well-conditioned input")


def assert_adaptive(kind, B, losses, t, s1, s2, oracle):
    """the unskewed criterion of test_presorted_adaptive_rules_match_the_oracle, for every row"""
    ref, r1, r2, want_losses = oracle
    for b, want in enumerate(want_losses):
        print(f"loss {b}: {abs(losses[b].item() / B - want) / max(abs(want), 1e-3):.2e}")
        assert abs(losses[b].item() / B - want) <= 2 * TOL * max(abs(want), 1e-3), b
    tol = 3 * TOL
    for k in ref:
        got = t[k].cpu().numpy()
        print(f"{k}: worst row {worst_row(got, ref[k]):.2e} (allowed {tol:.2e})")
        assert t_mine._rows_within(got, ref[k], tol) == 1.0, k
        assert t_mine._rows_within(s1[k].cpu().numpy(), r1[k], 1e-3) == 1.0, k
        if kind == "sparse_adam":
            assert t_mine._rows_within(s2[k].cpu().numpy(), r2[k], 1e-3) == 1.0, k
        assert rel_err(got, ref[k]) < 0.05, k


@pytest.mark.parametrize("kind", ["sparse_adam", "adagrad"])
@pytest.mark.parametrize("net,D", cells("presorted SparseAdam / Adagrad", RAGGED + FULL))
def test_presorted_adaptive_rules(net, D, kind):
    ops = _ops()
    B, nb = 192, 3
    hp = hyper(kind)
    p = make_params(net, D, 0)
    u, i, j, oracle = conditioned_adaptive_case(net, kind, hp, p, D, B, nb)
    lin = lin_names(net)
    names = ["user.weight", "item.weight", lin[0], lin[1]]
    g = Guards()
    t, T, keep = guarded_tables(net, p, g)
    err = zero_err()
    ps = ops.EpochPresort(nb, B, NU, NI, DEV)
    ps.run(None, None, 0, 0, 0, err, given_ids=[dev_i32(a) for a in (u, i, j)])
    ids, sk, sv, udup, usorted, idup = ps.step_args(0)
    gz, du, ustage = torch.empty((2, B), device=DEV), g.staging("du", B, D), g.staging("ustage", B, D)
    losses = torch.zeros(nb, device=DEV)
    s1 = {k: g.table("s1 of " + k, np.zeros_like(p[k]), rows_of=k) for k in names}
    s2 = {k: g.table("s2 of " + k, np.zeros_like(p[k]), rows_of=k) for k in names}
    gacc = g.table("gacc", np.zeros_like(p["item.weight"]), rows_of="item.weight")
    gacc_lin = g.table("gacc_lin", np.zeros_like(p[lin[1]]), rows_of=lin[1])
    cut_rows = torch.empty(2 * B // 64 + 64, dtype=torch.int32, device=DEV)
    cut_count = torch.zeros(2, dtype=torch.int32, device=DEV)
    o = opt_struct(kind, hp)
    o.user_s1, o.item_s1, o.user_lin_s1, o.item_lin_s1 = (ops.ptr(s1[k]) for k in names)
    if kind == "sparse_adam":
        o.user_s2, o.item_s2, o.user_lin_s2, o.item_lin_s2 = (ops.ptr(s2[k]) for k in names)
    o.gacc, o.gacc_lin, o.cut_rows, o.cut_count = ops.ptr(gacc), ops.ptr(gacc_lin), ops.ptr(cut_rows), ops.ptr(cut_count)
    o.cut_capacity = cut_rows.numel()
    ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, nb, hp[0], *ids, gz, du, losses, err,
                        ops.train_scratch(NU, NI, B, D, DEV), 1, None, sk, sv, ps.key_bytes, udup, ustage, usorted, o)
    torch.cuda.synchronize()
    assert_adaptive(kind, B, losses, t, s1, s2, oracle)
    assert float(gacc.abs().max()) == 0.0 and float(gacc_lin.abs().max()) == 0.0  # accumulator left clean
    assert err.item() == 0
    g.check(referenced_rows(p, u, i, j))


# ------------------------------------------------------------------------------------------------- metadata scorers
def meta_stage(ops, net, ps, tab, sizes, g, B, D, M, meta_sorted, staged_fields, ids_from_presort=True):
    """trs_meta_stage of the presorted metadata step, staging buffers guarded; -> (struct, keep-alive)."""
    from torchrecsys_amd import _lib
    R = 3 + 2 * M
    xstage = g.staging("xstage", 2 if net == "fm" else 1, B, D)
    ms = _lib.TrsMetaStage()
    ms.item_meta_tab, ms.xstage = ops.ptr(tab), ops.ptr(xstage)
    keep = [xstage, tab]
    if staged_fields:
        grad_rows, grad_lin = g.staging("grad_rows", R, B, D), torch.zeros((R, B), device=DEV)
        meta_ids = torch.empty((2, B, M), dtype=torch.int32, device=DEV)
        ms.grad_rows, ms.grad_lin, ms.meta_ids = ops.ptr(grad_rows), ops.ptr(grad_lin), ops.ptr(meta_ids)
        keep += [grad_rows, grad_lin, meta_ids]
    if meta_sorted:
        for m, (k_, v_) in enumerate(ps.meta_step_args(0)):
            ms.sorted_keys[m], ms.sorted_vals[m] = k_, v_
        lin_scratch = torch.zeros(max(sizes), device=DEV)
        ms.lin_scratch = ops.ptr(lin_scratch)
        keep.append(lin_scratch)
        if ids_from_presort:
            pm, nm = ps.meta_id_args(0)
            ms.pos_meta_ids, ms.neg_meta_ids = ops.ptr(pm), ops.ptr(nm)
            keep += [pm, nm]
    return ms, keep


META_M3 = [8, 36, 132, 516]  # G = 2, 16, 64 and K = 4
META_CELLS = [(n, D, 1, True) for n, D in cells("presorted step with metadata", ALL)] + \
             [(n, D, 1, v) for v in (False, "hot") for n, D in cells("presorted step with metadata", RAGGED)] + \
             [(n, D, 3, True) for n, D in cells("presorted step with metadata", META_M3)]


# (builder, its distinct argument tuples): what tests/test_step_sensitivity_host.py walks
STEP_CASES = [(generic_step_case, cells("generic step: score_fwd_bwd + score_sgd_update", ALL)),
              (three_kernel_step_case, cells("3-kernel step", ALL)),
              (two_launch_step_case, cells("presorted two-launch step", ALL)),
              (metadata_step_case, sorted({(n, D, M, v == "hot") for n, D, M, v in META_CELLS}))]


@pytest.mark.parametrize("net,D,M,meta_sorted", META_CELLS)
def test_presorted_step_with_metadata(net, D, M, meta_sorted):
    """launch_meta_stage[_mt] / score_kernel MODE 2 + the sorted item, user and metadata runs
    (trs_launch_sorted_meta_update) or the atomic scatter of the staged fields (meta_sorted False): 3 batches == oracle
    steps, as test_presorted_step_with_metadata_matches_oracle.  "hot": 90 % of the items in category 0 — that row's run
    is cut into pieces of 64.  (Step sizes and criterion: metadata_step_case.)"""
    ops = _ops()
    case = metadata_step_case(net, D, M, meta_sorted == "hot")
    p, u, i, j, B, nb, lr, item_meta, sizes = case.p, case.u, case.i, case.j, case.B, case.nb, case.lr, case.item_meta, case.sizes
    g = Guards()
    t, T, keep = guarded_tables(net, p, g)
    err = zero_err()
    tab = dev_i32(item_meta)
    ps = ops.EpochPresort(nb, B, NU, NI, DEV, **(dict(item_meta=tab, n_meta=sizes) if meta_sorted else {}))
    ps.run(None, None, 0, 0, 0, err, given_ids=[dev_i32(a) for a in (u, i, j)])
    ids, sk, sv, udup, usorted, idup = ps.step_args(0)
    gz, du, ustage = torch.empty((2, B), device=DEV), g.staging("du", B, D), g.staging("ustage", B, D)
    # (one ragged and one full case keep the table look-up inside K1, as the D = 16 case of the launcher's own test)
    ms, keepm = meta_stage(ops, net, ps, tab, sizes, g, B, D, M, meta_sorted, True, ids_from_presort=D not in (12, 16))
    losses = torch.zeros(nb, device=DEV)
    ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, nb, lr, *ids, gz, du, losses, err,
                        ops.train_scratch(NU, NI, B, D, DEV), 1, None, sk, sv, ps.key_bytes, udup, ustage, usorted, None, ms)
    torch.cuda.synchronize()
    assert_step(case, t, losses)
    assert err.item() == 0
    g.check(referenced_rows(p, u, i, j, item_meta))


META_ADAPTIVE_WIDTHS = [32, 64, 128, 256]  # the widths trs_train_steps_sgd takes for this combination: all FULL


@pytest.mark.parametrize("kind", ["sparse_adam", "adagrad"])
@pytest.mark.parametrize("net,D", cells("presorted metadata + adaptive rules", RAGGED + META_ADAPTIVE_WIDTHS))
def test_presorted_metadata_with_adaptive_rules(net, D, kind):
    """As test_presorted_adaptive_rules_with_metadata_match_the_oracle (M = 1, unskewed), every row held to the unskewed
    criterion of the rules' own test.  The library takes this combination at D = 32, 64, 128 and 256 only and refuses
    every other width as an argument error before it launches anything: at the ragged widths that refusal is what is
    checked, with every table, state and staging buffer left bit-identical."""
    from torchrecsys_amd import _lib
    ops = _ops()
    B, nb, M = 192, 3, 1
    hp = hyper(kind)
    rs = np.random.RandomState(D)
    p = make_params(net, D, M)
    item_meta, sizes = make_item_meta(rs, p, M)
    if D in META_ADAPTIVE_WIDTHS:
        u, i, j, oracle = conditioned_adaptive_case(net, kind, hp, p, D, B, nb, item_meta)
    else:  # (refused before any launch: no oracle to compare with)
        u, i, j = adaptive_ids(rs, nb * B)
    lin = lin_names(net)
    names = ["user.weight", "item.weight", lin[0], lin[1]]
    g = Guards()
    t, T, keep = guarded_tables(net, p, g)
    err = zero_err()
    tab = dev_i32(item_meta)
    ps = ops.EpochPresort(nb, B, NU, NI, DEV, item_meta=tab, n_meta=sizes)
    ps.run(None, None, 0, 0, 0, err, given_ids=[dev_i32(a) for a in (u, i, j)])
    ids, sk, sv, udup, usorted, idup = ps.step_args(0)
    gz, du, ustage = torch.empty((2, B), device=DEV), g.staging("du", B, D), g.staging("ustage", B, D)
    ms, keepm = meta_stage(ops, net, ps, tab, sizes, g, B, D, M, True, False)
    s1 = {k: g.table("s1 of " + k, np.zeros_like(v), rows_of=k) for k, v in p.items()}
    s2 = {k: g.table("s2 of " + k, np.zeros_like(v), rows_of=k) for k, v in p.items()}
    gacc = {k: g.table("gacc of " + k, np.zeros_like(v), rows_of=k) for k, v in p.items()}
    cap = 2 * B // 64 + 64
    cut_rows = torch.empty((1 + M, cap), dtype=torch.int32, device=DEV)
    cut_count = torch.zeros((1 + M, 2), dtype=torch.int32, device=DEV)
    lin_state = [torch.zeros((3, sizes[m]), device=DEV) for m in range(M)]  # Linear: no 1-wide metadata tables
    o = opt_struct(kind, hp)
    o.user_s1, o.item_s1, o.user_lin_s1, o.item_lin_s1 = (ops.ptr(s1[k]) for k in names)
    o.user_s2, o.item_s2, o.user_lin_s2, o.item_lin_s2 = (ops.ptr(s2[k]) for k in names)
    o.gacc, o.gacc_lin = ops.ptr(gacc["item.weight"]), ops.ptr(gacc[lin[1]])
    o.cut_rows, o.cut_count, o.cut_capacity = ops.ptr(cut_rows[0]), ops.ptr(cut_count[0]), cap
    for m in range(M):
        k = f"metadata.{m}.weight"
        o.meta_s1[m], o.meta_s2[m], o.meta_gacc[m] = ops.ptr(s1[k]), ops.ptr(s2[k]), ops.ptr(gacc[k])
        if net == "fm":
            kl = f"linear_metadata.{m}.weight"
            o.meta_lin_s1[m], o.meta_lin_s2[m], o.meta_gacc_lin[m] = ops.ptr(s1[kl]), ops.ptr(s2[kl]), ops.ptr(gacc[kl])
        else:
            o.meta_lin_s1[m], o.meta_lin_s2[m], o.meta_gacc_lin[m] = (ops.ptr(lin_state[m][q]) for q in range(3))
        o.meta_cut_rows[m], o.meta_cut_count[m] = ops.ptr(cut_rows[1 + m]), ops.ptr(cut_count[1 + m])
    losses = torch.zeros(nb, device=DEV)
    step = lambda: ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, nb, hp[0], *ids, gz, du, losses, err,  # noqa: E731
                                       ops.train_scratch(NU, NI, B, D, DEV), 1, None, sk, sv, ps.key_bytes, udup, ustage,
                                       usorted, o, ms)
    if D not in META_ADAPTIVE_WIDTHS:
        with pytest.raises(_lib.TrsError, match=r"adaptive rules on metadata scorers need .* D in \{32, 64, 128, 256\}"):
            step()
        assert err.item() == 0
        g.check()
        return
    step()
    torch.cuda.synchronize()
    assert_adaptive(kind, B, losses, t, s1, s2, oracle)
    for k in gacc:
        assert float(gacc[k].abs().max()) == 0.0, k  # accumulators left clean
    assert err.item() == 0
    g.check(referenced_rows(p, u, i, j, item_meta))


# ------------------------------------------------------------------------------------------------- mining
@pytest.mark.parametrize("net,D", cells("batch_prepare_mined", ALL))
def test_mined_choice_is_bit_exact_on_exact_arithmetic(net, D, tune):
    """8 candidates, the best one: ids and choice equal tests/mining_ref.py bit for bit on tables of small integers, as
    test_choice_is_bit_exact_on_exact_arithmetic; nothing written beyond the batch, no table touched."""
    ops = _ops()
    tune(GRID_CAP=2)
    N, B, K, t0, seed = 1000, 131, 8, 301, 5
    rs = np.random.RandomState(D)
    p, _ = t_mine.make_params(net, NU, NI, D, 0, rs, exact=True)
    su, si = t_mine.make_stream(rs, NU, NI, N)
    su[t0], su[t0 + 1], si[t0], si[t0 + 1] = 0, NU - 1, 0, NI - 1  # (identity shuffle: the batch is rows t0 .. t0 + B - 1)
    g = Guards()
    t, T, keep = guarded_tables(net, p, g)
    dev, ref_s, (su_d, si_d) = t_mine.samplers(su, si, NU, NI, 1, False, K, 1)
    names = ("user", "pos", "neg", "chosen")
    out = {k: torch.full((B + 64,), -7, dtype=torch.int32, device=DEV) for k in names}
    ops.batch_prepare_mined(su_d, si_d, 0, t0, B, NI, seed, t0, net, T, dev, None, out=out, return_chosen=True)
    torch.cuda.synchronize()
    ref = mining_ref.mined_batch(su, si, 0, t0, B, NI, seed, t0, net, p, K, 1, ref_s, None)
    assert ref["user"][0] == 0 and ref["user"][1] == NU - 1 and {0, NI - 1} <= set(ref["cand"].reshape(-1).tolist())
    zs = np.sort(ref["z"], axis=1)
    print(f"exact ties at the top: {int((zs[:, -1] == zs[:, -2]).sum())} of {B}")
    for name in names:
        got = out[name].cpu().numpy()
        assert np.array_equal(got[:B], ref[name]), name
        assert (got[B:] == -7).all(), (name, "written beyond the batch")
    g.check()


# ------------------------------------------------------------------------------------------------- K negatives, WARP
class TablesAsNet:
    """What run_kernel / pair_kernel_columns of test_gpu_multineg.py and test_gpu_warp.py ask of a scorer."""

    def __init__(self, T, t):
        self.T, self.t = T, t

    def tables(self):
        return self.T

    def table_params(self):
        return [self.t["user.weight"]]


def multineg_rows(rs, B, K):
    """forced_rows of the multi-negative tests, with the first and last row of both tables present."""
    user, items = t_multi.forced_rows(rs, NU, NI, B, K)
    user[0], user[2] = 0, NU - 1
    for col, row in ((3, 0), (5, NI - 1)):
        items[0, col] = row
        items[1:, col][items[1:, col] == row] = NI // 2
    return user, items


MULTI_CELLS = [(n, D, 3, "train") for n, D in cells("score_multi_fwd_bwd", ALL)] + \
              [(n, D, 17, "train") for n, D in cells("score_multi_fwd_bwd", RAGGED)] + \
              [(n, D, 3, "forward") for n, D in cells("score_multi_fwd_bwd", RAGGED)]


@pytest.mark.parametrize("net,D,K,mode", MULTI_CELLS)
def test_multi_negative_losses(net, D, K, mode, tune):
    """trs_score_multi_fwd_bwd.  train: the sampled softmax against the float64 restatement (loss and every table's staged
    block at 1e-5, as test_sampled_softmax_matches_the_float64_oracle) and the mean of K hinge pairs against K calls of the
    pair kernel (1e-6, as test_mean_of_k_pairs_matches_k_calls_of_the_pair_kernel).  forward: the forward-only mode gives
    the same loss and AUC count bit for bit and writes nothing else (one workgroup, as
    test_forward_only_mode_writes_the_same_loss_and_nothing_else)."""
    tune(GRID_CAP=1 if mode == "forward" else 2)
    B, tau = 131, 0.5
    W, _ = t_warp.table_params_numpy(net, 0, NU, NI, D, D + K)
    user, items = multineg_rows(np.random.RandomState(K), B, K)
    g = Guards()
    t, T, keep = guarded_tables(net, W, g)
    shim = TablesAsNet(T, t)
    ids = t_multi.device_ids(user, items, None)
    F = multineg_ref.n_fields(K, 0)
    blocks = t_multi.table_blocks(K, 0)
    if mode == "forward":
        for loss in (SM, "hinge"):
            l1, a1, gr, gl = t_multi.run_kernel(net, shim, ids, loss, tau)
            poison_r, poison_l = torch.full_like(gr, 7.25), torch.full_like(gl, -3.5)
            l0, a0, r0, r1 = t_multi.run_kernel(net, shim, ids, loss, tau, forward_only=True, grad_rows=poison_r,
                                                grad_lin=poison_l)
            assert r0 is None and r1 is None
            assert l0.item() == l1.item() and l1.item() > 0 and int(a0.item()) == int(a1.item())
            assert bool((poison_r == 7.25).all()) and bool((poison_l == -3.5).all())
        g.check()
        return
    # sampled softmax
    gr, gl = g.staging("grad_rows[softmax]", F, B, D), g.staging("grad_lin[softmax]", F, B)
    loss_sum, auc, _, _ = t_multi.run_kernel(net, shim, ids, SM, tau, grad_rows=gr, grad_lin=gl)
    want_loss, wr, wl, z = multineg_ref.staged(net, W, user, items, None, SM, tau)
    assert abs(loss_sum.item() / B - want_loss) <= TOL * abs(want_loss)
    gr_, gl_ = gr.cpu().numpy(), gl.cpu().numpy()
    for sl in blocks:
        print(f"softmax fields {sl.start}..{sl.stop - 1}: rows {rel_err(gr_[sl], wr[sl]):.2e} 1-wide {rel_err(gl_[sl], wl[sl]):.2e}")
        assert rel_err(gr_[sl], wr[sl]) <= TOL, sl
        assert rel_err(gl_[sl], wl[sl]) <= TOL, sl
    assert not gl_[0].any()  # the user's 1-wide gradient: exactly 0
    # mean of K hinge pairs against the pair kernel
    gr, gl = g.staging("grad_rows[hinge]", F, B, D), g.staging("grad_lin[hinge]", F, B)
    loss_sum, auc, _, _ = t_multi.run_kernel(net, shim, ids, "hinge", 1.0, grad_rows=gr, grad_lin=gl)
    cols = t_multi.pair_kernel_columns(net, shim, ids, K, 0, "hinge")
    want_r, want_l = np.zeros(gr.shape), np.zeros(gl.shape)
    for c, (_, _, cr, cl) in enumerate(cols):
        multi, pair = t_multi.pair_fields(K, 0, c)
        want_r[multi] += cr.cpu().numpy().astype(np.float64)[pair] / K
        want_l[multi] += cl.cpu().numpy().astype(np.float64)[pair] / K
    want_loss = float(np.mean([c[0].item() for c in cols]))
    gr_, gl_ = gr.cpu().numpy(), gl.cpu().numpy()
    assert abs(loss_sum.item() - want_loss) <= 1e-6 * abs(want_loss)
    for sl in blocks:
        print(f"hinge fields {sl.start}..{sl.stop - 1}: rows {rel_err(gr_[sl], want_r[sl]):.2e}")
        assert rel_err(gr_[sl], want_r[sl]) <= 1e-6, sl
    assert rel_err(gl_[1:], want_l[1:]) <= 1e-6
    assert np.abs(gl_[0] - want_l[0]).max() <= 1e-6 * np.abs(want_l[1:]).max()
    assert int(auc.item()) == int(cols[0][1].item())  # pairwise on (p, c_0)
    ref_loss, wr, wl, _ = multineg_ref.staged(net, W, user, items, None, "hinge")
    assert abs(loss_sum.item() / B - ref_loss) <= TOL * abs(ref_loss)
    for sl in blocks:
        assert rel_err(gr_[sl], wr[sl]) <= TOL, sl
    g.check()


@pytest.mark.parametrize("net,D", cells("score_warp_fwd_bwd", ALL))
def test_warp_controlled_selection(net, D, tune):
    """K = 3 candidates on tables that make every z exact, as test_controlled_selection_is_exact: trials, chosen ids and
    zero rows exactly, loss and gradients at 1e-5."""
    tune(GRID_CAP=2)
    B, K, M = 131, 3, 0
    W, _ = t_warp.exact_tables(net, M, NU, NI, D)
    rs = np.random.RandomState(D + K)
    items, f = t_warp.controlled_block(rs, NI, B, K, t_warp.round_size(D))
    user = rs.randint(0, NU, B)
    user[0], user[1], items[0, 0] = 0, NU - 1, 0
    items[1, np.nonzero(f < 0)[0][0]] = NI - 1  # (a cold candidate of a row without a violator)
    g = Guards()
    t, T, keep = guarded_tables(net, W, g)
    weights = warp_ref.rank_weights(100_000, K, "log")
    gr, gl = g.staging("grad_rows", 3, B, D), g.staging("grad_lin", 3, B)
    got = t_warp.run_kernel(net, TablesAsNet(T, t), t_warp.device_ids(user, items, None), 1.0, weights, grad_rows=gr,
                            grad_lin=gl)
    ref = warp_ref.staged(net, W, user, items, None, 1.0, weights)
    assert np.array_equal(ref["trials"], f + 1) and (ref["h"][f >= 0, f[f >= 0]] == 1.0).all()  # (the block is as built)
    assert np.array_equal(got["trials"].cpu().numpy(), ref["trials"])
    assert np.array_equal(got["neg"].cpu().numpy(), ref["neg"])
    want_loss = weights[f[f >= 0]].sum()
    assert abs(got["loss_sum"].item() - want_loss) <= TOL * want_loss
    gr_, gl_ = gr.cpu().numpy(), gl.cpu().numpy()
    for fields in t_warp.table_fields(M):
        print(f"fields {fields}: rows {rel_err(gr_[fields], ref['gr'][fields]):.2e}")
        assert rel_err(gr_[fields], ref["gr"][fields]) <= TOL, fields
        assert rel_err(gl_[fields], ref["gl"][fields]) <= TOL, fields
    assert not gr_[:, f < 0].any() and not gl_[:, f < 0].any()  # no violator: every field exactly 0
    assert not gl_[0].any()
    assert int(got["auc"].item()) == int((ref["z"][:, 0] > ref["z"][:, 1]).sum())
    g.check()


# ------------------------------------------------------------------------------------------------- what ran
def test_every_path_meets_every_shape_and_tail_variant():
    """Runs last: the (VEC, G, K, FULL) set of every path's test ids is the full set (12 shapes + 8 FULL variants), and
    the branch every one-launch cell took."""
    ragged_only = {v for v in row_shapes.ALL_VARIANTS if not v[3]}
    for path, got in COVERAGE.items():
        # (the adaptive rules on the metadata step: the ragged widths, which the library refuses, and its own four)
        want = ragged_only | {row_shapes.variant(D) for D in META_ADAPTIVE_WIDTHS} \
            if path == "presorted metadata + adaptive rules" else row_shapes.ALL_VARIANTS
        print(f"{path}: {len(got)} of {len(want)} (VEC, G, K, FULL): {sorted(got)}")
        assert got == want, (path, sorted(want - got))
    for shape in sorted(BRANCH):
        print(f"one-launch step {shape}: " + ", ".join(f"{m}: {b}" for m, b in sorted(BRANCH[shape].items())))
