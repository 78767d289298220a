# -*- coding: utf-8 -*-
"""The one-launch flag-mode step with flagged-first batches, applying its flagged references INSIDE the main loop
(csrc/fast_step.hip fwd_stage_kernel<..., INL 3>, `inloop`; knob K1_APPLY_IN_LOOP), against the fp64-checked oracle
and the one-lost-reference criteria of tests/step_sensitivity.py.

A wave looks at the arrival counter once, behind phase nph - 4 of its nph = (trip count rounded up to even) phases, if
the workgroups count themselves in at least one phase earlier (fi < nph - 3, fi = ceil(flagged triples / stride)); it
then applies a round of 2 references (1 where a row is 4 dwords per lane) behind each of its last three phases; what is
left goes to the tail.  Row shapes with K > 1 (D > 256) do not have the path.  With
K1_APPLY_STATS the kernel counts the references it applied in the loop and in the tail into the last two words of the
sync buffer, which is how these tests see which path ran.

Every case: two C calls of 2 + 1 steps (the counter carries over), oracle parity, err == 0, arrivals == 3 x grid,
in-loop + tail == the flagged references of the three batches (from the presort's flags), and in-loop > 0 or == 0 as
the rules above say.  Batches are built so that exactly the first nf triples of a batch carry flags: pairs of triples
that share one row (or all three), every other row named once.

(Waves of one launch differ by at most one iteration, and early mode needs fi below the launch's trip count, so a wave
with fewer iterations than fi does not occur in early mode; the ragged case here is the one that does occur: the last
waves one iteration short, their last lane groups partly beyond the batch.)"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import step_sensitivity as sens
from row_shapes import pick_row_cfg
from test_gpu_kernels import DEV, lr_of, make_case

pytestmark = pytest.mark.gpu

NB = 3
STAT_LOOP, STAT_TAIL = 286, 287  # TRS_SYNC_WORDS - 2, - 1


def tpw_of(D):
    return 64 // pick_row_cfg(D)[1]


def grid_of(B, D, iters):
    """launch_fwd_stage with K1_ITERS = iters"""
    tpw = tpw_of(D)
    return max(1, min(4096, ((B + tpw - 1) // tpw + 4 * iters - 1) // (4 * iters)))


def inloop_allowed(B, D, iters, nf):
    """Whether the waves with a full trip count take the in-loop path: fi < nph - 3."""
    stride = grid_of(B, D, iters) * 4 * tpw_of(D)
    total = (B + stride - 1) // stride
    fi = (nf + stride - 1) // stride
    nph = (total + 1) & ~1
    return nf > 0 and fi < total and fi < nph - 3


@functools.lru_cache(maxsize=64)
def inloop_case(net, D, B, nf, share_all=False, NU=None, NI=None):
    """NB batches of B triples; in every batch nf (even) triples are flagged: pairs that share the user, the positive or
    the negative row (share_all: all three, so every flagged triple lists three references); all other rows are named
    once per batch.  nf odd: the last flagged triple shares its user with the first pair's, so some wave holds an odd
    number of references.  The triples of a batch are shuffled: the presort puts the flagged ones first."""
    assert nf != 1 and nf <= B
    NU, NI = NU or max(2 * B, 1024), NI or max(4 * B, 2048)

    def build(bump):
        rs = np.random.RandomState(1000 * bump + D + B + nf)
        p, _, _ = make_case(net, D, 0, 8, NU=NU, NI=NI, seed=4)
        us, is_, js = [], [], []
        for _ in range(NB):
            u = rs.permutation(NU)[:B]
            it = rs.permutation(NI)
            i, j = it[:B].copy(), it[B:2 * B].copy()
            a, b = np.arange(0, nf - 1, 2), np.arange(1, nf, 2)
            kind = rs.randint(0, 3, a.size)
            for k, arr in enumerate((u, i, j)):
                m = np.ones(a.size, bool) if share_all else kind == k
                arr[b[m]] = arr[a[m]]
            if nf % 2:
                u[nf - 1] = u[0]
            o = rs.permutation(B)
            us.append(u[o]); is_.append(i[o]); js.append(j[o])
        u, i, j = np.concatenate(us), np.concatenate(is_), np.concatenate(js)
        return sens.StepCase(net, sens.condition_tables(net, p), sens.batches_of(u, i, j, B, NB), lr_of(B, D, None), D=D,
                             NU=NU, NI=NI, u=u, i=i, j=j, nf=nf)
    return sens.conditioned(build)


def run_inloop(case, tune, iters, knob, nt=None, expect_loop=None):
    """check_flag_mode's ordered one-launch form (tests/test_gpu_kernels.py) with the knobs of this path.  Returns
    (references applied in the loop, in the tail)."""
    from torchrecsys_amd import ops
    knobs = dict(K1_ITERS=iters, K1_APPLY_IN_LOOP=knob, K1_APPLY_STATS=1)
    if nt is not None:
        knobs["K1_NT"] = nt
    tune(**knobs)
    net, p, D, NU, NI, B, nb, lr = case.net, case.p, case.D, case.NU, case.NI, case.B, case.nb, case.lr
    lin = ("user_bias.weight", "item_bias.weight") if net == "linear" else ("linear_user.weight", "linear_item.weight")
    t = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in p.items()}
    T, keep = ops.make_tables(t["user.weight"], t["item.weight"], t[lin[0]], t[lin[1]])
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ef = ops.EpochFlags(nb, B, NU, NI, DEV, ordered=True)
    ef.run(None, None, 0, 0, 0, err, given_ids=[torch.from_numpy(a.astype(np.int32)).to(DEV) for a in (case.u, case.i, case.j)])
    ids, udup, idup = ef.step_args(0)
    uo, io, jo = (t_[:nb * B].cpu().numpy().astype(np.int64) for t_ in ids)
    ud, idp = udup[:nb * B].cpu().numpy() != 0, idup[:nb * B].cpu().numpy() != 0
    for b in range(nb):  # the batch as built: exactly nf flagged triples, all of them first
        sl = slice(b * B, (b + 1) * B)
        anyf = ud[sl] | idp[sl].any(axis=1)
        assert int(ef.n_flagged[b].item()) == case.nf == int(anyf.sum()) and anyf[:case.nf].all()
    n_refs = int(ud.sum()) + int(idp.sum())  # every flagged reference of the three launches
    run = case.oracle_on(sens.batches_of(uo, io, jo, B, nb))  # (as the steps see them)
    gz, du = torch.empty((2, B), device=DEV), torch.empty((B, D), device=DEV)
    losses = torch.zeros(nb, device=DEV)
    sync = (torch.zeros(288, dtype=torch.int32, device=DEV), ctypes.c_uint32(0))
    scratch, ustage = ops.train_scratch(NU, NI, B, D, DEV), torch.empty((B, D), device=DEV)
    ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, 2, lr, *ids, gz, du, losses, err, scratch, 1, None,
                        user_dup=udup, item_dup=idup, ustage=ustage, sync=sync, n_flagged=ef.n_flagged_from(0))
    ids2, udup2, idup2 = ef.step_args(2)
    ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, 1, lr, *ids2, gz, du, losses[2:], err, scratch, 3, None,
                        user_dup=udup2, item_dup=idup2, ustage=ustage, sync=sync, n_flagged=ef.n_flagged_from(2))
    torch.cuda.synchronize()
    words = sync[0].cpu().numpy().astype(np.int64)
    n_loop, n_tail = int(words[STAT_LOOP]), int(words[STAT_TAIL])
    print(f"grid {grid_of(B, D, iters)}, flagged references {n_refs}: applied in the loop {n_loop}, in the tail {n_tail}")
    assert sync[1].value == 3 * grid_of(B, D, iters) and int(words[0]) == sync[1].value
    assert err.item() == 0
    sens.assert_losses(case, losses.cpu().numpy(), run)
    sens.criterion_for(case)({k: t[k].cpu().numpy() for k in run.after}, run.after, p)
    assert n_loop + n_tail == n_refs
    if expect_loop is None:
        expect_loop = bool(knob) and inloop_allowed(B, D, iters, case.nf)
    assert (n_loop > 0) == expect_loop, (n_loop, n_tail, expect_loop)
    return n_loop, n_tail


def batch_for(D, iters, wgs=8):
    """exactly `iters` strides of a grid of `wgs` workgroups"""
    return wgs * 4 * tpw_of(D) * iters


@pytest.mark.parametrize("knob", [1, 0])
@pytest.mark.parametrize("nt", [0, 3])
@pytest.mark.parametrize("net,D", [("fm", 128), ("linear", 32)])
def test_c4_loop_shape_in_small(net, D, nt, knob, tune):
    """8 iterations, a batch of exactly 8 strides (D = 128: 8 workgroups x 64 triples), 3/16 of the triples flagged:
    fi = 2, the look behind phase 4."""
    B = batch_for(D, 8)
    case = inloop_case(net, D, B, 3 * B // 16)
    assert inloop_allowed(B, D, 8, case.nf)
    run_inloop(case, tune, 8, knob, nt, expect_loop=bool(knob))


@pytest.mark.parametrize("knob", [1, 0])
def test_full_waves(knob, tune):
    """Every triple of the first two iterations carries three flagged references: 12 per wave at D = 128 — three in-loop
    rounds of 2 and a remainder of 6 in the tail."""
    D = 128
    B = batch_for(D, 8)
    case = inloop_case("fm", D, B, B // 4, share_all=True)
    n_loop, n_tail = run_inloop(case, tune, 8, knob, expect_loop=bool(knob))
    if knob:
        assert n_loop == n_tail == 3 * 6 * (B // 16)  # per launch: every wave 6 + 6


@pytest.mark.parametrize("knob", [1, 0])
@pytest.mark.parametrize("D", [132, 256])
def test_wide_rows_take_rounds_of_one_row(D, knob, tune):
    """(4, 64, 1), ragged and whole: one triple per wave and iteration, the triples of the first two iterations with three
    flagged references each — 6 per wave, of which three rounds of ONE row take 3 in the loop."""
    B = batch_for(D, 8, wgs=4)
    case = inloop_case("fm", D, B, B // 4, share_all=True)
    n_loop, n_tail = run_inloop(case, tune, 8, knob, expect_loop=bool(knob))
    if knob:
        assert n_loop == n_tail == 3 * 3 * (B // 8)  # per launch: every wave 3 + 3


BOUNDARIES = {
    # name: (iterations, batch in strides of 8 workgroups (None: see below), flagged triples in strides, in-loop path)
    "fi0": (8, 8, 0, False),            # no flagged reference at all
    "fi_before": (8, 8, 3.5, True),     # fi = 4: counted in one phase before the look's phase
    "fi_at": (8, 8, 4.5, False),        # fi = 5
    "fi_behind": (8, 8, 5.5, False),    # fi = 6
    "odd7": (7, 7, 1.5, True),          # the padded eighth phase
    "trip2": (2, 2, 0.5, False),
    "trip3": (3, 3, 0.5, False),
    "trip4": (4, 4, 0.5, False),
    "ragged": (8, None, 1.5, True),     # the last waves one iteration short, the last lane group half valid
    "ragged7": (7, -20, 1.5, True),     # 7 strides less 20 triples: the last waves have 6 iterations, so 6 phases and
    #                                     their look two phases earlier (behind phase 2) than the others' (behind phase 4)
    "odd_refs": (8, 8, 3 / 64, True),   # three flagged triples: waves with 1 and 3 references, a round of 1 of 2 rows
}


@pytest.mark.parametrize("knob", [1, 0])
@pytest.mark.parametrize("name", list(BOUNDARIES))
def test_boundaries_of_the_apply_point(name, knob, tune):
    D = 128
    iters, strides, nf_strides, allowed = BOUNDARIES[name]
    stride = batch_for(D, 1)
    B = 8 * stride - 37 if strides is None else (iters * stride + strides if strides < 0 else strides * stride)
    nf = int(nf_strides * stride)
    assert grid_of(B, D, iters) == 8 and inloop_allowed(B, D, iters, nf) == allowed
    if name == "ragged7":  # (waves 22 ... 31 start behind 6 strides)
        assert (B + stride - 1) // stride == 7 and B - 2 * 31 <= 6 * stride < B - 2 * 21
    case = inloop_case("fm", D, B, nf)
    n_loop, n_tail = run_inloop(case, tune, iters, knob, expect_loop=bool(knob) and allowed)
    if name == "odd_refs" and knob:
        assert n_tail == 0  # (at most 4 references per wave: two rounds)


@pytest.mark.parametrize("knob", [1, 0])
@pytest.mark.parametrize("D", [10, 80, 64, 16, 33, 132, 256, 260])
def test_other_row_shapes(D, knob, tune):
    """A ragged width (10: lane group 16), two staged dwords per lane on a ragged row (80), lane groups 16 and 4 with 4 and
    16 triples per wave (64, 16), a (1, 64, 1) width (33), the (4, 64, 1) shape ragged and whole (132, 256: four staged
    dwords per lane, rounds of ONE row), at 8 iterations; and a K = 2 shape (260), for which the in-loop path is not
    compiled (no registers to spare): everything in the tail, whatever the knob."""
    B = batch_for(D, 8, wgs=4)
    case = inloop_case("fm", D, B, 3 * B // 16)
    run_inloop(case, tune, 8, knob, expect_loop=bool(knob) and pick_row_cfg(D)[2] == 1)


@pytest.mark.parametrize("iters", [8, 4])
def test_flag_counts_of_another_origin_with_the_in_loop_path(iters, tune):
    """test_one_launch_step_reports_flag_counts_of_another_origin with the in-loop path on: zeroed counts for batches
    that do hold flagged triples — the workgroups count themselves in before their first iteration, waves look and
    apply inside the loop while flagged references still turn up behind them; err bit 3 is raised, every reference is
    applied once (in the loop or in the tail) and nothing hangs."""
    from torchrecsys_amd import ops
    rs = np.random.RandomState(5)
    NU, NI, B, D = 4000, 5000, 2048, 64
    tune(K1_ITERS=iters, K1_APPLY_IN_LOOP=1, K1_APPLY_STATS=1)
    p, _, _ = make_case("fm", D, 0, 8, NU=NU, NI=NI, seed=1)
    t = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in p.items()}
    T, keep = ops.make_tables(t["user.weight"], t["item.weight"], t["linear_user.weight"], t["linear_item.weight"])
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ef = ops.EpochFlags(1, B, NU, NI, DEV)
    ef.run(None, None, 0, 0, 0, err,
           given_ids=[torch.from_numpy(rs.randint(0, n, B).astype(np.int32)).to(DEV) for n in (NU, NI, NI)])
    assert 0 < int(ef.n_flagged[0].item()) < B
    ef.n_flagged.zero_()
    ids, udup, idup = ef.step_args(0)
    n_refs = int((udup[:B] != 0).sum().item()) + int((idup[:B] != 0).sum().item())
    sync = (torch.zeros(288, dtype=torch.int32, device=DEV), ctypes.c_uint32(0))
    ops.train_steps_sgd("fm", T, None, None, 0, 0, 0, B, 1, 0.05, *ids, torch.empty((2, B), device=DEV),
                        torch.empty((B, D), device=DEV), torch.zeros(1, device=DEV), err,
                        ops.train_scratch(NU, NI, B, D, DEV), 1, None, user_dup=udup, item_dup=idup,
                        ustage=torch.empty((B, D), device=DEV), sync=sync, n_flagged=ef.n_flagged_from(0))
    torch.cuda.synchronize()
    words = sync[0].cpu().numpy().astype(np.int64)
    print(f"flagged references {n_refs}: applied in the loop {int(words[STAT_LOOP])}, in the tail {int(words[STAT_TAIL])}")
    assert sync[1].value == grid_of(B, D, iters) and int(words[0]) == sync[1].value
    assert int(err.item()) == 8  # bit 3 alone: no time-out (bit 2), no bad id
    assert int(words[STAT_LOOP]) + int(words[STAT_TAIL]) == n_refs
    assert int(words[STAT_LOOP]) > 0  # (4 iterations: the look comes behind phase 0, whose triples hold flagged references)
