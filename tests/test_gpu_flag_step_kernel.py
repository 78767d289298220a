# -*- coding: utf-8 -*-
"""flag_step_kernel (csrc/flag_step.hip) against fwd_stage_kernel<INL 3> and the step's float64 oracle.

One step of the flag form with an arrival counter and flagged-first batches, from identical table copies, once with
K1_FLAG_KERNEL = 0 (the old kernel) and once with 1: every whole-row width D = 4 G, Linear and FM, K1_NT 0 / 1 / 3, batches
whose flagged triples end in the wave's iteration fi = 0, 1, 2 (rows held in registers) and 3 (the overflow to global
staging), trip counts of 2 to 8 iterations per wave.  The id blocks and their flags are built here, flagged triples
first, so that fi is what the case says."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import step_sensitivity as sens
import test_gpu_row_shapes as rs_
from test_gpu_kernels import DEV, make_case

pytestmark = pytest.mark.gpu

NU, NI = 700, 1500
SYNC_WORDS = 288            # include/trs.h TRS_SYNC_WORDS; the last two: references applied in the loop / behind it
GEOMETRIES = [(192, 0), (512, 2), (512, 4), (512, 5), (512, 6), (512, 8)]  # (B, K1_ITERS; 0 = by batch)
WIDTHS = [32, 64, 128, 256]


def _ops():
    from torchrecsys_amd import ops
    return ops


def geometry(B, D, iters):
    """(grid, stride, trip count of the first wave) of launch_fwd_stage for a batch of B at width D."""
    tpw = 64 // (D // 4)
    it = iters if iters > 0 else -(-B // (512 * 4 * tpw))
    it = max(it, 2)
    if iters <= 0:
        it = min(it, 8)
    grid = max(1, min(4096, -(-(-(-B // tpw)) // (4 * it))))
    stride = grid * 4 * tpw
    return grid, stride, -(-B // stride)


@functools.lru_cache(maxsize=8)
def flag_case(net, D, B, iters, fi):
    """One batch of B on NU users and NI items whose first nf triples carry a flagged reference, nf such that the last of
    them is read in iteration fi - 1 of its lane group (fi = 0: none).  Flagged triples come in pairs that share a user,
    a positive, a negative, or one's positive with the other's negative, and six of them name one hot item; every other
    row of the batch is named once."""
    grid, stride, niter = geometry(B, D, iters)
    nf = 0 if fi == 0 else min(B, (fi - 1) * stride + max(2, stride // 2))
    nf -= nf % 2
    assert nf == 0 or -(-nf // stride) == fi, (nf, stride, fi)

    def build(bump):
        rs = np.random.RandomState(1000 * bump + D + 7 * B + 31 * iters + fi)
        u = rs.permutation(NU)[:B]
        items = rs.permutation(NI)[:2 * B]
        i, j = items[:B].copy(), items[B:].copy()
        for k in range(0, nf, 2):  # triples k and k + 1 share a row
            kind = (k // 2) % 4
            if kind == 0:
                u[k + 1] = u[k]
            elif kind == 1:
                i[k + 1] = i[k]
            elif kind == 2:
                j[k + 1] = j[k]
            else:
                j[k + 1] = i[k]
        if nf >= 12:
            i[[0, 5, 10]] = items[0]
            j[[3, 6, 11]] = items[0]
        p, _, _ = make_case(net, D, 0, 8, NU=NU, NI=NI, seed=2)
        return sens.StepCase(net, sens.condition_tables(net, p), sens.batches_of(u, i, j, B, 1), sens.step_lr(B), D=D, u=u, i=i, j=j)
    case = sens.conditioned(build)
    u, i, j = case.u, case.i, case.j
    case.udup = (np.bincount(u, minlength=NU)[u] > 1).astype(np.uint8)
    cnt = np.bincount(np.concatenate([i, j]), minlength=NI)
    case.idup = np.stack([cnt[i] > 1, cnt[j] > 1], axis=1).astype(np.uint8)
    anyf = (case.udup != 0) | case.idup.any(axis=1)
    assert int(anyf.sum()) == nf and anyf[:nf].all(), (int(anyf.sum()), nf)
    case.nf, case.grid, case.niter = nf, grid, niter
    case.n_flagged_refs = int(case.udup.sum() + case.idup.sum())
    # rows of the tables with a flagged reference (everything else must not depend on the kernel at all)
    case.flagged_rows = {"user": np.unique(u[case.udup != 0]),
                         "item": np.unique(np.concatenate([i[case.idup[:, 0] != 0], j[case.idup[:, 1] != 0]]))}
    return case


def run_step(case, tune, knob, iters, nt=-1, n_flagged="nf", stats=True):
    """One step on fresh guarded copies of the case's tables; -> (tables as numpy, loss sum, err, arrivals, stats words)."""
    ops = _ops()
    net, D, B = case.net, case.D, case.B
    tune(K1_FLAG_KERNEL=knob, K1_ITERS=iters, K1_APPLY_STATS=int(stats))
    if nt >= 0:
        tune(K1_NT=nt)
    g = rs_.Guards()
    t, T, keep = rs_.guarded_tables(net, case.p, g)
    err = rs_.zero_err()
    ids = [rs_.dev_i32(a) for a in (case.u, case.i, case.j)]
    udup = torch.from_numpy(case.udup).to(DEV)
    idup = torch.from_numpy(case.idup).to(DEV)
    nfl = None if n_flagged is None else torch.tensor([case.nf if n_flagged == "nf" else n_flagged], dtype=torch.int32, device=DEV)
    gz, du, ustage = torch.empty((2, B), device=DEV), g.staging("du", B, D), g.staging("ustage", B, D)
    losses = torch.zeros(1, device=DEV)
    sync = (torch.zeros(SYNC_WORDS, dtype=torch.int32, device=DEV), ctypes.c_uint32(0))
    ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, 1, case.lr, *ids, gz, du, losses, err, ops.train_scratch(NU, NI, B, D, DEV),
                        1, None, user_dup=udup, item_dup=idup, ustage=ustage, sync=sync, n_flagged=nfl)
    torch.cuda.synchronize()
    g.check(rs_.referenced_rows(case.p, case.u, case.i, case.j))
    words = sync[0].cpu().numpy()
    return ({k: v.cpu().numpy() for k, v in t.items()}, losses.cpu().numpy(), int(err.item()), sync[1].value,
            (int(words[0]), int(words[-2]), int(words[-1])))


def unflagged_rows_identical(case, a, b):
    """(a) every row none of whose references is flagged: bit-identical between the two kernels"""
    lin = rs_.lin_names(case.net)
    for k in a:
        which = "user" if k in ("user.weight", lin[0]) else "item"
        keep = np.ones(a[k].shape[0], bool)
        keep[case.flagged_rows[which]] = False
        same = (a[k].view(np.int32) == b[k].view(np.int32)).all(axis=1)
        assert same[keep].all(), f"{k}: rows {np.nonzero(keep & ~same)[0][:8].tolist()} carry no flagged reference and differ"


def matches_oracle(case, tables, losses):
    """(b) the bar of test_flag_mode_matches_oracle, against the float64 oracle of the same step"""
    run = case.oracle(np.float64)
    sens.assert_losses(case, losses, run)
    sens.criterion_for(case)(tables, {k: v.astype(np.float32) for k, v in run.after.items()}, case.p)


def check_pair(case, tune, iters, nt=-1):
    old, l_old, e_old, arr_old, _ = run_step(case, tune, 0, iters, nt)
    new, l_new, e_new, arr_new, (ctr, in_loop, behind) = run_step(case, tune, 1, iters, nt)
    print(f"{case.net} D={case.D} B={case.B} iters={iters} trip count {case.niter} grid {case.grid} nf={case.nf}: "
          f"{case.n_flagged_refs} flagged references, {in_loop} applied in the loop, {behind} behind it")
    assert e_old == 0 and e_new == 0, (e_old, e_new)
    assert arr_old == case.grid and arr_new == case.grid and ctr == case.grid  # (d) one launch, every workgroup counted in
    unflagged_rows_identical(case, old, new)                                    # (a)
    matches_oracle(case, old, l_old)                                            # (b)
    matches_oracle(case, new, l_new)
    assert in_loop + behind == case.n_flagged_refs, (in_loop, behind, case.n_flagged_refs)  # (c)
    return in_loop, behind


@pytest.mark.parametrize("fi", [0, 1, 2, 3])
@pytest.mark.parametrize("nt", [0, 1, 3])
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("net", ["linear", "fm"])
def test_every_instance_matches_the_old_kernel_and_the_oracle(net, D, nt, fi, tune):
    """The 24 instances (2 nets x 4 widths x 3 K1_NT), 8 iterations per wave: fi = 0 (nothing flagged), 1 and 2 (held in
    registers; with a trip count of 8 the look finds them), 3 (the third iteration's triples overflow to global staging)."""
    case = flag_case(net, D, 512, 8, fi)
    in_loop, behind = check_pair(case, tune, 8, nt)
    if fi == 3:
        assert behind > 0  # (staged references are the tail's)


# (a batch of B has an iteration fi only where (fi - 1) strides fit into it: the other combinations do not exist)
TRIP_CELLS = [(net, D, B, iters, fi)
              for net, D in [("fm", 32), ("linear", 64), ("fm", 128), ("linear", 256), ("linear", 32), ("fm", 256)]
              for B, iters in GEOMETRIES for fi in (0, 1, 2, 3) if fi == 0 or (fi - 1) * geometry(B, D, iters)[1] + 2 <= B]


@pytest.mark.parametrize("net,D,B,iters,fi", TRIP_CELLS)
def test_every_trip_count(net, D, B, iters, fi, tune):
    """B = 192 as the launcher cuts it, and 512 triples at 2, 4, 5, 6 and 8 iterations per wave (the in-loop apply needs a
    trip count of 5 or more; with fewer everything is applied behind the loop, and where fi reaches the trip count the
    batch is not an early one at all: every wave counts itself in behind its last iteration)."""
    check_pair(flag_case(net, D, B, iters, fi), tune, iters)


@pytest.mark.parametrize("net,D", [("fm", 128), ("linear", 32), ("fm", 64)])
@pytest.mark.parametrize("how", ["nflag NULL", "nf = B", "knob 0"])
def test_other_forms_still_match(net, D, how, tune):
    """(e) without the flagged-first counts and with the knob at 0 the old kernel runs; a batch reported as left in its
    order (nf = B) is only known on the device: whichever kernel runs it must count every workgroup in and match."""
    case = flag_case(net, D, 512, 8, 2)
    tables, losses, err, arrivals, (ctr, in_loop, behind) = run_step(
        case, tune, 0 if how == "knob 0" else 1, 8, n_flagged=None if how == "nflag NULL" else (case.B if how == "nf = B" else "nf"))
    assert err == 0 and arrivals == case.grid and ctr == case.grid
    matches_oracle(case, tables, losses)
    if how != "nflag NULL":  # (the form without counts lists its references per workgroup and keeps no statistics per wave)
        assert in_loop + behind == case.n_flagged_refs
    if how == "nf = B":
        assert in_loop == 0


@pytest.mark.parametrize("net,D", [("fm", 128), ("linear", 32)])
def test_flagged_reference_behind_nf_raises_err_bit_3(net, D, tune):
    """(f) counts that do not describe the arrays (0 for a batch that does hold flagged triples)"""
    case = flag_case(net, D, 512, 8, 2)
    _, _, err, arrivals, _ = run_step(case, tune, 1, 8, n_flagged=0)
    assert arrivals == case.grid and err & 8
