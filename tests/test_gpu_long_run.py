# -*- coding: utf-8 -*-
"""The state that persists across steps, at the values a long training run reaches (every other test starts the world
at zero).  GPU only; the host side of the same counters is tests/test_long_run_host.py.

1. The arrival counter of the one-launch flag-mode step (trs_train_args.sync_dev / sync_count_host): three launches in
   two C calls on a counter, host count and flag lines prefilled as a long run leaves them.  The layout is the
   kernel's: word 0 is the counter, word 32 * (1 + k), k < 8, the flag lines (csrc/fast_step.hip, fwd_stage_kernel).
2. Stale flag lines.  Reading the kernel settles it: the hazard was real.  Only a launch that waits (n_flagged_dev NULL,
   or a batch whose count reports no unflagged tail) publishes its target on the lines; launches that count in early
   never write them.  A waiting launch polls `(int32)(line - target) < 0`, which is false at first look once the line is
   2^31 or more arrivals behind, so after that many early arrivals a waiting launch's workgroups would have applied their
   flagged references without waiting for the grid — silently.  trs_train_steps_sgd therefore rebases: before a step
   that finds the host count at TRS_SYNC_REBASE (2^30) or above it zeroes the 288 words on the stream and the count
   with them.  No two values on the buffer are then ever a sign bit apart.  The race itself is not tested (a lottery);
   the invariant is: count and lines after a sequence are what `expected_count` says, host and device agree, the
   results meet the oracle.  Bases at 2^31 and 2^32 are tests of the rebase; bases just below 2^30 run the kernel's own
   compares on large values, the second launch ending exactly on or across the threshold.
3. Step stamps of the duplicate-detection scratch with the high bit set and at the C guard, on a scratch that holds
   the marks of an older step, on every path that takes the scratch (the harnesses of tests/test_gpu_kernels.py).
5. rows_apply_kernel's int32 owner-election stamp at 2^31 - 2, and engine.apply_rows across RowState's restart.
6. One epoch through model.make_runner per path with the trainer's stamp about to reset (and, flag mode, the arrival
   counter about to rebase), against the oracle over the same batches."""
import ctypes
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import rel_err
from oracle import nets as onets
from oracle import optim as ooptim
from test_gpu_kernels import (DEV, TOL, check_fast_sgd_step, check_flag_mode, check_presorted_adaptive_rules,
                              check_presorted_item_update, check_presorted_step_with_metadata, make_case)

pytestmark = pytest.mark.gpu

REBASE = 1 << 30  # TRS_SYNC_REBASE (tests/test_long_run_host.py holds it to include/trs.h)
M32 = 0xFFFFFFFF
LINES = [32 * (1 + k) for k in range(8)]


def _ops():
    from torchrecsys_amd import ops
    return ops


def _lin(net):
    return ("user_bias.weight", "item_bias.weight") if net == "linear" else ("linear_user.weight", "linear_item.weight")


def sync_at(base, lines=None):
    """(device words, host count) as a run leaves them whose launches scheduled `base` arrivals and whose last waiting
    launch published `lines` (default: the same value)."""
    w = np.zeros(288, np.uint32)
    w[0] = base & M32
    w[LINES] = (base if lines is None else lines) & M32
    return torch.from_numpy(w.view(np.int32).copy()).to(DEV), ctypes.c_uint32(base & M32)


def sync_words(sync):
    w = sync[0].cpu().numpy().view(np.uint32)
    return int(w[0]), [int(x) for x in w[LINES]]


def expected_count(base, g, launches):
    """The library's rule: a step that finds the count at REBASE or above starts again from zero."""
    c = base & M32
    for _ in range(launches):
        if c >= REBASE:
            c = 0
        c = (c + g) & M32
    return c


# --------------------------------------------------------------------------------- 1 + 2: the arrival counter
FORMS = {  # form -> (users, items, batch, flagged-first order)
    "wait": (300, 57, 512, False),        # no n_flagged: count in after the last iteration, poll the flag line
    "mid": (16000, 20000, 2048, True),    # 0 < n_flagged < B: count in mid-loop (K1_ITERS = 4), look at the counter
    "none": (4096, 8192, 2048, True),     # n_flagged == 0: count in before the first iteration
}
NB, LR = 3, 0.05


@functools.lru_cache(maxsize=None)
def flag_case(form, net, D):
    """Ids and flags of three batches, the oracle's three SGD steps on them (computed once, read by every base), and the
    grid g of the one-launch step from a run at base 0."""
    ops = _ops()
    NU, NI, B, ordered = FORMS[form]
    rs = np.random.RandomState(D + len(form))
    p, _, _ = make_case(net, D, 0, 8, NU=NU, NI=NI, seed=2)
    if form == "none":  # no row twice in a batch
        u = np.concatenate([rs.permutation(NU)[:B] for _ in range(NB)])
        it = [rs.permutation(NI) for _ in range(NB)]
        i, j = np.concatenate([x[:B] for x in it]), np.concatenate([x[B:2 * B] for x in it])
    else:
        u, i, j = rs.randint(0, NU, NB * B), rs.randint(0, NI, NB * B), rs.randint(0, NI, NB * B)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ef = ops.EpochFlags(NB, B, NU, NI, DEV, ordered=ordered)
    ef.run(None, None, 0, 0, 0, err, given_ids=[torch.from_numpy(a.astype(np.int32)).to(DEV) for a in (u, i, j)])
    torch.cuda.synchronize()
    assert err.item() == 0
    u, i, j = (t_[:NB * B].cpu().numpy().astype(np.int64) for t_ in ef.ids)  # (ordered: flagged triples first)
    nf = ef.n_flagged.tolist() if ordered else None
    if form == "mid":
        assert all(0 < x < B for x in nf), nf
    if form == "none":
        assert nf == [0] * NB
    ref = {k: v.copy() for k, v in p.items()}
    losses = []
    for b in range(NB):
        sl = slice(b * B, (b + 1) * B)
        _, _, loss, grads = onets.train_forward_backward(net, ref, {"user_id": u[sl], "pos_item_id": i[sl],
                                                                     "neg_item_id": j[sl]})
        ooptim.sgd_step(ref, grads, LR)
        losses.append(float(loss))
    for v in ref.values():
        v.setflags(write=False)
    case = dict(form=form, net=net, D=D, NU=NU, NI=NI, B=B, p=p, ef=ef, ref=ref, losses=losses, g=None)
    sync = sync_at(0)
    run_flag_steps(case, sync)
    assert sync[1].value > 0 and sync[1].value % NB == 0, "the one-launch form did not run"
    case["g"] = sync[1].value // NB
    assert sync_words(sync)[0] == sync[1].value
    return case


def run_flag_steps(case, sync, calls=((2, True), (1, True))):
    """The batches of `case` from its initial tables on `sync`, one C call per (steps, pass n_flagged) pair; checked
    against the oracle: every step's loss and every table at TOL, err == 0."""
    ops = _ops()
    net, D, B, ef = case["net"], case["D"], case["B"], case["ef"]
    lin = _lin(net)
    t = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in case["p"].items()}
    T, keep = ops.make_tables(t["user.weight"], t["item.weight"], t[lin[0]], t[lin[1]])
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    gz, du = torch.empty((2, B), device=DEV), torch.empty((B, D), device=DEV)
    losses = torch.zeros(NB, device=DEV)
    scratch, ustage = ops.train_scratch(case["NU"], case["NI"], B, D, DEV), torch.empty((B, D), device=DEV)
    b = 0
    for n, with_counts in calls:
        ids, udup, idup = ef.step_args(b)
        ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, n, LR, *ids, gz, du, losses[b:], err, scratch, 1 + b, None,
                            user_dup=udup, item_dup=idup, ustage=ustage, sync=sync,
                            n_flagged=ef.n_flagged_from(b) if with_counts else None)
        b += n
    assert b == NB
    torch.cuda.synchronize()
    assert err.item() == 0, err.item()  # (bit 2: a grid wait ran into its 50 ms bound)
    got = losses.cpu().numpy() / B
    for b in range(NB):
        print("loss", b, got[b], case["losses"][b])
        assert abs(got[b] - case["losses"][b]) <= TOL * max(abs(case["losses"][b]), 1e-3), b
    for k, v in case["ref"].items():
        e = rel_err(t[k].cpu().numpy(), v)
        print(k, e)
        assert e < TOL, k


def base_for(kind, g):
    top, how = kind
    return {"across": top - g - g // 2,  # launch 2 crosses `top` while its workgroups arrive; 1 ends below, 3 starts above
            "exact": top - 2 * g,        # launch 2's target is exactly `top`
            "below": top - 3 * g - 5}[how]  # all three launches end below `top`


BASES = [(1 << 31, "across"), (1 << 31, "exact"), (1 << 32, "across"), (1 << 32, "exact"),
         (REBASE, "across"), (REBASE, "exact"), (REBASE, "below")]


@pytest.mark.parametrize("kind", BASES, ids=lambda k: "2^%d-%s" % (k[0].bit_length() - 1, k[1]))
@pytest.mark.parametrize("net,D", [("fm", 64), ("linear", 32), ("fm", 10)])
@pytest.mark.parametrize("form", list(FORMS))
def test_arrival_counter_across_the_threshold_the_sign_bit_and_the_wrap(form, net, D, kind, tune):
    if form != "wait":
        tune(K1_ITERS=4)
    case = flag_case(form, net, D)
    g = case["g"]
    assert g > 0
    base = base_for(kind, g) & M32
    sync = sync_at(base)
    run_flag_steps(case, sync)
    want = expected_count(base, g, NB)
    if kind == (REBASE, "below"):
        assert want == base + NB * g  # (no rebase: the kernel's compares ran on values just below 2^30)
    if kind == (REBASE, "exact"):
        assert want == g  # launch 2 ended exactly on the threshold, launch 3 started from zero
    if kind[0] > REBASE:
        assert want == NB * g  # rebased before the first launch
    counter, lines = sync_words(sync)
    assert sync[1].value == want  # every launch ran as one launch and the host knows what it scheduled
    assert counter == want
    if form == "wait":
        assert lines == [want] * 8  # the last launch's target, published by its last arriver


@pytest.mark.parametrize("base,lines", [((1 << 31) + 12345, 0), ((1 << 32) - 7, 0), (REBASE + 1, 1),
                                        (1 << 29, 0), (REBASE - 100000, REBASE - 100000)],
                         ids=["2^31+,lines0", "2^32-,lines0", "2^30+,lines1", "2^29,lines0", "2^30-,lines="])
@pytest.mark.parametrize("net,D", [("fm", 64), ("linear", 32), ("fm", 10)])
def test_waiting_launch_behind_early_launches_never_meets_a_line_a_sign_bit_away(net, D, base, lines, tune):
    """Two early launches (they leave the lines alone), then a waiting one on the same buffer.  Lines at 0 under a count
    beyond 2^31 is the state in which the waiting launch would not have waited; the library must have rebased before
    it gets there.  The two last cases: lines behind by less than the threshold, as between two rebases."""
    tune(K1_ITERS=4)
    case = flag_case("mid", net, D)
    g = case["g"]
    sync = sync_at(base, lines)
    run_flag_steps(case, sync, calls=((2, True), (1, False)))
    want = expected_count(base, g, NB)
    counter, got_lines = sync_words(sync)
    assert sync[1].value == want and counter == want
    assert got_lines == [want] * 8
    assert want < REBASE + g
    if base >= REBASE:
        assert want == NB * g


# ------------------------------------------------------------------------------------------ 3: step stamps
SIGN = 0x7FFFFFFE  # the steps cross the sign bit


def guard_top(n_steps):
    return 0xFFFFFFFF - 1 - n_steps  # the largest first stamp trs_train_steps_sgd accepts for n_steps steps


def older_marks(first_stamp):
    """prepare_scratch of the harnesses: one plain-path step with other ids on throw-away tables, stamped just below
    the run's first stamp, so the scratch holds ownership and duplicate marks of an older step on every row."""
    def prepare(scratch, net, NU, NI, B, D):
        if scratch is None:
            return
        ops = _ops()
        rs = np.random.RandomState(1234)
        p, _, _ = make_case(net, D, 0, 8, NU=NU, NI=NI, seed=9)
        lin = _lin(net)
        t = {k: torch.from_numpy(v).to(DEV) for k, v in p.items()}
        T, keep = ops.make_tables(t["user.weight"], t["item.weight"], t[lin[0]], t[lin[1]])
        u, i, j = rs.randint(0, NU, B), rs.randint(0, NI, B), rs.randint(0, NI, B)
        ids = [torch.from_numpy(a.astype(np.int32)).to(DEV) for a in (u, i, j)]
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, 1, 0.05, *ids, torch.empty((2, B), device=DEV),
                            torch.empty((B, D), device=DEV), torch.zeros(1, device=DEV), err, scratch, first_stamp - 1)
        torch.cuda.synchronize()
        assert err.item() == 0 and int((scratch != 0).sum()) > 0
    return prepare


@pytest.mark.parametrize("first", [SIGN, guard_top(3)], ids=hex)
@pytest.mark.parametrize("net,D", [("fm", 64), ("linear", 32), ("fm", 10), ("linear", 7)])
def test_plain_step_with_stamps_of_a_long_run(net, D, first):
    check_fast_sgd_step(net, D, first_stamp=first, prepare_scratch=older_marks(first))


@pytest.mark.parametrize("first", [SIGN, guard_top(3)], ids=hex)
@pytest.mark.parametrize("net,D,skew", [("fm", 64, True), ("linear", 32, True), ("fm", 10, True), ("fm", 80, False)])
def test_flag_mode_two_launches_with_stamps_of_a_long_run(net, D, skew, first, tune):
    check_flag_mode(net, D, skew, 300, False, tune, first_stamp=first, prepare_scratch=older_marks(first))


@pytest.mark.parametrize("first", [SIGN, guard_top(3)], ids=hex)
@pytest.mark.parametrize("inline_user", [False, True, "items", "userflags"])
@pytest.mark.parametrize("net,D,skew", [("fm", 64, True), ("linear", 32, True), ("fm", 10, True)])
def test_presorted_sgd_with_stamps_of_a_long_run(net, D, skew, inline_user, first):
    check_presorted_item_update(net, D, skew, inline_user, first_stamp=first, prepare_scratch=older_marks(first))


@pytest.mark.parametrize("first", [SIGN, SIGN - 1, guard_top(4), guard_top(4) - 1],
                         ids=["sign-even", "sign-odd", "top-even", "top-odd"])
@pytest.mark.parametrize("kind", ["sparse_adam", "adagrad"])
@pytest.mark.parametrize("net,D", [("fm", 64), ("linear", 32), ("fm", 10)])
def test_presorted_adaptive_rules_with_stamps_of_a_long_run(net, D, kind, first):
    """The skewed cases: the hot item's run is cut, so the cut-run list of the stamp's parity is in use."""
    cuts = check_presorted_adaptive_rules(net, D, True, kind, first_stamp=first, prepare_scratch=older_marks(first))
    assert cuts > 0


@pytest.mark.parametrize("first", [SIGN, guard_top(3)], ids=hex)
@pytest.mark.parametrize("net,D,M,skew", [("fm", 64, 1, False), ("fm", 16, 3, True), ("linear", 32, 1, True),
                                          ("linear", 8, 2, False), ("fm", 10, 1, True)])
def test_presorted_metadata_step_hot_row_with_stamps_of_a_long_run(net, D, M, skew, first):
    check_presorted_step_with_metadata(net, D, M, skew, "hot", 2048, first_stamp=first,
                                       prepare_scratch=older_marks(first))


# ------------------------------------------------------------------------- 5: the generic row optimisers' int32 stamp
@pytest.mark.parametrize("D", [1, 7, 64, 80])
@pytest.mark.parametrize("kind", ["adam", "adagrad"])
def test_row_optimisers_elect_one_owner_per_row_at_the_top_of_int32(D, kind):
    """step_id = 2^31 - 2, the largest RowState hands out; half the rows carry the previous step's stamp, the rest 0;
    every row of the batch is named several times: exactly one update per distinct row (a second owner would find the
    accumulator cleared and decay the moments again), untouched rows bit-identical.  Bar of
    test_coalescing_row_optimisers."""
    ops = _ops()
    rs = np.random.RandomState(D)
    n_rows, n, step_id = 40, 150, 2 ** 31 - 2
    W = rs.normal(0, 1, (n_rows, D)).astype(np.float32)
    m0 = rs.normal(0, 0.1, (n_rows, D)).astype(np.float32)
    v0 = (rs.normal(0, 0.1, (n_rows, D)) ** 2).astype(np.float32)
    if kind == "adagrad":
        m0 = v0.copy()  # (its one state table is a sum of squares)
    idx = rs.randint(0, n_rows // 2, n).astype(np.int64)  # rows >= n_rows/2 stay untouched
    assert np.bincount(idx).max() > 1
    vals = rs.normal(0, 1, (n, D)).astype(np.float32)
    old = np.where(np.arange(n_rows) % 2 == 0, step_id - 1, 0).astype(np.int32)
    tW, s1, s2 = (torch.from_numpy(a.copy()).to(DEV) for a in (W, m0, v0))
    acc = torch.zeros_like(tW)
    stamp = torch.from_numpy(old.copy()).to(DEV)
    tidx = torch.from_numpy(idx).to(DEV)
    ops.rows_scatter_add(acc, tidx, torch.from_numpy(vals).to(DEV), 1.0)
    G = np.zeros_like(W)
    np.add.at(G, idx, vals)
    rows = np.unique(idx)
    ref, m, v = W.copy(), m0.copy(), v0.copy()
    if kind == "adam":
        ops.rows_apply_sparse_adam(tW, acc, s1, s2, stamp, tidx, step_id, 0.01, 0.9, 0.999, 1e-8, 3)
        ooptim.sparse_adam_rows(ref, G, rows, m, v, 3, 0.01)
    else:
        ops.rows_apply_adagrad(tW, acc, s1, stamp, tidx, step_id, 0.05, 1e-10)
        ooptim.adagrad_rows(ref, G, rows, m, 1, 0.05)
    torch.cuda.synchronize()
    assert float(acc.abs().max()) == 0.0
    assert rel_err(tW.cpu().numpy(), ref) < 5e-5
    assert rel_err(s1.cpu().numpy(), m) < 5e-5
    if kind == "adam":
        assert rel_err(s2.cpu().numpy(), v) < 5e-5
    assert np.array_equal(tW.cpu().numpy()[n_rows // 2:], W[n_rows // 2:])
    want_stamp = old.copy()
    want_stamp[rows] = step_id
    assert np.array_equal(stamp.cpu().numpy(), want_stamp)


@pytest.mark.parametrize("D", [7, 64])
@pytest.mark.parametrize("kind", ["sparse_adam", "adagrad"])
def test_apply_rows_across_the_restart_of_the_owner_stamps(D, kind):
    """engine.apply_rows five times on one table from step_id 2^31 - 4: ids 2^31 - 3, 2^31 - 2, then the restart (stamps
    zeroed) at 1, 2, 3 — against oracle/optim.py on the coalesced gradients."""
    from torchrecsys_amd.engine import RowState, apply_rows
    rs = np.random.RandomState(D)
    n_rows, n = 60, 200
    W = rs.normal(0, 1, (n_rows, D)).astype(np.float32)
    p = torch.nn.Parameter(torch.from_numpy(W.copy()).to(DEV))
    opt = torch.optim.SparseAdam([p], lr=0.01) if kind == "sparse_adam" else torch.optim.Adagrad([p], lr=0.05)
    st = RowState(p)
    st.step_id = 2 ** 31 - 4
    ref, m, v = W.copy(), np.zeros_like(W), np.zeros_like(W)
    ids = []
    for step in range(1, 6):
        idx = rs.randint(0, n_rows // 2, n).astype(np.int64)
        vals = rs.normal(0, 1, (n, D)).astype(np.float32)
        apply_rows(kind, opt, p, st, torch.from_numpy(idx).to(DEV), torch.from_numpy(vals).to(DEV))
        ids.append(st.step_id)
        G = np.zeros_like(W)
        np.add.at(G, idx, vals)
        if kind == "sparse_adam":
            ooptim.sparse_adam_rows(ref, G, np.unique(idx), m, v, step, 0.01)
        else:
            ooptim.adagrad_rows(ref, G, np.unique(idx), m, step, 0.05)
        torch.cuda.synchronize()
        assert float(st.acc.abs().max()) == 0.0
        stamps = st.stamp.cpu().numpy()
        assert set(np.unique(stamps[np.unique(idx)])) == {st.step_id}
    assert ids == [2 ** 31 - 3, 2 ** 31 - 2, 1, 2, 3]
    assert rel_err(p.data.cpu().numpy(), ref) < 5e-5
    state = opt.state[p]
    assert rel_err((state["exp_avg"] if kind == "sparse_adam" else state["sum"]).cpu().numpy(), m) < 5e-5
    assert np.array_equal(p.data.cpu().numpy()[n_rows // 2:], W[n_rows // 2:])


# ----------------------------------------------------------------------------------- 6: through the front door
LIMIT = 0xFFFFFFF0  # SparseScorerTrainer._stamps restarts before it


def front_door_model(net_type, D, hot):
    from torchrecsys_amd.model import TorchRecSys
    import contextlib
    import io
    rs = np.random.RandomState(11)
    n_u, n_i, n = 400, 300, 4000
    users = np.concatenate([np.arange(n_u), rs.randint(0, n_u, n - n_u)])
    items = np.concatenate([np.arange(n_i), rs.randint(0, n_i, n - n_i)])
    if hot:
        items[n_i:][rs.rand(n - n_i) < 0.4] = 7  # one item's run is cut in every batch
    df = pd.DataFrame({"user": users, "item": items})
    np.random.seed(5)
    torch.manual_seed(5)
    with contextlib.redirect_stdout(io.StringIO()):
        return TorchRecSys(dataset=df, user_id_col="user", item_id_col="item", n_factors=D, net_type=net_type,
                           dynamic_neg_sampling=True)


def epoch_batches(runner, B):
    ep = {k: v.cpu().numpy().astype(np.int64) for k, v in runner.ep.items()}
    n = ep["user"].shape[0]
    return [{"user_id": ep["user"][s:s + B], "pos_item_id": ep["pos"][s:s + B], "neg_item_id": ep["neg"][s:s + B]}
            for s in range(0, n, B)]


@pytest.mark.parametrize("path,base", [("flags", REBASE - 1), ("flags", (1 << 32) - 3), ("sorted", None)],
                         ids=["flags-2^30", "flags-2^32", "sorted"])
@pytest.mark.parametrize("net_type,D", [("fm", 64), ("linear", 16)])
def test_one_sgd_epoch_through_the_runner_with_counters_of_a_long_run(net_type, D, path, base, monkeypatch):
    """Flag mode (TRS_SPARSE_REGIME=1) / presorted SGD: the stamp restarts behind the epoch's fourth step; flag mode: the
    arrival counter is rebased behind the first launch (base 2^30 - 1) or before it (2^32 - 3).  Oracle SGD over the
    same batches, bar of the end-to-end fixtures (2e-5)."""
    monkeypatch.setenv("TRS_SPARSE_REGIME", "1" if path == "flags" else "0")
    model = front_door_model(net_type, D, hot=False)
    B, lr = 256, 0.05
    ref = {k: v.cpu().numpy().copy() for k, v in model.net.state_dict().items()}
    runner = model.make_runner(torch.optim.SGD(model.parameters(), lr=lr), B)
    tr = runner.trainer
    assert tr.fast_kind == "sgd" and tr.wants_presort(B) and tr.sparse_regime(B) == (path == "flags")
    tr.stamp = LIMIT - 6
    if base is not None:
        tr.sync = sync_at(base)
    model.net.train()
    runner.begin_epoch()
    batches = epoch_batches(runner, B)
    assert runner.num_batches == len(batches) >= 12 and batches[-1]["user_id"].shape[0] < B  # (a partial last batch)
    stamps = []
    while runner.next_batch < runner.num_batches:
        assert runner.run_steps(4) > 0
        stamps.append(tr.stamp)
    assert stamps[0] == LIMIT - 2 and stamps[1] == 5 and stamps[-1] == len(batches) - 4 + 1  # restarted behind step 4
    got_loss = runner.end_epoch()  # (checks the error flag)
    sums = runner.loss_sums.cpu().numpy()
    want_loss = 0.0
    for b, batch in enumerate(batches):
        _, _, loss, grads = onets.train_forward_backward(net_type, ref, batch)
        ooptim.sgd_step(ref, grads, lr)
        nb = batch["user_id"].shape[0]
        assert abs(sums[b] / nb - float(loss)) <= 2e-5 * max(abs(float(loss)), 1e-3), b
        want_loss += float(loss) / len(batches)
    assert abs(got_loss - want_loss) <= 2e-5 * want_loss
    for k, v in ref.items():
        assert rel_err(model.net.state_dict()[k].cpu().numpy(), v) < 2e-5, k
    if base is not None:
        counter, _ = sync_words(tr.sync)
        full = len(batches) - 1
        launches = full - 1 if base < REBASE else full  # one-launch steps behind the rebase
        assert 0 < counter == tr.sync[1].value < REBASE and counter % launches == 0  # (the same grid every step)


@pytest.mark.parametrize("net_type,D", [("fm", 64), ("linear", 16)])
def test_one_sparse_adam_epoch_through_the_runner_with_the_stamp_restart(net_type, D, monkeypatch):
    """Presorted SparseAdam with a hot item (cut runs in every step).  The last stamp before the restart and the first
    one after it are both odd: the restart must leave that parity's cut-run counter empty.  Oracle SparseAdam on the
    coalesced gradients of the rows present in each batch; bar of test_presorted_adaptive_rules_match_the_oracle's
    skewed cases."""
    from oracle.nets import touched_rows
    monkeypatch.delenv("TRS_SPARSE_REGIME", raising=False)
    model = front_door_model(net_type, D, hot=True)
    B, lr = 256, 0.01
    names = list(model.net.state_dict().keys())
    params = dict(model.net.named_parameters())
    ref = {k: v.cpu().numpy().copy() for k, v in model.net.state_dict().items()}
    r1 = {k: np.zeros_like(v) for k, v in ref.items()}
    r2 = {k: np.zeros_like(v) for k, v in ref.items()}
    opt = torch.optim.SparseAdam(list(model.parameters()), lr=lr)
    runner = model.make_runner(opt, B)
    tr = runner.trainer
    assert tr.fast_kind == "sparse_adam" and tr.wants_presort(B)
    tr.stamp = LIMIT - 6
    model.net.train()
    runner.begin_epoch()
    batches = epoch_batches(runner, B)
    cuts = []
    while runner.next_batch < runner.num_batches:
        assert runner.run_steps(4) > 0
        cuts.append(int(tr.cut_count[0].max().item()))
    # restarted behind step 4 (the partial last batch takes the generic path: no stamp); every C call's last step listed cut runs
    assert tr.stamp == len(batches) - 1 - 4 + 1 and min(cuts[:-1]) > 0
    got_loss = runner.end_epoch()
    want_loss = 0.0
    for b, batch in enumerate(batches):
        _, _, loss, grads = onets.train_forward_backward(net_type, ref, batch)
        rows = touched_rows(net_type, ref, batch)
        for k in names:
            ooptim.sparse_adam_rows(ref[k], grads[k], rows[k], r1[k], r2[k], b + 1, lr)
        want_loss += float(loss) / len(batches)
    assert abs(got_loss - want_loss) <= 2.01e-4  # (the bar of the printed epoch losses in tests/test_gpu_model.py)

    def rows_within(got, want, tol):
        return float((np.abs(got - want).max(axis=1) <= tol * np.abs(want).max()).mean())

    for k in names:
        p_ = params[k]
        got = model.net.state_dict()[k].cpu().numpy()
        assert rows_within(got, ref[k], 1e-3) >= 0.97, k
        assert rows_within(opt.state[p_]["exp_avg"].cpu().numpy(), r1[k], 1e-3) >= 0.97, k
        assert rows_within(opt.state[p_]["exp_avg_sq"].cpu().numpy(), r2[k], 1e-3) >= 0.97, k
        assert rel_err(got, ref[k]) < 0.05, k
