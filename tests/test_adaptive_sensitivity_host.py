# -*- coding: utf-8 -*-
"""Can the adaptive-rule parity tests see one lost reference, and every narrow fault of the cut-run path?  No GPU: the
inputs and the criterion of tests/test_gpu_adaptive_parity.py (the same `*_case()` functions), the oracle in oracle/, and
the faults of tests/adaptive_sensitivity.py.

For every case of every cell:

  conditioning          the builder took the first seed whose fp32 and float64 oracle runs differ by at most a third of a
                        quarter reference on every row, whose hinge arguments stay 100 roundings away from the kink, and
                        in which every step moves some table.
  one lost reference    every ONE-sided reference of every step has a detection ratio of at least 3 on the weights and on
                        SparseAdam's exp_avg, in every table; the weakest of each table is built (the oracle re-run with
                        that contribution missing from the row's gradient) and refused.  Of the TWO-sided references
                        (FM's linear_user; linear_metadata where both items share the category) at least half per case.
                        exp_avg_sq and Adagrad's sum are quadratic in the gradient: row-level faults only.
  row-level faults      a whole piece of a cut run lost; a cut row not written by the last step; state read as zero; the
                        last step not applied; the accumulator left dirty; the step counter off by one (asserted on
                        the step0 = 3 cases — at step0 = 1000 SparseAdam's first bias correction has converged, the
                        second moves by 3e-4 of itself per step and Adagrad's clr by 1e-3: there the fault may be
                        legitimately invisible, and what the criterion says is printed).  A fault on a 1-wide table
                        (sums of +-slopes that cancel, Linear's item_bias exactly) is asserted where it amounts to at
                        least one reference of the row; the D-wide table beside it always.
  a row no id names, and Linear's user_bias: one changed bit in weights or state is refused.

test_bulk_criterion_accepts_an_unwritten_hot_row records why these tests exist."""
import numpy as np
import pytest

import adaptive_sensitivity as ads
import step_sensitivity as sens
import test_gpu_adaptive_parity as P
from test_gpu_kernels import make_case


def _params():
    return [pytest.param(fn, args, id=fn.__name__[:-5] + "-" + "-".join(map(str, args))) for fn, args in P.all_cases()]


def cut_tables(case):
    return ["item.weight"] + [f"metadata.{m}.weight" for m in range(case.M)]


def lin_of(case, table):
    """the 1-wide table updated beside a D-wide one (None: a Linear scorer's metadata column)"""
    if table == "item.weight":
        return P._lin(case.net)[1]
    return "linear_" + table if case.net == "fm" else None


@pytest.mark.parametrize("build,args", _params())
def test_every_reference_and_every_fault_is_seen(build, args):
    case = build(*args)
    crit, ref, before = case.criterion(), ads.results(case.oracle()), case.before
    refused = lambda got: ads.raises(crit, got, ref, before)  # noqa: E731
    ok, text = ads.conditioning(case)
    print(f"{case.kind}, step0 {case.step0}, B {case.B}, {case.nb} steps, seed bump {case.seed}: {text}")
    assert ok, text
    crit(ref, ref, before, verbose=False)  # the oracle's own result passes
    for seed in (0, 1):  # ... and so does a second correct fp32 evaluation: the same triples in another order
        crit(ads.reordered(case, seed), ref, before, verbose=False)
    fails, line = [], []

    # one lost reference
    for n in ads.linear_tensors(case):
        for k, (r, soft, st, ix) in ads.reference_ratios(case, n).items():
            if k in crit.zero_grad and r.size:
                fails.append(f"{k}: the criterion takes the table for unmoved, but it has references")
            elif (~soft).any():
                w = np.nonzero(~soft)[0][np.argmin(r[~soft])]
                line.append(f"{n} {k[:-7]} {r[w]:.1f}")
                if r[w] < sens.MIN_RATIO:
                    fails.append(f"{n} {k}: weakest reference at {r[w]:.2f} allowances (< {sens.MIN_RATIO:g})")
                if n == "w" or "w" not in case.judged:  # built and judged for real (one re-run of the oracle per table)
                    if not refused(ads.without_reference(case, int(st[w]), k, int(ix[w]))):
                        fails.append(f"{n} {k}: step {st[w]}, reference {ix[w]} lost: accepted")
        shares = {k: v for (n_, k), v in ads.two_sided_shares(case).items() if n_ == n}
        tot, good = (sum(v[q] for v in shares.values()) for q in (0, 1))
        line.append(" ".join(f"{n} {k[:-7]} {g}/{t}" for k, (t, g) in shares.items()))
        if 2 * good < tot:
            fails.append(f"{n}: {good} of {tot} two-sided references meet the bar (< half)")

    # the cut-run path: the longest cut row of every sorted table, in the D-wide table and in the 1-wide one beside it.
    # The 1-wide gradient of a row is a sum of +-slopes (Linear's item_bias: of +-1/B) that may cancel, exactly even: a
    # piece, a stale accumulator or a whole step of it that amounts to less than ONE reference of the row is no fault
    # the result could show, and is counted as such (printed), never the D-wide one.
    faint = 0
    for k in cut_tables(case):
        both = [k] + ([lin_of(case, k)] if lin_of(case, k) else [])
        for st in sorted({0, case.nb - 1}):  # (the first step and the last)
            hot = int(ads.cut_rows_of(ads.sorted_references(case.batches[st], k))[0])
            for tab in both:
                rows, trip, soft, c, eff = case.effects()[st][tab]
                mine = (rows == hot) & ~soft
                one = np.abs(c[mine]).max(axis=1).min() if mine.any() else np.inf  # the row's smallest reference
                seen = lambda dg: tab == k or np.abs(dg).max() >= one  # noqa: E731
                if not seen(c[ads.piece_of(case, st, tab, hot)].sum(axis=0)):
                    faint += 1
                elif not refused(ads.without_piece(case, st, tab, hot)):
                    fails.append(f"{tab}: a piece of row {hot} lost in step {st}: accepted")
                if case.step0 and not refused(ads.state_read_as_zero(case, st, tab, hot)):
                    fails.append(f"{tab}: state of row {hot} read as zero in step {st}: accepted")
                if st + 1 < case.nb:
                    if not seen(case.oracle().befores[st]["g"][tab][hot]):
                        faint += 1
                    elif not refused(ads.accumulator_left_dirty(case, st, tab, hot)):
                        fails.append(f"{tab}: gradient of row {hot} of step {st} still in the accumulator: accepted")
        last = case.oracle().befores[-1]
        for row in ads.cut_rows_of(ads.sorted_references(case.batches[-1], k)):  # EVERY cut row of the last step
            for tab in both:
                moved = max(float((np.abs(ref[n][tab][row].astype(np.float64) - last[n][tab][row]).max()
                                   / crit.allow[n][tab][row])) for n in case.judged)
                if tab != k and moved < sens.MIN_RATIO:  # (the step leaves the 1-wide row within its allowance)
                    faint += 1
                elif not refused(ads.row_unwritten(case, tab, int(row))):
                    fails.append(f"{tab}: cut row {row} left unwritten by the last step: accepted")
    line.append(f"{faint} 1-wide faults below one reference")
    if case.step0:  # state read as zero off the cut path: a user run, the first row the last step touches
        for tab in ("user.weight", P._lin(case.net)[0]):
            if tab not in crit.zero_grad:
                row = int(case.oracle().befores[-1]["rows"][tab][0])
                if not refused(ads.state_read_as_zero(case, case.nb - 1, tab, row)):
                    fails.append(f"{tab}: state of row {row} read as zero: accepted")
    if not refused(ads.last_step_not_applied(case)):
        fails.append("last step not applied: accepted")
    if case.step0 == 3:
        if not refused(ads.step_counter_off_by_one(case)):
            fails.append("step counter off by one: accepted")
    elif case.step0:
        line.append(f"step counter off by one at step0 = {case.step0}: " +
                    ("refused" if refused(ads.step_counter_off_by_one(case)) else "invisible (converged)"))

    # rows no id names, and the table without a gradient: one bit
    for n in case.judged:
        for k in case.p:
            free = np.nonzero(crit.allow[n][k] == 0)[0]
            if free.size:
                got = {m: {q: v.copy() for q, v in tabs.items()} for m, tabs in ref.items()}
                got[n][k].view(np.int32)[free[0], 0] ^= 1
                if not refused(got):
                    fails.append(f"{n} {k}: a changed bit in row {free[0]}, which no reference reaches: accepted")
    if case.net == "linear":
        assert "user_bias.weight" in crit.zero_grad
    print(" | ".join(line))
    assert not fails, fails


def test_without_the_gradient_rounding_floor_two_fp32_evaluations_disagree():
    """Why AdaptiveRowCriterion has a third floor: held to a quarter reference, 3 x the fp32-vs-float64 difference and two
    fp32 steps of the value alone, the fp32 oracle on the same triples in another order is REFUSED on Adagrad's sum of
    FM's linear_user (a quadratic tensor of a gradient that is a difference of sigmoid slopes: 2 g dg reaches four fp32
    steps of the sum).  Oracle runs only."""
    case = P.presorted_case("fm", 64, False, "adagrad", 1000)
    ref = ads.results(case.oracle())
    bare = ads.AdaptiveRowCriterion(case, gradient_roundings=0)
    refused = [seed for seed in range(3) if ads.raises(bare, ads.reordered(case, seed), ref, case.before)]
    print(f"reordered fp32 oracle refused without the floor: seeds {refused}")
    assert refused
    for seed in range(3):
        case.criterion()(ads.reordered(case, seed), ref, case.before, verbose=False)


def test_bulk_criterion_accepts_an_unwritten_hot_row():
    """The "before": on the skewed SparseAdam case of test_presorted_adaptive_rules_match_the_oracle (FM, D = 64, cold
    start, 4 steps, 97 % of the rows within 1e-3 and rel_err < 0.05) the hot item — the one row of 57 whose run is cut
    into pieces — may be left unwritten in ALL four steps, in weights and in both moments, and the criterion accepts.
    This asserts nothing about the kernels."""
    net, D, skew, nb, B = "fm", 64, True, 4, 512
    rs = np.random.RandomState(D + skew)
    p, _, _ = make_case(net, D, 0, 8, NU=P.NU, NI=P.NI, seed=2)
    u, i, j = rs.randint(0, P.NU, nb * B), rs.randint(0, P.NI, nb * B), rs.randint(0, P.NI, nb * B)
    i[rs.rand(nb * B) < 0.4] = P.HOT_ITEM
    j[rs.rand(nb * B) < 0.4] = P.HOT_ITEM
    case = ads.AdaptiveCase(net, p, sens.batches_of(u, i, j, B, nb), "sparse_adam", 0, M=0)
    ref = ads.results(case.oracle())
    got = {n: {k: v.copy() for k, v in tabs.items()} for n, tabs in ref.items()}
    for n in got:
        for k in ("item.weight", "linear_item.weight"):
            got[n][k][P.HOT_ITEM] = case.before[n][k][P.HOT_ITEM]
    moved = float(np.abs(ref["w"]["item.weight"][P.HOT_ITEM] - p["item.weight"][P.HOT_ITEM]).max())
    print(f"hot row moved by {moved:.3f} over {nb} steps, max|table| {np.abs(ref['w']['item.weight']).max():.2f}")
    assert moved > 0.03
    assert ads.bulk_criterion_accepts(got, ref)
    # the same result on the warm case of the same shape: refused
    warm = P.presorted_case(net, D, skew, "sparse_adam", 1000)
    wref = ads.results(warm.oracle())
    wgot = {n: {k: v.copy() for k, v in tabs.items()} for n, tabs in wref.items()}
    for n in wgot:
        for k in ("item.weight", "linear_item.weight"):
            wgot[n][k][P.HOT_ITEM] = warm.before[n][k][P.HOT_ITEM]
    assert ads.raises(warm.criterion(), wgot, wref, warm.before)
