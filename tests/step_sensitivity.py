# -*- coding: utf-8 -*-
"""What an SGD-step parity test can see.  Pure numpy + oracle/: imports without a GPU.

A step test feeds the kernel B triples per step; every triple is one REFERENCE to its user row, to its item rows and to
its metadata rows, and the step moves each of those rows by lr x (the triple's own share of the mean-reduced gradient).
The faults the step kernels risk are narrow — one flagged reference not applied, one lone row not written, one float
atomic dropped — so a test guards the step only if its criterion rejects the oracle's result with ONE such share
missing.  This module computes those shares (lost_reference_effects), builds the faulty results (without_reference, the
no-op variants), and measures a criterion against them (detection_ratio).  tests/test_step_sensitivity_host.py asserts,
for every case of every SGD-step parity test, that the ratio is at least 3.

The tests themselves are split the same way: a StepCase (ids, parameters, lr, B, nb, metadata: no GPU), the GPU run,
and a criterion on numpy tables (got, ref, before) — the GPU test and the host test share the first and the last.
"""
import contextlib

import numpy as np

from conftest import rel_err
from oracle import nets as onets
from oracle import optim as ooptim

TOL = 1e-5                 # the parity tests' norm-wise bar (tests/test_gpu_kernels.py)
MIN_RATIO = 3.0            # 2 from the triangle inequality (a passing result lies within one allowance of ref, so a
#                            fault of more than two leaves it outside), 1 for evaluating the effect at the oracle's tables
LR_PER_TRIPLE = 3.0 / 512  # lr / B at which one reference moves user and item rows by several TOL of max|table|, and
#                            more than half of FM's linear_user references by 3 TOL (measured on the oracle: the host test)
HOT_ROW = 1.0 / 3.0             # ... times this where one row takes thousands of references per step (see step_lr)


@contextlib.contextmanager
def float64_oracle():
    """oracle/ computes in numpy fp32 (its module constant F32); with the constant swapped, the same code runs in
    float64 on float64 tables — the yardstick for how far fp32 rounding alone moves a result."""
    onets.F32 = ooptim.F32 = np.float64
    try:
        yield
    finally:
        onets.F32 = ooptim.F32 = np.float32


def step_lr(B, at_least=0.05, hot=False, D=None):
    """The step size of a case with batches of B: LR_PER_TRIPLE per triple, never below the tests' former step size.
    hot: a row that takes most of a batch of 2048.  The fp32 oracle adds that row's ~3 700 contributions one by one, and at
    the full step size its own rounding reaches the criterion's allowance (its float64 run differs by 0.4 ... 1.0
    allowances); a third of the step keeps the oracle a valid yardstick and every reference above the bar."""
    return max(at_least, LR_PER_TRIPLE * B * (HOT_ROW if hot else 1.0))


NARROW = 4  # widths up to this get their D-wide values moved away from zero


def condition_tables(net, p):
    """What the builders do to the N(0, 0.3) tables of make_case (in place) so that every reference CAN be seen.
    Narrow rows (D <= 4): a reference moves a row by lr / B x g x (the other side's row), and with one to four components
    that row is within rounding of zero for a few triples of every batch — invisible at any step size; the D-wide values
    become |v| + 0.1 (one sign, so sums of rows do not cancel either).  Linear's user row receives the DIFFERENCE of the
    two sides' item (+ metadata) rows, which at D = 1 vanishes whenever two values nearly agree: there every column of the
    item table is a shuffled lattice 0.1 + 0.02 k, the metadata tables a finer one (steps of 0.0025, below 0.02), so two
    sides that differ at all differ by a step.  Such references are still small against max|table|: the narrow widths
    are judged by the per-row criterion as well (criterion_for).  FM: tame_fm."""
    D = p["user.weight"].shape[1]
    if D <= NARROW:
        rs = np.random.RandomState(D)
        for k in sorted(p):
            if not k.startswith(("user.", "item.", "metadata.")):
                continue
            n = p[k].shape[0]
            if net == "linear" and k.startswith("item."):
                p[k] = np.stack([0.1 + 0.02 * rs.permutation(n) for _ in range(D)], axis=1).astype(np.float32)
            elif net == "linear" and k.startswith("metadata."):
                p[k] = np.stack([0.0025 * rs.permutation(n) for _ in range(D)], axis=1).astype(np.float32)
            else:
                p[k] = ((np.abs(p[k]) + np.float32(0.1)) * np.float32(1.0)).astype(np.float32)
    return tame_fm(net, p)


def tame_fm(net, p):
    """FM only: scale the D-wide tables (in place) so that the pairwise term of a score keeps a standard deviation of
    0.5 whatever D and the number of fields.  At the tables' N(0, 0.3) a wide FM saturates its sigmoid (D = 1024: the
    pairwise term alone has sigma 2.9), s (1 - s) of such a triple is ~0 and so is everything it contributes: a reference
    no criterion can see, at any step size.  The ratio of one reference to max|table| does not depend on the scale."""
    if net != "fm":
        return p
    wide = [k for k in p if k.startswith(("user.", "item.", "metadata."))]
    D, F = p["user.weight"].shape[1], len(wide)
    sigma = 0.09 * np.sqrt(D * F * (F - 1) / 2.0)
    f = np.float32(np.sqrt(min(1.0, 0.5 / sigma)))
    for k in wide:
        p[k] *= f
    return p


def batch_of(u, i, j, item_meta=None, sl=slice(None)):
    b = {"user_id": u[sl].astype(np.int64), "pos_item_id": i[sl].astype(np.int64), "neg_item_id": j[sl].astype(np.int64)}
    if item_meta is not None and item_meta.shape[1]:
        b["pos_metadata_id"] = item_meta[i[sl]].astype(np.int64)
        b["neg_metadata_id"] = item_meta[j[sl]].astype(np.int64)
    return b


# ------------------------------------------------------------------------------------------------- the input
class StepCase:
    """The input of one SGD-step parity case and the oracle's run on it.  p: the tables before the first step (fp32);
    batches: one oracle batch dict per step; extra: what only the GPU run needs (ids as arrays, the item -> metadata
    table, where the rows sit in a larger table)."""

    def __init__(self, net, p, batches, lr, tol=TOL, **extra):
        self.net, self.p, self.batches, self.lr, self.tol = net, p, list(batches), lr, tol
        self.B, self.nb = int(self.batches[0]["user_id"].size), len(self.batches)
        self.seed = None
        self.__dict__.update(extra)
        self._runs = {}

    def oracle(self, dtype=np.float32):
        if dtype not in self._runs:
            self._runs[dtype] = oracle_sgd(self.net, self.p, self.batches, self.lr, dtype)
        return self._runs[dtype]

    def oracle_on(self, batches):
        """The fp32 oracle on the same triples in another order within each batch (what a presort that reorders them
        hands to the steps)."""
        return oracle_sgd(self.net, self.p, batches, self.lr)

    @property
    def ref(self):
        return self.oracle().after


def batches_of(u, i, j, B, nb, item_meta=None):
    return [batch_of(u, i, j, item_meta, slice(b * B, (b + 1) * B)) for b in range(nb)]


class OracleRun:
    def __init__(self):
        self.befores, self.losses, self.pos, self.neg, self.after = [], [], [], [], None


def oracle_sgd(net, p, batches, lr, dtype=np.float32):
    """Oracle SGD steps on the batches, in fp32 (oracle/ as it is) or in float64 (float64_oracle)."""
    run = OracleRun()
    cur = {k: v.astype(dtype) for k, v in p.items()}
    with (float64_oracle() if dtype == np.float64 else contextlib.nullcontext()):
        for batch in batches:
            run.befores.append({k: v.copy() for k, v in cur.items()})
            sp, sn, loss, grads = onets.train_forward_backward(net, cur, batch)
            ooptim.sgd_step(cur, grads, lr)
            run.losses.append(float(loss))
            run.pos.append(np.asarray(sp).reshape(-1))
            run.neg.append(np.asarray(sn).reshape(-1))
    run.after = cur
    return run


def assert_losses(case, losses, run=None, tol=TOL):
    """Every step's summed loss (as the kernels report it) against the oracle's mean."""
    run = run or case.oracle()
    for b, want in enumerate(run.losses):
        assert abs(float(losses[b]) / case.B - want) <= tol * max(abs(want), 1e-3), (b, float(losses[b]) / case.B, want)


# ------------------------------------------------------------------------------------------------- the criterion
class ValueCriterion:
    """The parity tests' criterion on the tables after the last step: rel_err(got, ref) < tol per table, i.e. every
    element within tol * max|ref table|; and a table the oracle does not move at all (identically zero gradient:
    Linear's user_bias, which cancels in pos - neg) must come back bit-identical to its initial value.
    __call__(got, ref, before) raises AssertionError; allowance(ref, before) is the distance it tolerates, per row."""

    def __init__(self, tol=TOL):
        self.tol = tol

    @staticmethod
    def unmoved(ref_k, before_k):
        return np.array_equal(np.asarray(ref_k, np.float32).view(np.int32), np.asarray(before_k, np.float32).view(np.int32))

    def allowance(self, ref, before):
        out = {}
        for k, v in ref.items():
            a = 0.0 if self.unmoved(v, before[k]) else self.tol * float(np.abs(v).max())
            out[k] = np.full(v.shape[0], a)
        return out

    def __call__(self, got, ref, before, verbose=True):
        for k, v in ref.items():
            g = np.asarray(got[k])
            if self.unmoved(v, before[k]):
                assert self.unmoved(g, before[k]), \
                    f"{k}: its gradient is identically zero, but the table is not bit-identical to its initial value"
                continue
            e = rel_err(g, v)
            if verbose:
                print(f"{k}: {e:.2e}")
            if not e < self.tol:
                rows = np.abs(g.astype(np.float64) - v).max(axis=1)
                worst = np.argsort(-rows)[:8]
                raise AssertionError(f"{k}: {e:.2e} >= {self.tol:.0e}; rows {worst.tolist()} deviate by "
                                     f"{(rows[worst] / np.abs(v).max()).round(7).tolist()} of max|table|")


def two_sided(net, table, batch):
    """Per triple: both passes name the same row of this 1-wide FM table, so the reference receives the DIFFERENCE of
    two sigmoid slopes, which can be arbitrarily small at any step size — every reference of linear_user, and those of
    linear_metadata.m whose positive and negative item share the category.  (linear_item with pos == neg: exactly 0, no
    reference.)"""
    n = batch["user_id"].size
    if net != "fm":
        return np.zeros(n, bool)
    if table == "linear_user.weight":
        return np.ones(n, bool)
    if table.startswith("linear_metadata."):
        m = int(table.split(".")[1])
        return batch["pos_metadata_id"][:, m] == batch["neg_metadata_id"][:, m]
    return np.zeros(n, bool)


class RowChangeCriterion:
    """Per row, next to the value criterion: max_d |(got - before) - (ref - before)| <= a quarter of the smallest
    single-reference effect on that row over the case's steps (lost_reference_effects; in a table that has both kinds,
    the smallest ONE-sided one: a two-sided reference can vanish, see two_sided, and would put the row's allowance below
    the fp32 noise of summing its seventy-odd other references in any order), floored at 3 x the fp32-vs-float64
    difference of the oracle on that row, and at two fp32 steps of the row's largest value: the row is STORED in fp32, and
    where a 1-wide row's smallest reference is a difference of two sigmoid slopes the oracle's two runs can agree to a
    hundredth of that step by chance (fm, D = 8, linear_metadata: 6e-10 of max|table|), which no fp32 result can be held
    to.  All three numbers come from the oracle and the number format, never from the kernel.  Rows without a reference
    are left to the value criterion."""

    def __init__(self, case):
        r32, r64 = case.oracle(np.float32), case.oracle(np.float64)
        self.allow = {}
        for k, v in r32.after.items():
            self.allow[k] = np.full(v.shape[0], np.inf)
        for step, batch in enumerate(case.batches):
            for k, (rows, trip, eff) in lost_reference_effects(case.net, r32.befores[step], batch, case.lr).items():
                soft = two_sided(case.net, k, batch)[trip]
                if not soft.all():  # (linear_metadata: the one-sided references set the row's allowance; see two_sided)
                    rows, eff = rows[~soft], eff[~soft]
                np.minimum.at(self.allow[k], rows, 0.25 * np.abs(eff).max(axis=1))
        for k, v in r32.after.items():
            floor = 3.0 * np.abs(v.astype(np.float64) - r64.after[k]).max(axis=1)
            floor = np.maximum(floor, 2.0 * np.spacing(np.abs(v).max(axis=1).astype(np.float32)).astype(np.float64))
            self.allow[k] = np.where(np.isfinite(self.allow[k]), np.maximum(self.allow[k], floor), np.inf)

    def allowance(self, ref, before):
        return self.allow

    def __call__(self, got, ref, before, verbose=True):
        for k, v in ref.items():
            b = np.asarray(before[k], np.float64)
            d = np.abs((np.asarray(got[k], np.float64) - b) - (v.astype(np.float64) - b)).max(axis=1)
            with np.errstate(divide="ignore", invalid="ignore"):
                q = np.where(d > 0, d / self.allow[k], 0.0)
            if verbose:
                print(f"{k}: worst row at {q.max():.2f} of its allowance (a quarter of its smallest reference)")
            if (q > 1).any():
                worst = np.argsort(-q)[:8]
                raise AssertionError(f"{k}: rows {worst.tolist()} deviate by {(4 * q[worst]).round(2).tolist()} of their "
                                     f"smallest single-reference effect")


class Both:
    def __init__(self, *criteria):
        self.criteria = criteria

    def allowance(self, ref, before):
        allows = [c.allowance(ref, before) for c in self.criteria]
        return {k: np.minimum.reduce([a[k] for a in allows]) for k in allows[0]}

    def __call__(self, got, ref, before, verbose=True):
        for c in self.criteria:
            c(got, ref, before, verbose)


def criterion_for(case):
    """The value criterion at the case's bar; at the narrow widths (D <= NARROW), where a reference's effect has one to
    four components and a long lower tail against max|table|, and where the case asks for it (per_row: a case that keeps
    its small step size), the per-row criterion as well."""
    value = ValueCriterion(case.tol)
    if case.p["user.weight"].shape[1] > NARROW and not getattr(case, "per_row", False):
        return value
    if getattr(case, "_both", None) is None:
        case._both = Both(value, RowChangeCriterion(case))
    return case._both


def detection_ratio(criterion, ref, before, faulty):
    """The fault's distance divided by the criterion's allowance at the place where the fault lands (the largest such
    quotient over all rows of all tables; inf where nothing is allowed)."""
    allow = criterion.allowance(ref, before)
    best = 0.0
    for k, v in ref.items():
        d = np.abs(np.asarray(faulty[k], np.float64) - v).max(axis=1)
        hit = d > 0
        if hit.any():
            with np.errstate(divide="ignore"):
                best = max(best, float((d[hit] / allow[k][hit]).max()))
    return best


def raises(criterion, got, ref, before):
    try:
        criterion(got, ref, before, verbose=False)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------- the faults
def lost_reference_effects(net, params_before, batch, lr, item_meta=None):
    """{table: (rows[n], triples[n], effect[n, width])}: for every triple t of the batch and every row t touches, lr x
    the triple's own contribution to that row's gradient — the gradient of the single-triple batch divided by B — in
    float64 (float64_oracle).  Both passes of a triple count as ONE reference per row (pos == neg item, or the same
    category on both sides); a contribution that is exactly 0 (an inactive Linear hinge triple) is not a reference.

    Computed in one oracle call: the batch is restated on tables in which no two triples share a row (triple t: user
    row t, item rows 2t and 2t + 1, ...), so every row's gradient there IS its triple's contribution."""
    u, i, j = (np.asarray(batch[k]) for k in ("user_id", "pos_item_id", "neg_item_id"))
    pm, nm = batch.get("pos_metadata_id"), batch.get("neg_metadata_id")
    if pm is None and item_meta is not None and item_meta.shape[1]:
        pm, nm = item_meta[i].astype(np.int64), item_meta[j].astype(np.int64)
    B, t = u.size, np.arange(u.size)
    M = onets._n_meta(params_before, "metadata")

    def two_sided(a, b):
        """compact rows of the pos / neg side (shared where both name the same row), and the reference list"""
        ca, cb = 2 * t, np.where(a == b, 2 * t, 2 * t + 1)
        second = a != b
        return ca, cb, np.concatenate([a, b[second]]), np.concatenate([t, t[second]]), np.concatenate([ca, cb[second]])

    ci, cj, irows, itrip, icomp = two_sided(i, j)
    refs, compact = {}, {}
    for k, v in params_before.items():
        v = np.asarray(v, np.float64)
        if k.startswith(("metadata.", "linear_metadata.")):
            m = int(k.split(".")[1])
            ca, cb, rows, trip, comp = two_sided(pm[:, m], nm[:, m])
            tab = np.zeros((2 * B, v.shape[1]))
            tab[ca], tab[cb] = v[pm[:, m]], v[nm[:, m]]
        elif "user" in k:
            tab, rows, trip, comp = v[u], u, t, t
        else:
            tab = np.zeros((2 * B, v.shape[1]))
            tab[ci], tab[cj] = v[i], v[j]
            rows, trip, comp = irows, itrip, icomp
        compact[k], refs[k] = tab, (rows, trip, comp)
    cbatch = {"user_id": t, "pos_item_id": ci, "neg_item_id": cj}
    if M:
        cbatch["pos_metadata_id"] = np.stack([2 * t] * M, axis=1)
        cbatch["neg_metadata_id"] = np.stack([np.where(pm[:, m] == nm[:, m], 2 * t, 2 * t + 1) for m in range(M)], axis=1)
    with float64_oracle():
        grads = onets.train_forward_backward(net, compact, cbatch)[3]
    out = {}
    for k, (rows, trip, comp) in refs.items():
        eff = lr * grads[k][comp]
        live = (eff != 0).any(axis=1)
        out[k] = (rows[live], trip[live], eff[live])
    return out


def without_reference(ref_after, effects, table, row, triple):
    """The oracle's result with that one contribution not applied (the step subtracts it: it is added back)."""
    rows, trip, eff = effects[table]
    (hit,) = np.nonzero((rows == row) & (trip == triple))
    assert hit.size == 1, (table, row, triple, hit.size)
    out = {k: v.copy() for k, v in ref_after.items()}
    out[table][row] = (out[table][row].astype(np.float64) + eff[hit[0]]).astype(out[table].dtype)
    return out


def reference_ratios(criterion, ref, before, effects):
    """detection_ratio of without_reference for EVERY reference of `effects`, per table, without building the tables:
    the fault lands on one row, its distance is the largest component of the effect."""
    allow = criterion.allowance(ref, before)
    out = {}
    for k, (rows, trip, eff) in effects.items():
        with np.errstate(divide="ignore"):
            out[k] = np.abs(eff).max(axis=1) / allow[k][rows]
    return out


def last_step_not_applied(run):
    return {k: v.astype(np.float32) for k, v in run.befores[-1].items()}


def no_step_applied(run):
    return {k: v.astype(np.float32) for k, v in run.befores[0].items()}


def row_unwritten(run, table, row):
    """ref with one row the last step moves left at its value before that step"""
    out = {k: v.copy() for k, v in run.after.items()}
    out[table][row] = run.befores[-1][table][row]
    return out


def cancelling_table(net, k):
    """FM's 1-wide tables: a row's references carry both signs of a sigmoid slope and may cancel"""
    return net == "fm" and k.startswith("linear_")


def written_rows(run):
    """{table: rows the last step moves}"""
    return {k: np.nonzero((run.after[k] != run.befores[-1][k]).any(axis=1))[0] for k in run.after}


# ------------------------------------------------------------------------------------------------- conditioning
def conditioning(case, criterion):
    """(ok, text).  The input is well-conditioned when (1) the fp32 and the float64 oracle differ by at most a third
    of the criterion's allowance everywhere, and (2) every |hinge argument| of the fp32 oracle exceeds 100 x the
    fp32-vs-float64 difference of the scores (no triple sits on the kink, where two correct implementations may
    decide differently), and (3) every step moves some table (a batch of one whose hinge is inactive, or whose two items
    coincide, makes "the last step not applied" the correct result), and (4) no row's references of the last step cancel
    to less than the allowance (a row that is correctly left as it was; FM's 1-wide tables, where that is common, are
    judged by their share instead: cancelling_table)."""
    r32, r64 = case.oracle(np.float32), case.oracle(np.float64)
    allow = criterion.allowance(r32.after, r32.befores[0])
    worst = 0.0
    for k, v in r32.after.items():
        d = np.abs(v.astype(np.float64) - r64.after[k]).max(axis=1)
        hit = d > 0
        if hit.any():
            with np.errstate(divide="ignore"):
                worst = max(worst, float((d[hit] / allow[k][hit]).max()))
    dscore = max(max(np.abs(a - b).max(), np.abs(c - d).max())
                 for a, b, c, d in zip(r32.pos, r64.pos, r32.neg, r64.neg))
    hmin = min(np.abs(n.astype(np.float64) - p_ + 1.0).min() for p_, n in zip(r32.pos, r32.neg))
    moves = all(any((a[k] != b[k]).any() for k in a) for a, b in zip(r32.befores, r32.befores[1:] + [r32.after]))
    faint = [k for k, rows in written_rows(r32).items() if rows.size and not cancelling_table(case.net, k) and
             (np.abs(r32.after[k][rows].astype(np.float64) - r32.befores[-1][k][rows]).max(axis=1) <= allow[k][rows]).any()]
    ok = worst <= 1.0 / 3.0 and hmin > 100.0 * dscore and moves and not faint
    text = f"fp32 vs float64 oracle {worst:.2e} of the allowance, min |hinge argument| {hmin:.2e}, score difference {dscore:.2e}"
    if not moves:
        text = "a step that moves nothing, " + text
    if faint:
        text = f"a row of {faint} moved by less than the allowance, " + text
    return ok, text


def conditioned(build, criterion=None, tries=8, first=False, bump=None):
    """build(bump) -> StepCase for bump = 0, 1, ...: the first whose input is well-conditioned (the ids' seed moves by
    1000 per bump, as conditioned_adaptive_case of tests/test_gpu_row_shapes.py); prints which one was taken.
    bump given: that seed, taken without running the oracle (a case whose tables make the two extra oracle runs cost more
    than the GPU test itself); case.unverified is set, and tests/test_step_sensitivity_host.py asserts the conditions."""
    if bump is not None:
        case = build(bump)
        case.seed, case.unverified = bump, True
        return case
    for bump in range(tries):
        case = build(bump)
        ok, text = conditioning(case, criterion or criterion_for(case))
        print(f"ids of seed bump {bump}: {text}{'' if ok else ' -> next seed'}")
        if ok or first:  # (first: a given step size, judged as it is — the host test's "before")
            case.seed = bump
            case._runs.pop(np.float64, None)  # (cases are kept and shared: the float64 run is recomputed on demand)
            return case
    raise AssertionError("no seed gives a well-conditioned input")
