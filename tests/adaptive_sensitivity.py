# -*- coding: utf-8 -*-
"""What a parity test of the ADAPTIVE rules (SparseAdam, Adagrad on the presorted step) can see.  Pure numpy + oracle/:
imports without a GPU.  Built on tests/step_sensitivity.py.

Both rules divide by a norm of the row's own gradient history.  From all-zero state the first step is +-lr * sign(g): a
coalesced gradient that cancels to rounding becomes a step of random sign, and no strict criterion can be held against
two correct fp32 evaluations.  With a WARM state — the denominators already hold a history of the gradient's size, which
is where training spends all but its first step — every row is a smooth function of its gradient, and a step test can be
held to the rule of DESIGN.md 2: per row, a quarter of the smallest single reference.

An AdaptiveCase is the input (tables, batches, rule, hyper-parameters, step0, initial state of every table) and the
oracle's runs on it; AdaptiveRowCriterion judges weights and each state tensor of a result; the fault builders make the
results a kernel with one narrow defect would give.  tests/test_adaptive_sensitivity_host.py asserts that the criterion
refuses every one of them, for every case tests/test_gpu_adaptive_parity.py runs.
"""
import contextlib

import numpy as np

import step_sensitivity as sens
from oracle import nets as onets
from oracle import optim as ooptim

# (lr, beta1, beta2, eps, lr_decay): the values of test_presorted_adaptive_rules_match_the_oracle
HYPER = {"sparse_adam": (0.01, 0.9, 0.999, 1e-8, 0.0), "adagrad": (0.05, 0.0, 0.0, 1e-10, 0.02)}
RUN_CHUNK = 64  # csrc/presort.hip: the sorted references of a step are walked in chunks of this many; a run that crosses
#                 a chunk boundary is CUT (its pieces meet in the gradient accumulator, the rule is applied by a third launch)


def linear_tensors(case):
    """The judged tensors on which one reference has a first-order effect: the weights, and SparseAdam's exp_avg.
    exp_avg_sq and Adagrad's sum are quadratic in the gradient — a reference can have almost no effect on them where the
    rest of the row's gradient is small — and are held to the row-level faults only."""
    return tuple(n for n in (("w", "s1") if case.kind == "sparse_adam" else ("w",)) if n in case.judged)


def tensors_of(kind):
    """w: the weights; s1: exp_avg | sum; s2: exp_avg_sq (SparseAdam only)"""
    return ("w", "s1", "s2") if kind == "sparse_adam" else ("w", "s1")


def apply_rule(kind, hyper, t, p, g, rows, s1, s2):
    """One oracle step of the rule on `rows` of one table, in place (oracle/optim.py; t: 1-based step count)."""
    lr, b1, b2, eps, lr_decay = hyper
    if kind == "sparse_adam":
        ooptim.sparse_adam_rows(p, g, rows, s1, s2, t, lr, b1, b2, eps)
    else:
        ooptim.adagrad_rows(p, g, rows, s1, t, lr, lr_decay, eps)


def rule64(case, t, w, g, s1, s2):
    """The rule in float64 on stand-alone rows (w, g, s1, s2: (n, width)) -> {"w", "s1", "s2"} after the step."""
    w, s1, s2 = (np.array(a, np.float64) for a in (w, s1, s2))
    with sens.float64_oracle():
        apply_rule(case.kind, case.hyper, t, w, np.asarray(g, np.float64), np.arange(w.shape[0]), s1, s2)
    return {"w": w, "s1": s1, "s2": s2}


def _copy(d):
    return {k: v.copy() for k, v in d.items()}


# ------------------------------------------------------------------------------------------------- the input
class AdaptiveRun:
    """befores[st]: {"w", "s1", "s2": tables before step st; "g": its coalesced gradients; "rows": its touched rows};
    after: {"w", "s1", "s2"}."""

    def __init__(self):
        self.befores, self.losses, self.pos, self.neg, self.after = [], [], [], [], None


class AdaptiveCase:
    """p: the tables before the first step (fp32, metadata tables included); batches: one oracle batch dict per step;
    kind: "sparse_adam" | "adagrad"; hyper: (lr, b1, b2, eps, lr_decay); step0: the optimiser's step count before the
    first step; s1, s2: the state before the first step, per table (zeros: cold start); extra: what only the GPU run needs."""

    def __init__(self, net, p, batches, kind, step0, hyper=None, **extra):
        self.net, self.p, self.batches, self.kind, self.step0 = net, p, list(batches), kind, int(step0)
        self.hyper = hyper or HYPER[kind]
        self.B, self.nb = int(self.batches[0]["user_id"].size), len(self.batches)
        self.tensors = tensors_of(kind)
        self.judged = self.tensors  # the tensors AdaptiveRowCriterion judges (cold start: the state only)
        self.s1 = {k: np.zeros_like(v) for k, v in p.items()}
        self.s2 = {k: np.zeros_like(v) for k, v in p.items()}
        self.seed = None
        self.__dict__.update(extra)
        self._runs, self._effects, self._crit = {}, None, None

    def set_state(self, s1, s2):
        self.s1, self.s2 = s1, s2
        self._runs, self._effects, self._crit = {}, None, None

    @property
    def before(self):
        return {"w": self.p, "s1": self.s1, "s2": self.s2}

    def oracle(self, dtype=np.float32):
        if dtype not in self._runs:
            self._runs[dtype] = oracle_adaptive(self, dtype)
        return self._runs[dtype]

    def effects(self):
        if self._effects is None:
            self._effects = reference_effects(self)
        return self._effects

    def criterion(self):
        if self._crit is None:
            self._crit = AdaptiveRowCriterion(self)
        return self._crit


def oracle_adaptive(case, dtype=np.float32, fault=None):
    """The oracle's steps from the case's state, in fp32 (oracle/ as it is) or in float64.  fault(st, k, g, t, s1, s2) ->
    (g, t): what a defective step would feed the rule of table k in step st (g is a copy; s1, s2 may be changed in place)."""
    run = AdaptiveRun()
    w = {k: v.astype(dtype) for k, v in case.p.items()}
    s1 = {k: v.astype(dtype) for k, v in case.s1.items()}
    s2 = {k: v.astype(dtype) for k, v in case.s2.items()}
    with (sens.float64_oracle() if dtype == np.float64 else contextlib.nullcontext()):
        for st, batch in enumerate(case.batches):
            sp, sn, loss, grads = onets.train_forward_backward(case.net, w, batch)
            rows = onets.touched_rows(case.net, w, batch)
            run.befores.append({"w": _copy(w), "s1": _copy(s1), "s2": _copy(s2), "g": grads, "rows": rows})
            for k in w:
                g, t = grads[k], case.step0 + st + 1
                if fault is not None:
                    g, t = fault(st, k, g.copy(), t, s1[k], s2[k])
                apply_rule(case.kind, case.hyper, t, w[k], g, rows[k], s1[k], s2[k])
            run.losses.append(float(loss))
            run.pos.append(np.asarray(sp).reshape(-1))
            run.neg.append(np.asarray(sn).reshape(-1))
    run.after = {"w": w, "s1": s1, "s2": s2}
    return run


def assert_losses(case, losses, tol=2 * sens.TOL):
    """Every step's summed loss (as the kernels report it) against the fp32 oracle's mean."""
    for b, want in enumerate(case.oracle().losses):
        got = float(losses[b]) / case.B
        assert abs(got - want) <= tol * max(abs(want), 1e-3), (b, got, want)


def warm_state(case, seed):
    """State as training leaves it, from the oracle's first-batch gradient alone: sigma = the rms of that gradient
    (float64) over the touched rows of each table; SparseAdam: exp_avg = 0.3 sigma N(0, 1), exp_avg_sq = sigma^2
    U(0.5, 2); Adagrad: sum = sigma^2 U(5, 20).  EVERY row gets state, so that "state not read" and "state of another row
    read" differ.  A table whose gradient is identically zero (Linear's user_bias) has sigma = 0 and keeps zero state:
    there the rule moves nothing."""
    with sens.float64_oracle():
        p64 = {k: v.astype(np.float64) for k, v in case.p.items()}
        grads = onets.train_forward_backward(case.net, p64, case.batches[0])[3]
        rows = onets.touched_rows(case.net, p64, case.batches[0])
    s1, s2 = {}, {}
    for n, k in enumerate(sorted(case.p)):
        rs = np.random.RandomState(seed + 7919 * n)
        sigma = float(np.sqrt(np.mean(grads[k][rows[k]] ** 2)))
        shape = case.p[k].shape
        if sigma == 0.0:  # (plain zeros: 0 x N(0, 1) would leave -0.0, which the rule turns into +0.0)
            s1[k], s2[k] = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        elif case.kind == "sparse_adam":
            s1[k] = (0.3 * sigma * rs.normal(0, 1, shape)).astype(np.float32)
            s2[k] = (sigma ** 2 * rs.uniform(0.5, 2.0, shape)).astype(np.float32)
        else:
            s1[k] = (sigma ** 2 * rs.uniform(5.0, 20.0, shape)).astype(np.float32)
            s2[k] = np.zeros(shape, np.float32)
    case.set_state(s1, s2)
    return case


# ------------------------------------------------------------------------------------------------- one reference
def reference_effects(case):
    """Per step: {table: (rows[n], triples[n], two_sided[n], contribution[n, width], {tensor: effect[n, width]})} — for
    every reference, the change of the row's (w, s1, s2) after the step when that reference's contribution (its share of
    the coalesced gradient: lost_reference_effects at lr = 1, at the float64 run's tables) is taken out of the row's
    gradient before the rule.  The rule is evaluated in float64 from the float64 run's state."""
    r64 = case.oracle(np.float64)
    out = []
    for st, batch in enumerate(case.batches):
        b, t = r64.befores[st], case.step0 + st + 1
        per = {}
        for k, (rows, trip, c) in sens.lost_reference_effects(case.net, b["w"], batch, 1.0).items():
            args = (b["w"][k][rows], b["s1"][k][rows], b["s2"][k][rows])
            full = rule64(case, t, args[0], b["g"][k][rows], args[1], args[2])
            less = rule64(case, t, args[0], b["g"][k][rows] - c, args[1], args[2])
            soft = sens.two_sided(case.net, k, batch)[trip]
            per[k] = (rows, trip, soft, c, {n: less[n] - full[n] for n in case.tensors})
        out.append(per)
    return out


def sorted_references(batch, table):
    """The row ids of the step's 2B references of the item table or of one metadata column, as the presort groups them."""
    if table.startswith(("metadata.", "linear_metadata.")):
        m = int(table.split(".")[1])
        both = np.concatenate([batch["pos_metadata_id"][:, m], batch["neg_metadata_id"][:, m]])
    else:
        both = np.concatenate([batch["pos_item_id"], batch["neg_item_id"]])
    return np.sort(both.astype(np.int64))


def runs_of(keys):
    """(rows, starts, ends) of the runs of equal keys in a sorted list"""
    keys = np.asarray(keys)
    starts = np.nonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))[0]
    ends = np.concatenate([starts[1:], [keys.size]])
    return keys[starts], starts, ends


def cut_rows_of(keys):
    """Rows whose run crosses a chunk boundary (they go through the accumulator and cut_rows_apply_kernel), longest first."""
    rows, starts, ends = runs_of(keys)
    cut = starts // RUN_CHUNK != (ends - 1) // RUN_CHUNK
    order = np.argsort(-(ends - starts)[cut], kind="stable")
    return rows[cut][order]


UNIT_ROUNDOFF = 2.0 ** -24
GRADIENT_ROUNDINGS = 4  # of each pass's part of a coalesced gradient: exp, 1 / (1 + e), s (1 - s), x g / B — then the sum


def pass_gradients(net, w, batch):
    """(gradients of the positive pass, of the negative pass): the two parts a row's coalesced gradient is the sum of."""
    u, p, n = batch["user_id"], batch["pos_item_id"], batch["neg_item_id"]
    pm, nm = batch.get("pos_metadata_id"), batch.get("neg_metadata_id")
    fwd, bwd = (onets.linear_forward, onets.linear_backward) if net == "linear" else (onets.fm_forward, onets.fm_backward)
    gp, gn = onets.hinge_grad(fwd(w, u, p, pm), fwd(w, u, n, nm))
    return bwd(w, u, p, pm, gp), bwd(w, u, n, nm, gn)


def gradient_rounding_effects(case, roundings=GRADIENT_ROUNDINGS):
    """{tensor: {table: per row}}: how far fp32 rounding of the coalesced gradient alone moves a row, summed over the
    case's steps.  A row's gradient is the sum of its positive-pass and its negative-pass part, and each part carries
    GRADIENT_ROUNDINGS unit roundoffs of its OWN size whatever order it is summed in; where the parts cancel (FM's 1-wide
    tables: differences of sigmoid slopes) that is far more than a rounding of the gradient, and exp_avg_sq / sum, which
    are quadratic, see it as 2 g dg.  The rule is evaluated in float64 at g +- dg from the float64 run's state.  Two
    correct fp32 evaluations differ by this much: the fp32 oracle on the same triples in another order within each batch
    leaves Adagrad's sum of linear_user 4 fp32 steps from the oracle's own result (test_adaptive_sensitivity_host.py)."""
    r64 = case.oracle(np.float64)
    out = {n: {k: np.zeros(v.shape[0]) for k, v in case.p.items()} for n in case.tensors}
    for st, batch in enumerate(case.batches):
        b, t = r64.befores[st], case.step0 + st + 1
        with sens.float64_oracle():
            parts = pass_gradients(case.net, b["w"], batch)
        for k, rows in b["rows"].items():
            dg = roundings * UNIT_ROUNDOFF * (np.abs(parts[0][k][rows]) + np.abs(parts[1][k][rows]))
            args = (b["w"][k][rows], b["s1"][k][rows], b["s2"][k][rows])
            base = rule64(case, t, args[0], b["g"][k][rows], args[1], args[2])
            for sign in (1.0, -1.0):
                alt = rule64(case, t, args[0], b["g"][k][rows] + sign * dg, args[1], args[2])
                for n in case.tensors:
                    out[n][k][rows] += 0.5 * np.abs(alt[n] - base[n]).max(axis=1)
    return out


# ------------------------------------------------------------------------------------------------- the criterion
class AdaptiveRowCriterion:
    """Over (got, ref32, before), each {"w", "s1", "s2"} -> {table: array}; judged for the weights and for each state
    tensor separately.  Per row, max_d |got - ref32| <= a quarter of the row's smallest ONE-sided single-reference
    effect on that tensor over the case's steps (a table whose references are all two-sided: the smallest of those),
    floored — as RowChangeCriterion — at 3 x the row's fp32-vs-float64 oracle difference and at two fp32 steps of the
    row's largest value, and at what fp32 rounding of the row's coalesced gradient alone does to the tensor
    (gradient_rounding_effects: without it the fp32 oracle on reordered batches is refused).  A row that ids name but no live reference reaches (inactive hinge triples only) is held to the
    floors.  A row no id names, and every row of a table whose gradient is identically zero (Linear's user_bias), must be
    bit-identical to `before`, in weights and in state.  All numbers come from the oracle and the number format."""

    def __init__(self, case, gradient_roundings=None):
        r32, r64 = case.oracle(np.float32), case.oracle(np.float64)
        self.judged = case.judged
        self.raw = {n: {k: np.full(v.shape[0], np.inf) for k, v in case.p.items()} for n in case.tensors}
        for per in case.effects():
            for k, (rows, trip, soft, c, eff) in per.items():
                keep = ~soft if not soft.all() else np.ones(soft.size, bool)
                for n in case.tensors:
                    np.minimum.at(self.raw[n][k], rows[keep], 0.25 * np.abs(eff[n][keep]).max(axis=1))
        named = {k: np.zeros(v.shape[0], bool) for k, v in case.p.items()}
        for b in r64.befores:
            for k, rows in b["rows"].items():
                named[k][rows] = True
        self.named = named
        self.zero_grad = {k for k in case.p if not any(b["g"][k].any() for b in r64.befores)}
        noise = gradient_rounding_effects(case, GRADIENT_ROUNDINGS if gradient_roundings is None else gradient_roundings)
        self.allow = {}
        for n in case.tensors:
            self.allow[n] = {}
            for k, v in r32.after[n].items():
                floor = 3.0 * np.abs(v.astype(np.float64) - r64.after[n][k]).max(axis=1)
                floor = np.maximum(floor, 2.0 * np.spacing(np.abs(v).max(axis=1).astype(np.float32)).astype(np.float64))
                floor = np.maximum(floor, noise[n][k])
                a = np.maximum(np.where(np.isfinite(self.raw[n][k]), self.raw[n][k], 0.0), floor)
                self.allow[n][k] = np.where(named[k] & (k not in self.zero_grad), a, 0.0)

    def allowance(self, ref=None, before=None):
        return self.allow

    def __call__(self, got, ref, before, verbose=True):
        for n in self.judged:
            for k, v in ref[n].items():
                g, a = np.asarray(got[n][k]), self.allow[n][k]
                fixed = a == 0
                same = (g.astype(np.float32).view(np.int32) == np.asarray(before[n][k], np.float32).view(np.int32)).all(axis=1)
                if (fixed & ~same).any():
                    raise AssertionError(f"{n} {k}: rows {np.nonzero(fixed & ~same)[0][:8].tolist()} have no reference "
                                         f"but are not bit-identical to their initial value")
                d = np.abs(g.astype(np.float64) - v.astype(np.float64)).max(axis=1)
                q = np.zeros(d.size)
                np.divide(d, a, out=q, where=~fixed)
                if verbose:
                    print(f"{n} {k}: worst row at {q.max():.2f} of its allowance (a quarter of its smallest reference)")
                if (q > 1).any():
                    worst = np.argsort(-q)[:8]
                    raise AssertionError(f"{n} {k}: rows {worst.tolist()} deviate by {q[worst].round(2).tolist()} allowances "
                                         f"(a quarter of the row's smallest single-reference effect)")


def raises(criterion, got, ref, before):
    try:
        criterion(got, ref, before, verbose=False)
    except AssertionError:
        return True
    return False


def reference_ratios(case, tensor):
    """{table: (ratio[n], two_sided[n], step[n], index[n])}: |effect of losing the reference| / allowance of its row, for
    every reference of every step (detection_ratio of the one-row fault, without building the tables)."""
    allow = case.criterion().allow[tensor]
    out = {}
    for st, per in enumerate(case.effects()):
        for k, (rows, trip, soft, c, eff) in per.items():
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.abs(eff[tensor]).max(axis=1) / allow[k][rows]
            prev = out.get(k, (np.zeros(0), np.zeros(0, bool), np.zeros(0, int), np.zeros(0, int)))
            out[k] = tuple(np.concatenate([a, b]) for a, b in zip(prev, (r, soft, np.full(r.size, st), np.arange(r.size))))
    return out


# ------------------------------------------------------------------------------------------------- conditioning
def conditioning(case):
    """(ok, text).  The input is well-conditioned when (1) on every row with a one-sided reference the fp32 and the
    float64 oracle differ by at most a third of the allowance BEFORE its floors (a quarter of the smallest reference), on
    the weights and the first state — with the floors the statement would hold by construction; (2) every |hinge
    argument| of the fp32 oracle exceeds 100 x the fp32-vs-float64 difference of the scores; (3) every step moves some
    table; (4) of the two-sided references of each case (FM's linear_user; linear_metadata where both items share the
    category) at least half reach MIN_RATIO — the SGD rule's cap, a condition on the input.  (Per case, not per table: a
    row of linear_metadata is allowed a quarter of its smallest ONE-sided reference, and a difference of two sigmoid
    slopes rarely is three times that — as in the SGD step tests that judge per row, that table's share is reported.)"""
    r32, r64, crit = case.oracle(np.float32), case.oracle(np.float64), case.criterion()
    worst = 0.0
    for n in linear_tensors(case):
        for k, v in r32.after[n].items():
            d = np.abs(v.astype(np.float64) - r64.after[n][k]).max(axis=1)
            one_sided = np.zeros(d.size, bool)
            for per in case.effects():
                if k in per and not per[k][2].all():
                    one_sided[per[k][0][~per[k][2]]] = True
            hit = one_sided & (d > 0) & (k not in crit.zero_grad)
            if hit.any():
                worst = max(worst, float((d[hit] / crit.raw[n][k][hit]).max()))
    dscore = max(max(np.abs(a - b).max(), np.abs(c - d).max()) for a, b, c, d in zip(r32.pos, r64.pos, r32.neg, r64.neg))
    hmin = min(np.abs(n_.astype(np.float64) - p_ + 1.0).min() for p_, n_ in zip(r32.pos, r32.neg))
    afters = [b["w"] for b in r32.befores[1:]] + [r32.after["w"]]
    moves = all(any((b["w"][k] != a[k]).any() for k in a) for b, a in zip(r32.befores, afters))
    short = []
    for n in linear_tensors(case):  # per case and tensor: the tables' two-sided references pooled
        tot, good = (sum(v[q] for (n_, k), v in two_sided_shares(case).items() if n_ == n) for q in (0, 1))
        if 2 * good < tot:
            short.append(f"{n} {good}/{tot}")
    ok = worst <= 1.0 / 3.0 and hmin > 100.0 * dscore and moves and not short
    text = (f"fp32 vs float64 oracle {worst:.2e} of a quarter reference, min |hinge argument| {hmin:.2e}, score "
            f"difference {dscore:.2e}")
    if not moves:
        text = "a step that moves nothing, " + text
    if short:
        text = f"two-sided references below half: {short}, " + text
    return ok, text


def two_sided_shares(case):
    """{(tensor, table): (number of two-sided references, of which reach MIN_RATIO)} on weights and first state"""
    out = {}
    for n in linear_tensors(case):
        for k, (r, soft, _, _) in reference_ratios(case, n).items():
            if soft.any():
                out[(n, k)] = (int(soft.sum()), int((r[soft] >= sens.MIN_RATIO).sum()))
    return out


def conditioned(build, tries=8):
    """build(bump) -> AdaptiveCase for bump = 0, 1, ...: the first whose input is well-conditioned (the ids' seed moves by
    1000 per bump, as step_sensitivity.conditioned); prints which one was taken."""
    for bump in range(tries):
        case = build(bump)
        ok, text = conditioning(case)
        print(f"ids of seed bump {bump}: {text}{'' if ok else ' -> next seed'}")
        if ok:
            case.seed = bump
            return case
    raise AssertionError("no seed gives a well-conditioned input")


# ------------------------------------------------------------------------------------------------- the faults
def reordered(case, seed):
    """The fp32 oracle's result on the same triples in another order within each batch: a second correct fp32 evaluation
    (the presort hands the kernels the references in yet another one)."""
    import copy
    rs, other = np.random.RandomState(seed), copy.copy(case)
    other.batches = []
    for b in case.batches:
        order = rs.permutation(case.B)
        other.batches.append({k: v[order] for k, v in b.items()})
    return results(oracle_adaptive(other))


def results(run):
    """a run's result as fp32 tables, the form a GPU run is downloaded in"""
    return {n: {k: v.astype(np.float32) for k, v in tabs.items()} for n, tabs in run.after.items()}


def faulty_run(case, fault):
    return results(oracle_adaptive(case, np.float32, fault))


def without_reference(case, st, table, index):
    """One reference lost: reference `index` of reference_effects(case)[st][table] does not reach its row's gradient."""
    rows, trip, soft, c, eff = case.effects()[st][table]

    def fault(s, k, g, t, s1, s2):
        if s == st and k == table:
            g[rows[index]] -= c[index].astype(g.dtype)
        return g, t
    return faulty_run(case, fault)


def piece_of(case, st, table, row, n=RUN_CHUNK):
    """indices (into reference_effects(case)[st][table]) of n consecutive references of the row, from the middle of its
    run; fewer where the run is shorter (then all but its first)"""
    rows = case.effects()[st][table][0]
    (mine,) = np.nonzero(rows == row)
    n = min(n, mine.size - 1)
    assert n > 0, (table, row, mine.size)
    first = (mine.size - n + 1) // 2
    return mine[first:first + n]


def without_piece(case, st, table, row):
    """One whole piece of a cut run lost: 64 consecutive references of the row are missing from its gradient."""
    c = case.effects()[st][table][3]
    lost = c[piece_of(case, st, table, row)].sum(axis=0)

    def fault(s, k, g, t, s1, s2):
        if s == st and k == table:
            g[row] -= lost.astype(g.dtype)
        return g, t
    return faulty_run(case, fault)


def row_unwritten(case, table, row):
    """A cut row not written by the last step: weights, s1 and s2 keep their values before it."""
    run = case.oracle()
    out = results(run)
    for n in out:
        out[n][table][row] = run.befores[-1][n][table][row]
    return out


def state_read_as_zero(case, st, table, row):
    """The rule of that row applied from zero state in step st (a state pointer, or a row offset, gone wrong)."""
    def fault(s, k, g, t, s1, s2):
        if s == st and k == table:
            s1[row], s2[row] = 0, 0
        return g, t
    return faulty_run(case, fault)


def step_counter_off_by_one(case):
    """t = step0 + st instead of step0 + st + 1, in every step and table."""
    return faulty_run(case, lambda s, k, g, t, s1, s2: (g, t - 1))


def last_step_not_applied(case):
    b = case.oracle().befores[-1]
    return {n: {k: v.astype(np.float32) for k, v in b[n].items()} for n in case.tensors}


def accumulator_left_dirty(case, st, table, row):
    """gacc not cleared: the row's coalesced gradient of step st is added once more in step st + 1."""
    stale = case.oracle().befores[st]["g"][table][row].copy()

    def fault(s, k, g, t, s1, s2):
        if s == st + 1 and k == table:
            g[row] += stale
        return g, t
    return faulty_run(case, fault)


# ------------------------------------------------------------------------------------------------- the "before"
def bulk_criterion_accepts(got, ref, need=0.97, tol=1e-3):
    """The criterion of test_presorted_adaptive_rules_match_the_oracle (skewed cases): per table and tensor, `need` of the
    rows within tol * max|ref|, and rel_err(weights) < 0.05."""
    from conftest import rel_err
    for n in got:
        for k, v in ref[n].items():
            share = float((np.abs(got[n][k] - v).max(axis=1) <= tol * np.abs(v).max()).mean())
            if share < need:
                return False
            if n == "w" and not rel_err(got[n][k], v) < 0.05:
                return False
    return True
