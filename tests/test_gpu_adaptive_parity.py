# -*- coding: utf-8 -*-
"""SparseAdam / Adagrad on the presorted step, judged per row with no exempt rows.  GPU only.

The kernel-level adaptive tests of test_gpu_kernels.py start at step0 = 0 with all-zero state and allow a share of the
rows to deviate (the cold start turns a gradient that cancels to rounding into a step of random sign).  Here the state is
WARM (adaptive_sensitivity.warm_state) and step0 > 0, which is what the engine hands the kernel for all of training but
its first step: the rules are then smooth in the gradient, and weights, exp_avg | sum and exp_avg_sq of EVERY row are
held to a quarter of the row's smallest single reference (adaptive_sensitivity.AdaptiveRowCriterion).  Each cell is a
case (`*_case()`: no GPU), the GPU run and the criterion; tests/test_adaptive_sensitivity_host.py asserts without a GPU
that the criterion refuses one lost reference, one lost piece of a cut run, an unwritten cut row, state read as zero, a
step counter off by one, a missing last step and a dirty accumulator, for every case below.  DESIGN.md 2."""
import functools

import numpy as np
import pytest
import torch

import adaptive_sensitivity as ads
import step_sensitivity as sens
from test_gpu_kernels import make_case, tables_to_host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NU, NI = 300, 57
HOT_ITEM = 7

KINDS = ["sparse_adam", "adagrad"]
PRESORTED = [("fm", 64, True), ("linear", 32, True), ("fm", 10, True), ("fm", 64, False)]
STEP0 = [1000, 3]
PRESORTED_META = [("fm", 64, 1, False, True), ("linear", 64, 1, True, False), ("fm", 32, 3, True, False)]  # net, D, M, skew, hot
EDGES = [("fm", 64, 256), ("linear", 32, 256), ("fm", 64, 250), ("linear", 32, 250)]
COLD = [("fm", 64), ("linear", 32)]


def _ops():
    from torchrecsys_amd import ops
    return ops


def _lin(net):
    return ("user_bias.weight", "item_bias.weight") if net == "linear" else ("linear_user.weight", "linear_item.weight")


# ------------------------------------------------------------------------------------------------- the cases (no GPU)
def _ids(rs, n, skew):
    u, i, j = rs.randint(0, NU, n), rs.randint(0, NI, n), rs.randint(0, NI, n)
    if skew:
        i[rs.rand(n) < 0.4] = HOT_ITEM
        j[rs.rand(n) < 0.4] = HOT_ITEM
    return u, i, j


@functools.lru_cache(maxsize=None)
def presorted_case(net, D, skew, kind, step0):
    """4 batches of 512 on 300 users and 57 items (the input of test_presorted_adaptive_rules_match_the_oracle; one hot
    item with 40 % of the references under skew), warm state, step0 optimiser steps behind it."""
    def build(bump):
        B, nb = 512, 4
        u, i, j = _ids(np.random.RandomState(D + skew + 1000 * bump), nb * B, skew)
        p, _, _ = make_case(net, D, 0, 8, NU=NU, NI=NI, seed=2)
        case = ads.AdaptiveCase(net, sens.condition_tables(net, p), sens.batches_of(u, i, j, B, nb), kind, step0,
                                D=D, M=0, u=u, i=i, j=j, item_meta=None, sizes=[])
        return ads.warm_state(case, seed=D + 10 * step0)
    return ads.conditioned(build)


@functools.lru_cache(maxsize=None)
def presorted_metadata_case(net, D, M, skew, hot, kind):
    """4 batches of 512 with M sorted metadata columns; hot: batches of 2048 and 90 % of the items in category 0 of the
    first column — its run is ~3 700 of the step's 4096 references, cut into 58 pieces.  Warm state, step0 = 1000."""
    def build(bump):
        B, nb = (2048 if hot else 512), 4
        rs = np.random.RandomState(D + M + skew + 1000 * bump)
        p, _, _ = make_case(net, D, M, 8, NU=NU, NI=NI, seed=2)
        sizes = [p[f"metadata.{m}.weight"].shape[0] for m in range(M)]
        item_meta = np.stack([rs.randint(0, sizes[m], NI) for m in range(M)], axis=1).astype(np.int32)
        if hot:
            item_meta[rs.rand(NI) < 0.9, 0] = 0
        u, i, j = _ids(rs, nb * B, skew)
        case = ads.AdaptiveCase(net, sens.condition_tables(net, p), sens.batches_of(u, i, j, B, nb, item_meta), kind, 1000,
                                D=D, M=M, u=u, i=i, j=j, item_meta=item_meta, sizes=sizes)
        return ads.warm_state(case, seed=D + M)
    return ads.conditioned(build)


def edge_item_counts(rs, n_refs, step):
    """References per item row (ascending row = the order of the sorted list) such that the list holds, from its start:
    runs of 1, 2, 3, 4 and 5; a run that ends exactly at reference 64 with the next row starting the chunk; a run of 63;
    a run whose head is slot 63 of its chunk (reference 127); a run of >= 150 that holds at least one whole chunk; and,
    where n_refs is no multiple of 64, a last run that starts in the last full chunk and ends with the batch."""
    head = [1, 2, 3, 4, 5, 49, 63, 11, 150 + 43 * step]
    tail = [n_refs % ads.RUN_CHUNK + 8] if n_refs % ads.RUN_CHUNK else []
    free = NI - len(head) - len(tail)
    rest = n_refs - sum(head) - sum(tail)
    mid = 1 + rs.multinomial(rest - free, np.ones(free) / free)
    return np.concatenate([head, mid, tail]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def run_shape_edges_case(net, D, B, kind):
    """2 batches of B = 256 (512 references = 8 chunks of 64) or 250 (a partial last chunk) whose item ids are dealt from
    edge_item_counts.  Warm state, step0 = 1000."""
    def build(bump):
        nb = 2
        rs = np.random.RandomState(D + B + 1000 * bump)
        u = rs.randint(0, NU, nb * B)
        i, j = np.zeros(nb * B, np.int64), np.zeros(nb * B, np.int64)
        for st in range(nb):
            refs = rs.permutation(np.repeat(np.arange(NI), edge_item_counts(rs, 2 * B, st)))
            i[st * B:(st + 1) * B], j[st * B:(st + 1) * B] = refs[:B], refs[B:]
        p, _, _ = make_case(net, D, 0, 8, NU=NU, NI=NI, seed=2)
        case = ads.AdaptiveCase(net, sens.condition_tables(net, p), sens.batches_of(u, i, j, B, nb), kind, 1000,
                                D=D, M=0, u=u, i=i, j=j, item_meta=None, sizes=[])
        return ads.warm_state(case, seed=D + B)
    return ads.conditioned(build)


@functools.lru_cache(maxsize=None)
def cold_start_case(net, D, kind):
    """ONE batch of 512 (skewed) from step0 = 0 and all-zero state.  The state after the step is judged by the
    criterion (exp_avg is linear in the gradient; exp_avg_sq and sum get the same allowance), the weights against the
    rule evaluated from the state the kernel stored (check_cold_weights)."""
    def build(bump):
        B, nb = 512, 1
        u, i, j = _ids(np.random.RandomState(D + 1 + 1000 * bump), nb * B, True)
        p, _, _ = make_case(net, D, 0, 8, NU=NU, NI=NI, seed=2)
        case = ads.AdaptiveCase(net, sens.condition_tables(net, p), sens.batches_of(u, i, j, B, nb), kind, 0,
                                D=D, M=0, u=u, i=i, j=j, item_meta=None, sizes=[])
        case.judged = case.tensors[1:]
        return case
    return ads.conditioned(build)


def all_cases():
    """[(builder, args)] of every case a test below runs — what the host test walks."""
    out = []
    for kind in KINDS:
        for a in PRESORTED:
            for step0 in STEP0:
                out.append((presorted_case, a + (kind, step0)))
        for a in PRESORTED_META:
            out.append((presorted_metadata_case, a + (kind,)))
        for a in EDGES:
            out.append((run_shape_edges_case, a + (kind,)))
        for a in COLD:
            out.append((cold_start_case, a + (kind,)))
    return out


# ------------------------------------------------------------------------------------------------- the GPU run
def run_on_gpu(case, steps_per_call=None):
    """The case's steps through trs_train_steps_sgd with a trs_opt whose state and step0 come from the case; in one C
    call, or in calls of steps_per_call steps (consecutive first_stamp, step0 advanced by the caller, same buffers).
    -> (got {"w", "s1", "s2"}, losses, sorted item keys per step, cut rows listed by the last step per table)."""
    from torchrecsys_amd import _lib
    ops = _ops()
    net, D, M, B, nb, sizes = case.net, case.D, case.M, case.B, case.nb, case.sizes
    lin = _lin(net)
    names = ["user.weight", "item.weight", lin[0], lin[1]]
    dev = lambda d: {k: torch.from_numpy(v.copy()).to(DEV) for k, v in d.items()}  # noqa: E731
    t, s1, s2 = dev(case.p), dev(case.s1), dev(case.s2)
    metas = [t[f"metadata.{m}.weight"] for m in range(M)]
    meta_lins = [t[f"linear_metadata.{m}.weight"] for m in range(M)] if net == "fm" else []
    T, keep = ops.make_tables(t["user.weight"], t["item.weight"], t[lin[0]], t[lin[1]], metas, meta_lins)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    tab = torch.from_numpy(case.item_meta).to(DEV) if M else None
    ps = ops.EpochPresort(nb, B, NU, NI, DEV, **(dict(item_meta=tab, n_meta=sizes) if M else {}))
    ps.run(None, None, 0, 0, 0, err, given_ids=[torch.from_numpy(a.astype(np.int32)).to(DEV) for a in (case.u, case.i, case.j)])
    assert ps.key_bytes == 4
    gz, du = torch.empty((2, B), device=DEV), torch.empty((B, D), device=DEV)
    ustage = torch.empty((B, D), device=DEV)
    xstage = torch.empty((2 if net == "fm" else 1, B, D), device=DEV)
    gacc = {k: torch.zeros_like(v) for k, v in t.items()}
    cap = 2 * B // 64 + 64
    cut_rows = torch.full((1 + M, cap), -1, dtype=torch.int32, device=DEV)
    cut_count = torch.zeros((1 + M, 2), dtype=torch.int32, device=DEV)
    lin_state = [torch.zeros((3, sizes[m]), device=DEV) for m in range(M)]  # Linear: no 1-wide metadata tables
    lin_scratch = torch.zeros(max(sizes), device=DEV) if M else None
    o = _lib.TrsOpt()
    lr, b1, b2, eps, lr_decay = case.hyper
    o.kind, o.lr, o.beta1, o.beta2, o.eps, o.lr_decay = (1 if case.kind == "sparse_adam" else 2), lr, b1, b2, eps, lr_decay
    o.user_s1, o.item_s1, o.user_lin_s1, o.item_lin_s1 = (ops.ptr(s1[k]) for k in names)
    if case.kind == "sparse_adam" or M:
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
    scratch = ops.train_scratch(NU, NI, B, D, DEV)
    per_call = steps_per_call or nb
    for b in range(0, nb, per_call):
        n = min(per_call, nb - b)
        ids, sk, sv, udup, usorted, idup = ps.step_args(b)
        ms = None
        if M:
            ms = _lib.TrsMetaStage()
            ms.item_meta_tab, ms.xstage, ms.lin_scratch = ops.ptr(tab), ops.ptr(xstage), ops.ptr(lin_scratch)
            for m, (k_, v_) in enumerate(ps.meta_step_args(b)):
                ms.sorted_keys[m], ms.sorted_vals[m] = k_, v_
            pm, nm = ps.meta_id_args(b)
            ms.pos_meta_ids, ms.neg_meta_ids = ops.ptr(pm), ops.ptr(nm)
        o.step0 = case.step0 + b
        ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, n, lr, *ids, gz, du, losses[b:], err, scratch, 1 + b, None,
                            sk, sv, ps.key_bytes, udup, ustage, usorted, o, ms)
    torch.cuda.synchronize()
    assert err.item() == 0
    for k, v in gacc.items():  # every accumulator left clean
        assert float(v.abs().max()) == 0.0, k
    for m in range(M):
        assert float(lin_state[m][2].abs().max()) == 0.0, m
    got = {"w": tables_to_host(t), "s1": tables_to_host(s1), "s2": tables_to_host(s2)}
    first = (ps.sorted_keys - ps.keys.data_ptr()) // 4
    keys = ps.keys.view(torch.uint32)[first:first + 2 * B * nb].cpu().numpy().astype(np.int64).reshape(nb, 2 * B)
    parity = (1 + nb - 1) & 1  # the steps alternate between the two counters by their stamp; the last step's list
    counts = cut_count.cpu().numpy()[:, parity]
    listed = [np.sort(cut_rows[q, :counts[q]].cpu().numpy()) for q in range(1 + M)]
    return got, losses.cpu().numpy(), keys, listed


def check(case, steps_per_call=None):
    """The asserts of every cell: losses, the criterion on weights and state of every table (rows no id names:
    bit-identical — part of the criterion), and the cut rows of the last step against the sorted layout."""
    got, losses, keys, listed = run_on_gpu(case, steps_per_call)
    ads.assert_losses(case, losses)
    for st, batch in enumerate(case.batches):
        assert np.array_equal(keys[st], ads.sorted_references(batch, "item.weight")), st
    tables = ["item.weight"] + [f"metadata.{m}.weight" for m in range(case.M)]
    for q, k in enumerate(tables):
        want = np.sort(ads.cut_rows_of(ads.sorted_references(case.batches[-1], k)))
        assert np.array_equal(listed[q], want), (k, listed[q], want)
    ref = ads.results(case.oracle())
    case.criterion()(got, ref, case.before)
    return got, keys


# ------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("step0", STEP0)
@pytest.mark.parametrize("net,D,skew", PRESORTED)
@pytest.mark.parametrize("kind", KINDS)
def test_presorted_adaptive_step_from_warm_state(net, D, skew, kind, step0):
    """(a) 4 steps in one C call: users referenced once by K1, duplicated users and item rows by their sorted runs, the
    hot item's run of ~400 through the accumulator and cut_rows_apply_kernel; ragged width at D = 10."""
    check(presorted_case(net, D, skew, kind, step0))


@pytest.mark.parametrize("net,D,M,skew,hot", PRESORTED_META)
@pytest.mark.parametrize("kind", KINDS)
def test_presorted_adaptive_step_with_metadata_from_warm_state(net, D, M, skew, hot, kind):
    """(b) sorted metadata columns, each table with its own state, accumulator and cut list."""
    check(presorted_metadata_case(net, D, M, skew, hot, kind))


def assert_run_shapes(keys, partial):
    """The sorted layout of one step really has the shapes of edge_item_counts."""
    C = ads.RUN_CHUNK
    rows, starts, ends = ads.runs_of(keys)
    lens, n = ends - starts, keys.size
    whole = starts // C == (ends - 1) // C  # the run lies in one chunk: not cut
    for want in (1, 2, 3, 4, 5):
        assert (whole & (lens == want)).any(), want
    # ends exactly at a chunk boundary, the next row starts the next chunk: NOT a cut run
    assert (whole & (ends % C == 0) & (ends < n) & (lens > 1)).any()
    # head in the last slot of a chunk: a head piece of length 1
    assert ((starts % C == C - 1) & (lens > 1)).any()
    # a piece that is neither head nor tail: a whole chunk strictly inside the run
    first_inner = (starts + C - 1) // C * C
    assert ((lens >= 2 * C + 1) & (starts % C != 0) & (first_inner + C < ends)).any()
    if partial:  # the last run starts in the last full chunk and ends with the batch, in a partial chunk
        assert n % C != 0 and ends[-1] == n and starts[-1] < n // C * C


@pytest.mark.parametrize("net,D,B", EDGES)
@pytest.mark.parametrize("kind", KINDS)
def test_run_shape_edges_of_the_sorted_item_update(net, D, B, kind):
    """(c) runs of 1 ... 5 (SI_MEMB = 3 and the first turn of the TU loop), a run that ends at a chunk boundary, a head
    in the last slot of a chunk, a run with whole middle chunks, a run that ends the batch in a partial chunk (B = 250).
    The layout is read back from the presort's sorted keys and asserted before the result is judged; check() compares the
    cut rows the step listed with the rows cut in that layout."""
    case = run_shape_edges_case(net, D, B, kind)
    got, keys = check(case)
    for st in range(case.nb):
        assert_run_shapes(keys[st], partial=(2 * B) % ads.RUN_CHUNK != 0)


@pytest.mark.parametrize("kind", KINDS)
def test_four_calls_of_one_step_equal_one_call_of_four(kind):
    """(d) the engine issues the steps in calls of varying length: the parity of the cut counters (first_stamp) and
    step0 carry across calls.  Same criterion, same oracle run."""
    check(presorted_case("fm", 64, True, kind, 1000), steps_per_call=1)


def check_cold_weights(case, got):
    """Cold start, one step: the weights against the rule evaluated from the state the kernel itself stored — a pure
    function of stored fp32 numbers, so every row counts however its gradient cancelled.  SparseAdam from zero state:
    numer = exp_avg, denom = sqrt(exp_avg_sq) + eps.  Adagrad: |g| = sqrt(sum), so |dw| = clr sqrt(sum) / (sqrt(sum) +
    eps); its sign from the float64 gradient wherever |g| exceeds 100 x its own fp32-vs-float64 difference.  Allowance:
    3 x the distance between the fp32 oracle rule and float64 on the same stored values, at least two fp32 steps of w
    (see below for whose size)."""
    lr, b1, b2, eps, lr_decay = case.hyper
    r32, r64 = case.oracle(np.float32), case.oracle(np.float64)
    for k, w0 in case.p.items():
        rows = r32.befores[0]["rows"][k]
        dw = got["w"][k].astype(np.float64) - w0
        m = got["s1"][k]
        if case.kind == "sparse_adam":
            v = got["s2"][k]
            step = lr * np.sqrt(1 - b2) / (1 - b1)
            want = -step * m.astype(np.float64) / (np.sqrt(v.astype(np.float64)) + eps)
            want32 = (-np.float32(step) * (m / (np.sqrt(v, dtype=np.float32) + np.float32(eps)))).astype(np.float64)
        else:
            root = np.sqrt(m.astype(np.float64))
            want = lr * root / (root + eps)
            root32 = np.sqrt(m, dtype=np.float32)
            want32 = (np.float32(lr) * (root32 / (root32 + np.float32(eps)))).astype(np.float64)
            g32, g64 = r32.befores[0]["g"][k], r64.befores[0]["g"][k]
            sure = np.abs(g64) > 100.0 * np.abs(g32 - g64)
            assert (np.sign(dw[sure]) == -np.sign(g64[sure])).all(), k
            dw = np.abs(dw)
        # The step is rounded at its OWN size before it is added (sqrt, quotient, product: half a step each; Adagrad one
        # more, |g| = sqrt(sum) to half a step), the sum at the size of the result: two (Adagrad: three) fp32 steps of
        # the largest of the row before, the row after and the step — where a weight changes sign that is the step.
        w64 = w0.astype(np.float64)
        after = np.abs(w64 + want) if case.kind == "sparse_adam" else np.minimum(np.abs(w64 + want), np.abs(w64 - want))
        size = np.maximum(np.maximum(np.abs(w64), after), np.abs(want)).astype(np.float32)
        steps = 2.0 if case.kind == "sparse_adam" else 3.0
        allow = np.maximum(3.0 * np.abs(want32 - want), steps * np.spacing(size).astype(np.float64))
        q = np.abs(dw - want)[rows] / allow[rows]
        print(f"w {k}: worst element at {q.max():.2f} of its allowance")
        assert (q <= 1).all(), (k, rows[np.nonzero((q > 1).any(axis=1))[0][:8]].tolist())
        rest = np.setdiff1d(np.arange(w0.shape[0]), rows)
        assert np.array_equal(got["w"][k][rest].view(np.int32), w0[rest].view(np.int32)), k


@pytest.mark.parametrize("net,D", COLD)
@pytest.mark.parametrize("kind", KINDS)
def test_cold_start_one_step_every_row(net, D, kind):
    """(e) step0 = 0, zero state: no row is left out in either rule."""
    case = cold_start_case(net, D, kind)
    got, keys = check(case)
    check_cold_weights(case, got)
