# -*- coding: utf-8 -*-
"""The one tail of every per-step loss (engine.SparseScorerTrainer._apply_staged) and the one layout of the staging
buffers (engine.staged_layout): the layout on the host against the three enumerations the step methods used to write
out, and on the MI355X the launch sequence of each step method under plain SGD with one learning rate."""
import numpy as np
import pytest
import torch

SLOTS, COLUMNS = (1, 2, 4, 9), (0, 1, 3)


# ------------------------------------------------------------------------------------------------ 1. the layout (host)
def pair_fields(M):
    """step() / warp_step(): S = 2, fields 0 | 1:3 | 3+2m : 5+2m"""
    return slice(0, 1), slice(1, 3), [slice(3 + 2 * m, 5 + 2 * m) for m in range(M)]


def softmax_fields(M):
    """softmax_step(): S = 1, fields 0 | 1 | 2+m"""
    return slice(0, 1), slice(1, 2), [slice(2 + m, 3 + m) for m in range(M)]


def multineg_fields(K, M):
    """multineg_step(): S = 1 + K, fields 0 | 1:1+S | 1+S+mS : 1+S+(m+1)S"""
    S = 1 + K
    return slice(0, 1), slice(1, 1 + S), [slice(1 + S + m * S, 1 + S + (m + 1) * S) for m in range(M)]


def enumerated(S, M, has_meta_lin):
    """The table order every one of those tails walked: user, item, their 1-wide tables, then per column the metadata
    table and (FM) its 1-wide table at table_params()[4 + M + m]."""
    user, item, cols = {1: softmax_fields(M), 2: pair_fields(M)}.get(S) or multineg_fields(S - 1, M)
    want = [(0, "user", user, True), (1, "item", item, True), (2, "user", user, False), (3, "item", item, False)]
    for m in range(M):
        want.append((4 + m, m, cols[m], True))
        if has_meta_lin:
            want.append((4 + M + m, m, cols[m], False))
    return want


@pytest.mark.parametrize("has_meta_lin", [False, True])
@pytest.mark.parametrize("M", COLUMNS)
@pytest.mark.parametrize("S", SLOTS)
def test_layout_is_the_three_enumerations(S, M, has_meta_lin):
    from torchrecsys_amd.engine import staged_layout
    got = staged_layout(S, M, has_meta_lin)
    assert got == enumerated(S, M, has_meta_lin)
    F = 1 + S * (1 + M)
    wide = [f for _, _, fields, w in got if w for f in range(fields.start, fields.stop)]
    assert wide == list(range(F))  # the wide tables' slices tile 0 .. F - 1 exactly once, in order
    narrow = [f for _, _, fields, w in got if not w for f in range(fields.start, fields.stop)]
    assert narrow == list(range(F if has_meta_lin else 1 + S))  # 1-wide: the same tiling, or user + item slots alone
    tables = [t for t, _, _, _ in got]
    assert sorted(tables) == list(range(4 + (2 if has_meta_lin else 1) * M))  # every table once, none past the last
    if not has_meta_lin:
        assert all(w or t in (2, 3) for t, _, _, w in got)  # no 1-wide metadata table


def test_layout_written_out():
    from torchrecsys_amd.engine import staged_layout
    assert staged_layout(2, 1, True) == [
        (0, "user", slice(0, 1), True), (1, "item", slice(1, 3), True), (2, "user", slice(0, 1), False),
        (3, "item", slice(1, 3), False), (4, 0, slice(3, 5), True), (5, 0, slice(3, 5), False)]
    assert staged_layout(1, 3, False) == [
        (0, "user", slice(0, 1), True), (1, "item", slice(1, 2), True), (2, "user", slice(0, 1), False),
        (3, "item", slice(1, 2), False), (4, 0, slice(2, 3), True), (5, 1, slice(3, 4), True),
        (6, 2, slice(4, 5), True)]
    assert staged_layout(4, 3, True) == [
        (0, "user", slice(0, 1), True), (1, "item", slice(1, 5), True), (2, "user", slice(0, 1), False),
        (3, "item", slice(1, 5), False), (4, 0, slice(5, 9), True), (7, 0, slice(5, 9), False),
        (5, 1, slice(9, 13), True), (8, 1, slice(9, 13), False), (6, 2, slice(13, 17), True),
        (9, 2, slice(13, 17), False)]
    assert staged_layout(9, 0, True) == staged_layout(9, 0, False) == [
        (0, "user", slice(0, 1), True), (1, "item", slice(1, 10), True), (2, "user", slice(0, 1), False),
        (3, "item", slice(1, 10), False)]


# ------------------------------------------------------------------------------------------------ 2. launches (GPU)
NU, NI, D, B, K, M, CAP, LR = 300, 200, 20, 37, 3, 2, 64, 0.25
FUSED = [("score_sgd_update",)]
# rows_scatter_add calls of the tail, (table_params() index, 'u' = B user entries | 's' = S * B slot entries, width):
# user, item, their 1-wide tables, then per column the metadata table and (FM) its 1-wide table
SCATTERS = {"fm": [(0, "u", D), (1, "s", D), (2, "u", 1), (3, "s", 1), (4, "s", D), (6, "s", 1), (5, "s", D),
                   (7, "s", 1)],
            "linear": [(0, "u", D), (1, "s", D), (2, "u", 1), (3, "s", 1), (4, "s", D), (5, "s", D)]}


def scatters(net_type, S, skip_user_lin=False):
    return [("rows_scatter_add", t, B if n == "u" else S * B, ld, -LR) for t, n, ld in SCATTERS[net_type]
            if not (skip_user_lin and t == 2)]


def launches_of_one_step(path, net_type, l2, monkeypatch):
    """The calls of the row-update launchers (and of the L2 launch) one step of `path` makes under SGD, one lr."""
    import test_gpu_l2 as t
    from torchrecsys_amd import ops
    from torchrecsys_amd.engine import SparseScorerTrainer
    net, item_meta = t.build_net(net_type, M, NU, NI, D, 5)
    tr = SparseScorerTrainer(net, torch.optim.SGD(net.parameters(), lr=LR), CAP)
    assert tr.kind == "sgd"
    tr.l2 = l2
    tr.kernel_events = {}
    table_no = {p.data_ptr(): i for i, p in enumerate(net.table_params())}
    calls = []

    def spy(name, describe=lambda *a, **kw: ()):
        orig = getattr(ops, name)

        def wrapped(*a, **kw):
            calls.append((name, *describe(*a, **kw)))
            return orig(*a, **kw)
        monkeypatch.setattr(ops, name, wrapped)

    spy("rows_scatter_add", lambda table, idx, vals, alpha, ld=None, err_flag=None: (
        table_no.get(table.data_ptr()), idx.numel(), ld, alpha))
    for name in ("rows_apply_sparse_adam", "rows_apply_adagrad", "score_sgd_update", "stage_add_l2"):
        spy(name)
    rs = np.random.RandomState(8)
    loss = torch.zeros(1, device=t.DEV)
    if path == "step":
        user, items = t.forced_rows(rs, NU, NI, B, 2)
        tr.step(t.pair_ids(user, items, item_meta), loss)
    elif path == "softmax":
        user, items = t.forced_rows(rs, NU, NI, B, 1)
        ids = t.pair_ids(user, np.concatenate([items, items]), item_meta)
        tr.softmax = (0.5, None)
        tr.softmax_step(ids, loss)
    elif path in ("multineg_sm", "multineg_hinge"):
        user, items = t.forced_rows(rs, NU, NI, B, 1 + K)
        tr.multineg = (K, t.loss_id(t.SM if path == "multineg_sm" else "hinge"), 0.5 if path == "multineg_sm" else 1.0)
        tr.multineg_step(t.multi_ids(user, items, item_meta), loss)
    else:
        user, items = t.forced_rows(rs, NU, NI, B, 1 + K)
        tr.warp = (K, 1.0, ops.warp_rank_weights(NI, K, "log", t.DEV))
        tr.warp_step(t.multi_ids(user, items, item_meta), loss)
    tr.check_errors()
    assert np.isfinite(loss.item())
    return calls, tr


L2_CASES = [None, (0.01, 0.01, 0.01), (0.0, 0.01, 0.01)]
gpu = pytest.mark.gpu


def penalty(l2):
    return [("stage_add_l2",)] if l2 is not None else []


@gpu
@pytest.mark.parametrize("l2", L2_CASES)
@pytest.mark.parametrize("net_type", ["fm", "linear"])
def test_launches_of_step(net_type, l2, monkeypatch):
    """step(): the fused pair update, one launch, between the timing events bench.py reads."""
    calls, tr = launches_of_one_step("step", net_type, l2, monkeypatch)
    assert calls == penalty(l2) + FUSED
    assert sorted(tr.kernel_events) == ["score_kernel<fwd_bwd>", "score_sgd_update_kernel"]
    assert all(len(v) == 1 for v in tr.kernel_events.values())


@gpu
@pytest.mark.parametrize("l2", L2_CASES)
@pytest.mark.parametrize("net_type", ["fm", "linear"])
def test_launches_of_warp_step(net_type, l2, monkeypatch):
    """warp_step(): the fused pair update on (user, positive, chosen candidate)."""
    calls, tr = launches_of_one_step("warp", net_type, l2, monkeypatch)
    assert calls == penalty(l2) + FUSED


@gpu
@pytest.mark.parametrize("l2", L2_CASES)
@pytest.mark.parametrize("net_type", ["fm", "linear"])
def test_launches_of_softmax_step(net_type, l2, monkeypatch):
    """softmax_step(): one scatter per table on S = 1 slot, the user's 1-wide table included; never the fused update."""
    calls, tr = launches_of_one_step("softmax", net_type, l2, monkeypatch)
    assert calls == penalty(l2) + scatters(net_type, 1)


@gpu
@pytest.mark.parametrize("l2", L2_CASES)
@pytest.mark.parametrize("path", ["multineg_sm", "multineg_hinge"])
@pytest.mark.parametrize("net_type", ["fm", "linear"])
def test_launches_of_multineg_step(net_type, path, l2, monkeypatch):
    """multineg_step(): one scatter per table on S = 1 + K slots; under the sampled softmax the user's 1-wide table is
    skipped (its block is exactly zero) unless the user group's penalty was added to it; never the fused update."""
    calls, tr = launches_of_one_step(path, net_type, l2, monkeypatch)
    skip = path == "multineg_sm" and not (l2 is not None and l2[0] > 0)
    assert calls == penalty(l2) + scatters(net_type, 1 + K, skip_user_lin=skip)
