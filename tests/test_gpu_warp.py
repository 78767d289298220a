# -*- coding: utf-8 -*-
"""WARP loss on the MI355X (trs_score_warp_fwd_bwd, csrc/multineg.hip warp_kernel): the choice of the
first violator on tables that make every z exact, random float tables against the float64 restatement tests/warp_ref.py
(itself held to float64 autograd by tests/test_warp_host.py), the forward-only mode, an out-of-range id, K = 1 against
the pair kernel's hinge, one warp_step per optimiser class, fit() / evaluate() end to end against a host replay, and the
paths of every other loss."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

import row_shapes
import warp_ref
from conftest import rel_err
from oracle import optim as ooptim

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
META_SIZES = (13, 7)
TOL = 1e-5  # the project's bar for fp32 scores, losses and gradients (norm-wise relative)
SHAPES = [(1, 2, 5), (20, 1, 37), (33, 17, 37), (64, 8, 257), (128, 64, 257), (512, 9, 37)]  # (D, K, B)


def _ops():
    from torchrecsys_amd import ops
    return ops


def round_size(D):
    """Candidates per round of warp_kernel for row width D (csrc: pick_row_cfg, MULTI_ROW_VGPRS = 16)."""
    if D % 4 == 0:
        chunks = D // 4
        g = 2
        while g < chunks and g < 64:
            g <<= 1
        n = 4 * (1 if chunks <= 64 else 2 if chunks <= 128 else 4)
    else:
        g, n = (4, 1) if D <= 4 else (16, 1) if D <= 16 else (64, 1) if D <= 64 else (64, 4)
    return min(g, 8, max(1, 16 // n))


def table_params_numpy(net_type, M, NU, NI, D, seed):
    """Seeded random normal weights by state_dict name: tables N(0, 0.3), 1-wide terms N(0, 0.1); item -> metadata."""
    rs = np.random.RandomState(seed)
    W = {}
    for name in warp_ref.table_names(net_type, M):
        rows = NU if "user" in name else NI
        if "metadata" in name:
            rows = META_SIZES[int(name.split(".")[1])]
        wide = name in ("user.weight", "item.weight") or name.startswith("metadata.")
        W[name] = rs.normal(0, 0.3 if wide else 0.1, (rows, D if wide else 1)).astype(np.float32)
    item_meta = np.stack([rs.randint(0, META_SIZES[m], NI) for m in range(M)], 1).astype(np.int32) if M else None
    return W, item_meta


def net_from(net_type, M, NU, NI, D, W):
    from torchrecsys_amd.collaborative.fm import FM
    from torchrecsys_amd.collaborative.linear import Linear
    cls = Linear if net_type == "linear" else FM
    with contextlib.redirect_stdout(io.StringIO()):
        net = cls(NU, NI, {f"m{m}": META_SIZES[m] for m in range(M)}, D, use_metadata=M > 0).to(DEV)
    assert sorted(W) == sorted(net.state_dict().keys())
    with torch.no_grad():
        for k, p in net.state_dict().items():
            p.copy_(torch.from_numpy(W[k]))
    return net


def params_of(net):
    return {k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()}


def device_ids(user, items, item_meta):
    ids = {"user": torch.from_numpy(user.astype(np.int32)).to(DEV),
           "items": torch.from_numpy(np.ascontiguousarray(items.astype(np.int32))).to(DEV)}
    if item_meta is not None:
        safe = np.clip(items, 0, item_meta.shape[0] - 1)
        ids["meta"] = torch.from_numpy(np.ascontiguousarray(item_meta[safe].astype(np.int32))).to(DEV)
    return ids


def run_kernel(net_type, net, ids, margin, weights, forward_only=False, grad_rows=None, grad_lin=None, err=None):
    """-> dict loss_sum, auc, neg, neg_meta, trials, gr, gl (device tensors)."""
    ops = _ops()
    loss_sum = torch.zeros(1, device=DEV)
    auc = torch.zeros(1, dtype=torch.int32, device=DEV)
    w = torch.from_numpy(np.asarray(weights, dtype=np.float64).astype(np.float32)).to(DEV)
    neg, neg_meta, trials, gr, gl = ops.score_warp_fwd_bwd(net_type, net.tables(), ids["user"], ids["items"],
                                                           ids.get("meta"), margin, w, loss_sum, auc,
                                                           grad_rows=grad_rows, grad_lin=grad_lin, err_flag=err,
                                                           forward_only=forward_only)
    torch.cuda.synchronize()
    return {"loss_sum": loss_sum, "auc": auc, "neg": neg, "neg_meta": neg_meta, "trials": trials, "gr": gr, "gl": gl}


def table_fields(M):
    """Field lists of the staging buffers, one per table: user, item, metadata columns."""
    return [[0], [1, 2]] + [[3 + 2 * m, 4 + 2 * m] for m in range(M)]


def random_rows(rs, NU, NI, B, K, n_pos=None):
    """user (B,), items (1 + K, B): repeated users, candidates that repeat inside a row and across rows; positives from
    the first n_pos items (default: any), candidates never equal to their row's positive."""
    user = rs.randint(0, NU, B)
    items = rs.randint(0, NI, (1 + K, B))
    if n_pos:
        items[0] = rs.randint(0, n_pos, B)
    if B >= 3:
        user[1::3] = user[0]
    if K >= 2:
        items[2, ::5] = items[1, ::5]
    clash = items[1:] == items[0][None, :]
    items[1:][clash] = (items[0][None, :].repeat(K, 0)[clash] + 1) % NI
    return user, items


# ------------------------------------------------------------------------------------------ 1. controlled selection
def exact_tables(net_type, M, NU, NI, D):
    """Every user row e_0, item i's row v_i * e_0 with v = 0 for i < NI / 2 and -5 beyond, every other table 0: then
    z(u, i) = v_i exactly in fp32 for both nets (FM: 0.5 * ((1 + v)^2 - 1 - v^2) = v)."""
    W, item_meta = table_params_numpy(net_type, M, NU, NI, D, 0)
    for k in W:
        W[k][:] = 0
    W["user.weight"][:, 0] = 1
    W["item.weight"][NI // 2:, 0] = -5
    return W, item_meta


def controlled_block(rs, NI, B, K, C):
    """items (1 + K, B) and f (B,): the positive from items 0..9 (v = 0), hot candidates from 10 .. NI/2 - 1 (v = 0:
    h = 1, a violator), cold ones from NI/2 .. (v = -5: h = -4).  Row t's first hot candidate sits at f(t), cycling over
    {0, C, K - 1, none} (slots the row does not have left out); later slots are hot or cold at random."""
    slots = sorted({s for s in (0, C, K - 1) if s < K}) + [-1]
    f = np.array([slots[t % len(slots)] for t in range(B)])
    hot = rs.randint(10, NI // 2, (K, B))
    cold = rs.randint(NI // 2, NI, (K, B))
    j = np.arange(K)[:, None]
    is_hot = np.where(f[None, :] < 0, False, (j == f[None, :]) | ((j > f[None, :]) & (rs.rand(K, B) < 0.5)))
    items = np.concatenate([rs.randint(0, 10, (1, B)), np.where(is_hot, hot, cold)], axis=0)
    return items, f


@pytest.mark.parametrize("D,K,B", SHAPES)
@pytest.mark.parametrize("M", [0, 2])
@pytest.mark.parametrize("net_type", ["linear", "fm"])
def test_controlled_selection_is_exact(net_type, M, D, K, B):
    """Every lane-group width (one group per wave up to 32), K below / at / not a multiple of a round, B not a multiple of
    the rows per wave; every wave holds groups that finish in the first round, in a later round, in the last slot and
    never.  trials, the chosen ids and the zero rows exactly; the loss and the gradients at 1e-5."""
    NU, NI = 50, 60
    W, item_meta = exact_tables(net_type, M, NU, NI, D)
    net = net_from(net_type, M, NU, NI, D, W)
    rs = np.random.RandomState(D + K)
    items, f = controlled_block(rs, NI, B, K, round_size(D))
    user = rs.randint(0, NU, B)
    weights = warp_ref.rank_weights(100_000, K, "log")
    got = run_kernel(net_type, net, device_ids(user, items, item_meta), 1.0, weights)
    ref = warp_ref.staged(net_type, W, user, items, item_meta, 1.0, weights)
    assert np.array_equal(ref["trials"], f + 1) and (ref["h"][f >= 0, f[f >= 0]] == 1.0).all()  # (the block is as built)
    assert np.array_equal(got["trials"].cpu().numpy(), ref["trials"])
    assert np.array_equal(got["neg"].cpu().numpy(), ref["neg"])
    if M:
        assert np.array_equal(got["neg_meta"].cpu().numpy(), ref["neg_meta"])
    want_loss = weights[f[f >= 0]].sum()  # sum of w[f] * 1
    print(f"loss {got['loss_sum'].item():.8g} want {want_loss:.8g}")
    assert abs(got["loss_sum"].item() - want_loss) <= TOL * want_loss
    gr, gl = got["gr"].cpu().numpy(), got["gl"].cpu().numpy()
    assert gr.shape == (3 + 2 * M, B, D) and gl.shape == (3 + 2 * M, B)
    for fields in table_fields(M):
        print(f"fields {fields}: rows {rel_err(gr[fields], ref['gr'][fields]):.2e}")
        assert rel_err(gr[fields], ref["gr"][fields]) <= TOL, fields
        assert rel_err(gl[fields], ref["gl"][fields]) <= TOL, fields
    assert not gr[:, f < 0].any() and not gl[:, f < 0].any()  # no violator: every field exactly 0
    assert not gl[0].any()  # the user's 1-wide gradient: exactly 0
    assert int(got["auc"].item()) == int((ref["z"][:, 0] > ref["z"][:, 1]).sum())  # (exact z: rows whose c_0 is cold)


# ------------------------------------------------------------------------------------------ 2. random float tables
def random_case(net_type, M, seed=3):
    """D = 64 (rounds of 4), K = 8, B = 2048.  The positives come from the first 10 items, whose 1-wide term is raised by
    0.6: with margin 0.25 about a quarter of the candidates violate, so the trial counts cover 0, 1, the first round, a
    later round and K."""
    NU, NI, D, K, B, margin = 300, 400, 64, 8, 2048, 0.25
    W, item_meta = table_params_numpy(net_type, M, NU, NI, D, seed)
    W["user.weight"] *= 0.5
    W[warp_ref.lin_names(net_type)[1]][:10] += 0.6
    user, items = random_rows(np.random.RandomState(seed + 1), NU, NI, B, K, n_pos=10)
    return NU, NI, D, K, B, margin, W, item_meta, user, items


@pytest.mark.parametrize("kind", ["log", "harmonic"])
@pytest.mark.parametrize("M", [0, 2])
@pytest.mark.parametrize("net_type", ["linear", "fm"])
def test_random_tables_match_the_float64_restatement(net_type, M, kind):
    NU, NI, D, K, B, margin, W, item_meta, user, items = random_case(net_type, M)
    C = round_size(D)
    weights = warp_ref.rank_weights(NI, K, kind)
    ref = warp_ref.staged(net_type, W, user, items, item_meta, margin, weights)
    # the inputs, from the reference alone: few rows near a tie, every kind of trial count present
    skip = warp_ref.near_ties(ref["z"], margin, TOL)
    tr = ref["trials"]
    assert skip.sum() <= 0.01 * B
    assert (tr == 0).any() and (tr == 1).any() and ((tr > 1) & (tr <= C)).any() and ((tr > C) & (tr < K)).any() \
        and (tr == K).any(), np.bincount(tr, minlength=K + 1)
    net = net_from(net_type, M, NU, NI, D, W)
    got = run_kernel(net_type, net, device_ids(user, items, item_meta), margin, weights)
    keep = ~skip
    g_tr, g_neg = got["trials"].cpu().numpy(), got["neg"].cpu().numpy()
    print(f"left out {int(skip.sum())} of {B}; trials {np.bincount(tr, minlength=K + 1).tolist()}")
    assert np.array_equal(g_tr[keep], tr[keep]) and np.array_equal(g_neg[keep], ref["neg"][keep])
    if M:
        assert np.array_equal(got["neg_meta"].cpu().numpy()[keep], ref["neg_meta"][keep])
    # the loss sum holds the left-out rows too: theirs from the device's own choice and the reference's h
    Jd = g_tr[skip] - 1
    own = np.where(Jd >= 0, weights[np.maximum(Jd, 0)] * ref["h"][skip, np.maximum(Jd, 0)], 0.0)
    want_loss = ref["row_loss"][keep].sum() + own.sum()
    print(f"loss {got['loss_sum'].item():.8g} want {want_loss:.8g}")
    assert abs(got["loss_sum"].item() - want_loss) <= TOL * want_loss
    gr, gl = got["gr"].cpu().numpy(), got["gl"].cpu().numpy()
    for fields in table_fields(M):
        a, b = gr[fields][:, keep], ref["gr"][fields][:, keep]
        print(f"fields {fields}: rows {rel_err(a, b):.2e}")
        assert rel_err(a, b) <= TOL, fields
        assert rel_err(gl[fields][:, keep], ref["gl"][fields][:, keep]) <= TOL, fields
    assert not gl[0].any()
    assert not gr[:, keep & (tr == 0)].any() and not gl[:, keep & (tr == 0)].any()
    s = ref["z"]
    clear = np.abs(s[:, 0] - s[:, 1]) > 1e-5 * np.abs(s).max()  # AUC on (p, c_0), away from fp32 ties
    assert abs(int(got["auc"].item()) - int((s[:, 0] > s[:, 1])[clear].sum())) <= int((~clear).sum())


# ------------------------------------------------------------------------------------------ 3. forward only
@pytest.mark.parametrize("net_type,M,D,K", [("fm", 2, 64, 8), ("linear", 0, 33, 17), ("fm", 0, 128, 3)])
def test_forward_only_mode_writes_the_same_outputs_and_nothing_else(net_type, M, D, K, tune):
    """grad_rows == NULL: loss, AUC count, chosen ids and trials of the training mode, bit for bit (one workgroup walks
    the batch, so the loss sums see their terms in the same order); a sentinel-filled staging buffer stays as it was."""
    tune(GRID_CAP=1)
    NU, NI, B, margin = 50, 60, 257, 0.2
    W, item_meta = table_params_numpy(net_type, M, NU, NI, D, D + 1)
    net = net_from(net_type, M, NU, NI, D, W)
    user, items = random_rows(np.random.RandomState(6), NU, NI, B, K)
    ids = device_ids(user, items, item_meta)
    weights = warp_ref.rank_weights(NI, K, "log")
    a = run_kernel(net_type, net, ids, margin, weights)
    poison_r, poison_l = torch.full_like(a["gr"], 7.25), torch.full_like(a["gl"], -3.5)
    b = run_kernel(net_type, net, ids, margin, weights, forward_only=True, grad_rows=poison_r, grad_lin=poison_l)
    assert b["gr"] is None and b["gl"] is None
    assert b["loss_sum"].item() == a["loss_sum"].item() and a["loss_sum"].item() > 0
    assert int(b["auc"].item()) == int(a["auc"].item())
    assert torch.equal(a["neg"], b["neg"]) and torch.equal(a["trials"], b["trials"])
    assert 0 < int((a["trials"] > 0).sum()) and int(a["trials"].max()) > 1
    if M:
        assert torch.equal(a["neg_meta"], b["neg_meta"])
    assert bool((poison_r == 7.25).all()) and bool((poison_l == -3.5).all())


# ------------------------------------------------------------------------------------------ 4. a bad id
@pytest.mark.parametrize("net_type,M", [("fm", 2), ("linear", 0)])
def test_out_of_range_id_sets_the_flag_and_is_not_used_as_an_address(net_type, M):
    NU, NI, D, K, B, margin = 50, 60, 64, 8, 37, 0.2
    W, item_meta = table_params_numpy(net_type, M, NU, NI, D, 9)
    net = net_from(net_type, M, NU, NI, D, W)
    user, items = random_rows(np.random.RandomState(8), NU, NI, B, K)
    bad_user, bad_items = user.copy(), items.copy()
    bad_items[3, 4] = 2 ** 30       # a candidate far outside the item table
    bad_items[0, 9] = -7            # a negative positive id
    bad_user[20] = NU               # one past the user table
    bad_rows = [4, 9, 20]
    ids = device_ids(bad_user, bad_items, item_meta)
    if M:  # a metadata id outside its table, in a row of its own
        ids["meta"][5, 30, 1] = META_SIZES[1]
        bad_rows.append(30)
    weights = warp_ref.rank_weights(NI, K, "log")
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = run_kernel(net_type, net, ids, margin, weights, err=err)
    assert int(err.item()) & 1
    ref = warp_ref.staged(net_type, W, user, items, item_meta, margin, weights)
    good = np.ones(B, bool)
    good[bad_rows] = False
    good_cmp = good & ~warp_ref.near_ties(ref["z"], margin, TOL)
    gr, gl, tr = got["gr"].cpu().numpy(), got["gl"].cpu().numpy(), got["trials"].cpu().numpy()
    assert np.array_equal(tr[good_cmp], ref["trials"][good_cmp]) and (ref["trials"][good_cmp] > 0).any()
    assert np.array_equal(got["neg"].cpu().numpy()[good_cmp], ref["neg"][good_cmp])
    assert rel_err(gr[:, good_cmp], ref["gr"][:, good_cmp]) <= TOL
    assert rel_err(gl[:, good_cmp], ref["gl"][:, good_cmp]) <= TOL
    assert not gr[:, ~good].any() and not gl[:, ~good].any() and not tr[~good].any()  # a dead row: zeros, trials 0 ...
    assert good_cmp.sum() == good.sum()  # (no near tie among these rows: the loss sum below is the good rows')
    want = ref["row_loss"][good].sum()
    assert abs(got["loss_sum"].item() - want) <= TOL * want  # ... and no loss
    # clean ids leave the flag alone
    err.zero_()
    run_kernel(net_type, net, device_ids(user, items, item_meta), margin, weights, err=err)
    assert int(err.item()) == 0


# ------------------------------------------------------------------------------------------ 5. K = 1
@pytest.mark.parametrize("D", row_shapes.ALL)
@pytest.mark.parametrize("M", [0, 2])
def test_one_candidate_with_unit_weight_is_the_linear_hinge(M, D):
    """K = 1, Linear (its hinge is on the score itself), rank_weight = [1], margin 1, at every row shape's ragged and
    largest width: trials in {0, 1}, the negative is c_0, and the staged gradients are trs_score_fwd_bwd's hinge
    gradients at 1e-5."""
    ops = _ops()
    from torchrecsys_amd import _lib
    NU, NI, B = 50, 60, 257
    W, item_meta = table_params_numpy("linear", M, NU, NI, D, D)
    for k in W:
        W[k] *= 3.0  # score differences beyond the margin on both sides
    net = net_from("linear", M, NU, NI, D, W)
    user, items = random_rows(np.random.RandomState(5), NU, NI, B, 1)
    ids = device_ids(user, items, item_meta)
    got = run_kernel("linear", net, ids, 1.0, np.ones(1))
    tr = got["trials"].cpu().numpy()
    assert set(tr.tolist()) == {0, 1}
    assert torch.equal(got["neg"], ids["items"][1])
    if M:
        assert torch.equal(got["neg_meta"], ids["meta"][1])
    Bt, keep = ops.make_batch(ids["user"], ids["items"][0], ids["items"][1], ids["meta"][0] if M else None,
                              ids["meta"][1] if M else None, None)
    ls = torch.zeros(1, device=DEV)
    auc = torch.zeros(1, dtype=torch.int32, device=DEV)
    _, _, cr, cl = ops.score_fwd_bwd("linear", net.tables(), Bt, B, D, M, DEV, ls, auc, want_scores=False,
                                     loss=_lib.LOSS_ID["hinge"])
    torch.cuda.synchronize()
    gr, gl, cr, cl = (x.cpu().numpy() for x in (got["gr"], got["gl"], cr, cl))
    for fields in table_fields(M):
        assert rel_err(gr[fields], cr[fields]) <= TOL, fields
    assert rel_err(gl[1:], cl[1:]) <= TOL
    assert np.abs(gl[0] - cl[0]).max() <= TOL * np.abs(cl[1:]).max()  # (gp + gn there, an exact 0 here)
    assert abs(got["loss_sum"].item() - ls.item()) <= TOL * ls.item() and ls.item() > 0
    assert int(got["auc"].item()) == int(auc.item())


# ------------------------------------------------------------------------------------------ 6. optimisers
def optimiser_case(net_type, M):
    NU, NI, D, K, B, margin = 300, 200, 16, 5, 150, 0.25
    W, item_meta = table_params_numpy(net_type, M, NU, NI, D, 5)
    W[warp_ref.lin_names(net_type)[1]][:10] += 0.4
    user, items = random_rows(np.random.RandomState(8), NU, NI, B, K, n_pos=10)
    return NU, NI, D, K, B, margin, W, item_meta, user, items


def optimiser_rule(kind, k, rows):
    """fn(w0, g) -> the table after one step of the optimiser class `kind` on the coalesced fp32 gradient g."""
    lr_of = lambda name: 0.5 if (kind != "sgd_two_lr" or name == "user.weight") else 0.25

    def rule(w0, g):
        w = w0.copy()
        if kind in ("sgd", "sgd_two_lr", "sgd_momentum"):  # (the momentum buffer of a first step is the gradient)
            w -= np.float32(lr_of(k)) * g
        elif kind == "sparse_adam":
            ooptim.sparse_adam_rows(w, g, rows, np.zeros_like(w), np.zeros_like(w), 1, 0.01)
        else:
            ooptim.adagrad_rows(w, g, rows, np.zeros_like(w), 1, 0.05)
        return w
    return rule


def optimiser_reference(net_type, M, kind):
    """The whole host replay of one step, from the float64 restatement alone: (inputs, {name: (want, touched rows)},
    mean loss, the input's condition per table)."""
    case = optimiser_case(net_type, M)
    NU, NI, D, K, B, margin, W, item_meta, user, items = case
    weights = warp_ref.rank_weights(NI, K, "log")
    ref_loss, grads, st = warp_ref.loss_and_grads(net_type, W, user, items, item_meta, margin, weights)
    term_sums = warp_ref.coalesce(net_type, W, user, items[0], st["neg"], item_meta, np.abs(st["gr"]), np.abs(st["gl"]))
    rows = warp_ref.touched(net_type, W, user, items[0], st["neg"], item_meta)
    out, moved = {}, {}
    for k in W:
        rule = optimiser_rule(kind, k, rows[k])
        g, d = grads[k].astype(np.float32), (1e-6 * term_sums[k]).astype(np.float32)
        want = rule(W[k], g)
        moved[k] = max(rel_err(rule(W[k], g + d), want), rel_err(rule(W[k], g - d), want))
        out[k] = (want, rows[k])
    return case, weights, st, out, ref_loss, moved


@pytest.mark.parametrize("kind", ["sgd", "sgd_two_lr", "sparse_adam", "adagrad", "sgd_momentum"])
@pytest.mark.parametrize("net_type,M", [("fm", 2), ("linear", 2), ("fm", 0)])
def test_one_warp_step_per_optimiser_class(net_type, M, kind):
    """engine.SparseScorerTrainer.warp_step against the restatement's gradient pushed through oracle.optim's rules: 1e-5
    on the tables, rows outside the step's index lists bit-identical (tests/test_gpu_multineg.py's bars for the same
    comparison, with its condition on the input: moving every coalesced entry by 1e-6 of the sum of its terms'
    magnitudes must move no table by more than a third of the bar — computed from the float64 restatement alone)."""
    from torchrecsys_amd.engine import SparseScorerTrainer
    case, weights, st, want, ref_loss, moved = optimiser_reference(net_type, M, kind)
    NU, NI, D, K, B, margin, W, item_meta, user, items = case
    assert not warp_ref.near_ties(st["z"], margin, TOL).any()  # (the choice is the same in fp32)
    assert (st["trials"] == 0).any() and (st["trials"] > 1).any()
    net = net_from(net_type, M, NU, NI, D, W)
    ps = net.table_params()
    if kind == "sgd":
        opt = torch.optim.SGD(net.parameters(), lr=0.5)
    elif kind == "sgd_two_lr":
        opt = torch.optim.SGD([{"params": [ps[0]], "lr": 0.5}, {"params": ps[1:], "lr": 0.25}], lr=0.5)
    elif kind == "sgd_momentum":  # a dense-state torch optimiser: sparse COO gradients + optimizer.step()
        opt = torch.optim.SGD(net.parameters(), lr=0.5, momentum=0.9)
    elif kind == "sparse_adam":
        opt = torch.optim.SparseAdam(list(net.parameters()), lr=0.01)
    else:
        opt = torch.optim.Adagrad(net.parameters(), lr=0.05)
    tr = SparseScorerTrainer(net, opt, 256)  # B < capacity: prefix views of the staging buffers
    assert tr.kind == {"sgd_momentum": "generic", "sgd_two_lr": "sgd"}.get(kind, kind)
    tr.warp = (K, margin, torch.from_numpy(weights.astype(np.float32)).to(DEV))
    loss = torch.zeros(1, device=DEV)
    tr.warp_step(device_ids(user, items, item_meta), loss)
    tr.check_errors()
    assert abs(loss.item() / B - ref_loss) <= TOL * abs(ref_loss)
    after = params_of(net)
    for k, (w, rows) in want.items():
        assert moved[k] <= TOL / 3, (k, moved[k])  # the input's condition (docstring), from the restatement alone
        print(f"{k}: {rel_err(after[k], w):.2e} (touched rows {rel_err(after[k][rows], w[rows]):.2e})")
        assert rel_err(after[k], w) <= TOL, k
        assert rel_err(after[k][rows], w[rows]) <= TOL, k
        keep = np.ones(w.shape[0], bool)
        keep[rows] = False
        assert np.array_equal(after[k][keep], W[k][keep]), k
    lu = warp_ref.lin_names(net_type)[0]
    assert np.array_equal(after[lu], W[lu])  # the user-side 1-wide table: an exact 0 moves nothing under any rule


# ------------------------------------------------------------------------------------------ 7. end to end
def _model(net_type, neg_sampling=None, seed=1, n_factors=16, n_u=200, n_i=300, n=5000):
    from torchrecsys_amd.model import TorchRecSys
    rs = np.random.RandomState(4)
    users = torch.from_numpy(np.concatenate([np.arange(n_u), rs.randint(0, n_u, n - n_u)]).astype(np.int64)).to(DEV)
    items = torch.from_numpy(np.concatenate([np.arange(n_i), rs.randint(0, n_i, n - n_i)]).astype(np.int64)).to(DEV)
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        return TorchRecSys.from_tensors(users, items, n_users=n_u, n_items=n_i, n_factors=n_factors, net_type=net_type,
                                        dynamic_neg_sampling=True, seed=seed, neg_sampling=neg_sampling)


@pytest.mark.parametrize("net_type,neg_sampling,kind,margin", [
    ("fm", None, "log", 0.3), ("linear", None, "harmonic", 0.01),
    ("fm", {"popularity": True, "reject_seen": True, "max_tries": 4}, "log", 0.3)])
def test_fit_and_evaluate_against_a_host_replay(net_type, neg_sampling, kind, margin):
    """200 users x 300 items, 5 000 interactions, 2 epochs of batch 512, WARP over 5 candidates, SGD: the ids from
    ops.batch_prepare_multi under the runner's keys and sampler, the steps from the float64 restatement.  Final tables at
    5e-5 (the project's multi-step trajectory bar), printed epoch losses to 4 decimals, evaluate()'s loss at 1e-5.  The
    margins sit inside the spread of z at initialisation (FM: the 1-wide terms are N(0, 1); Linear: the biases start at
    0 and z is a dot product of N(0, 1/16) rows), so that rows stop at every trial count."""
    from torchrecsys_amd import model as model_mod
    ops = _ops()
    K, B, lr, epochs, EB = 5, 512, 0.05, 2, 128
    model = _model(net_type, neg_sampling)
    W = {k: v.astype(np.float64) for k, v in params_of(model.net).items()}
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        model.fit(torch.optim.SGD(model.parameters(), lr=lr), epochs=epochs, batch_size=B, loss="warp", n_negatives=K,
                  margin=margin, rank_weight=kind)
        model.evaluate(batch_size=EB)
    printed = [float(x) for x in re.findall(r"Training Loss: ([-0-9.]+)", buf.getvalue())]
    assert len(printed) == epochs
    weights = warp_ref.rank_weights(model.n_items, K, kind)
    st = model._device_stream("train")
    N = st["user"].numel()
    near, hist = 0, np.zeros(K + 1, int)
    for e in range(epochs):
        key, seed = model_mod._mix64(model.seed, 2 * e + 1), model_mod._mix64(model.seed, 2 * e + 2)
        means = []
        for s in range(0, N, B):
            n = min(B, N - s)
            ids = ops.batch_prepare_multi(st["user"], st["pos"], key, s, n, model.n_items, seed, s, K, None,
                                          sampler=model._sampler())
            user, items = ids["user"].cpu().numpy(), ids["items"].cpu().numpy()
            val, grads, ref = warp_ref.loss_and_grads(net_type, W, user, items, None, margin, weights)
            near += int(warp_ref.near_ties(ref["z"], margin, TOL).sum())
            hist += np.bincount(ref["trials"], minlength=K + 1)
            means.append(val)
            for k in W:
                W[k] -= lr * grads[k]
        want = float(np.mean(means))
        print(f"epoch {e + 1}: printed {printed[e]:.4f} replay {want:.6f}")
        assert abs(printed[e] - want) <= 0.5e-4 + 1e-5 * abs(want)  # the printed value is the replay's to 4 decimals
    print(f"trials {hist.tolist()}, rows near a tie {near}")
    assert hist[1] > 0 and hist[2:].sum() > 0  # the choice mattered
    after = params_of(model.net)
    for k in W:
        print(k, f"{rel_err(after[k], W[k]):.2e}")
        assert rel_err(after[k], W[k]) <= 5e-5, k
    # evaluate(): the test split in order, K candidates per row, one loss per batch, unweighted mean over the batches
    tt = model._device_stream("test")
    eval_seed = model_mod._mix64(model.seed, 0xE7A1)
    final = {k: v.astype(np.float64) for k, v in after.items()}
    vals, auc = [], []
    NT = tt["user"].numel()
    for s in range(0, NT, EB):
        n = min(EB, NT - s)
        ids = ops.batch_prepare_multi(tt["user"], tt["pos"], 0, s, n, model.n_items, eval_seed, s, K, None,
                                      sampler=model._eval_sampler())
        ref = warp_ref.staged(net_type, final, ids["user"].cpu().numpy(), ids["items"].cpu().numpy(), None, margin,
                              weights)
        vals.append(ref["loss"])
        auc.append(float((ref["z"][:, 0] > ref["z"][:, 1]).mean()))
    got = model.eval_results
    assert abs(got["loss"] - np.mean(vals)) <= TOL * np.mean(vals), (got, np.mean(vals))
    assert abs(got["auc"] - np.mean(auc)) <= 2.0 / EB  # pairwise on (p, c_0); a near-tie or two may flip in fp32
    assert "Testing loss: %.4f" % got["loss"] in buf.getvalue()


# ------------------------------------------------------------------------------------------ 8. paths
def test_every_other_loss_keeps_its_paths(monkeypatch):
    """Runs with loss in hinge / bpr / softmax / sampled_softmax, with or without n_negatives and mining, never call
    score_warp_fwd_bwd or warp_step; a WARP run calls both once per step."""
    from torchrecsys_amd import ops
    from torchrecsys_amd.engine import SparseScorerTrainer
    calls = {"kernel": 0, "step": 0}

    def spy(obj, name, key):
        orig = getattr(obj, name)

        def wrapped(*a, **kw):
            calls[key] += 1
            return orig(*a, **kw)
        monkeypatch.setattr(obj, name, wrapped)

    spy(ops, "score_warp_fwd_bwd", "kernel")
    spy(SparseScorerTrainer, "warp_step", "step")

    def fit(neg_sampling=None, **kw):
        model = _model("fm", neg_sampling, n=1500)
        with contextlib.redirect_stdout(io.StringIO()):
            model.fit(torch.optim.SGD(model.parameters(), lr=0.05), epochs=1, batch_size=256, **kw)
            model.evaluate(batch_size=256)
        return model

    mine = {"mine": "hardest", "candidates": 4}
    for ns, kw in ((None, {}), (None, dict(loss="hinge")), (None, dict(loss="bpr")), (None, dict(loss="softmax")),
                   (None, dict(loss="sampled_softmax", n_negatives=3)), (None, dict(loss="hinge", n_negatives=3)),
                   (None, dict(loss="bpr", n_negatives=2)), (mine, dict(loss="hinge")), (mine, dict(loss="bpr"))):
        fit(ns, **kw)
        assert calls == {"kernel": 0, "step": 0}, (ns, kw)
    model = fit(None, loss="warp", n_negatives=3)
    steps = -(-model._device_stream("train")["user"].numel() // 256)
    assert calls["step"] == steps and calls["kernel"] > steps  # (evaluate() adds its forward-only launches)
