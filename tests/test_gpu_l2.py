# -*- coding: utf-8 -*-
"""fit(l2=...) on the MI355X (trs_stage_add_l2, csrc/l2.hip): the launch at every row shape bit for
bit, every staging layout against float64, the id guard, one step of each per-step path against the same step without
the penalty, one step per optimiser class against the oracle's rules, fit() end to end against a host replay, and the
paths a run takes with and without a coefficient."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

import l2_ref
import multineg_ref
import row_shapes
from conftest import rel_err
from oracle import optim as ooptim

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
META_SIZES = (13, 7)
TOL = 1e-5  # the project's bar for one step (norm-wise relative); 5e-5 for a multi-step trajectory
SM = multineg_ref.SAMPLED_SOFTMAX
LAM = (0.3, 0.2, 0.1)


def _ops():
    from torchrecsys_amd import ops
    return ops


def loss_id(loss):
    from torchrecsys_amd import _lib
    return _lib.LOSS_SAMPLED_SOFTMAX if loss == SM else _lib.LOSS_ID[loss]


def build_net(net_type, M, NU, NI, D, seed):
    """A Linear / FM scorer with seeded random normal weights: tables N(0, 0.3), 1-wide terms N(0, 0.1)."""
    from torchrecsys_amd.collaborative.fm import FM
    from torchrecsys_amd.collaborative.linear import Linear
    cls = Linear if net_type == "linear" else FM
    with contextlib.redirect_stdout(io.StringIO()):
        net = cls(NU, NI, {f"m{m}": META_SIZES[m] for m in range(M)}, D, use_metadata=M > 0).to(DEV)
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        for p in net.table_params():
            p.copy_(torch.from_numpy(rs.normal(0, 0.3 if p.shape[1] > 1 else 0.1, p.shape).astype(np.float32)))
    item_meta = np.stack([rs.randint(0, META_SIZES[m], NI) for m in range(M)], 1).astype(np.int32) if M else None
    return net, item_meta


def params_of(net):
    return {k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()}


def forced_rows(rs, NU, NI, B, S):
    """user (B,), items (S, B): repeated users, one item in many rows and in several slots, a slot repeated inside every
    row; slots 1.. never equal slot 0 (the sampler's guarantee for a row's candidates)."""
    user = rs.randint(0, NU, B)
    items = rs.randint(0, NI, (S, B))
    if B >= 3:
        user[1::3] = user[0]
        items[1:, ::2] = 5  # item 5: in every later slot of every second row ...
        items[0, 1] = 5     # ... and in slot 0 of row 1
    if S >= 3:
        items[2] = items[1]
    if S >= 2:
        clash = items[1:] == items[0][None, :]
        items[1:][clash] = (items[0][None, :].repeat(S - 1, 0)[clash] + 1) % NI
    return user, items


def meta_of(items, item_meta):
    return None if item_meta is None else item_meta[np.clip(items, 0, item_meta.shape[0] - 1)]


def device_blocks(user, items, meta):
    """The int32 id blocks on the device: user (B,), items (S, B), meta (S, B, M) or None."""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32))).to(DEV)
    return dev(user), dev(items), None if meta is None else dev(meta)


def random_staging(rs, F, B, D, extra=0):
    """Staging buffers pre-filled with random fp32 values, as views of allocations `extra` elements longer."""
    flat_r = torch.from_numpy(rs.normal(0, 1, F * B * D + extra).astype(np.float32)).to(DEV)
    flat_l = torch.from_numpy(rs.normal(0, 1, F * B + extra).astype(np.float32)).to(DEV)
    return flat_r, flat_l, flat_r[:F * B * D].view(F, B, D), flat_l[:F * B].view(F, B)


def add_l2(net_type, net, blocks, coefs, gr, gl, err=None):
    _ops().stage_add_l2(net_type, net.tables(), blocks[0], blocks[1], blocks[2], coefs, gr, gl, err)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 1. every row shape
@pytest.mark.parametrize("D", row_shapes.ALL)
def test_every_row_shape_bit_for_bit(D):
    """FM, S = 2, M = 1, B = 37 (with G = 2 a wave holds 32 references: ragged at the wave's end), duplicate ids, a
    pre-filled buffer.  The coefficients are powers of two, so c * w is exact and g + c * w rounds once: numpy float32
    computes the same bits."""
    net_type, S, M, B, NU, NI = "fm", 2, 1, 37, 11, 17
    rs = np.random.RandomState(D)
    net, item_meta = build_net(net_type, M, NU, NI, D, D)
    user, items = forced_rows(rs, NU, NI, B, S)
    meta = meta_of(items, item_meta)
    F = 1 + S * (1 + M)
    _, _, gr, gl = random_staging(rs, F, B, D)
    g0, l0 = gr.cpu().numpy(), gl.cpu().numpy()
    coefs = (0.5, 0.25, 0.125)
    add_l2(net_type, net, device_blocks(user, items, meta), coefs, gr, gl)
    want_r, want_l, _, _ = l2_ref.staged_add(net_type, params_of(net), user, items, meta, coefs, g0, l0, np.float32)
    assert want_r.dtype == np.float32 and not np.array_equal(want_r, g0) and not np.array_equal(want_l, l0)
    assert np.array_equal(gr.cpu().numpy(), want_r)
    assert np.array_equal(gl.cpu().numpy(), want_l)


# ------------------------------------------------------------------------------------------------ 2. layouts
def within_two_roundings(got, want, mag):
    """|got - want| <= 2^-22 (|g| + |c w|): two fp32 roundings, each at most 2^-24 relative to a value no larger than
    |g| + |c w|, with a factor 2 of slack for the float32 conversion of c."""
    err = np.abs(got.astype(np.float64) - want)
    bad = err > 2.0 ** -22 * mag
    worst = float((err / np.maximum(mag, 1e-300)).max()) if err.size else 0.0
    return not bad.any(), worst


@pytest.mark.parametrize("D,B", [(20, 1), (64, 300)])
@pytest.mark.parametrize("S", [1, 2, 9])
@pytest.mark.parametrize("M", [0, 2])
@pytest.mark.parametrize("net_type", ["linear", "fm"])
def test_every_layout_against_float64(net_type, M, S, D, B):
    NU, NI = 50, 60
    rs = np.random.RandomState(7 * S + M + B)
    net, item_meta = build_net(net_type, M, NU, NI, D, S + D)
    user, items = forced_rows(rs, NU, NI, B, S)
    meta = meta_of(items, item_meta)
    blocks = device_blocks(user, items, meta)
    F = 1 + S * (1 + M)
    EXTRA = 1000
    flat_r, flat_l, gr, gl = random_staging(rs, F, B, D, EXTRA)
    f0_r, f0_l = flat_r.cpu().numpy(), flat_l.cpu().numpy()
    g0, l0 = gr.cpu().numpy(), gl.cpu().numpy()
    coefs = (0.3 / B, 0.2 / B, 0.1 / B)
    P = params_of(net)
    add_l2(net_type, net, blocks, coefs, gr, gl)
    want_r, want_l, mag_r, mag_l = l2_ref.staged_add(net_type, P, user, items, meta, coefs, g0, l0)
    got_r, got_l = gr.cpu().numpy(), gl.cpu().numpy()
    ok_r, worst_r = within_two_roundings(got_r, want_r, mag_r)
    ok_l, worst_l = within_two_roundings(got_l, want_l, mag_l)
    print(f"rows {worst_r / 2.0 ** -22:.3f} 1-wide {worst_l / 2.0 ** -22:.3f} of the bound")
    assert ok_r and ok_l
    assert not np.array_equal(got_r[0], g0[0]) and not np.array_equal(got_l[1], l0[1])
    if M:
        assert not np.array_equal(got_r[1 + S:], g0[1 + S:])
        if net_type == "linear":  # no 1-wide metadata tables: those fields are not touched
            assert np.array_equal(got_l[1 + S:], l0[1 + S:])
        else:
            assert not np.array_equal(got_l[1 + S:], l0[1 + S:])
    # elements beyond F * B * D of a larger allocation stay as they were
    assert np.array_equal(flat_r.cpu().numpy()[F * B * D:], f0_r[F * B * D:])
    assert np.array_equal(flat_l.cpu().numpy()[F * B:], f0_l[F * B:])
    # one coefficient 0: that group's fields stay bit-identical, the others get their terms
    groups = [slice(0, 1), slice(1, 1 + S), slice(1 + S, F)]
    for z in range(3 if M else 2):
        c = tuple(0.0 if i == z else coefs[i] for i in range(3))
        gr.copy_(torch.from_numpy(g0))
        gl.copy_(torch.from_numpy(l0))
        add_l2(net_type, net, blocks, c, gr, gl)
        r, l = gr.cpu().numpy(), gl.cpu().numpy()
        assert np.array_equal(r[groups[z]], g0[groups[z]]) and np.array_equal(l[groups[z]], l0[groups[z]]), z
        for o in range(3 if M else 2):
            if o != z:
                assert np.array_equal(r[groups[o]], got_r[groups[o]]) and np.array_equal(l[groups[o]], got_l[groups[o]])


# ------------------------------------------------------------------------------------------------ 3. the guard
@pytest.mark.parametrize("net_type", ["fm", "linear"])
def test_out_of_range_ids_set_the_flag_and_are_not_used_as_addresses(net_type):
    NU, NI, D, S, M, B = 50, 60, 64, 3, 2, 37
    rs = np.random.RandomState(8)
    net, item_meta = build_net(net_type, M, NU, NI, D, 9)
    user, items = forced_rows(rs, NU, NI, B, S)
    meta = meta_of(items, item_meta)
    F = 1 + S * (1 + M)
    coefs = (0.3 / B, 0.2 / B, 0.1 / B)
    P = params_of(net)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    # clean ids leave the flag alone
    _, _, gr, gl = random_staging(rs, F, B, D)
    add_l2(net_type, net, device_blocks(user, items, meta), coefs, gr, gl, err)
    assert int(err.item()) == 0
    bad_user, bad_items, bad_meta = user.copy(), items.copy(), meta.copy()
    bad_items[1, 4] = NI             # one past the item table
    bad_user[20] = -1
    bad_meta[0, 30, 1] = META_SIZES[1]
    skip = np.zeros((F, B), bool)
    skip[1 + 1, 4] = skip[0, 20] = skip[1 + S + 1 * S + 0, 30] = True
    _, _, gr, gl = random_staging(rs, F, B, D)
    g0, l0 = gr.cpu().numpy(), gl.cpu().numpy()
    add_l2(net_type, net, device_blocks(bad_user, bad_items, bad_meta), coefs, gr, gl, err)
    assert int(err.item()) & 1
    got_r, got_l = gr.cpu().numpy(), gl.cpu().numpy()
    assert np.array_equal(got_r[skip], g0[skip]) and np.array_equal(got_l[skip], l0[skip])
    want_r, want_l, mag_r, mag_l = l2_ref.staged_add(net_type, P, bad_user, bad_items, bad_meta, coefs, g0, l0,
                                                     skip=skip)
    assert within_two_roundings(got_r, want_r, mag_r)[0] and within_two_roundings(got_l, want_l, mag_l)[0]
    changed = (got_r != g0).any(axis=2)
    assert changed[~skip].all() and not changed[skip].any()  # exactly those references are unchanged
    # an empty batch returns without error
    e = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=DEV)
    _ops().stage_add_l2(net_type, net.tables(), e(0, dt=torch.int32), e(S, 0, dt=torch.int32),
                        e(S, 0, M, dt=torch.int32), coefs, e(F, 0, D), e(F, 0), err)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. the engine's steps
def pair_ids(user, items, item_meta, dtype=np.int32):
    """ids of step(): the triples (user, items[0], items[1]); int64 is what the reference-RNG path carries."""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)
    ids = {"user": dev(user), "pos": dev(items[0]), "neg": dev(items[1])}
    if item_meta is not None:
        ids["pos_meta"], ids["neg_meta"] = dev(item_meta[items[0]]), dev(item_meta[items[1]])
    return ids


def multi_ids(user, items, item_meta):
    u, i, m = device_blocks(user, items, meta_of(items, item_meta))
    ids = {"user": u, "items": i}
    if m is not None:
        ids["meta"] = m
    return ids


def run_step(path, net_type, M, opt_of, l2, NU, NI, D, B, K, cap, seed=5, ids_seed=8, id_dtype=np.int32):
    """One step of `path` from seeded tables on forced ids.  Returns (tables before, tables after, loss slot, the id
    blocks (user, items (S, B)) the step's staged references name, item_meta, trainer)."""
    from torchrecsys_amd.engine import SparseScorerTrainer
    ops = _ops()
    net, item_meta = build_net(net_type, M, NU, NI, D, seed)
    W = params_of(net)
    tr = SparseScorerTrainer(net, opt_of(net), cap)
    tr.l2 = l2
    rs = np.random.RandomState(ids_seed)
    loss = torch.zeros(1, device=DEV)
    if path == "step":
        user, items = forced_rows(rs, NU, NI, B, 2)
        tr.step(pair_ids(user, items, item_meta, id_dtype), loss)
    elif path == "softmax":
        user, items = forced_rows(rs, NU, NI, B, 1)
        ids = pair_ids(user, np.concatenate([items, items]), item_meta, id_dtype)
        ids.pop("neg_meta", None)
        tr.softmax = (0.5, None)
        tr.softmax_step(ids, loss)
    elif path in ("multineg_sm", "multineg_hinge"):
        user, items = forced_rows(rs, NU, NI, B, 1 + K)
        tr.multineg = (K, loss_id(SM if path == "multineg_sm" else "hinge"), 0.5 if path == "multineg_sm" else 1.0)
        tr.multineg_step(multi_ids(user, items, item_meta), loss)
    elif path == "warp":
        user, items = forced_rows(rs, NU, NI, B, 1 + K)
        tr.warp = (K, 1.0, ops.warp_rank_weights(NI, K, "log", DEV))
        tr.warp_step(multi_ids(user, items, item_meta), loss)
        items = np.stack([items[0], tr._warp_neg[:B].cpu().numpy().astype(np.int64)])  # (positive, chosen candidate)
    else:
        raise ValueError(path)
    tr.check_errors()
    return W, params_of(net), loss.item(), (user, items), item_meta, tr


ENGINE_PATHS = [("step", 0), ("step", 2), ("softmax", 2), ("multineg_sm", 2), ("multineg_hinge", 2), ("warp", 2),
                ("warp", 0)]


@pytest.mark.parametrize("path,M", ENGINE_PATHS)
@pytest.mark.parametrize("net_type", ["fm", "linear"])
def test_each_step_with_l2_is_todays_step_minus_lr_times_the_penalty_gradient(net_type, path, M):
    """SGD, lr 0.5: the same tables and ids once with l2=None and once with l2=(0.3, 0.2, 0.1).  The penalty reads the
    pre-update rows, so the two results differ by lr times l2_ref's gradient; the loss slot holds the data loss in both;
    rows no id references are bit-identical to the start."""
    NU, NI, D, B, K, lr = 300, 200, 16, 150, 5, 0.5
    cap = B if path == "step" else 256  # (B < capacity: prefix views of the staging buffers)
    sgd = lambda net: torch.optim.SGD(net.parameters(), lr=lr)
    W, after_0, loss_0, (user, items), item_meta, _ = run_step(path, net_type, M, sgd, None, NU, NI, D, B, K, cap)
    W2, after_l2, loss_l2, (user2, items2), _, _ = run_step(path, net_type, M, sgd, LAM, NU, NI, D, B, K, cap)
    assert all(np.array_equal(W[k], W2[k]) for k in W)
    assert np.array_equal(user, user2) and np.array_equal(items, items2)  # (WARP: the same chosen candidates)
    meta = meta_of(items, item_meta)
    pen = l2_ref.grads(net_type, W, user, items, meta, LAM, 1.0 / B)
    rows = l2_ref.touched(net_type, W, user, items, meta)
    assert sorted(pen) == sorted(W)
    print(f"loss slots {loss_0:.8g} {loss_l2:.8g}")
    assert abs(loss_l2 - loss_0) <= TOL * abs(loss_0) and loss_0 > 0
    for k in W:
        want = after_0[k].astype(np.float64) - lr * pen[k]
        print(f"{k}: {rel_err(after_l2[k], want):.2e}")
        assert rel_err(after_l2[k], want) <= TOL, k
        assert np.abs(pen[k]).max() > 0 and not np.array_equal(after_l2[k], after_0[k]), k
        keep = np.ones(W[k].shape[0], bool)
        keep[rows[k]] = False
        assert np.array_equal(after_l2[k][keep], W[k][keep]), k
    lu = multineg_ref.lin_names(net_type)[0]
    if path in ("multineg_sm", "warp", "softmax"):
        # the data gradient of the user's 1-wide table is an exact 0 there: without l2 it does not move, with l2 it must
        assert np.array_equal(after_0[lu], W[lu])
        assert (after_l2[lu][rows[lu]] != W[lu][rows[lu]]).all()


@pytest.mark.parametrize("path", ["step", "softmax"])
def test_int64_ids_take_the_same_step(path):
    """The reference-RNG path hands step() and softmax_step() int64 ids: converted once, the step is the int32 one (up
    to the order of the row updates' float atomics)."""
    NU, NI, D, B, K = 300, 200, 16, 150, 5
    sgd = lambda net: torch.optim.SGD(net.parameters(), lr=0.5)
    W, a32, l32, _, _, _ = run_step(path, "fm", 2, sgd, LAM, NU, NI, D, B, K, B)
    _, a64, l64, _, _, _ = run_step(path, "fm", 2, sgd, LAM, NU, NI, D, B, K, B, id_dtype=np.int64)
    assert abs(l64 - l32) <= TOL * abs(l32)
    for k in W:
        assert rel_err(a64[k], a32[k]) <= TOL and not np.array_equal(a32[k], W[k]), k


# ------------------------------------------------------------------------------------------------ 5. optimiser classes
def optimiser(kind):
    if kind == "sgd":
        return lambda net: torch.optim.SGD(net.parameters(), lr=0.5)
    if kind == "sgd_momentum":  # a dense-state torch optimiser: sparse COO gradients + optimizer.step()
        return lambda net: torch.optim.SGD(net.parameters(), lr=0.5, momentum=0.9)
    if kind == "sparse_adam":
        return lambda net: torch.optim.SparseAdam(list(net.parameters()), lr=0.01)
    return lambda net: torch.optim.Adagrad(net.parameters(), lr=0.05)


def oracle_step_inputs(net_type, path, W, user, items, item_meta, K):
    """(data loss, dense data gradients, sums of the staged terms' magnitudes) from the float64 restatement."""
    loss, tau = (SM, 0.5) if path == "multineg_sm" else ("hinge", 1.0)
    ref_loss, gr64, gl64, _ = multineg_ref.staged(net_type, W, user, items, item_meta, loss, tau)
    grads = multineg_ref.coalesce(net_type, W, user, items, item_meta, gr64, gl64)
    term_sums = multineg_ref.coalesce(net_type, W, user, items, item_meta, np.abs(gr64), np.abs(gl64))
    return ref_loss, grads, term_sums


def apply_rule(kind, w0, g, rows):
    w = w0.copy()
    if kind in ("sgd", "sgd_momentum"):  # (the momentum buffer of a first step is the gradient)
        w -= np.float32(0.5) * g
    elif kind == "sparse_adam":
        ooptim.sparse_adam_rows(w, g, rows, np.zeros_like(w), np.zeros_like(w), 1, 0.01)
    else:
        ooptim.adagrad_rows(w, g, rows, np.zeros_like(w), 1, 0.05)
    return w


@pytest.mark.parametrize("kind", ["sgd", "sparse_adam", "adagrad", "sgd_momentum"])
@pytest.mark.parametrize("path", ["step", "multineg_sm"])
def test_one_l2_step_per_optimiser_class(path, kind):
    """FM, M = 2, pair hinge and sampled softmax over K = 5: the oracle's data gradient plus l2_ref's gradient pushed
    through oracle.optim's rule (the penalised gradient goes through the rule unchanged); 1e-5 on the tables, rows no
    id touches bit-identical.

    The input is held to the condition of test_one_multineg_step_per_optimiser_class, computed from the float64
    oracle alone: moving every coalesced entry by 1e-6 of the sum of its terms' magnitudes (the penalty's terms
    included) must move no table by more than a third of the bar."""
    net_type, M = "fm", 2
    NU, NI, D, B, K, cap = 300, 200, 16, 150, 5, 256
    # ids_seed: the first seed of the forced ids whose batch meets the condition below under every rule on both paths
    W, after, loss, (user, items), item_meta, tr = run_step(path, net_type, M, optimiser(kind), LAM, NU, NI, D, B, K, cap,
                                                            ids_seed=11)
    assert tr.kind == ("generic" if kind == "sgd_momentum" else kind)
    ref_loss, grads, term_sums = oracle_step_inputs(net_type, path, W, user, items, item_meta, K)
    assert abs(loss / B - ref_loss) <= TOL * abs(ref_loss)
    meta = meta_of(items, item_meta)
    pen = l2_ref.grads(net_type, W, user, items, meta, LAM, 1.0 / B)
    rows = l2_ref.touched(net_type, W, user, items, meta)
    for k in multineg_ref.table_names(net_type, M):
        g = (grads[k] + pen[k]).astype(np.float32)
        d = (1e-6 * (term_sums[k] + np.abs(pen[k]))).astype(np.float32)
        want = apply_rule(kind, W[k], g, rows[k])
        moved = max(rel_err(apply_rule(kind, W[k], g + d, rows[k]), want),
                    rel_err(apply_rule(kind, W[k], g - d, rows[k]), want))
        assert moved <= TOL / 3, (k, moved)  # the input's condition (docstring), from the oracle alone
        print(f"{k}: {rel_err(after[k], want):.2e} (touched rows {rel_err(after[k][rows[k]], want[rows[k]]):.2e})")
        assert rel_err(after[k], want) <= TOL, k
        assert rel_err(after[k][rows[k]], want[rows[k]]) <= TOL, k
        keep = np.ones(want.shape[0], bool)
        keep[rows[k]] = False
        assert np.array_equal(after[k][keep], W[k][keep]), k


# ------------------------------------------------------------------------------------------------ 6. end to end
def _model(net_type, M=0, neg_sampling=None, seed=1, n_factors=16, n_u=80, n_i=300, n=2000):
    from torchrecsys_amd.model import TorchRecSys
    rs = np.random.RandomState(4)
    users = torch.from_numpy(np.concatenate([np.arange(n_u), rs.randint(0, n_u, n - n_u)]).astype(np.int64)).to(DEV)
    items = torch.from_numpy(np.concatenate([np.arange(n_i), rs.randint(0, n_i, n - n_i)]).astype(np.int64)).to(DEV)
    meta = torch.from_numpy(rs.randint(0, 6, (n_i, M)).astype(np.int64)).to(DEV) if M else None
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        return TorchRecSys.from_tensors(users, items, n_users=n_u, n_items=n_i, item_metadata=meta,
                                        metadata_names=[f"c{m}" for m in range(M)] if M else None,
                                        n_factors=n_factors, net_type=net_type, dynamic_neg_sampling=True, seed=seed,
                                        neg_sampling=neg_sampling)


@pytest.mark.parametrize("case", ["sampled_softmax", "hinge_metadata"])
def test_fit_with_l2_against_a_host_replay(case):
    """About 2 000 interactions, 2 epochs of batch 256, SGD lr 0.5.  The ids from the candidate schedule, the steps from
    the float64 restatements: W -= lr (data gradient + penalty gradient) per batch, the partial last batch with its own
    1 / B.  Final tables at 5e-5; the printed epoch losses are the replay's DATA loss to 4 decimals — the penalty is not
    in the printed loss."""
    from torchrecsys_amd import model as model_mod
    B, lr, epochs = 256, 0.5, 2
    if case == "sampled_softmax":
        M, K, loss, tau, l2, lam = 0, 4, SM, 0.5, {"user": 0.05, "item": 0.02}, (0.05, 0.02, 0.0)
        kw = dict(loss="sampled_softmax", n_negatives=K, temperature=tau)
    else:
        M, K, loss, tau, l2, lam = 1, 1, "hinge", 1.0, 0.03, (0.03, 0.03, 0.03)
        kw = dict(loss="hinge")
    model = _model("fm", M)
    W = {k: v.astype(np.float64) for k, v in params_of(model.net).items()}
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        model.fit(torch.optim.SGD(model.parameters(), lr=lr), epochs=epochs, batch_size=B, l2=l2, **kw)
    printed = [float(x) for x in re.findall(r"Training Loss: ([-0-9.]+)", buf.getvalue())]
    assert len(printed) == epochs
    st = model._device_stream("train")
    su, si = st["user"].cpu().numpy(), st["pos"].cpu().numpy()
    item_meta = None if st["item_meta"] is None else st["item_meta"].cpu().numpy()
    N = len(su)
    assert N % B != 0  # the last batch is partial
    W_data = {k: v.copy() for k, v in W.items()}  # the same replay without the penalty
    for e in range(epochs):
        key, seed = model_mod._mix64(model.seed, 2 * e + 1), model_mod._mix64(model.seed, 2 * e + 2)
        means = []
        for s in range(0, N, B):
            n = min(B, N - s)
            ids = multineg_ref.prepare(su, si, key, s, n, model.n_items, seed, s, K, None, item_meta)
            val, grads = multineg_ref.loss_and_grads("fm", W, ids["user"], ids["items"], item_meta, loss, tau)
            pen = l2_ref.grads("fm", W, ids["user"], ids["items"], ids["meta"], lam, 1.0 / n)
            means.append(val)
            for k in W:
                W[k] -= lr * (grads[k] + pen[k])
            _, grads = multineg_ref.loss_and_grads("fm", W_data, ids["user"], ids["items"], item_meta, loss, tau)
            for k in W_data:
                W_data[k] -= lr * grads[k]
        want = float(np.mean(means))
        print(f"epoch {e + 1}: printed {printed[e]:.4f} replay {want:.6f}")
        assert abs(printed[e] - want) <= 0.5e-4 + 1e-5 * abs(want)
    after = params_of(model.net)
    for k in W:
        print(k, f"{rel_err(after[k], W[k]):.2e} (the replay without the penalty: {rel_err(W_data[k], W[k]):.2e})")
        assert rel_err(after[k], W[k]) <= 5e-5, k
    # the penalty is far above that bar: a run that dropped it would miss
    assert rel_err(W_data["item.weight"], W["item.weight"]) > 5e-4 and rel_err(W_data["user.weight"], W["user.weight"]) > 5e-4


# ------------------------------------------------------------------------------------------------ 7. paths
def _unique_stream_model(seed, n=1024, n_items=1_000_000):
    """Every user and every item occurs once in the stream, and the catalogue is large: with the right sampler seed no
    table row is referenced twice inside a batch."""
    from torchrecsys_amd.model import TorchRecSys
    rs = np.random.RandomState(11)
    users = torch.from_numpy(rs.permutation(n).astype(np.int64)).to(DEV)
    items = torch.from_numpy(rs.choice(n_items, n, replace=False).astype(np.int64)).to(DEV)
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        return TorchRecSys.from_tensors(users, items, n_users=n, n_items=n_items, n_factors=16, net_type="fm",
                                        dynamic_neg_sampling=True, seed=seed)


def _rows_referenced_twice(model, epochs, B):
    """Host replay of the epochs' batches (the plain loader's ids): batches in which a user or an item row repeats."""
    from torchrecsys_amd import model as model_mod
    st = model._device_stream("train")
    su, si = st["user"].cpu().numpy(), st["pos"].cpu().numpy()
    bad = 0
    for e in range(epochs):
        key, seed = model_mod._mix64(model.seed, 2 * e + 1), model_mod._mix64(model.seed, 2 * e + 2)
        for s in range(0, len(su), B):
            n = min(B, len(su) - s)
            ids = multineg_ref.prepare(su, si, key, s, n, model.n_items, seed, s, 1)
            bad += int(np.unique(ids["items"]).size != 2 * n or np.unique(ids["user"]).size != n)
    return bad


def _reseeded(model, seed):
    model.seed = seed
    return model


def test_zero_coefficients_keep_todays_paths_and_a_coefficient_leaves_them(monkeypatch):
    """fit(), fit(l2=0.0) and fit(l2={'item': 0}) never call ops.stage_add_l2, run on the presorted path and give
    bit-identical tables (the unique-stream model of test_one_negative_pair_runs_keep_todays_paths: every row update of
    every step is a single add, so a fit is bit-identical to itself).  fit(l2=0.01) calls the launch once per step,
    never the presorted path, and ends elsewhere."""
    from torchrecsys_amd import ops
    from torchrecsys_amd.engine import SparseScorerTrainer
    calls = {"l2": 0, "sorted": 0, "step": 0}

    def spy(obj, name, key):
        orig = getattr(obj, name)

        def wrapped(*a, **kw):
            calls[key] += 1
            return orig(*a, **kw)
        monkeypatch.setattr(obj, name, wrapped)

    spy(ops, "stage_add_l2", "l2")
    spy(SparseScorerTrainer, "fast_sorted_steps", "sorted")
    spy(SparseScorerTrainer, "step", "step")
    EPOCHS, B = 2, 128
    probe = _unique_stream_model(1)
    seed = next(sd for sd in range(1, 40) if _rows_referenced_twice(_reseeded(probe, sd), EPOCHS, B) == 0)

    def fit(**kw):
        for key in calls:
            calls[key] = 0
        model = _unique_stream_model(seed)
        with contextlib.redirect_stdout(io.StringIO()):
            model.fit(torch.optim.SGD(model.parameters(), lr=0.1), epochs=EPOCHS, batch_size=B, **kw)
        steps = EPOCHS * -(-len(model._device_stream("train")["user"]) // B)
        return params_of(model.net), dict(calls), steps

    base, c, steps = fit()
    assert c["l2"] == 0 and c["sorted"] > 0 and c["step"] < steps  # (step(): the epochs' partial last batches)
    for kw in (dict(l2=0.0), dict(l2={"item": 0})):
        same, c, _ = fit(**kw)
        assert c["l2"] == 0 and c["sorted"] > 0, kw
        for k in base:
            assert np.array_equal(same[k], base[k]), (kw, k)
    other, c, _ = fit(l2=0.01)
    assert c["l2"] == c["step"] == steps and c["sorted"] == 0
    assert all(np.isfinite(v).all() for v in other.values())
    assert any(not np.array_equal(other[k], base[k]) for k in base)


def test_l2_runs_with_adagrad_and_with_mining():
    for neg_sampling, opt in ((None, lambda m: torch.optim.Adagrad(m.parameters(), lr=0.05)),
                              ({"mine": "hardest", "candidates": 4}, lambda m: torch.optim.SGD(m.parameters(), lr=0.1))):
        model = _model("fm", 1, neg_sampling)
        before = params_of(model.net)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            model.fit(opt(model), epochs=2, batch_size=256, l2=0.01)
        tl = [float(x) for x in re.findall(r"Training Loss: ([-0-9.]+)", buf.getvalue())]
        after = params_of(model.net)
        assert len(tl) == 2 and all(np.isfinite(tl))
        assert all(np.isfinite(v).all() for v in after.values())
        assert any(not np.array_equal(after[k], before[k]) for k in after)
