# -*- coding: utf-8 -*-
"""Training on K sampled negatives per positive on the MI355X (trs_batch_prepare_multi, trs_score_multi_fwd_bwd,
csrc/multineg.hip): the draws against the existing loader and tests/mining_ref.py, the sampled softmax
against the float64 restatement tests/multineg_ref.py (itself held to float64 autograd by tests/test_multineg_host.py),
the mean of K hinge / BPR pairs against K calls of the existing pair kernel, the forward-only mode, an out-of-range id,
one step per optimiser class, and fit() / evaluate() end to end against a host replay."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

import mining_ref
import multineg_ref
import row_shapes
from conftest import rel_err
from oracle import optim as ooptim

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
META_SIZES = (13, 7)
TOL = 1e-5  # the project's bar for fp32 scores, losses and gradients (norm-wise relative)
SM = multineg_ref.SAMPLED_SOFTMAX


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


def forced_rows(rs, NU, NI, B, K):
    """user (B,), items (1 + K, B): a repeated candidate inside a row, one item as a candidate of many rows and the
    positive of another, repeated users; no candidate equals its row's positive (the sampler's guarantee)."""
    user = rs.randint(0, NU, B)
    items = rs.randint(0, NI, (1 + K, B))
    if B >= 3:
        user[1::3] = user[0]
        items[1:, ::2] = 5  # item 5: a candidate of every second row ...
        items[0, 1] = 5     # ... and the positive of row 1
    if K >= 2:
        items[2] = items[1]  # the same candidate twice in every row
    clash = items[1:] == items[0][None, :]
    items[1:][clash] = (items[0][None, :].repeat(K, 0)[clash] + 1) % NI
    return user, items


def device_ids(user, items, item_meta):
    ids = {"user": torch.from_numpy(user.astype(np.int32)).to(DEV),
           "items": torch.from_numpy(np.ascontiguousarray(items.astype(np.int32))).to(DEV)}
    if item_meta is not None:
        safe = np.clip(items, 0, item_meta.shape[0] - 1)
        ids["meta"] = torch.from_numpy(np.ascontiguousarray(item_meta[safe].astype(np.int32))).to(DEV)
    return ids


def run_kernel(net_type, net, ids, loss, tau, forward_only=False, grad_rows=None, grad_lin=None, err=None):
    ops = _ops()
    loss_sum = torch.zeros(1, device=DEV)
    auc = torch.zeros(1, dtype=torch.int32, device=DEV)
    gr, gl = ops.score_multi_fwd_bwd(net_type, net.tables(), ids["user"], ids["items"], ids.get("meta"), loss_id(loss),
                                     tau, loss_sum, auc, grad_rows, grad_lin, err, forward_only=forward_only)
    torch.cuda.synchronize()
    return loss_sum, auc, gr, gl


def table_blocks(K, M):
    """Field slices of the staging buffers, one per table: user, item, metadata columns."""
    S1 = 1 + K
    return [slice(0, 1), slice(1, 1 + S1)] + [slice(1 + S1 + m * S1, 1 + S1 + (m + 1) * S1) for m in range(M)]


# ------------------------------------------------------------------------------------------------ 1. the draws
@pytest.mark.parametrize("variant", ["plain", "popularity+reject_seen", "two_visits"])
@pytest.mark.parametrize("K", [1, 3, 8, 64])
@pytest.mark.parametrize("B", [1, 257])
def test_draws_equal_the_loaders_under_the_candidate_schedule(B, K, variant):
    ops = _ops()
    rs = np.random.RandomState(B + K)
    NU, NI, N, M = 60, 90, 1000, 2
    su, si = rs.randint(0, NU, N).astype(np.int32), rs.randint(0, NI, N).astype(np.int32)
    si[rs.rand(N) < 0.1] = 7
    item_meta = np.stack([rs.randint(0, META_SIZES[m], NI) for m in range(M)], 1).astype(np.int32)
    su_d, si_d, im = (torch.from_numpy(a).to(DEV) for a in (su, si, item_meta))
    options, k = variant == "popularity+reject_seen", 2 if variant == "two_visits" else 1
    seen = ops.Sampler.seen_csr(su_d, si_d, NU, NI) if options else None
    sampler = ops.Sampler(k=k, popularity=options, seen=seen, stream_item=si_d, max_tries=8) \
        if (options or k > 1) else None
    ref_sampler = {"k": k, "max_tries": 8}
    if options:
        ref_sampler.update(popularity=True, seen=(seen[0].cpu().numpy(), seen[1].cpu().numpy()))
    key, seed = 0xFEED5, 0x1234567
    t0 = N * k - B - 3  # (two visits: positions beyond the first pass over the stream)
    got = ops.batch_prepare_multi(su_d, si_d, key, t0, B, NI, seed, t0, K, im, sampler=sampler)
    torch.cuda.synchronize()
    assert got["items"].shape == (1 + K, B) and got["meta"].shape == (1 + K, B, M)
    for j in range(K):
        want = ops.batch_prepare(su_d, si_d, None, key, t0, B, NI, (seed + j * mining_ref.KEY_STEP) & mining_ref.MASK64,
                                 t0, im, sampler=sampler)
        assert torch.equal(got["items"][1 + j], want["neg"]), j
        assert torch.equal(got["meta"][1 + j], want["neg_meta"]), j
        if j == 0:
            assert torch.equal(got["user"], want["user"]) and torch.equal(got["items"][0], want["pos"])
            assert torch.equal(got["meta"][0], want["pos_meta"])
            assert torch.equal(got["pos"], want["pos"]) and torch.equal(got["neg"], want["neg"])
    ref = multineg_ref.prepare(su, si, key, t0, B, NI, seed, t0, K, ref_sampler, item_meta)
    items = got["items"].cpu().numpy()
    assert np.array_equal(got["user"].cpu().numpy(), ref["user"]) and np.array_equal(items, ref["items"])
    assert np.array_equal(got["meta"].cpu().numpy(), item_meta[items])
    assert (items[1:] != items[0]).all() and items.min() >= 0 and items.max() < NI


# ------------------------------------------------------------------------------------------------ 2. sampled softmax
SHAPES = [(1, 2, 5, 1.0), (20, 1, 37, 1.0), (33, 17, 37, 1.0), (64, 8, 257, 0.05), (128, 64, 257, 0.1), (512, 9, 37, 0.2)]


@pytest.mark.parametrize("D,K,B,tau", SHAPES)
@pytest.mark.parametrize("M", [0, 2])
@pytest.mark.parametrize("net_type", ["linear", "fm"])
def test_sampled_softmax_matches_the_float64_oracle(net_type, M, D, K, B, tau):
    """Every lane-group width (D = 1 .. 512), a partial last wave, K below / equal to / above a round and not a
    multiple of it; loss at 1e-5 relative, every table's staged block at 1e-5 norm-wise."""
    NU, NI = 50, 60
    net, item_meta = build_net(net_type, M, NU, NI, D, D + K)
    user, items = forced_rows(np.random.RandomState(K), NU, NI, B, K)
    loss_sum, auc, gr, gl = run_kernel(net_type, net, device_ids(user, items, item_meta), SM, tau)
    want_loss, wr, wl, z = multineg_ref.staged(net_type, params_of(net), user, items, item_meta, SM, tau)
    got = loss_sum.item() / B
    print(f"loss {got:.8g} oracle {want_loss:.8g} rel {abs(got - want_loss) / abs(want_loss):.2e}")
    gr, gl = gr.cpu().numpy(), gl.cpu().numpy()
    for sl in table_blocks(K, M):
        print(f"fields {sl.start}..{sl.stop - 1}: rows {rel_err(gr[sl], wr[sl]):.2e} 1-wide {rel_err(gl[sl], wl[sl]):.2e}")
    assert abs(got - want_loss) <= TOL * abs(want_loss)
    assert gr.shape == wr.shape == (multineg_ref.n_fields(K, M), B, D)
    for sl in table_blocks(K, M):
        assert rel_err(gr[sl], wr[sl]) <= TOL, sl
        assert rel_err(gl[sl], wl[sl]) <= TOL, sl
    assert not gl[0].any()  # the user's 1-wide gradient: exactly 0
    if net_type == "linear" and M:
        assert not gl[2 + K:].any()  # Linear has no 1-wide metadata tables
    s = z if net_type == "linear" else 1.0 / (1.0 + np.exp(-z))
    clear = np.abs(s[:, 0] - s[:, 1]) > 1e-5 * np.abs(s).max()  # AUC on (p, c_0), away from fp32 ties
    assert abs(int(auc.item()) - int((s[:, 0] > s[:, 1])[clear].sum())) <= int((~clear).sum())


# ------------------------------------------------------------------------------------------------ 3. mean of K pairs
def pair_kernel_columns(net_type, net, ids, K, M, loss):
    """K calls of the existing pair kernel, one per candidate column: [(loss sum, auc, grad_rows, grad_lin)]."""
    ops = _ops()
    from torchrecsys_amd import _lib
    B, D = ids["user"].shape[0], net.table_params()[0].shape[1]
    out = []
    for j in range(K):
        Bt, keep = ops.make_batch(ids["user"], ids["items"][0], ids["items"][1 + j],
                                  ids["meta"][0] if M else None, ids["meta"][1 + j] if M else None, None)
        ls = torch.zeros(1, device=DEV)
        auc = torch.zeros(1, dtype=torch.int32, device=DEV)
        _, _, gr, gl = ops.score_fwd_bwd(net_type, net.tables(), Bt, B, D, M, DEV, ls, auc, want_scores=False,
                                         loss=_lib.LOSS_ID[loss])
        torch.cuda.synchronize()
        out.append((ls, auc, gr, gl))
    return out


def pair_fields(K, M, j):
    """(fields of the multi-negative staging, fields of the pair kernel's staging for candidate column j): the user,
    the positive, the candidate, then (positive, candidate) of every metadata column."""
    S1 = 1 + K
    multi = [0, 1, 2 + j] + [f for m in range(M) for f in (1 + S1 + m * S1, 1 + S1 + m * S1 + 1 + j)]
    return multi, list(range(3 + 2 * M))


@pytest.mark.parametrize("loss", ["hinge", "bpr"])
@pytest.mark.parametrize("D,K,B", [(20, 3, 37), (64, 8, 257)])
@pytest.mark.parametrize("M", [0, 2])
@pytest.mark.parametrize("net_type", ["linear", "fm"])
def test_mean_of_k_pairs_matches_k_calls_of_the_pair_kernel(net_type, M, D, K, B, loss):
    """The scores are the same pass_forward's, so the hinge decisions cannot differ; the only difference is the order of
    the K-term sums: 1e-6 norm-wise, the bar between two orderings of the same fp32 sums.  One block has a bar of its
    own: the user's 1-wide gradient is gp + sum_j gn_j, which cancels (for Linear to rounding, the true value being 0),
    so a norm-wise bar relative to itself means nothing; it is held to 1e-6 of the largest 1-wide term it sums."""
    NU, NI = 50, 60
    net, item_meta = build_net(net_type, M, NU, NI, D, 3 * D + K)
    user, items = forced_rows(np.random.RandomState(K + 1), NU, NI, B, K)
    ids = device_ids(user, items, item_meta)
    loss_sum, auc, gr, gl = run_kernel(net_type, net, ids, loss, 1.0)
    cols = pair_kernel_columns(net_type, net, ids, K, M, loss)
    want_r = np.zeros(gr.shape)
    want_l = np.zeros(gl.shape)
    for j, (_, _, cr, cl) in enumerate(cols):
        multi, pair = pair_fields(K, M, j)
        want_r[multi] += cr.cpu().numpy().astype(np.float64)[pair] / K
        want_l[multi] += cl.cpu().numpy().astype(np.float64)[pair] / K
    want_loss = float(np.mean([c[0].item() for c in cols]))
    gr, gl = gr.cpu().numpy(), gl.cpu().numpy()
    for sl in table_blocks(K, M):
        print(f"fields {sl.start}..{sl.stop - 1}: rows {rel_err(gr[sl], want_r[sl]):.2e}")
    assert abs(loss_sum.item() - want_loss) <= 1e-6 * abs(want_loss)
    for sl in table_blocks(K, M):
        assert rel_err(gr[sl], want_r[sl]) <= 1e-6, sl
    # 1-wide terms: the item / metadata slots; the user's is a sum that cancels (Linear: to rounding), so it is held to
    # the size of its terms
    assert rel_err(gl[1:], want_l[1:]) <= 1e-6
    assert np.abs(gl[0] - want_l[0]).max() <= 1e-6 * np.abs(want_l[1:]).max()
    assert int(auc.item()) == int(cols[0][1].item())  # pairwise on (p, c_0)
    # the restatement agrees too (fp32 against float64: the project's 1e-5)
    ref_loss, wr, wl, _ = multineg_ref.staged(net_type, params_of(net), user, items, item_meta, loss)
    assert abs(loss_sum.item() / B - ref_loss) <= TOL * abs(ref_loss)
    for sl in table_blocks(K, M):
        assert rel_err(gr[sl], wr[sl]) <= TOL, sl


@pytest.mark.parametrize("loss", ["hinge", "bpr"])
@pytest.mark.parametrize("D", row_shapes.ALL)
@pytest.mark.parametrize("M", [0, 2])
@pytest.mark.parametrize("net_type", ["linear", "fm"])
def test_one_negative_is_the_pair_kernel_bit_for_bit(net_type, M, D, loss, tune):
    """K = 1: the staged blocks, the loss and the AUC count of trs_score_fwd_bwd, bit for bit, at every row shape's
    ragged and largest width (both kernels write item slots through stage_item_slot of csrc/score_kernels.h).  One
    workgroup walks the whole batch in both kernels (GRID_CAP = 1), so the loss sums see their terms in the same order;
    with more workgroups the order of their atomic adds is not fixed in either kernel."""
    tune(GRID_CAP=1)
    NU, NI, B, K = 50, 60, 257, 1
    net, item_meta = build_net(net_type, M, NU, NI, D, D)
    user, items = forced_rows(np.random.RandomState(5), NU, NI, B, K)
    ids = device_ids(user, items, item_meta)
    loss_sum, auc, gr, gl = run_kernel(net_type, net, ids, loss, 1.0)
    (ls, ac, cr, cl), = pair_kernel_columns(net_type, net, ids, K, M, loss)
    multi, pair = pair_fields(K, M, 0)
    assert torch.equal(gr[multi], cr[pair]) and torch.equal(gl[multi], cl[pair])
    assert loss_sum.item() == ls.item() and ls.item() > 0
    assert int(auc.item()) == int(ac.item())


# ------------------------------------------------------------------------------------------------ 4. forward only
@pytest.mark.parametrize("loss", [SM, "hinge", "bpr"])
@pytest.mark.parametrize("net_type,M,D,K", [("fm", 2, 64, 8), ("linear", 0, 33, 17), ("fm", 0, 128, 3)])
def test_forward_only_mode_writes_the_same_loss_and_nothing_else(net_type, M, D, K, loss, tune):
    """grad_rows == NULL: the loss and the AUC count of the training mode, bit for bit (one workgroup, see above), and a
    poisoned gradient buffer handed to the forward-only call stays as it was."""
    tune(GRID_CAP=1)
    NU, NI, B, tau = 50, 60, 257, 0.2
    net, item_meta = build_net(net_type, M, NU, NI, D, D + 1)
    user, items = forced_rows(np.random.RandomState(6), NU, NI, B, K)
    ids = device_ids(user, items, item_meta)
    l1, a1, gr, gl = run_kernel(net_type, net, ids, loss, tau)
    poison_r, poison_l = torch.full_like(gr, 7.25), torch.full_like(gl, -3.5)
    l0, a0, r0, r1 = run_kernel(net_type, net, ids, loss, tau, forward_only=True, grad_rows=poison_r, grad_lin=poison_l)
    assert r0 is None and r1 is None
    assert l0.item() == l1.item() and l1.item() > 0 and int(a0.item()) == int(a1.item())
    assert bool((poison_r == 7.25).all()) and bool((poison_l == -3.5).all())


# ------------------------------------------------------------------------------------------------ 5. a bad id
@pytest.mark.parametrize("loss", [SM, "hinge"])
@pytest.mark.parametrize("net_type,M", [("fm", 2), ("linear", 0)])
def test_out_of_range_id_sets_the_flag_and_is_not_used_as_an_address(net_type, M, loss):
    NU, NI, D, K, B, tau = 50, 60, 64, 8, 37, 0.5
    net, item_meta = build_net(net_type, M, NU, NI, D, 9)
    user, items = forced_rows(np.random.RandomState(8), NU, NI, B, K)
    bad_user, bad_items = user.copy(), items.copy()
    bad_items[3, 4] = 2 ** 30       # a candidate far outside the item table
    bad_items[0, 9] = -7            # a negative positive id
    bad_user[20] = NU               # one past the user table
    bad_rows = [4, 9, 20]
    ids = device_ids(bad_user, bad_items, item_meta)
    if M:  # a metadata id outside its table, in a row of its own
        ids["meta"][5, 30, 1] = META_SIZES[1]
        bad_rows.append(30)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    loss_sum, auc, gr, gl = run_kernel(net_type, net, ids, loss, tau, err=err)
    assert int(err.item()) & 1
    _, wr, wl, z = multineg_ref.staged(net_type, params_of(net), user, items, item_meta, loss, tau)
    row_loss, _ = multineg_ref.slot_weights(net_type, z, loss, tau)
    good = np.ones(B, bool)
    good[bad_rows] = False
    gr, gl = gr.cpu().numpy(), gl.cpu().numpy()
    assert rel_err(gr[:, good], wr[:, good]) <= TOL and rel_err(gl[:, good], wl[:, good]) <= TOL
    assert not gr[:, ~good].any() and not gl[:, ~good].any()  # a dead row carries zero gradients ...
    assert abs(loss_sum.item() - row_loss[good].sum()) <= TOL * row_loss[good].sum()  # ... and no loss
    # clean ids leave the flag alone
    err.zero_()
    run_kernel(net_type, net, device_ids(user, items, item_meta), loss, tau, err=err)
    assert int(err.item()) == 0


# ------------------------------------------------------------------------------------------------ 6. optimisers
@pytest.mark.parametrize("kind", ["sgd", "sgd_two_lr", "sparse_adam", "adagrad", "sgd_momentum"])
@pytest.mark.parametrize("net_type,M", [("fm", 2), ("linear", 2), ("fm", 0)])
def test_one_multineg_step_per_optimiser_class(net_type, M, kind):
    """engine.SparseScorerTrainer.multineg_step: the oracle's gradient pushed through oracle.optim's rules; 1e-5 on the
    tables, rows no id touches bit-identical.

    The adaptive rules' first step is u = lr * g / (c |g| + eps): where a coalesced gradient entry cancels down to the
    size of eps (an item that is the positive of one row and a candidate of others), u is linear in g with slope
    lr / eps and turns the fp32 rounding of the staged terms into table errors above 1e-5 for any fp32 staging.  That is
    a property of the input, so the input is held to a condition computed from the float64 oracle alone: moving every
    coalesced entry by 1e-6 of the sum of its terms' magnitudes (fp32 terms whose exponentials take arguments up to
    ~10) must move no table by more than a third of the bar."""
    from torchrecsys_amd.engine import SparseScorerTrainer
    NU, NI, D, K, B, tau, cap = 300, 200, 16, 5, 150, 0.5, 256
    net, item_meta = build_net(net_type, M, NU, NI, D, 5)
    names = multineg_ref.table_names(net_type, M)
    assert sorted(names) == sorted(net.state_dict().keys())
    W = params_of(net)
    if kind == "sgd":
        opt = torch.optim.SGD(net.parameters(), lr=0.5)
    elif kind == "sgd_two_lr":  # the user embedding table at 0.5, every other table at 0.25
        ps = net.table_params()
        opt = torch.optim.SGD([{"params": [ps[0]], "lr": 0.5}, {"params": ps[1:], "lr": 0.25}], lr=0.5)
    elif kind == "sgd_momentum":  # a dense-state torch optimiser: sparse COO gradients + optimizer.step()
        opt = torch.optim.SGD(net.parameters(), lr=0.5, momentum=0.9)
    elif kind == "sparse_adam":
        opt = torch.optim.SparseAdam(list(net.parameters()), lr=0.01)
    else:
        opt = torch.optim.Adagrad(net.parameters(), lr=0.05)
    tr = SparseScorerTrainer(net, opt, cap)  # B < capacity: prefix views of the staging buffers
    assert tr.kind == {"sgd_momentum": "generic", "sgd_two_lr": "sgd"}.get(kind, kind)
    tr.multineg = (K, loss_id(SM), tau)
    user, items = forced_rows(np.random.RandomState(8), NU, NI, B, K)
    loss = torch.zeros(1, device=DEV)
    tr.multineg_step(device_ids(user, items, item_meta), loss)
    tr.check_errors()
    ref_loss, gr64, gl64, _ = multineg_ref.staged(net_type, W, user, items, item_meta, SM, tau)
    grads = multineg_ref.coalesce(net_type, W, user, items, item_meta, gr64, gl64)
    term_sums = multineg_ref.coalesce(net_type, W, user, items, item_meta, np.abs(gr64), np.abs(gl64))
    assert abs(loss.item() / B - ref_loss) <= TOL * abs(ref_loss)
    rows = multineg_ref.touched(net_type, W, user, items, item_meta)
    after = params_of(net)

    def rule(w0, g):
        w = w0.copy()
        if kind in ("sgd", "sgd_two_lr", "sgd_momentum"):  # (the momentum buffer of a first step is the gradient)
            w -= np.float32(0.5 if (kind != "sgd_two_lr" or k == "user.weight") else 0.25) * g
        elif kind == "sparse_adam":
            ooptim.sparse_adam_rows(w, g, rows[k], np.zeros_like(w), np.zeros_like(w), 1, 0.01)
        else:
            ooptim.adagrad_rows(w, g, rows[k], np.zeros_like(w), 1, 0.05)
        return w

    for k in names:
        g, d = grads[k].astype(np.float32), (1e-6 * term_sums[k]).astype(np.float32)
        want = rule(W[k], g)
        moved = max(rel_err(rule(W[k], g + d), want), rel_err(rule(W[k], g - d), want))
        assert moved <= TOL / 3, (k, moved)  # the input's condition (docstring), from the oracle alone
        print(f"{k}: {rel_err(after[k], want):.2e} (touched rows {rel_err(after[k][rows[k]], want[rows[k]]):.2e})")
        assert rel_err(after[k], want) <= TOL, k
        assert rel_err(after[k][rows[k]], want[rows[k]]) <= TOL, k
        keep = np.ones(want.shape[0], bool)
        keep[rows[k]] = False
        assert np.array_equal(after[k][keep], W[k][keep]), k
    lu = multineg_ref.lin_names(net_type)[0]
    assert np.array_equal(after[lu], W[lu])  # the user-side 1-wide table: an exact 0 moves nothing under any rule


def test_multineg_step_mean_of_pairs_sgd():
    from torchrecsys_amd.engine import SparseScorerTrainer
    NU, NI, D, K, B = 300, 200, 24, 4, 200
    for net_type, loss in (("fm", "bpr"), ("linear", "hinge")):
        net, item_meta = build_net(net_type, 2, NU, NI, D, 6)
        W = params_of(net)
        tr = SparseScorerTrainer(net, torch.optim.SGD(net.parameters(), lr=0.5), B)
        tr.multineg = (K, loss_id(loss), 1.0)
        user, items = forced_rows(np.random.RandomState(3), NU, NI, B, K)
        out = torch.zeros(1, device=DEV)
        tr.multineg_step(device_ids(user, items, item_meta), out)
        tr.check_errors()
        ref_loss, grads = multineg_ref.loss_and_grads(net_type, W, user, items, item_meta, loss)
        assert abs(out.item() / B - ref_loss) <= TOL * abs(ref_loss)
        after = params_of(net)
        for k in W:
            assert rel_err(after[k], W[k] - np.float32(0.5) * grads[k]) <= TOL, (net_type, k)


# ------------------------------------------------------------------------------------------------ 7. end to end
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


@pytest.mark.parametrize("net_type,M", [("fm", 0), ("linear", 0), ("fm", 1)])
def test_fit_and_evaluate_against_a_host_replay(net_type, M):
    """About 2 000 interactions, 2 epochs of batch 256, sampled softmax over 4 negatives at temperature 0.5, SGD: the ids
    from tests/mining_ref.py's candidate schedule, the steps from the float64 restatement.  Final tables at 5e-5 (the
    project's multi-step trajectory bar), printed epoch losses to 4 decimals, evaluate()'s loss at 1e-5."""
    from torchrecsys_amd import model as model_mod
    K, tau, B, lr, epochs, EB = 4, 0.5, 256, 0.5, 2, 100
    model = _model(net_type, M)
    W = {k: v.astype(np.float64) for k, v in params_of(model.net).items()}
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        model.fit(torch.optim.SGD(model.parameters(), lr=lr), epochs=epochs, batch_size=B, loss="sampled_softmax",
                  n_negatives=K, temperature=tau)
        model.evaluate(batch_size=EB)
    printed = [float(x) for x in re.findall(r"Training Loss: ([-0-9.]+)", buf.getvalue())]
    assert len(printed) == epochs
    st = model._device_stream("train")
    su, si = st["user"].cpu().numpy(), st["pos"].cpu().numpy()
    item_meta = None if st["item_meta"] is None else st["item_meta"].cpu().numpy()
    N = len(su)
    for e in range(epochs):
        key, seed = model_mod._mix64(model.seed, 2 * e + 1), model_mod._mix64(model.seed, 2 * e + 2)
        means = []
        for s in range(0, N, B):
            n = min(B, N - s)
            ids = multineg_ref.prepare(su, si, key, s, n, model.n_items, seed, s, K, None, item_meta)
            val, grads = multineg_ref.loss_and_grads(net_type, W, ids["user"], ids["items"], item_meta, SM, tau)
            means.append(val)
            for k in W:
                W[k] -= lr * grads[k]
        want = float(np.mean(means))
        print(f"epoch {e + 1}: printed {printed[e]:.4f} replay {want:.6f}")
        assert abs(printed[e] - want) <= 0.5e-4 + 1e-5 * abs(want)  # the printed value is the replay's to 4 decimals
    after = params_of(model.net)
    for k in W:
        print(k, f"{rel_err(after[k], W[k]):.2e}")
        assert rel_err(after[k], W[k]) <= 5e-5, k
    # evaluate(): the test split in order, K candidates per row, one loss per batch, unweighted mean over the batches
    tt = model._device_stream("test")
    tu, ti = tt["user"].cpu().numpy(), tt["pos"].cpu().numpy()
    eval_seed = model_mod._mix64(model.seed, 0xE7A1)
    final = {k: v.astype(np.float64) for k, v in after.items()}
    vals, auc = [], []
    for s in range(0, len(tu), EB):
        n = min(EB, len(tu) - s)
        ids = multineg_ref.prepare(tu, ti, 0, s, n, model.n_items, eval_seed, s, K, None, item_meta)
        val, _, _, z = multineg_ref.staged(net_type, final, ids["user"], ids["items"], item_meta, SM, tau)
        vals.append(val)
        auc.append(float((z[:, 0] > z[:, 1]).mean()))
    got = model.eval_results
    assert abs(got["loss"] - np.mean(vals)) <= TOL * np.mean(vals), (got, np.mean(vals))
    assert abs(got["auc"] - np.mean(auc)) <= 2.0 / EB  # pairwise on (p, c_0); a near-tie or two may flip in fp32
    assert "Testing loss: %.4f" % got["loss"] in buf.getvalue()


def test_fit_mean_of_pairs_with_sampler_options_and_adagrad():
    """The other front-door combinations run and learn: BPR over 3 negatives, popularity + reject_seen + two visits per
    positive, metadata, Adagrad; evaluate() reports the same loss."""
    model = _model("fm", 1, {"popularity": True, "reject_seen": True, "k": 2, "max_tries": 4})
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        model.fit(torch.optim.Adagrad(model.parameters(), lr=0.05), epochs=3, batch_size=256, loss="bpr", n_negatives=3)
        model.evaluate(batch_size=128)
    tl = [float(x) for x in re.findall(r"Training Loss: ([-0-9.]+)", buf.getvalue())]
    assert len(tl) == 3 and all(np.isfinite(tl)) and tl[2] < tl[0], buf.getvalue()
    assert np.isfinite(model.eval_results["loss"]) and 0 <= model.eval_results["auc"] <= 1


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


def test_one_negative_pair_runs_keep_todays_paths(monkeypatch):
    """fit(n_negatives=1, loss='hinge') calls neither new entry point (nor multineg_step) and leaves every table
    bit-identical to the same fit without the keyword; n_negatives=2 leaves those paths.

    The comparison needs a fit that is bit-identical to itself: where a row is referenced several times in a batch the
    existing step adds its partial sums in an order that is not fixed.  So the stream holds every user and item once,
    the catalogue has a million items, and the sampler seed is the first whose two epochs — replayed on the host — draw
    no negative that meets another reference of its batch: every row update of every step is then a single add."""
    from torchrecsys_amd import ops
    from torchrecsys_amd.engine import SparseScorerTrainer
    calls = {"prepare_multi": 0, "score_multi": 0, "step": 0, "sorted": 0}

    def spy(obj, name, key):
        orig = getattr(obj, name)

        def wrapped(*a, **kw):
            calls[key] += 1
            return orig(*a, **kw)
        monkeypatch.setattr(obj, name, wrapped)

    spy(ops, "batch_prepare_multi", "prepare_multi")
    spy(ops, "score_multi_fwd_bwd", "score_multi")
    spy(SparseScorerTrainer, "multineg_step", "step")
    spy(SparseScorerTrainer, "fast_sorted_steps", "sorted")
    EPOCHS, B = 2, 128
    probe = _unique_stream_model(1)
    seed = next(sd for sd in range(1, 40)
                if _rows_referenced_twice(_reseeded(probe, sd), EPOCHS, B) == 0)

    def fit(**kw):
        for key in calls:
            calls[key] = 0
        model = _unique_stream_model(seed)
        assert _rows_referenced_twice(model, EPOCHS, B) == 0
        with contextlib.redirect_stdout(io.StringIO()):
            model.fit(torch.optim.SGD(model.parameters(), lr=0.1), epochs=EPOCHS, batch_size=B, **kw)
        return params_of(model.net), dict(calls)

    base, c = fit()
    assert c["prepare_multi"] == c["score_multi"] == c["step"] == 0 and c["sorted"] > 0
    same, c = fit(loss="hinge", n_negatives=1)
    assert c["prepare_multi"] == c["score_multi"] == c["step"] == 0 and c["sorted"] > 0
    for k in base:
        assert np.array_equal(same[k], base[k]), k
    other, c = fit(loss="hinge", n_negatives=2)
    assert c["prepare_multi"] == c["score_multi"] == c["step"] > 0 and c["sorted"] == 0
    assert any(not np.array_equal(other[k], base[k]) for k in base)


def _reseeded(model, seed):
    model.seed = seed
    return model
