# -*- coding: utf-8 -*-
"""Every table-indexing kernel at row offsets beyond 32 bits.  A kernel addresses a row as table + row * D; a table of
large_tables.n_rows_for(D) fp32 rows (2^31 elements and 4099 rows more, about 8.6 GB) passes the three places where a
narrowed offset goes wrong (a signed and an unsigned 32-bit byte offset, a signed 32-bit element offset: the bands b1,
b2, b3 of tests/large_tables.py; tests/test_large_tables_host.py shows that ids from band_rows make each narrowing
visible on exactly its bands).

Every case follows one pattern: ids from large_tables.band_rows (every band, both sides of every boundary, row 0 and
the last row — asserted on the id set); the kernel runs on the large table, filled with device-generated random values
everywhere (a read that wraps lands on a row with other contents); the family's existing float64 reference runs on the
COMPACTED rows (referenced rows -> small dense table, ids remapped); the comparison is the criterion of the family's
existing small-shape test, named at each use — no tolerance is new here; where the call writes a table, every row the
ids do not name is bit-identical (per-row checksums); the error flag ends at 0.  Only the table under test is large,
at two widths: 64 (16-byte lanes) and 10 (the scalar-tail path); Linear's flag step runs at its own 32.

Out of scope: the unsigned 32-bit ELEMENT band (2^32 elements and more, 17 GB per table: beyond any shape the project
documents), and 1-wide tables as the table under test (they reach b1 only from 2^29 rows on; the 1-wide user tables
here have the large table's row count and are checked for untouched rows, but stay in b0).
Not here either: the coalescing rules rows_apply_sparse_adam / rows_apply_adagrad (table, accumulator and moments: four
large tables).

Cases; N(w) = n_rows_for(w) rows, Dp = the folded row width (64 -> 64, 10 -> 16); seconds per test on an MI355X:
  1  flag mode, 3 forms x (fm 64, linear 32, fm 10)    user (N(D), D) + (N(D), 1)                         0.1 - 0.8
     trs_epoch_flags_ordered, trs_train_steps_sgd (K1, flagged_update_kernel, one-launch form, flag_step.hip)
  2  presorted step, SparseAdam / Adagrad              user tables and their 1 - 2 state tables, (N(D), D)  0.1 - 0.3
     trs_epoch_presort, trs_epoch_user_dups, trs_train_steps_sgd with a trs_opt
  3  staged kernels (B = 257, K = 3)                   user side (N(D), D), or item side for multineg / l2  < 0.1
     trs_score_multi_fwd_bwd, trs_score_warp_fwd_bwd, trs_stage_add_l2, trs_batch_prepare_mined, trs_softmax_stage /
     _rows / _grads, trs_rows_scatter_add          (the tables are built once per side and width: 1.7 s)
  4  fold-ins                              item table (N(Dp), D) + fold (N(Dp), Dp + 1); user (N(D), D)  0.1 - 0.9
     trs_item_fold, trs_fold_in_users, trs_fold_in_items
  5  ALS                                               (N(D), D) as `other`, as rows_inout, under trs_als_gram
     trs_als_solve, trs_als_gram                                                                 < 0.2; Gram < 2
  6  retrieval, 45 queries, k = 10         item table (N(Dp), D) + fold; user table (N(Dp), D) + fold     0.1 - 2.4
     trs_item_fold, trs_retrieve_topk, trs_item_ranks, trs_neighbour_fold, trs_neighbours_topk, trs_mmr_rerank,
     trs_list_ild
  7  through a model (FM, 64)              user (N(64), 64) + (N(64), 1), and similar_users' fold of it   9, mostly the build
     fit (trs_batch_prepare_multi, trs_score_multi_fwd_bwd, trs_stage_add_l2, the staged tail), recommend, rank_items,
     fold_in_items, similar_users: the host-side id arithmetic of model.py, ops.py and evaluate/"""
import numpy as np
import pytest
import torch

import als_ref
import foldin_items_ref
import foldin_ref
import l2_ref
import large_tables as lt
import mining_ref
import mmr_ref
import multineg_ref
import neighbours_ref
import test_gpu_als as AL
import test_gpu_foldin as FU
import test_gpu_foldin_items as FI
import test_gpu_kernels as K
import test_gpu_l2 as L2
import test_gpu_mining as MI
import test_gpu_multineg as MN
import test_gpu_softmax as SX
import test_gpu_warp as WP
import warp_ref
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDE, TAIL = 64, 10  # tests/row_shapes.py: (4, 16, 1) at its largest width, (1, 16, 1) between its two
TOL = MN.TOL         # 1e-5, the bar of tests/test_gpu_multineg.py, test_gpu_warp.py and test_gpu_mining.py


def _ops():
    from torchrecsys_amd import ops
    return ops


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32))).to(DEV)


# ------------------------------------------------------------------------------------ 1. the flag step and its siblings
@pytest.mark.parametrize("net,D,skew", [("fm", WIDE, True), ("linear", 32, True), ("fm", TAIL, True)])
@pytest.mark.parametrize("one_launch", [False, True, "ordered"])
def test_flag_mode_on_a_large_user_table(net, D, skew, one_launch, tune):
    """trs_epoch_flags(_ordered) + trs_train_steps_sgd in flag mode (K1 + flagged_update_kernel; the one-launch form of
    csrc/fast_step.hip; csrc/flag_step.hip for "ordered") on user tables of n_rows_for(D) rows: test_flag_mode_matches_
    oracle's check (tables, triples, step size, oracle and sens.criterion_for(case) unchanged) with the users that occur
    at band_rows, random rows everywhere else, and every other row of both user tables bit-identical afterwards."""
    K.check_flag_mode(net, D, skew, lt.n_rows_for(D), one_launch, tune, bands=True)


# ------------------------------------------------------------------------------------ 2. presorted step, adaptive rules
@pytest.mark.parametrize("net,D,skew", [("fm", WIDE, False), ("fm", TAIL, True)])
@pytest.mark.parametrize("kind", ["sparse_adam", "adagrad"])
def test_presorted_adaptive_rules_on_a_large_user_table(net, D, skew, kind):
    """trs_epoch_presort + trs_epoch_user_dups + the presorted two-launch step with SparseAdam / Adagrad (csrc/rows.hip,
    csrc/opt_rows.h): the user tables AND their state tables have n_rows_for(D) rows, the 300 users sit at band_rows.
    Reference and criteria: test_presorted_adaptive_rules_match_the_oracle's (oracle/optim.py on the compacted rows,
    the same bulk / 3e-5 / 1e-3 bars), plus untouched rows of parameters and state."""
    K.check_presorted_adaptive_rules(net, D, skew, kind, bands=True)


# ------------------------------------------------------------------------------------ 3. the staged per-step kernels
SIDES = [("fm", WIDE), ("linear", TAIL)]
B_STAGED, K_STAGED, N_SMALL = 257, 3, 60


def cover(rs, n, size):
    """`size` ids below n in random order, every id at least once."""
    assert size >= n
    a = np.concatenate([np.arange(n), rs.randint(0, n, size - n)])
    rs.shuffle(a)
    return a


class OneLargeSide:
    """Linear / FM tables (no metadata) whose user side or item side has n_rows_for(D) rows — the D-wide table and the
    1-wide table of that side, N(0, 0.3) and N(0, 0.1) as build_net of tests/test_gpu_multineg.py draws them — and
    N_SMALL rows on the other side.  rows: band_rows on the large side; P: the tables compacted to those rows, by
    state_dict name; the ids a test uses are COMPACT ids (positions in rows) mapped through actual()."""

    def __init__(self, net, D, side, per_band):
        self.net, self.D, self.side, self.N = net, D, side, lt.n_rows_for(D)
        self.rows = lt.band_rows(self.N, D, per_band, seed=D + (side == "item"))
        lt.assert_covers(self.rows, self.N, D)
        rs = np.random.RandomState(D)
        lu, li = multineg_ref.lin_names(net)
        self.names = ("user.weight", "item.weight", lu, li)
        self.large = ("user.weight", lu) if side == "user" else ("item.weight", li)
        self.t = {}
        for n_, k in enumerate(self.names):
            w, scale = (D, 0.3) if k in ("user.weight", "item.weight") else (1, 0.1)
            if k in self.large:
                self.t[k] = lt.fill(torch.empty((self.N, w), device=DEV), seed=100 * D + n_, scale=scale)
            else:
                self.t[k] = torch.from_numpy(rs.normal(0, scale, (N_SMALL, w)).astype(np.float32)).to(DEV)
        self.T, self.keep = _ops().make_tables(*(self.t[k] for k in self.names))
        self.P = {k: lt.gather_small(v, self.rows) if k in self.large else v.cpu().numpy() for k, v in self.t.items()}
        self.sums = {k: lt.row_checksums(self.t[k]) for k in self.large}
        self.nu = self.rows.size if side == "user" else N_SMALL
        self.ni = self.rows.size if side == "item" else N_SMALL
        self.err = torch.zeros(1, dtype=torch.int32, device=DEV)

    def blocks(self, seed, B=B_STAGED, K=K_STAGED):
        """COMPACT ids user (B,), items (1 + K, B).  The large side names every one of its rows; the candidate slots hold
        an item repeated in every second row and a slot repeated inside every row (forced_rows of tests/test_gpu_
        multineg.py), never their row's positive."""
        rs = np.random.RandomState(seed)
        user = cover(rs, self.nu, B) if self.side == "user" else rs.randint(0, self.nu, B)
        items = rs.randint(0, self.ni, (1 + K, B))
        if self.side == "item":
            items[0] = cover(rs, self.ni, B)
        items[1:, ::2] = 5
        items[2] = items[1]
        clash = items[1:] == items[0][None, :]
        items[1:][clash] = (items[0][None, :].repeat(K, 0)[clash] + 1) % self.ni
        named = user if self.side == "user" else items
        assert np.unique(named).size == self.rows.size  # every band row is named: the ids cover what self.rows covers
        return user, items

    def actual(self, user, items):
        """The compact ids as rows of the tables: int32 device blocks."""
        if self.side == "user":
            return dev32(self.rows[user]), dev32(items)
        return dev32(user), dev32(self.rows[items])

    def done(self):
        """Every case ends here: the error flag is 0 and every row of the large tables is as it was filled."""
        torch.cuda.synchronize()
        assert self.err.item() == 0
        for k in self.large:
            lt.assert_untouched(self.sums[k], lt.row_checksums(self.t[k]), [], k)

    def free(self):
        self.t.clear()
        self.sums.clear()
        self.T = self.keep = None
        torch.cuda.empty_cache()


def check_multineg(s, loss):
    """trs_score_multi_fwd_bwd against multineg_ref.staged on the compacted rows.  Criteria: test_sampled_softmax_
    matches_the_float64_oracle (loss and every table's staged block, D-wide and 1-wide, at TOL; the user's 1-wide
    gradient exactly 0) and, for the mean of K pairs, the restatement lines of test_mean_of_k_pairs_matches_k_calls_of_
    the_pair_kernel (loss and the D-wide blocks at TOL), both of tests/test_gpu_multineg.py."""
    B, Kn, tau = B_STAGED, K_STAGED, 1.0
    user_c, items_c = s.blocks(seed=3)
    user, items = s.actual(user_c, items_c)
    loss_sum = torch.zeros(1, device=DEV)
    auc = torch.zeros(1, dtype=torch.int32, device=DEV)
    gr, gl = _ops().score_multi_fwd_bwd(s.net, s.T, user, items, None, MN.loss_id(loss), tau, loss_sum, auc, err_flag=s.err)
    torch.cuda.synchronize()
    want_loss, wr, wl, _ = multineg_ref.staged(s.net, s.P, user_c, items_c, None, loss, tau)
    got, gr, gl = loss_sum.item() / B, gr.cpu().numpy(), gl.cpu().numpy()
    assert gr.shape == wr.shape == (multineg_ref.n_fields(Kn, 0), B, s.D)
    for sl in MN.table_blocks(Kn, 0):
        print(f"{loss} fields {sl.start}..{sl.stop - 1}: rows {rel_err(gr[sl], wr[sl]):.2e} 1-wide {rel_err(gl[sl], wl[sl]):.2e}")
    assert abs(got - want_loss) <= TOL * abs(want_loss), (got, want_loss)
    for sl in MN.table_blocks(Kn, 0):
        assert rel_err(gr[sl], wr[sl]) <= TOL, sl
        if loss == MN.SM:
            assert rel_err(gl[sl], wl[sl]) <= TOL, sl
    if loss == MN.SM:
        assert not gl[0].any()
    s.done()
    return user_c, user, gr


def check_l2(s):
    """trs_stage_add_l2 on pre-filled staging buffers against l2_ref.staged_add in float64; criterion: within_two_
    roundings of test_every_layout_against_float64 (tests/test_gpu_l2.py), coefficients as there."""
    B, S = B_STAGED, 1 + K_STAGED
    user_c, items_c = s.blocks(seed=5)
    user, items = s.actual(user_c, items_c)
    _, _, gr, gl = L2.random_staging(np.random.RandomState(6), 1 + S, B, s.D)
    g0, l0 = gr.cpu().numpy(), gl.cpu().numpy()
    coefs = (0.3 / B, 0.2 / B, 0.1 / B)
    _ops().stage_add_l2(s.net, s.T, user, items, None, coefs, gr, gl, s.err)
    torch.cuda.synchronize()
    want_r, want_l, mag_r, mag_l = l2_ref.staged_add(s.net, s.P, user_c, items_c, None, coefs, g0, l0)
    got_r, got_l = gr.cpu().numpy(), gl.cpu().numpy()
    ok_r, worst_r = L2.within_two_roundings(got_r, want_r, mag_r)
    ok_l, worst_l = L2.within_two_roundings(got_l, want_l, mag_l)
    print(f"rows {worst_r / 2.0 ** -22:.3f} 1-wide {worst_l / 2.0 ** -22:.3f} of the bound")
    assert ok_r and ok_l
    assert not np.array_equal(got_r[0], g0[0]) and not np.array_equal(got_r[1:], g0[1:]) and not np.array_equal(got_l, l0)
    s.done()


class TestStagedKernels:
    """The tables of a side and width are built once for the tests that read them, and freed before the next ones are
    built; nothing of them is left when the class is done."""

    @pytest.fixture(scope="class", params=SIDES, ids=lambda p: f"{p[0]}-{p[1]}")
    def user_side(self, request):
        """72 users at band_rows of a large user table: B_STAGED = 257 rows name each of them."""
        s = OneLargeSide(*request.param, "user", 16)
        yield s
        s.free()

    @pytest.fixture(scope="class", params=SIDES, ids=lambda p: f"{p[0]}-{p[1]}")
    def item_side(self, request):
        """248 items at band_rows of a large item table: the 257 positives name each of them."""
        s = OneLargeSide(*request.param, "item", 60)
        yield s
        s.free()

    @pytest.mark.parametrize("loss", ["hinge", "bpr", MN.SM])
    def test_multineg_staging_on_a_large_user_table(self, user_side, loss):
        check_multineg(user_side, loss)

    def test_warp_staging_on_a_large_user_table(self, user_side):
        """trs_score_warp_fwd_bwd against warp_ref.staged; the criteria of test_random_tables_match_the_float64_restatement
        (tests/test_gpu_warp.py): rows near a tie left out (at most 1 % of them, from the reference alone), trials and the
        chosen negative exactly, the loss and every table's fields at TOL, the user's 1-wide gradient exactly 0."""
        s, B, Kn, margin = user_side, B_STAGED, K_STAGED, 0.25
        user_c, items_c = s.blocks(seed=4)
        user, items = s.actual(user_c, items_c)
        weights = warp_ref.rank_weights(N_SMALL, Kn, "log")
        ref = warp_ref.staged(s.net, s.P, user_c, items_c, None, margin, weights)
        skip, tr = warp_ref.near_ties(ref["z"], margin, TOL), ref["trials"]
        assert skip.sum() <= 0.01 * B and (tr == 0).any() and (tr > 0).any()
        loss_sum = torch.zeros(1, device=DEV)
        w = torch.from_numpy(weights.astype(np.float32)).to(DEV)
        neg, _, trials, gr, gl = _ops().score_warp_fwd_bwd(s.net, s.T, user, items, None, margin, w, loss_sum, err_flag=s.err)
        torch.cuda.synchronize()
        keep = ~skip
        g_tr, g_neg = trials.cpu().numpy(), neg.cpu().numpy()
        assert np.array_equal(g_tr[keep], tr[keep]) and np.array_equal(g_neg[keep], ref["neg"][keep])
        Jd = g_tr[skip] - 1
        own = np.where(Jd >= 0, weights[np.maximum(Jd, 0)] * ref["h"][skip, np.maximum(Jd, 0)], 0.0)
        want_loss = ref["row_loss"][keep].sum() + own.sum()
        assert abs(loss_sum.item() - want_loss) <= TOL * want_loss
        gr, gl = gr.cpu().numpy(), gl.cpu().numpy()
        for fields in WP.table_fields(0):
            print(f"fields {fields}: rows {rel_err(gr[fields][:, keep], ref['gr'][fields][:, keep]):.2e}")
            assert rel_err(gr[fields][:, keep], ref["gr"][fields][:, keep]) <= TOL, fields
            assert rel_err(gl[fields][:, keep], ref["gl"][fields][:, keep]) <= TOL, fields
        assert not gl[0].any()
        s.done()

    def test_l2_staging_on_a_large_user_table(self, user_side):
        check_l2(user_side)

    def test_mining_on_a_large_user_table(self, user_side):
        """trs_batch_prepare_mined scoring 8 candidates per triple under the large user table, against mining_ref.mined_
        batch on the compacted rows; the rule of test_float_tables_mine_the_float64_argmax_item (tests/test_gpu_mining.py):
        users and positives exactly, the mined item the float64 arg-max or within TOL * max|z| of it, for at most
        NEAR_TIE_CAP of the triples — none of 257.  So that this is a statement about the kernel, the INPUT is held to a
        condition taken from the float64 reference alone: the sampler seed is the first under which every triple's best two
        candidate values are 10 * TOL * max|z| apart — ten times the rule's own near-tie band — or are the same item."""
        s, B, Kc, key = user_side, B_STAGED, 8, 0x77AA1
        rs = np.random.RandomState(7)
        su_c, si = cover(rs, s.nu, B), rs.randint(0, s.ni, B)  # a stream of B rows: the batch is a permutation of all of it
        for seed in range(31, 47):
            ref = mining_ref.mined_batch(su_c, si, key, 0, B, s.ni, seed, 0, s.net, s.P, Kc, 1, {"k": 1, "max_tries": 8})
            order = np.argsort(-ref["z"], axis=1, kind="stable")[:, :2]
            top2 = np.take_along_axis(ref["z"], order, axis=1)
            same = np.take_along_axis(ref["cand"], order, axis=1)
            if ((top2[:, 0] - top2[:, 1] > 10 * TOL * np.abs(ref["z"]).max()) | (same[:, 0] == same[:, 1])).all():
                break
        else:
            raise AssertionError("no sampler seed keeps every triple's best two candidates apart")
        assert np.unique(ref["user"]).size == s.rows.size
        ops = _ops()
        su_d, si_d = dev32(s.rows[su_c]), dev32(si)
        sampler = ops.Sampler(k=1, stream_item=si_d, max_tries=8, mine="hardest", candidates=Kc, top=1)
        out = ops.batch_prepare_mined(su_d, si_d, key, 0, B, s.ni, seed, 0, s.net, s.T, sampler, None, return_chosen=True)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        assert np.array_equal(got["user"], s.rows[ref["user"]]) and np.array_equal(got["pos"], ref["pos"])
        n = MI.check_near_ties(got["neg"], ref, f"{s.net} D={s.D}")
        assert n <= MI.NEAR_TIE_CAP * B, n
        cand_of_chosen = np.take_along_axis(ref["cand"], got["chosen"][:, None].astype(np.int64), axis=1)[:, 0]
        assert np.array_equal(cand_of_chosen, got["neg"])
        s.done()

    def test_in_batch_softmax_on_a_large_user_table(self, user_side):
        """trs_softmax_stage / trs_softmax_rows / trs_softmax_grads (ops.InBatchSoftmax) against the float64 autograd oracle
        of tests/test_gpu_softmax.py, with test_one_sgd_step_matches_autograd's step size and criteria applied to the step
        the staged rows describe: loss at 1e-5, every table after the step at 1e-5, the step itself at 1e-3, the user-side
        1-wide gradient exactly 0."""
        s, B, tau, lr = user_side, B_STAGED, 1.0, 0.5
        ops = _ops()
        _, p, pm = SX.make_batch(B, s.nu, s.ni, 0, seed=8)
        u_c = cover(np.random.RandomState(8), s.nu, B)
        user, pos = dev32(s.rows[u_c]), dev32(p)
        Bt, keep = ops.make_batch(user, pos, pos, err_flag=s.err)
        gr, gl = torch.empty((2, B, s.D), device=DEV), torch.empty((2, B), device=DEV)
        loss_sum = torch.zeros(1, device=DEV)
        ops.InBatchSoftmax(B, s.D, DEV)(s.net, s.T, Bt, tau, None, loss_sum, gr, gl)
        torch.cuda.synchronize()
        W0 = [s.P[k].astype(np.float64) for k in s.names]
        ref_loss, grads = SX.oracle(s.net, W0, 0, u_c, p, pm, tau, None)
        assert abs(loss_sum.item() / B - ref_loss) <= 1e-5 * max(abs(ref_loss), 1e-6), (loss_sum.item() / B, ref_loss)
        gr, gl = gr.cpu().numpy().astype(np.float64), gl.cpu().numpy().astype(np.float64)
        for k, (ids, staged) in enumerate(((u_c, gr[0]), (p, gr[1]), (u_c, gl[0][:, None]), (p, gl[1][:, None]))):
            G = np.zeros(W0[k].shape)
            np.add.at(G, ids, staged)
            print(f"{s.names[k]}: table {rel_err(W0[k] - lr * G, W0[k] - lr * grads[k]):.2e}")
            assert rel_err(W0[k] - lr * G, W0[k] - lr * grads[k]) <= 1e-5, k
            if np.abs(grads[k]).max() > 0:
                assert rel_err(-lr * G, -lr * grads[k]) <= 1e-3, k
        assert not gl[0].any()
        s.done()

    def test_staged_rows_scatter_into_a_large_user_table(self, user_side):
        """trs_rows_scatter_add of the sampled softmax's staged user rows into the large user table (the tail of a staged
        SGD step: tests/test_staged_tail.py), alpha = -B so that the step is as large as the rows it lands on.  Criterion:
        test_row_optimisers_int32_ids_strided_values_and_ids_out_of_range's 1e-6 norm-wise on the scattered rows against
        the float64 sum of the same staged values — at most 16 references per row here, 16 roundings of 2^-24 — and every
        other row bit-identical.  The rows are put back afterwards (checked: the whole table has its first checksums)."""
        s, B = user_side, B_STAGED
        user_c, user, gr = check_multineg(s, MN.SM)
        assert np.bincount(user_c).max() <= 16
        table = s.t["user.weight"]
        rows_t = torch.from_numpy(s.rows).to(DEV)
        saved = table[rows_t].clone()
        _ops().rows_scatter_add(table, user, torch.from_numpy(gr[0]).to(DEV), -float(B), err_flag=s.err)
        torch.cuda.synchronize()
        want = s.P["user.weight"].astype(np.float64)
        np.add.at(want, user_c, -float(B) * gr[0].astype(np.float64))
        got = table[rows_t].cpu().numpy()
        print(f"scattered rows {rel_err(got, want):.2e}, the step {rel_err(got - s.P['user.weight'], want - s.P['user.weight']):.2e}")
        assert rel_err(got, want) < 1e-6
        assert np.abs(want - s.P["user.weight"]).max() > 0.01 * np.abs(want).max()  # (the step is no rounding matter)
        lt.assert_untouched(s.sums["user.weight"], lt.row_checksums(table), s.rows, "user.weight")
        assert s.err.item() == 0
        table[rows_t] = saved
        s.done()

    @pytest.mark.parametrize("loss", ["hinge", "bpr", MN.SM])
    def test_multineg_staging_on_a_large_item_table(self, item_side, loss):
        check_multineg(item_side, loss)

    def test_l2_staging_on_a_large_item_table(self, item_side):
        check_l2(item_side)


# ------------------------------------------------------------------------------------ 4. the fold-ins
FOLD_E, FOLD_LR, FOLD_L2, FOLD_SEED = 4, 0.05, 2.0 ** -3, 7  # test_smooth_losses_against_float64 of both fold-in modules
FOLD_PER_BAND = 48  # 200 rows: N_ITEMS of tests/test_gpu_foldin.py, N_USERS of tests/test_gpu_foldin_items.py


def fold_close(got, want, tol, what):
    """test_smooth_losses_against_float64's criterion (atol = rtol = the module's TOL)."""
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print(f"{what}: max |got - float64| = {err.max():.3g} (TOL {tol:.3g})")
    assert np.all(err <= tol + tol * np.abs(want)), (what, err.max())


def _csr_dev(lists):
    off, ids = als_ref.csr(lists)
    return torch.from_numpy(off).to(DEV), dev32(ids)


@pytest.mark.parametrize("D", [WIDE, TAIL])
def test_item_fold_and_fold_in_users_on_a_large_catalogue(D):
    """trs_item_fold writing, and trs_fold_in_users reading, an item fold of n_rows_for(Dp) rows (Dp: the fold's padded
    row width), Linear without metadata.  The fold: on band_rows its rows are the item rows, bit for bit, zero in the
    padding columns, its constants the item biases (without metadata that is the fold's definition, include/trs.h).
    The fold-in: the histories of tests/test_gpu_foldin.py (HISTS: lengths 0, 1, 2, 63, 64, 65, 150, 199, 200, then
    random) over the 200 band_rows items; its negatives are drawn over the whole catalogue, and they are known — the
    reference's own schedule (foldin_ref.schedules) on the real ids — so the compacted table holds the band rows and
    every negative, and the schedule, remapped, is handed to foldin_ref.fold_in through its schedule cache.  Case
    (Linear, BPR, lr, l2, epochs) and criterion: test_smooth_losses_against_float64, TOL of tests/test_gpu_foldin.py.
    The fold is only read by the fold-in: its rows are bit-identical afterwards."""
    ops = _ops()
    Dp = 16
    while Dp < D:
        Dp *= 2
    N = lt.n_rows_for(Dp)
    rows = lt.band_rows(N, Dp, FOLD_PER_BAND, seed=D + 8)
    hists = [np.asarray(h, dtype=np.int64) for h in FU.HISTS]
    assert rows.size == FU.N_ITEMS and max(h.size for h in hists) == rows.size  # (one history names every band row)
    lt.assert_covers(rows, N, Dp)
    item = lt.fill(torch.empty((N, D), device=DEV), seed=D + 9)
    item_bias = lt.fill(torch.empty((N, 1), device=DEV), seed=D + 10)
    T, keep = ops.make_tables(torch.zeros((1, D), device=DEV), item, torch.zeros((1, 1), device=DEV), item_bias)
    fold = ops.item_fold("linear", T, N, D, DEV)
    torch.cuda.synchronize()
    S, c = ops.fold_views(fold, N, D)
    assert S.shape == (N, Dp)
    rows_t = torch.from_numpy(rows).to(DEV)
    assert torch.equal(S[rows_t][:, :D], item[rows_t]) and not bool(S[rows_t][:, D:].any())
    assert torch.equal(c[rows_t], item_bias[rows_t, 0])
    del item, item_bias, T, keep  # (the fold-in reads the fold alone)
    sums = lt.row_checksums(ops.fold_rows(fold, N))
    kw = dict(seed=FOLD_SEED, shuffle=True, reject_seen=True, max_tries=8)
    real = [rows[h] for h in hists]
    sched = foldin_ref.schedules(real, N, FOLD_E, kw["seed"], kw["shuffle"], kw["reject_seen"], kw["max_tries"])
    used, _ = lt.compact([rows] + [n for sc in sched for (_, _, n) in sc])
    small = [np.searchsorted(used, h) for h in real]
    key = (tuple(h.astype(np.int64).tobytes() for h in small), int(used.size), FOLD_E, kw["seed"], True, True, 8)
    foldin_ref._SCHEDULES[key] = [[(r, np.searchsorted(used, p), np.searchsorted(used, n)) for (r, p, n) in sc]
                                  for sc in sched]
    used_t = torch.from_numpy(used).to(DEV)
    want = foldin_ref.fold_in(S[used_t].cpu().numpy().astype(np.float64), c[used_t].cpu().numpy().astype(np.float64),
                              small, "linear", "bpr", FOLD_E, FOLD_LR, FOLD_L2, D=D, **kw)
    del foldin_ref._SCHEDULES[key]
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    U, b, ls = ops.fold_in_users("linear", fold, N, D, _csr_dev(real), "bpr", FOLD_E, FOLD_LR, FOLD_L2, kw["seed"], True,
                                 True, 8, want_loss=True, err_flag=err)
    torch.cuda.synchronize()
    for name, got in (("U", U), ("b", b), ("loss", ls)):
        fold_close(got, want[name], FU.TOL, f"D={D} {name}")
    assert np.abs(want["U"]).max() > 0.05  # the rows moved
    lt.assert_untouched(sums, lt.row_checksums(ops.fold_rows(fold, N)), [], "the item fold")
    assert err.item() == 0


@pytest.mark.parametrize("D", [WIDE, TAIL])
def test_fold_in_items_on_a_large_user_table(D):
    """trs_fold_in_items reading a user table (and user-bias table) of n_rows_for(D) rows: the histories of tests/test_
    gpu_foldin_items.py (HISTS, over 200 users) made of band_rows users, Linear + BPR without metadata, no negative
    visits and no seen rejection (the positive visits' catalogue items then depend on a history's length alone, so the
    reference runs on the compacted user rows as it is).  Criterion: test_smooth_losses_against_float64, TOL of tests/
    test_gpu_foldin_items.py.  The user tables are only read: bit-identical afterwards."""
    from torchrecsys_amd import _lib
    ops = _ops()
    N, n_items = lt.n_rows_for(D), FI.N_ITEMS
    rows = lt.band_rows(N, D, FOLD_PER_BAND, seed=D + 11)
    hists = [np.asarray(h, dtype=np.int64) for h in FI.HISTS]
    assert rows.size == FI.N_USERS and max(h.size for h in hists) == rows.size  # (one history names every band row)
    lt.assert_covers(rows, N, D)
    user = lt.fill(torch.empty((N, D), device=DEV), seed=D + 12)
    user_bias = lt.fill(torch.empty((N, 1), device=DEV), seed=D + 13)
    sums = [lt.row_checksums(user), lt.row_checksums(user_bias)]
    rs = np.random.RandomState(D)
    item = torch.from_numpy((0.3 * rs.randn(n_items, D)).astype(np.float32)).to(DEV)
    item_bias = torch.from_numpy((0.3 * rs.randn(n_items, 1)).astype(np.float32)).to(DEV)
    T, keep = ops.make_tables(user, item, user_bias, item_bias)
    fold = ops.item_fold("linear", T, n_items, D, DEV)
    n_new = len(hists)
    new_fold = torch.zeros(_lib.load().trs_item_fold_bytes(n_new, D), dtype=torch.uint8, device=DEV)  # no metadata part
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    V, b, ls = ops.fold_in_items("linear", T, fold, n_items, new_fold, _csr_dev([rows[h] for h in hists]), None, None,
                                 None, "bpr", FOLD_E, FOLD_LR, FOLD_L2, 0, FOLD_SEED, True, False, 0, want_loss=True,
                                 err_flag=err)
    torch.cuda.synchronize()
    f64 = lambda t: t.cpu().numpy().astype(np.float64)
    S, c = ops.fold_views(fold, n_items, D)
    Tn, kappa = ops.fold_views(new_fold, n_new, D)
    none = np.zeros(0, dtype=np.int64)
    want = foldin_items_ref.fold_in(lt.gather_small(user, rows), lt.gather_small(user_bias, rows)[:, 0], f64(S), f64(c),
                                    f64(Tn), f64(kappa), hists, none, none, None, "linear", "bpr", FOLD_E, FOLD_LR,
                                    FOLD_L2, nu=0, seed=FOLD_SEED, shuffle=True, reject_seen=False, max_tries=0)
    for name, got in (("V", V), ("b", b), ("loss", ls)):
        fold_close(got, want[name], FI.TOL, f"D={D} {name}")
    assert np.abs(want["V"]).max() > 0.05  # the rows moved
    lt.assert_untouched(sums[0], lt.row_checksums(user), [], "the user table")
    lt.assert_untouched(sums[1], lt.row_checksums(user_bias), [], "the user biases")
    assert err.item() == 0


# ------------------------------------------------------------------------------------ 5. implicit ALS
ALS_ALPHA, ALS_LAMBDA, ALS_CG, ALS_TOL = AL.CASES["a10_l0.1_cg3"]  # tests/test_gpu_als.py: atol = rtol = 8 x 1.82e-6
ALS_PER_BAND = 28  # 120 rows, the catalogue size of tests/test_gpu_als.py (HISTS)


def als_close(got, want, what):
    """test_one_half_sweep_against_float64's criterion."""
    err = np.abs(got.astype(np.float64) - want)
    print(f"{what}: max |got - float64| / (1 + |float64|) = {(err / (1 + np.abs(want))).max():.3g} (TOL {ALS_TOL:.3g})")
    assert np.all(err <= ALS_TOL + ALS_TOL * np.abs(want)), (what, err.max())


@pytest.mark.parametrize("D", [WIDE, TAIL])
def test_als_solve_against_a_large_frozen_table(D):
    """trs_als_solve with the large table as `other`: 70 rows solved, their neighbour lists (lengths 0, 1, 2, 63, 64, 65,
    119, 120, then random, as HISTS of tests/test_gpu_als.py) made of band_rows rows.  The Gram matrix handed in is
    that of the compacted rows (ops.als_gram of them), so the float64 reference is als_ref.half_sweep on the compacted
    table as it stands; parameters and criterion: test_one_half_sweep_against_float64's first case.  `other` is only
    read: every row bit-identical afterwards."""
    ops = _ops()
    N = lt.n_rows_for(D)
    rows = lt.band_rows(N, D, ALS_PER_BAND, seed=D + 2)
    n = rows.size
    lists = als_ref.random_lists(70, n, D, (0, 1, 2, 63, 64, 65, n - 1, n))
    lt.assert_covers(rows[np.unique(np.concatenate(lists))], N, D)
    other = lt.fill(torch.empty((N, D), device=DEV), seed=D + 3)  # (als_ref.tables: 0.3 * randn)
    sums = lt.row_checksums(other)
    Y = lt.gather_small(other, rows)
    X = als_ref.tables(70, 1, D, D)[0]
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    G = ops.als_gram(torch.from_numpy(Y).to(DEV))
    off, ids = als_ref.csr([rows[h] for h in lists])
    Xd = torch.from_numpy(X.copy()).to(DEV)
    ops.als_solve(other, G, (torch.from_numpy(off).to(DEV), dev32(ids)), ALS_LAMBDA, ALS_ALPHA, ALS_CG, Xd, err)
    torch.cuda.synchronize()
    want = als_ref.half_sweep(X, Y, lists, ALS_LAMBDA, ALS_ALPHA, ALS_CG)
    als_close(Xd.cpu().numpy(), want, f"D={D}")
    assert np.abs(want - X).max() > 0.05  # the rows moved
    lt.assert_untouched(sums, lt.row_checksums(other), [], "the frozen table")
    assert err.item() == 0


@pytest.mark.parametrize("D", [WIDE, TAIL])
def test_als_solve_of_rows_of_a_large_table(D):
    """trs_als_solve with the large table as rows_inout: the band_rows rows have neighbour lists over a frozen table of
    120 rows, every other row an empty list.  The solved rows against als_ref.half_sweep (same case and criterion as
    above).  A row with an empty list is not left alone: its solution is 0 (test_empty_lists_give_zero_rows_... of
    tests/test_gpu_als.py), so instead of bit-identical rows the check is that EVERY row outside band_rows is zero —
    a solved row written to a wrapped address would leave non-zero values there, and a zero in its own place."""
    ops = _ops()
    N = lt.n_rows_for(D)
    rows = lt.band_rows(N, D, ALS_PER_BAND, seed=D + 4)
    lt.assert_covers(rows, N, D)
    n = rows.size
    lists = als_ref.random_lists(n, n, D + 1, (1, 2, 63, 64, 65, n - 1, n))
    lists = [h if h.size else np.array([k % n], np.int32) for k, h in enumerate(lists)]  # no empty list among them
    Y = als_ref.tables(1, n, D, D + 1)[1]
    Yd = torch.from_numpy(Y).to(DEV)
    table = lt.fill(torch.empty((N, D), device=DEV), seed=D + 5)
    rows_t = torch.from_numpy(rows).to(DEV)
    X = table[rows_t].cpu().numpy()
    lens = torch.zeros(N + 1, dtype=torch.int64, device=DEV)
    lens[rows_t + 1] = torch.tensor([h.size for h in lists], device=DEV)
    off = torch.cumsum(lens, 0)
    del lens
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.als_solve(Yd, ops.als_gram(Yd), (off, dev32(np.concatenate(lists))), ALS_LAMBDA, ALS_ALPHA, ALS_CG, table, err)
    torch.cuda.synchronize()
    want = als_ref.half_sweep(X, Y, lists, ALS_LAMBDA, ALS_ALPHA, ALS_CG)
    got = table[rows_t].cpu().numpy()
    als_close(got, want, f"D={D}")
    assert np.abs(want - X).max() > 0.05 and (np.abs(want).max(axis=1) > 0).all()
    nonzero_rows = sum(int((table[lo:hi] != 0).any(dim=1).sum()) for lo, hi in lt._row_chunks(table))
    assert nonzero_rows == n, (nonzero_rows, n)
    assert err.item() == 0


@pytest.mark.parametrize("D", [WIDE, TAIL])
def test_als_gram_of_a_whole_large_table(D):
    """trs_als_gram over all n_rows_for(D) rows against a float64 Gram matrix summed on the device in row chunks.
    Under the random fill alone a misread row is replaced by a row of the same distribution, which moves G by less than
    fp32 summation does; so the band_rows rows are raised to 10 000 times their size and carry most of every diagonal
    entry.  Criterion: test_gram_matrix_is_symmetric_repeatable_and_close_to_float64's — symmetric, and every entry
    within (number of fp32 additions behind it) * 2^-24 * sum |y_a y_b| — with the count of THIS shape, read from the
    kernel's layout (csrc/als.hip: at most 512 chunks, one fmaf chain over a chunk's rows, the chunk sums added in
    turn) where that test has its 150 rows' 200.  A band whose planted rows were not read moves every diagonal entry
    by a quarter of the planted mass: asserted, from the float64 side alone, to be over 3 bounds (2 for the
    triangle inequality, 1 to spare)."""
    ops = _ops()
    N = lt.n_rows_for(D)
    rows = lt.band_rows(N, D, ALS_PER_BAND, seed=D + 6)
    lt.assert_covers(rows, N, D)
    table = lt.fill(torch.empty((N, D), device=DEV), seed=D + 7)
    rows_t = torch.from_numpy(rows).to(DEV)
    table[rows_t] *= 1.0e4
    want = torch.zeros((D, D), dtype=torch.float64, device=DEV)
    mass = torch.zeros((D, D), dtype=torch.float64, device=DEV)
    def gram64(y, R=4096):  # y^T y in float64, the long dimension cut into a batch (one skinny product is slow)
        m = y.shape[0] // R * R
        blocks = y[:m].view(-1, R, D)
        return torch.bmm(blocks.transpose(1, 2), blocks).sum(dim=0) + y[m:].t() @ y[m:]

    for lo, hi in lt._row_chunks(table):
        y = table[lo:hi].double()
        want += gram64(y)
        mass += gram64(y.abs_())
    del y
    # gram_chunk_rows / gram_chunks of csrc/als.hip restated: THIS MUST TRACK THE KERNEL'S LAYOUT (a longer fmaf chain
    # than counted here would make the bound too tight, a shorter one too loose); the count is rounded up by a quarter,
    # as the small-shape test rounds its 160 additions up to 200
    per_chunk = -(-N // (256 if D > 128 else 512))  # gram_chunk_rows of csrc/als.hip
    chunk_rows = max(16, -(-per_chunk // 16) * 16)
    chunks = -(-N // chunk_rows)
    bound = 1.25 * (chunk_rows + chunks) * 2.0 ** -24 * mass
    planted = table[rows_t].double()
    band = torch.from_numpy(lt.band_of(rows, D)).to(DEV)
    for b in range(lt.N_BANDS):  # the input's condition: each band's planted rows stand out of the bound
        lost = (planted[band == b] ** 2).sum(0)
        assert bool((lost > 3 * bound.diagonal()).all()), b
    G = ops.als_gram(table)
    torch.cuda.synchronize()
    assert torch.equal(G, G.t())
    worst = float(((G.double() - want).abs() / bound).max())
    print(f"D={D}: {chunks} chunks of {chunk_rows} rows, worst entry at {worst:.3g} of its bound")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------ 6. retrieval over a large catalogue
RET_Q, RET_K, RET_G = 45, 10, 8  # queries, k, groups of planted rows (one coordinate axis each: RET_G <= TAIL)


class Catalogue:
    """A Linear scorer over n_rows_for(Dp) items (Dp: the item fold's padded row width) and RET_Q users, with the
    answers planted.  Items and item biases are N(0, 0.01) everywhere; the 4 * RET_K + 8 band_rows rows are overwritten:
    planted row i is s_i e_g, g = i mod RET_G, bias 0, with the strengths 1.0, 1.1, ... dealt at random inside each
    group; user q is e_g + 0.05 N(0, 1), g = q mod RET_G.  A query's best items are then its group's planted rows in the
    order of their strengths, from wherever in the table they sit.  The float64 values (item table and biases as they
    stand, never the fold) are computed on the device in item chunks: the planted columns, and per query the best
    value of all other items."""

    def __init__(self, D):
        ops = _ops()
        self.D, self.Dp = D, 16
        while self.Dp < D:
            self.Dp *= 2
        self.N = N = lt.n_rows_for(self.Dp)
        self.rows = rows = lt.band_rows(N, self.Dp, 4 * RET_K, seed=D + 20)
        lt.assert_covers(rows, N, self.Dp)
        rs = np.random.RandomState(D + 21)
        n = rows.size
        self.group = np.arange(n) % RET_G
        strength = np.empty(n)
        for g in range(RET_G):
            idx = np.flatnonzero(self.group == g)
            strength[idx] = 1.0 + 0.1 * rs.permutation(idx.size)
        planted = np.zeros((n, D), dtype=np.float32)
        planted[np.arange(n), self.group] = strength
        self.rows_t = torch.from_numpy(rows).to(DEV)
        self.item = lt.fill(torch.empty((N, D), device=DEV), seed=D + 22, scale=0.01)
        self.bias = lt.fill(torch.empty((N, 1), device=DEV), seed=D + 23, scale=0.01)
        self.item[self.rows_t] = torch.from_numpy(planted).to(DEV)
        self.bias[self.rows_t] = 0.0
        U = 0.05 * rs.randn(RET_Q, D)
        U[np.arange(RET_Q), np.arange(RET_Q) % RET_G] += 1.0
        self.user = torch.from_numpy(U.astype(np.float32)).to(DEV)
        self.user_bias = torch.from_numpy((0.1 * rs.randn(RET_Q, 1)).astype(np.float32)).to(DEV)
        self.T, self.keep = ops.make_tables(self.user, self.item, self.user_bias, self.bias)
        self.fold = ops.item_fold("linear", self.T, N, D, DEV)
        self.users = torch.arange(RET_Q, dtype=torch.int64, device=DEV)
        # ---- float64, in item chunks
        self.U64, self.ub64 = self.user.double(), self.user_bias.double()
        self.planted = self.values(self.item[self.rows_t], self.bias[self.rows_t]).cpu().numpy()  # (RET_Q, n)
        best = torch.full((RET_Q,), -np.inf, dtype=torch.float64, device=DEV)
        for lo, hi, v in self.chunks():
            inside = self.rows_t[(self.rows_t >= lo) & (self.rows_t < hi)] - lo
            v[:, inside] = -np.inf
            best = torch.maximum(best, v.max(dim=1).values)
        self.best_other = best.cpu().numpy()
        self.tau = 1e-5 * max(1.0, float(np.abs(self.planted).max()), float(np.abs(self.best_other).max()))
        # seen: per user its best and third-best planted row, and 16 rows of every band and boundary for everybody
        common = lt.band_rows(N, self.Dp, 2, seed=D + 24)
        order = np.argsort(-self.planted, axis=1)
        self.seen = [np.unique(np.concatenate([common, rows[order[q, [0, 2]]]])) for q in range(RET_Q)]
        lt.assert_covers(np.concatenate(self.seen), N, self.Dp)

    def values(self, item_rows, bias_rows):
        """(RET_Q, rows) float64 scores <U_q, item> + user_bias_q + item_bias."""
        return self.U64 @ item_rows.double().t() + self.ub64 + bias_rows.double().t()

    def chunks(self, step=1 << 20):
        for lo in range(0, self.N, step):
            hi = min(lo + step, self.N)
            yield lo, hi, self.values(self.item[lo:hi], self.bias[lo:hi])

    def expected(self, q, seen):
        """(ids, float64 values) of query q's candidates among the planted rows, best first, and the condition on the
        input: neighbours in that order, and the last of the first RET_K and everything else, are more than the 2 tau of
        test_random_weights_tolerance_contract (tests/test_ranking.py) apart — from the float64 side alone."""
        ok = ~np.isin(self.rows, self.seen[q]) if seen else np.ones(self.rows.size, bool)
        v, ids = self.planted[q][ok], self.rows[ok]
        order = np.argsort(-v)
        v, ids = v[order], ids[order]
        assert (np.diff(v[:RET_K + 1]) < -2 * self.tau).all() and v[RET_K - 1] > self.best_other[q] + 2 * self.tau
        return ids, v

    def free(self):
        self.item = self.bias = self.fold = self.T = self.keep = self.rank_counts = None
        torch.cuda.empty_cache()


class TestCatalogue:
    @pytest.fixture(scope="class", params=[WIDE, TAIL])
    def catalogue(self, request):
        c = Catalogue(request.param)
        yield c
        c.free()

    def test_item_fold_of_a_large_catalogue(self, catalogue):
        """trs_item_fold: on band_rows the fold's rows are the item rows bit for bit (Linear without metadata: the fold's
        definition), zero in the padding columns, its constants the item biases; likewise on 64 rows next to them."""
        c = catalogue
        S, const = _ops().fold_views(c.fold, c.N, c.D)
        for rows_t in (c.rows_t, (c.rows_t[4:-4:3] + 1)):
            assert torch.equal(S[rows_t][:, :c.D], c.item[rows_t]) and not bool(S[rows_t][:, c.D:].any())
            assert torch.equal(const[rows_t], c.bias[rows_t, 0])

    @pytest.mark.parametrize("seen", [False, True], ids=["all", "unseen"])
    def test_retrieve_topk_over_a_large_catalogue(self, catalogue, seen):
        """trs_retrieve_topk, with and without a seen CSR whose entries lie in every band: the ids are the planted order,
        the scores within tau = 1e-5 max(1, max|v|) of the float64 values (test_random_weights_tolerance_contract)."""
        c = catalogue
        csr = _csr_dev(c.seen) if seen else None
        ids, sc, _ = _ops().retrieve_topk("linear", c.T, c.fold, c.users, RET_K, seen=csr)
        torch.cuda.synchronize()
        ids, sc = ids.cpu().numpy(), sc.cpu().numpy().astype(np.float64)
        bands = set()
        for q in range(RET_Q):
            want, v = c.expected(q, seen)
            assert np.array_equal(ids[q], want[:RET_K]), (q, ids[q], want[:RET_K])
            assert np.all(np.abs(sc[q] - v[:RET_K]) <= c.tau), q
            assert len(set(lt.band_of(want[:RET_K], c.Dp).tolist())) >= 2, q  # (the answers come from several bands)
            bands |= set(lt.band_of(want[:RET_K], c.Dp).tolist())
        assert bands == set(range(lt.N_BANDS))

    @pytest.mark.parametrize("seen", [False, True], ids=["all", "unseen"])
    def test_item_ranks_over_a_large_catalogue(self, catalogue, seen):
        """trs_item_ranks for targets in every band — per query its group's planted rows and four unplanted rows, one per
        band — by test_every_rank_lies_in_the_float64_interval's criterion (tests/test_gpu_ranks.py): with tau as above, a
        rank lies in [#{v_i > v_t + 2 tau}, #{v_i >= v_t - 2 tau}] over the query's candidates without t.  The counts are
        float64, taken on the device in item chunks."""
        c = catalogue
        extra = np.setdiff1d(lt.band_rows(c.N, c.Dp, 1, seed=c.D + 25), lt.boundary_rows(c.N, c.Dp))
        assert sorted(lt.band_of(extra, c.Dp).tolist()) == list(range(lt.N_BANDS)) and not np.isin(extra, c.rows).any()
        targets = [np.union1d(c.rows[c.group == q % RET_G], extra) for q in range(RET_Q)]
        lt.assert_covers(np.concatenate(targets), c.N, c.Dp)
        J = targets[0].size
        assert all(t.size == J for t in targets)
        tg = torch.from_numpy(np.stack(targets)).to(DEV)                                     # (RET_Q, J)
        vt = torch.stack([c.values(c.item[tg[q]], c.bias[tg[q]])[q] for q in range(RET_Q)])  # (RET_Q, J) float64
        lo_thr, hi_thr = (vt + 2 * c.tau).unsqueeze(1), (vt - 2 * c.tau).unsqueeze(1)
        if getattr(c, "rank_counts", None) is None:  # over the whole catalogue, once for both cases
            lo = torch.zeros((RET_Q, J), dtype=torch.int64, device=DEV)
            hi = torch.zeros((RET_Q, J), dtype=torch.int64, device=DEV)
            for _, _, v in c.chunks(1 << 18):
                lo += (v.unsqueeze(2) > lo_thr).sum(dim=1)
                hi += (v.unsqueeze(2) >= hi_thr).sum(dim=1)
            c.rank_counts = (lo, hi - 1)  # (without the target itself)
        lo, hi = (t.clone() for t in c.rank_counts)
        if seen:  # the seen items are no candidates: take their part out again (a seen target keeps its row, as there)
            for q in range(RET_Q):
                s = torch.from_numpy(c.seen[q]).to(DEV)
                vs = c.values(c.item[s], c.bias[s])[q].unsqueeze(1)
                own = torch.from_numpy(np.isin(c.seen[q], targets[q])).to(DEV).unsqueeze(1) & (s.unsqueeze(1) == tg[q].unsqueeze(0))
                lo[q] -= (vs > lo_thr[q]).sum(dim=0)
                hi[q] -= ((vs >= hi_thr[q]) & ~own).sum(dim=0)
        ranks, _ = _ops().item_ranks("linear", c.T, c.fold, c.users, _csr_dev(targets), seen=_csr_dev(c.seen) if seen else None)
        torch.cuda.synchronize()
        got = ranks.view(RET_Q, J)
        bad = (got < lo) | (got > hi)
        assert not bool(bad.any()), (torch.nonzero(bad)[:5].tolist(), got[bad][:5].tolist(), lo[bad][:5].tolist(), hi[bad][:5].tolist())
        assert int(got.max()) > c.N // 4 and int(got.min()) == 0  # (planted targets lead, unplanted ones sit deep in the list)


def planted_neighbour_rows(D, n, bump):
    """n rows far above anything a background row reaches under either metric: row i is s_i e_g + a_i e_G, g = i mod G,
    G = min(D - 2, 40) groups, with strengths s uniform in [1, 2) and tilts a uniform in [0.1, 3).  (The background rows
    are e_{D-1} + N(0, 0.001): nearly orthogonal to every planted row.)"""
    rs = np.random.RandomState(D + 31 + 1000 * bump)
    G = min(D - 2, 40)
    P = np.zeros((n, D), dtype=np.float32)
    P[np.arange(n), np.arange(n) % G] = 1.0 + rs.rand(n)
    P[:, G] = 0.1 + 2.9 * rs.rand(n)
    return P


def planted_neighbours(D, n, qi, cosine):
    """(P, X, sims, tol, order, top, clear) of the first seed bump whose float64 order has under 1 % of its top-k
    positions within 2 tol of a neighbour in the order (_check_tolerance of tests/test_gpu_neighbours.py asserts the
    same share of its input); no GPU.  sims (RET_Q, n): float64 similarities of the query rows qi to every planted row,
    -inf at the query itself; clear: position p is more than 2 tol from both its neighbours in the order."""
    for bump in range(8):
        P = planted_neighbour_rows(D, n, bump)
        X = neighbours_ref.normalise(P.astype(np.float64)) if cosine else P.astype(np.float64)
        sims = X[qi] @ X.T
        sims[np.arange(len(qi)), qi] = -np.inf
        tol = neighbours_ref.tol(D) * (1.0 if cosine else max(1.0, float(sims.max())))
        order = np.argsort(-sims, axis=1)[:, :RET_K + 1]
        top = np.take_along_axis(sims, order, axis=1)
        clear = np.diff(top, axis=1) < -2 * tol
        clear = np.concatenate([np.ones((len(qi), 1), bool), clear[:, :-1]], axis=1) & clear
        if clear.mean() > 0.99:
            return P, X, sims, tol, order, top, clear
    raise AssertionError("no seed gives a float64 order that is clear at 99 % of its positions")


def plant_neighbours(table, rows_t, P):
    """The table (filled at a small scale) becomes the background e_{D-1} + noise, its rows rows_t the planted rows P."""
    table[:, table.shape[1] - 1] += 1.0
    table[rows_t] = torch.from_numpy(P).to(table.device)


def assert_planted_lead(table, rows_t, Xq, cosine, top, tol):
    """The input's condition, from the float64 side alone (the table in row chunks on the device): every query's k-th
    planted similarity is more than 2 tol above its best similarity to any unplanted row, so no such row can enter a
    top-k.  Xq: the queries' float64 rows (unit length under cosine)."""
    N = table.shape[0]
    Xq = torch.from_numpy(Xq).to(table.device)
    best = torch.full((Xq.shape[0],), -np.inf, dtype=torch.float64, device=table.device)
    for lo in range(0, N, 1 << 20):
        hi = min(lo + (1 << 20), N)
        y = table[lo:hi].double()
        if cosine:
            y = y / y.norm(dim=1, keepdim=True).clamp_min(1e-300)
        v = Xq @ y.t()
        v[:, rows_t[(rows_t >= lo) & (rows_t < hi)] - lo] = -np.inf
        best = torch.maximum(best, v.max(dim=1).values)
    assert (top[:, RET_K - 1] > best.cpu().numpy() + 2 * tol).all()


def check_neighbours(ids, sc, rows, queries, sims, tol, order, top, clear, what):
    """_check_tolerance's criterion (tests/test_gpu_neighbours.py): every id a planted row, none twice, never the query;
    its similarity within tol of the float64 one; ids off the float64 order only where that order has values within
    2 tol of each other."""
    assert np.isin(ids, rows).all()
    got_v = np.take_along_axis(sims, np.searchsorted(rows, ids), axis=1)
    want_ids = rows[order[:, :RET_K]]
    print(f"{what}: max |similarity - float64| = {np.abs(sc - got_v).max():.3e} (tol {tol:.3e}); positions off the "
          f"float64 order: {int((ids != want_ids).sum())}")
    assert np.all(np.abs(sc - got_v) <= tol) and np.all(np.abs(got_v - top[:, :RET_K]) <= 2 * tol)
    assert all(len(set(row.tolist())) == RET_K and q not in row for row, q in zip(ids, queries))
    assert np.array_equal(ids[clear], want_ids[clear])


@pytest.mark.parametrize("D", [WIDE, TAIL])
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_neighbours_in_a_large_user_table(D, metric):
    """trs_neighbour_fold + trs_neighbours_topk over a user table of n_rows_for(Dp) rows; queries: 45 of the planted
    band_rows rows, their neighbours the other planted rows.  The fold on band_rows (and on rows beside them) is the
    table row, or its normalise_f32, bit for bit (test_neighbour_fold_writes_the_restated_normalisation, tests/test_
    gpu_neighbours.py).  The top-k by _check_tolerance's criterion of that module, with tol = neighbours_ref.tol(D)
    (times the largest similarity under 'dot', where the rows are no unit vectors); the input is held, from the float64
    side alone, to a k-th planted similarity more than 2 tol above the best unplanted one, so every id must be a
    planted row, and where the float64 order is clear by 2 tol on both sides the id must be that order's."""
    ops = _ops()
    Dp = neighbours_ref.dp(D)
    N = lt.n_rows_for(Dp)
    rows = lt.band_rows(N, Dp, 4 * RET_K, seed=D + 30)
    lt.assert_covers(rows, N, Dp)
    n, rows_t = rows.size, torch.from_numpy(rows).to(DEV)
    qi = np.arange(RET_Q) * (n // RET_Q)  # the queries: planted rows of every band
    queries = rows[qi]
    assert set(lt.band_of(queries, Dp).tolist()) == set(range(lt.N_BANDS))
    cosine = metric == "cosine"
    P, X, sims, tol, order, top, clear = planted_neighbours(D, n, qi, cosine)
    table = lt.fill(torch.empty((N, D), device=DEV), seed=D + 32, scale=0.001)
    plant_neighbours(table, rows_t, P)
    assert_planted_lead(table, rows_t, X[qi], cosine, top, tol)
    fold = ops.neighbour_fold(table, N, D, cosine)
    S = ops.fold_views(fold, N, D)[0]
    for r in (rows, rows[4:-4:3] + 1):
        src = lt.gather_small(table, r)
        want = neighbours_ref.normalise_f32(src) if cosine else src
        got = lt.gather_small(S, r)
        assert np.array_equal(got[:, :D], want) and not got[:, D:].any()
    ids, sc = ops.neighbours_topk(fold, N, D, torch.from_numpy(queries).to(DEV), RET_K)
    torch.cuda.synchronize()
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy().astype(np.float64)
    check_neighbours(ids, sc, rows, queries, sims, tol, order, top, clear, f"{metric} D={D}")
    assert all(len(set(lt.band_of(row, Dp).tolist())) >= 2 for row in rows[order[:, :RET_K]])  # (from several bands)


@pytest.mark.parametrize("D", [WIDE, TAIL])
def test_mmr_rerank_and_list_ild_on_a_large_item_fold(D):
    """trs_mmr_rerank / trs_list_ild over a unit-length neighbour fold of n_rows_for(Dp) rows, the pools made of the 128
    band_rows rows (KMAX entries, some of them -1).  References on the compacted fold rows as the device wrote them
    (as tests/test_gpu_mmr.py takes them): mmr_ref.check_greedy with its eps(lambda, D), mmr_ref.ild within ild_tol(D)
    (test_list_ild_against_the_oracle).  The fold is only read by both: bit-identical afterwards."""
    ops = _ops()
    Dp = mmr_ref.dp(D)
    N = lt.n_rows_for(Dp)
    rows = lt.band_rows(N, Dp, 30, seed=D + 40)
    n, k, lam = rows.size, RET_K, 0.6
    assert n == mmr_ref.KMAX
    table = lt.fill(torch.empty((N, D), device=DEV), seed=D + 41, scale=1.0)  # (randn, as test_list_ild_against_the_oracle)
    nf = ops.neighbour_fold(table, N, D, True)
    del table
    sums = lt.row_checksums(ops.fold_rows(nf, N))
    small = lt.gather_small(ops.fold_views(nf, N, D)[0], rows)
    rs = np.random.RandomState(D + 42)
    pools = np.stack([rs.permutation(n) for _ in range(RET_Q)]).astype(np.int64)  # compact ids: every pool names every row
    scores = -np.sort(-rs.randn(RET_Q, n).astype(np.float32), axis=1)            # descending, as retrieve_topk returns them
    pools[1, n // 2:] = -1
    pools[2, 5] = -1
    lt.assert_covers(rows[pools[0]], N, Dp)
    real = np.where(pools >= 0, rows[np.maximum(pools, 0)], -1)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ids, sc, pos = ops.mmr_rerank(nf, N, D, torch.from_numpy(real).to(DEV), torch.from_numpy(scores).to(DEV), k, lam,
                                  want_pos=True, err_flag=err)
    ild = ops.list_ild(nf, N, D, ids)
    torch.cuda.synchronize()
    ids, sc, pos, ild = ids.cpu().numpy(), sc.cpu().numpy(), pos.cpu().numpy(), ild.cpu().numpy()
    assert np.isin(ids[ids >= 0], rows).all()
    compact = np.where(ids >= 0, np.searchsorted(rows, np.maximum(ids, 0)), -1)
    worst = mmr_ref.check_greedy(pools, scores, small, k, lam, D, compact, sc, pos, n_items=n)
    want = mmr_ref.ild(compact, small, n_items=n)
    print(f"D={D}: largest shortfall {worst:.3e} (eps {mmr_ref.eps(lam, D):.3e}); max |ild - oracle| = "
          f"{np.abs(ild - want).max():.3e} (tol {mmr_ref.ild_tol(D):.3e})")
    assert np.all(np.abs(ild - want) <= mmr_ref.ild_tol(D)) and want.min() > 0.5  # (random unit rows: nearly orthogonal)
    assert all(len(set(lt.band_of(row[row >= 0], Dp).tolist())) >= 2 for row in ids)  # (lists from several bands)
    lt.assert_untouched(sums, lt.row_checksums(ops.fold_rows(nf, N)), [], "the neighbour fold")
    assert err.item() == 0


# ------------------------------------------------------------------------------------ 7. once through a model
def test_through_a_model_with_a_large_user_table():
    """An FM model of n_rows_for(64) users x 300 items, D = 64, device RNG, whose 2 000 interactions name 100 band_rows
    users: where the host-side id arithmetic of model.py, ops.py and evaluate/ would show.  Every reference runs on the
    user tables compacted to those 100 rows (the item side is small as it is):
      fit             one epoch, batch 256, n_negatives = 3, l2 = 0.01, SGD: test_fit_with_l2_against_a_host_replay's
                      replay and bars (tests/test_gpu_l2.py): tables at 5e-5, the printed loss to 4 decimals, the penalty
                      three bars out; every user row no train interaction names bit-identical
      recommend       the contract of test_random_weights_tolerance_contract (tests/test_ranking.py), tau = 1e-5 max(1, |v|)
      rank_items      test_every_rank_lies_in_the_float64_interval (tests/test_gpu_ranks.py), seen targets among them
      fold_in_items   foldin_items_ref.fold_in on the compacted stream and seen sets, FM + BPR with one negative visit;
                      test_smooth_losses_against_float64's criterion, TOL of tests/test_gpu_foldin_items.py
      similar_users   cosine and dot, planted as in test_neighbours_in_a_large_user_table, same criterion
    The embedding tables are scaled to N(0, 0.3) first (the scale of all those references' own tests)."""
    import contextlib
    import io
    import re
    from torchrecsys_amd import model as model_mod
    from torchrecsys_amd import ops
    from torchrecsys_amd.model import TorchRecSys
    D, n_items, n_int, B, Kn, lr, lam = WIDE, 300, 2000, 256, 3, 0.5, 0.01
    N = lt.n_rows_for(D)
    rows = lt.band_rows(N, D, 23, seed=50)
    n, rows_t = rows.size, torch.from_numpy(rows).to(DEV)
    rs = np.random.RandomState(51)
    uc = np.concatenate([np.arange(n), rs.randint(0, n, n_int - n)])
    ic = np.concatenate([np.arange(n_items), rs.randint(0, n_items, n_int - n_items)])
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        model = TorchRecSys.from_tensors(torch.from_numpy(rows[uc]).to(DEV), torch.from_numpy(ic).to(DEV), n_users=N,
                                         n_items=n_items, n_factors=D, net_type="fm", dynamic_neg_sampling=True,
                                         rng="device", seed=1)
    names = multineg_ref.table_names("fm", 0)
    sd = model.net.state_dict()
    assert sorted(sd) == sorted(names) and sd["user.weight"].shape == (N, D)
    large = ("user.weight", "linear_user.weight")
    for k in ("user.weight", "item.weight"):
        sd[k].mul_(0.3 / float(sd[k][:1000].std()))

    def compacted():
        return {k: (lt.gather_small(sd[k], rows) if k in large else sd[k].cpu().numpy()).astype(np.float64) for k in names}

    st = model._device_stream("train")
    su_real, si = st["user"].cpu().numpy().astype(np.int64), st["pos"].cpu().numpy().astype(np.int64)
    su = np.searchsorted(rows, su_real)
    assert np.array_equal(rows[su], su_real)
    lt.assert_covers(su_real, N, D)  # the train split names every band and boundary
    n_train = su.size
    # ---- fit
    W = compacted()
    W_data = {k: v.copy() for k, v in W.items()}
    sums = {k: lt.row_checksums(sd[k]) for k in large}
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        model.fit(torch.optim.SGD(model.parameters(), lr=lr), epochs=1, batch_size=B, loss="hinge", n_negatives=Kn, l2=lam)
    torch.cuda.synchronize()
    printed = [float(x) for x in re.findall(r"Training Loss: ([-0-9.]+)", buf.getvalue())]
    key, seed = model_mod._mix64(model.seed, 1), model_mod._mix64(model.seed, 2)
    means = []
    for s in range(0, n_train, B):
        m = min(B, n_train - s)
        ids = multineg_ref.prepare(su, si, key, s, m, n_items, seed, s, Kn, None, None)
        val, grads = multineg_ref.loss_and_grads("fm", W, ids["user"], ids["items"], None, "hinge", 1.0)
        pen = l2_ref.grads("fm", W, ids["user"], ids["items"], None, (lam, lam, lam), 1.0 / m)
        means.append(val)
        for k in W:
            W[k] -= lr * (grads[k] + pen[k])
        _, grads = multineg_ref.loss_and_grads("fm", W_data, ids["user"], ids["items"], None, "hinge", 1.0)
        for k in W_data:
            W_data[k] -= lr * grads[k]
    assert len(printed) == 1 and abs(printed[0] - np.mean(means)) <= 0.5e-4 + 1e-5 * abs(np.mean(means))
    after = compacted()
    for k in names:
        print(f"fit {k}: {rel_err(after[k], W[k]):.2e} (the replay without the penalty: {rel_err(W_data[k], W[k]):.2e})")
        assert rel_err(after[k], W[k]) <= 5e-5, k
    # one epoch at l2 = 0.01 moves the tables by less than that test's two at 0.03 - 0.05: the penalty stands 3 bars out
    # (2 for the triangle inequality, 1 to spare), so a run that dropped it would still miss
    assert min(rel_err(W_data[k], W[k]) for k in ("user.weight", "item.weight")) > 3 * 5e-5
    for k in large:
        lt.assert_untouched(sums.pop(k), lt.row_checksums(sd[k]), np.unique(su_real), k)
    # ---- recommend and rank_items on the trained tables
    P = after
    z = P["user.weight"] @ P["item.weight"].T + P["linear_user.weight"] + P["linear_item.weight"].T  # (n, n_items) logits
    ov = 1.0 / (1.0 + np.exp(-z))
    off, seen_items = foldin_items_ref.seen_csr(su, si, n)
    seen = [set(seen_items[off[u]:off[u + 1]].tolist()) for u in range(n)]
    tau = 1e-5 * max(1.0, float(np.abs(ov).max()))
    k = 10
    ids, sc = model.recommend(rows.tolist(), top_k=k, return_scores=True)
    ids, sc = ids.numpy(), sc.numpy().astype(np.float64)
    for u in range(n):
        got = ids[u]
        assert np.all((got >= 0) & (got < n_items)) and len(set(got.tolist())) == k and not (set(got.tolist()) & seen[u])
        assert np.all(np.diff(sc[u]) <= 0) and np.all(np.abs(sc[u] - ov[u][got]) <= tau), u
        mask = np.ones(n_items, bool)
        mask[list(seen[u])] = False
        assert np.all(ov[u][got] >= np.sort(ov[u][mask])[::-1][k - 1] - 2 * tau), u
        mask[got] = False
        assert ov[u][mask].max() <= sc[u].min() + 2 * tau, u
    tau_z = 1e-5 * max(1.0, float(np.abs(z).max()))
    targets = [np.unique(np.concatenate([rs.choice(n_items, 5, replace=False), sorted(seen[u])[:2]])) for u in range(n)]
    pairs_u = np.concatenate([np.full(t.size, rows[u]) for u, t in enumerate(targets)])
    pairs_i = np.concatenate(targets)
    ranks = model.rank_items(pairs_u.tolist(), pairs_i.tolist()).numpy()
    at = 0
    for u, tg in enumerate(targets):
        cand = np.ones(n_items, bool)
        cand[list(seen[u])] = False
        for t in tg:
            c = cand.copy()
            c[t] = False
            lo, hi = np.sum(z[u][c] > z[u][t] + 2 * tau_z), np.sum(z[u][c] >= z[u][t] - 2 * tau_z)
            assert lo <= ranks[at] <= hi, (u, t, ranks[at], lo, hi)
            at += 1
    # ---- fold_in_items: new items from histories of band_rows users
    hists = als_ref.random_lists(30, n, 52, (0, 1, 2, 63, 64, 65, n - 1, n))
    kw = dict(seed=FOLD_SEED, shuffle=True, reject_seen=True, max_tries=8)
    V, b, ls = model.fold_in_items([rows[h] for h in hists], epochs=FOLD_E, lr=FOLD_LR, loss="bpr", l2=FOLD_L2,
                                   negative_visits=1, return_loss=True, **kw)
    f64 = lambda t: t.cpu().numpy().astype(np.float64)
    S, c = ops.fold_views(ops.item_fold("fm", model.net.tables(), n_items, D, DEV, None), n_items, D)
    Tn, kappa = ops.fold_views(model._new_item_fold(None, len(hists), DEV), len(hists), D)
    want = foldin_items_ref.fold_in(P["user.weight"], P["linear_user.weight"][:, 0], f64(S), f64(c), f64(Tn), f64(kappa),
                                    [np.asarray(h, dtype=np.int64) for h in hists], su, si, (off, seen_items), "fm", "bpr",
                                    FOLD_E, FOLD_LR, FOLD_L2, nu=1, **kw)
    for name, got in (("V", V), ("b", b), ("loss", ls)):
        fold_close(got, want[name], FI.TOL, f"fold_in_items {name}")
    assert np.abs(want["V"]).max() > 0.05
    # ---- similar_users: the user table becomes a planted one (nothing below reads the trained values)
    qi = np.arange(RET_Q) * (n // RET_Q)
    queries = rows[qi]
    assert set(lt.band_of(queries, D).tolist()) == set(range(lt.N_BANDS))
    table = sd["user.weight"]
    table.mul_(0.001 / 0.3)
    table[:, D - 1] += 1.0
    for metric in ("cosine", "dot"):
        cosine = metric == "cosine"
        Pn, X, sims, tol, order, top, clear = planted_neighbours(D, n, qi, cosine)
        table[rows_t] = torch.from_numpy(Pn).to(DEV)
        assert_planted_lead(table, rows_t, X[qi], cosine, top, tol)
        ids, sc = model.similar_users(queries.tolist(), top_k=RET_K, metric=metric, return_scores=True)
        check_neighbours(ids.numpy(), sc.numpy().astype(np.float64), rows, queries, sims, tol, order, top, clear,
                         f"similar_users {metric}")
