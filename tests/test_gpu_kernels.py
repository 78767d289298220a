# -*- coding: utf-8 -*-
"""Kernel-level parity: libtrs_hip.so (through the C-ABI) against oracle/ on the same seeded inputs.  GPU only.

The SGD-step tests are split into a case (`*_case()`: ids, tables, lr — no GPU, conditioned and sized so that one lost
row reference is at least three allowances of the criterion), the GPU run, and the criterion on numpy tables
(step_sensitivity.criterion_for); tests/test_step_sensitivity_host.py checks the first against the last without a GPU."""
import functools

import numpy as np
import pytest
import torch

import large_tables
import step_sensitivity as sens
from conftest import rel_err
from oracle import loader as oloader
from oracle import nets as onets
from oracle import optim as ooptim

pytestmark = pytest.mark.gpu

TOL = 1e-5  # north_star tolerance for fp32 scores / gradients (norm-wise relative, see conftest.rel_err)
DEV = "cuda:0"


def _ops():
    from torchrecsys_amd import ops
    return ops


def make_case(net, D, M, B, NU=50, NI=37, seed=0, idx_dtype=np.int64):
    rs = np.random.RandomState(seed)
    sizes = [5, 7, 4, 9, 3, 6, 8, 2][:M]
    p = {"user.weight": rs.normal(0, 0.3, (NU, D)), "item.weight": rs.normal(0, 0.3, (NI, D))}
    if net == "linear":
        p["user_bias.weight"] = rs.normal(0, 0.3, (NU, 1))
        p["item_bias.weight"] = rs.normal(0, 0.3, (NI, 1))
    else:
        p["linear_user.weight"] = rs.normal(0, 0.3, (NU, 1))
        p["linear_item.weight"] = rs.normal(0, 0.3, (NI, 1))
    for m in range(M):
        p[f"metadata.{m}.weight"] = rs.normal(0, 0.3, (sizes[m], D))
        if net == "fm":
            p[f"linear_metadata.{m}.weight"] = rs.normal(0, 0.3, (sizes[m], 1))
    p = {k: v.astype(np.float32) for k, v in p.items()}
    u, i, j = rs.randint(0, NU, B), rs.randint(0, NI, B), rs.randint(0, NI, B)
    if B > 12:
        u[1] = u[2] = u[3]
        i[4] = j[5] = i[6]
        j[7] = i[7]
    batch = {"user_id": u, "pos_item_id": i, "neg_item_id": j}
    if M:
        item_meta = np.stack([rs.randint(0, sizes[m], NI) for m in range(M)], axis=1)
        batch["pos_metadata_id"], batch["neg_metadata_id"] = item_meta[i], item_meta[j]
    batch = {k: v.astype(np.int64) for k, v in batch.items()}
    return p, batch, idx_dtype


def to_dev(net, p, batch, idx_dtype):
    ops = _ops()
    t = {k: torch.from_numpy(v).to(DEV) for k, v in p.items()}
    M = sum(1 for k in p if k.startswith("metadata."))
    lin = ("user_bias.weight", "item_bias.weight") if net == "linear" else ("linear_user.weight", "linear_item.weight")
    metas = [t[f"metadata.{m}.weight"] for m in range(M)]
    meta_lins = [t[f"linear_metadata.{m}.weight"] for m in range(M)] if net == "fm" else []
    T, keepT = ops.make_tables(t["user.weight"], t["item.weight"], t[lin[0]], t[lin[1]], metas, meta_lins)
    tdt = torch.int32 if idx_dtype == np.int32 else torch.int64
    ids = {k: torch.from_numpy(v).to(DEV).to(tdt).contiguous() for k, v in batch.items()}
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    Bt, keepB = ops.make_batch(ids["user_id"], ids["pos_item_id"], ids["neg_item_id"], ids.get("pos_metadata_id"),
                               ids.get("neg_metadata_id"), err)
    return t, T, Bt, ids, err, (keepT, keepB)


def dense_from_staging(net, p, batch, grad_rows, grad_lin):
    """Scatter the staged per-triple rows into dense-equivalent gradients (what p.grad.to_dense() is)."""
    M = sum(1 for k in p if k.startswith("metadata."))
    gr, gl = grad_rows.cpu().numpy().astype(np.float64), grad_lin.cpu().numpy().astype(np.float64)
    out = {k: np.zeros(v.shape, np.float64) for k, v in p.items()}
    lin = ("user_bias", "item_bias") if net == "linear" else ("linear_user", "linear_item")
    fields = [("user", lin[0], batch["user_id"]), ("item", lin[1], batch["pos_item_id"]),
              ("item", lin[1], batch["neg_item_id"])]
    for m in range(M):
        lm = f"linear_metadata.{m}" if net == "fm" else None
        fields.append((f"metadata.{m}", lm, batch["pos_metadata_id"][:, m]))
        fields.append((f"metadata.{m}", lm, batch["neg_metadata_id"][:, m]))
    for f, (name, lname, idx) in enumerate(fields):
        np.add.at(out[f"{name}.weight"], idx, gr[f])
        if lname:
            np.add.at(out[f"{lname}.weight"], idx, gl[f][:, None])
    return out


CASES = [("fm", 64, 0), ("fm", 8, 0), ("fm", 16, 1), ("fm", 128, 3), ("fm", 80, 0), ("fm", 10, 1), ("fm", 256, 0),
         ("fm", 512, 1), ("fm", 4, 0), ("fm", 1, 0), ("fm", 100, 2), ("fm", 33, 0),
         ("linear", 32, 0), ("linear", 8, 1), ("linear", 64, 3), ("linear", 80, 0), ("linear", 7, 2),
         ("linear", 1024, 0), ("fm", 201, 0)]


@pytest.mark.parametrize("net,D,M", CASES)
@pytest.mark.parametrize("idx_dtype", [np.int64, np.int32])
def test_forward_and_fwd_bwd(net, D, M, idx_dtype):
    ops = _ops()
    B = 203
    p, batch, _ = make_case(net, D, M, B, seed=D + M)
    t, T, Bt, ids, err, keep = to_dev(net, p, batch, idx_dtype)
    pos, neg = ops.score_forward(net, T, Bt, B, DEV)
    sp, sn, loss, grads = onets.train_forward_backward(net, {k: v.copy() for k, v in p.items()}, batch)
    assert rel_err(pos.cpu().numpy(), sp.reshape(-1)) < TOL
    assert rel_err(neg.cpu().numpy(), sn.reshape(-1)) < TOL
    loss_sum = torch.zeros(1, dtype=torch.float32, device=DEV)
    auc = torch.zeros(1, dtype=torch.int32, device=DEV)
    pos2, neg2, gr, gl = ops.score_fwd_bwd(net, T, Bt, B, D, M, DEV, loss_sum, auc)
    torch.cuda.synchronize()
    assert torch.equal(pos2, pos) and torch.equal(neg2, neg)
    assert abs(loss_sum.item() / B - float(loss)) <= TOL * max(abs(float(loss)), 1e-3)
    # counted on the kernel's own scores (saturated sigmoids tie at 1.0 and flip on the last bit)
    assert auc.item() == int((pos > neg).sum().item())
    dense = dense_from_staging(net, p, batch, gr, gl)
    for k, v in grads.items():
        assert rel_err(dense[k], v) < TOL, k
    assert err.item() == 0
    # backward from explicit upstream gradients == hinge path
    gp, gn = ops.hinge_backward(pos, neg)
    ogp, ogn = onets.hinge_grad(sp.reshape(-1), sn.reshape(-1))
    assert np.array_equal(gp.cpu().numpy(), ogp) and np.array_equal(gn.cpu().numpy(), ogn)
    gr2, gl2 = ops.score_backward(net, T, Bt, B, D, M, DEV, gp, gn)
    assert torch.equal(gr2, gr) and torch.equal(gl2, gl)
    # the one-sweep form (MLP step): trs_hinge_auc's sums and trs_hinge_backward's gradients, bit for bit
    for loss_id in (0, 1):
        ls1 = torch.zeros(1, dtype=torch.float32, device=DEV)
        a1 = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.hinge_auc(pos, neg, ls1, a1, loss=loss_id)
        g1p, g1n = ops.hinge_backward(pos, neg, loss=loss_id)
        ls2, a2 = torch.zeros_like(ls1), torch.zeros_like(a1)
        g2p, g2n = ops.hinge_auc_backward(pos, neg, ls2, a2, loss=loss_id)
        assert torch.equal(g2p, g1p) and torch.equal(g2n, g1n) and a1.item() == a2.item()
        assert g2p._base is g2n._base and g2p._base.numel() == 2 * B
        if B <= 1024:  # one workgroup: one atomic, the same sum
            assert ls1.item() == ls2.item()
        else:
            assert abs(ls1.item() - ls2.item()) <= 1e-5 * abs(ls1.item())


SGD_THREE_STEPS = [("fm", 64, 0), ("fm", 16, 2), ("linear", 32, 1), ("linear", 80, 0)]


def lr_of(B, D, lr, at_least=0.05, hot=False):
    """lr = None: the step size at which the table criterion sees one lost reference (tests/step_sensitivity.py)"""
    return sens.step_lr(B, at_least, hot, D) if lr is None else lr


@functools.lru_cache(maxsize=4)
def sgd_three_steps_case(net, D, M, lr=None):
    """The input of test_sgd_update_three_steps (no GPU): one batch of 300, three steps on it."""
    def build(bump):
        B = 300
        p, batch, _ = make_case(net, D, M, B, seed=3 + 1000 * bump)
        return sens.StepCase(net, sens.condition_tables(net, p), [batch] * 3, lr_of(B, D, lr), M=M, D=D)
    return sens.conditioned(build, first=lr is not None)


@pytest.mark.parametrize("net,D,M", SGD_THREE_STEPS)
def test_sgd_update_three_steps(net, D, M):
    ops = _ops()
    case = sgd_three_steps_case(net, D, M)
    p, batch, B, lr = case.p, case.batches[0], case.B, case.lr
    t, T, Bt, ids, err, keep = to_dev(net, p, batch, np.int64)
    losses = []
    for step in range(3):
        loss_sum = torch.zeros(1, dtype=torch.float32, device=DEV)
        _, _, gr, gl = ops.score_fwd_bwd(net, T, Bt, B, D, M, DEV, loss_sum, want_scores=False)
        ops.score_sgd_update(net, T, Bt, gr, gl, lr)
        losses.append(loss_sum.item())
    sens.assert_losses(case, losses)
    sens.criterion_for(case)(tables_to_host(t), case.ref, p)


def tables_to_host(t, names=None):
    return {k: t[k].cpu().numpy() for k in (names or t)}


@pytest.mark.parametrize("D", [1, 16, 64, 80, 200, 3, 7, 12, 40])
@pytest.mark.parametrize("kind", ["adam", "adagrad"])
def test_coalescing_row_optimisers(D, kind):
    """(the last four widths complete the lanes-per-row classes of csrc/rows.hip: 1, 4, 8, 16, 32, 64)"""
    ops = _ops()
    rs = np.random.RandomState(D)
    n_rows, n = 40, 150
    W = rs.normal(0, 1, (n_rows, D)).astype(np.float32)
    idx = rs.randint(0, n_rows // 2, n).astype(np.int64)  # rows >= n_rows/2 stay untouched
    tW = torch.from_numpy(W.copy()).to(DEV)
    acc = torch.zeros_like(tW)
    s1 = torch.zeros_like(tW)
    s2 = torch.zeros_like(tW)
    stamp = torch.zeros(n_rows, dtype=torch.int32, device=DEV)
    tidx = torch.from_numpy(idx).to(DEV)
    ref, m, v = W.copy(), np.zeros_like(W), np.zeros_like(W)
    for step in range(1, 4):
        vals = rs.normal(0, 1, (n, D)).astype(np.float32)
        vals[idx == 3] = 0.0  # a touched row with an all-zero gradient must still decay its moments
        tv = torch.from_numpy(vals).to(DEV)
        ops.rows_scatter_add(acc, tidx, tv, 1.0)
        G = np.zeros_like(W)
        np.add.at(G, idx, vals)
        rows = np.unique(idx)
        if kind == "adam":
            ops.rows_apply_sparse_adam(tW, acc, s1, s2, stamp, tidx, step, 0.01, 0.9, 0.999, 1e-8, step)
            ooptim.sparse_adam_rows(ref, G, rows, m, v, step, 0.01)
        else:
            ops.rows_apply_adagrad(tW, acc, s1, stamp, tidx, step, 0.05, 1e-10)
            ooptim.adagrad_rows(ref, G, rows, m, step, 0.05)
        torch.cuda.synchronize()
        assert float(acc.abs().max()) == 0.0  # accumulator cleared by the owners
    assert rel_err(tW.cpu().numpy(), ref) < 5e-5
    assert np.array_equal(tW.cpu().numpy()[n_rows // 2:], W[n_rows // 2:])  # lazy: untouched rows bit-identical
    assert rel_err(s1.cpu().numpy(), m) < 5e-5


LPR_WIDTHS = [1, 3, 7, 12, 40, 64, 200]  # one width per lanes-per-row class of csrc/rows.hip: 1, 4, 8, 16, 32, 64, 64 x 4


@pytest.mark.parametrize("n,cap", [(150, None), (1, None), (1000, 1)])
@pytest.mark.parametrize("D", LPR_WIDTHS)
@pytest.mark.parametrize("kind", ["adam", "adagrad"])
def test_row_optimisers_int32_ids_strided_values_and_ids_out_of_range(kind, D, n, cap, tune):
    """trs_rows_scatter_add with int32 ids, values that are a column slice of a wider buffer (ld > D) and alpha = -0.5,
    then the two apply kernels, 2 steps.  Table, accumulator and both moments are rows [1:-1] of buffers with a guard row
    at each end; the ids -1 and n_rows (the guard rows' positions) raise err_flag, are skipped by the scatter AND by the
    apply kernels, and leave every row they do not name bit-identical.  n = 1: a single element; n = 1000 with one
    workgroup: every wave runs many iterations of the owner election."""
    ops = _ops()
    if cap is not None:
        tune(GRID_CAP=cap)
    rs = np.random.RandomState(D + n)
    n_rows, GUARD = 40, np.float32(12345.0)

    def guarded(init):
        buf = torch.full((n_rows + 2, D), float(GUARD), device=DEV)
        buf[1:-1] = torch.from_numpy(init).to(DEV)
        return buf, buf[1:-1]

    W = rs.normal(0, 1, (n_rows, D)).astype(np.float32)
    zeros = np.zeros_like(W)
    (bW, tW), (bacc, acc), (bs1, s1), (bs2, s2) = guarded(W.copy()), guarded(zeros), guarded(zeros), guarded(zeros)
    idx = rs.randint(0, n_rows // 2, n).astype(np.int32)  # rows >= n_rows/2 stay untouched
    idx[0] = 0
    bad = n >= 3
    if bad:
        idx[1], idx[2] = -1, n_rows
    good = (idx >= 0) & (idx < n_rows)
    tidx = torch.from_numpy(idx).to(DEV)
    stamp = torch.zeros(n_rows, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ref, m, v = W.copy(), np.zeros_like(W), np.zeros_like(W)
    rows = np.unique(idx[good])
    for step in (1, 2):
        wide = rs.normal(0, 1, (n, D + 5)).astype(np.float32)
        twide = torch.from_numpy(wide).to(DEV)
        ops.rows_scatter_add(acc, tidx, twide[:, 2:2 + D], -0.5, err_flag=err)
        G = np.zeros(W.shape, np.float64)
        np.add.at(G, idx[good], -0.5 * wide[good, 2:2 + D].astype(np.float64))
        torch.cuda.synchronize()
        assert err.item() == (1 if bad else 0)
        assert rel_err(acc.cpu().numpy(), G) < 1e-6
        G = acc.cpu().numpy().copy()  # the optimiser's input: the accumulator as the device summed it
        if kind == "adam":
            ops.rows_apply_sparse_adam(tW, acc, s1, s2, stamp, tidx, step, 0.01, 0.9, 0.999, 1e-8, step)
            ooptim.sparse_adam_rows(ref, G, rows, m, v, step, 0.01)
        else:
            ops.rows_apply_adagrad(tW, acc, s1, stamp, tidx, step, 0.05, 1e-10)
            ooptim.adagrad_rows(ref, G, rows, m, step, 0.05)
        torch.cuda.synchronize()
        assert float(acc.abs().max()) == 0.0  # accumulator cleared by the owners
    assert rel_err(tW.cpu().numpy(), ref) < 5e-5
    assert rel_err(s1.cpu().numpy(), m) < 5e-5
    untouched = np.ones(n_rows, bool)
    untouched[rows] = False
    assert np.array_equal(tW.cpu().numpy()[untouched], W[untouched])  # lazy: untouched rows bit-identical
    for name, buf in (("table", bW), ("acc", bacc), ("s1", bs1), ("s2", bs2)):
        ends = buf[[0, -1]].cpu().numpy()
        assert (ends == GUARD).all(), f"{name}: a guard row was written"
        if name != "table":
            assert not buf[1:-1].cpu().numpy()[untouched].any(), name


def test_out_of_range_ids_are_flagged_not_dereferenced():
    ops = _ops()
    p, batch, _ = make_case("fm", 16, 0, 64, seed=1)
    batch["pos_item_id"][5] = 10_000_000
    batch["user_id"][9] = -3
    t, T, Bt, ids, err, keep = to_dev("fm", p, batch, np.int64)
    pos, neg = ops.score_forward("fm", T, Bt, 64, DEV)
    loss_sum = torch.zeros(1, dtype=torch.float32, device=DEV)
    _, _, gr, gl = ops.score_fwd_bwd("fm", T, Bt, 64, 16, 0, DEV, loss_sum)
    ops.score_sgd_update("fm", T, Bt, gr, gl, 0.1)
    torch.cuda.synchronize()
    assert err.item() == 1
    assert pos[5].item() == 0.0 and pos[9].item() == 0.0
    assert float(gr[:, 5].abs().max()) == 0.0 and float(gr[:, 9].abs().max()) == 0.0


@pytest.mark.parametrize("idx_dtype", [torch.int64, torch.int32])
def test_sample_neg_bit_exact(idx_dtype):
    ops = _ops()
    for n_items, B in ((2, 1000), (3, 1000), (100_000, 65_536), (7, 1)):
        pos = np.random.RandomState(B).randint(0, n_items, B)
        tpos = torch.from_numpy(pos).to(DEV).to(idx_dtype)
        neg = ops.sample_neg(tpos, n_items, seed=0x1234_5678_9ABC, offset=77)
        ref = oloader.device_negatives(pos, n_items, 0x1234_5678_9ABC, 77)
        assert np.array_equal(neg.cpu().numpy().astype(np.int64), ref)
        assert (ref != pos).all() and ref.min() >= 0 and ref.max() < n_items


@pytest.mark.parametrize("M", [0, 2])
@pytest.mark.parametrize("static", [False, True])
def test_batch_prepare_bit_exact(M, static):
    ops = _ops()
    rs = np.random.RandomState(5)
    N, NU, NI = 1000, 60, 41
    su, si = rs.randint(0, NU, N).astype(np.int32), rs.randint(0, NI, N).astype(np.int32)
    ns = rs.randint(0, NI, N).astype(np.int32) if static else None
    im = np.stack([rs.randint(0, 5 + m, NI) for m in range(M)], axis=1).astype(np.int32) if M else None
    d = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    seen = []
    for key in (0, 0xABCDEF0123):
        for t0, B in ((0, 256), (256, 256), (768, 232)):
            out = ops.batch_prepare(d(su), d(si), d(ns), key, t0, B, NI, 99, 1000 + t0, d(im))
            ref = oloader.device_batch(su, si, ns, key, t0, B, NI, 99, 1000 + t0, im)
            for k in ref:
                assert np.array_equal(out[k].cpu().numpy().astype(np.int64), np.asarray(ref[k]).astype(np.int64)), k
            if key:
                seen.append(out["user"].cpu().numpy())
    # identity key = shuffle=False: rows in stream order
    out = ops.batch_prepare(d(su), d(si), d(ns), 0, 10, 20, NI, 1, 0, d(im))
    assert np.array_equal(out["user"].cpu().numpy(), su[10:30])


@pytest.mark.parametrize("opts", [dict(k=1, reject_seen=True), dict(k=3), dict(k=1, popularity=True),
                                  dict(k=2, popularity=True, reject_seen=True, max_tries=4)])
def test_sampler_options_bit_exact_and_properties(opts):
    """Sampler options beyond the reference's (reject all of the user's positives, popularity-weighted
    candidates, k negatives per positive) in every generator of the device RNG mode — trs_batch_prepare, trs_epoch_flags,
    trs_epoch_presort — bit-exact against oracle/loader.py's restatement, plus what each option promises."""
    ops = _ops()
    rs = np.random.RandomState(11)
    N, NU, NI, B = 1200, 40, 37, 200
    su = rs.randint(0, NU, N).astype(np.int32)
    si = (rs.zipf(1.6, N) % NI).astype(np.int32)  # skewed popularity
    d = lambda a: torch.from_numpy(a).to(DEV)
    k = opts.get("k", 1)
    seen = ops.Sampler.seen_csr(d(su), d(si), NU, NI) if opts.get("reject_seen") else None
    sm = ops.Sampler(k=k, popularity=opts.get("popularity", False), seen=seen, stream_item=d(si),
                     max_tries=opts.get("max_tries", 8))
    oracle_opts = dict(k=k, popularity=opts.get("popularity", False), max_tries=opts.get("max_tries", 8),
                       seen=None if seen is None else (seen[0].cpu().numpy(), seen[1].cpu().numpy()))
    key, seed_ = 0xC0FFEE1234, 77
    nb = (N * k) // B
    got = {q: [] for q in ("user", "pos", "neg")}
    for b in range(nb):
        out = ops.batch_prepare(d(su), d(si), None, key, b * B, B, NI, seed_, b * B, sampler=sm)
        ref = oloader.device_batch(su, si, None, key, b * B, B, NI, seed_, b * B, sampler=oracle_opts)
        for q in got:
            assert np.array_equal(out[q].cpu().numpy().astype(np.int64), ref[q]), (q, b)
            got[q].append(ref[q])
    u, p, n = (np.concatenate(got[q]) for q in ("user", "pos", "neg"))
    assert (n != p).all() and n.min() >= 0 and n.max() < NI
    # k negatives per positive: over the epoch's k*N positions every stream row is visited exactly k times
    if (N * k) % B == 0:
        pairs, cnt = np.unique(u * NI + p, return_counts=True)
        ref_pairs, ref_cnt = np.unique(su.astype(np.int64) * NI + si, return_counts=True)
        assert np.array_equal(pairs, ref_pairs) and np.array_equal(cnt, ref_cnt * k)
    if opts.get("reject_seen") and not opts.get("popularity"):
        # uniform candidates, 8 tries: a seen negative needs 8 seen candidates in a row (users hold ~13 of 37 items)
        pos_of = {uu: set(si[su == uu].tolist()) for uu in range(NU)}
        bad = sum(int(nn in pos_of[uu]) for uu, nn in zip(u, n))
        assert bad <= max(1, int(0.002 * n.size)), bad
    if opts.get("popularity") and not opts.get("reject_seen"):  # negatives follow the stream's item frequencies (minus
        f_neg = np.bincount(n, minlength=NI) / n.size           # the draws that hit the row's own positive)
        f_pop = np.bincount(si, minlength=NI) / N
        assert np.corrcoef(f_neg, f_pop)[0, 1] > 0.9 and f_neg[np.argmax(f_pop)] > 3.0 / NI
    # the epoch-level generators produce the same triples (flags kernel and sorted presort)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ui = ops.interleave_stream(d(su), d(si))
    for cls, kw in ((ops.EpochFlags, {"ordered": False}), (ops.EpochPresort, {})):
        ep = cls(nb, B, NU, NI, DEV, **kw)
        ep.run(ui, None, key, seed_, 0, err, sampler=sm)
        torch.cuda.synchronize()
        for q, arr in zip(("user", "pos", "neg"), ep.ids):
            assert np.array_equal(arr[:nb * B].cpu().numpy().astype(np.int64), np.concatenate(got[q])), (cls.__name__, q)
    # ... and the flagged-first order is a permutation of every batch's triples
    ep = ops.EpochFlags(nb, B, NU, NI, DEV)
    ep.run(ui, None, key, seed_, 0, err, sampler=sm)
    trip = np.stack([a[:nb * B].cpu().numpy().astype(np.int64) for a in ep.ids], axis=1).reshape(nb, B, 3)
    want = np.stack([np.concatenate(got[q]) for q in ("user", "pos", "neg")], axis=1).reshape(nb, B, 3)
    for b in range(nb):
        assert np.array_equal(trip[b][np.lexsort(trip[b].T)], want[b][np.lexsort(want[b].T)]), b
    assert err.item() == 0


def test_hinge_auc():
    ops = _ops()
    rs = np.random.RandomState(0)
    for B in (1, 63, 1000, 70_001):
        pos, neg = rs.normal(0, 1, B).astype(np.float32), rs.normal(0, 1, B).astype(np.float32)
        neg[::7] = pos[::7] + 1.0  # h == 2, and ties pos == neg - 1
        ls = torch.zeros(1, dtype=torch.float32, device=DEV)
        ac = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.hinge_auc(torch.from_numpy(pos).to(DEV), torch.from_numpy(neg).to(DEV), ls, ac)
        assert abs(ls.item() / B - float(onets.hinge_loss(pos, neg))) < 1e-5 * max(1.0, float(onets.hinge_loss(pos, neg)))
        assert ac.item() == int((pos > neg).sum())


@pytest.mark.parametrize("NI,B,nb,skew", [(1, 5, 2, False), (91, 256, 4, False), (16_384, 1000, 3, False),
                                          (16_385, 4096, 2, True), (100_000, 65_536, 3, False),
                                          (100_000, 65_536, 2, True), (100_000, 8192, 5, True),
                                          (131_072, 3001, 2, False), (131_073, 512, 2, False),
                                          (50_000, 131_072, 1, True), (50_000, 131_073, 1, False)])
def test_item_references_grouped_by_row(NI, B, nb, skew):
    """trs_epoch_presort's grouping of every batch's 2B item references — the hand-written counting sort in LDS (tables up
    to 8 chunks of 16 384 rows in rounds 1-2, any number since round 3: the same kernel walks more chunks) — sizes either side
    of the chunk and hand-over boundaries, ragged batches, hot rows longer than the staging buffer (zipf: a quarter of a
    65 536-batch on one row): per batch the keys are the batch's pos / neg rows in ascending order, the payloads a
    permutation of 0..2B-1 with ids[payload] == key.  Bit-exact (index work)."""
    ops = _ops()
    rs = np.random.RandomState(NI % 997 + B)
    n = nb * B
    draw = (lambda: (rs.zipf(1.3, n) % NI)) if skew else (lambda: rs.randint(0, NI, n))
    user = rs.randint(0, 50, n).astype(np.int32)
    pos, neg = draw().astype(np.int32), draw().astype(np.int32)
    if NI > 1:
        pos[:3], neg[:3] = NI - 1, 0  # first / last row of the table
    d = lambda a: torch.from_numpy(a).to(DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ps = ops.EpochPresort(nb, B, 50, NI, DEV, user_sort=False, item_flags=True)
    ps.run(None, None, 0, 0, 0, err, given_ids=(d(user), d(pos), d(neg)))
    torch.cuda.synchronize()
    assert err.item() == 0
    keys = ps.keys.view(torch.uint32)[2 * n:4 * n].cpu().numpy().astype(np.int64)
    vals = ps.vals.view(torch.uint32)[2 * n:4 * n].cpu().numpy().astype(np.int64)
    idup = ps.item_dup.cpu().numpy()
    for b in range(nb):
        k_, v_ = keys[2 * b * B:2 * (b + 1) * B], vals[2 * b * B:2 * (b + 1) * B]
        both = np.stack([pos[b * B:(b + 1) * B], neg[b * B:(b + 1) * B]], 1).reshape(-1).astype(np.int64)  # [2t + w]
        assert np.array_equal(k_, np.sort(both)), b
        assert np.array_equal(np.sort(v_), np.arange(2 * B)), b
        assert np.array_equal(both[v_], k_), b
        cnt = np.bincount(both, minlength=NI)
        assert np.array_equal(idup[b * B:(b + 1) * B].reshape(-1), (cnt[both] > 1).astype(np.uint8)), b


@pytest.mark.parametrize("NU,B,nb,skew", [(3, 7, 2, False), (400, 1000, 3, False), (20_000, 65_536, 2, True),
                                          (131_072, 4096, 2, False), (131_073, 4096, 2, False)])
def test_users_grouped_by_row_for_the_duplicate_runs(NU, B, nb, skew):
    """trs_epoch_user_dups: every batch's users grouped by row (the counting sort with ONE reference per position for user
    tables of any size, incl. a hot user longer than the staging buffer and one row more than 8 chunks of 16 384) —
    keys ascending per batch, payloads the slice positions of the batch, user[payload] == key; the duplicate flags == a
    bincount.  Bit-exact."""
    ops = _ops()
    rs = np.random.RandomState(NU % 991 + B)
    n = nb * B
    user = ((rs.zipf(1.2, n) % NU) if skew else rs.randint(0, NU, n)).astype(np.int32)
    user[:2] = NU - 1
    item = rs.randint(0, 50, n).astype(np.int32)
    d = lambda a: torch.from_numpy(a).to(DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ps = ops.EpochPresort(nb, B, NU, 50, DEV, user_sort=True, item_flags=False)
    ps.run(None, None, 0, 0, 0, err, given_ids=(d(user), d(item), d(item)))
    torch.cuda.synchronize()
    assert err.item() == 0 and ps.sorted_ukeys is not None
    keys = ps.ukeys.view(torch.uint32)[n:2 * n].cpu().numpy().astype(np.int64)
    vals = ps.uvals.view(torch.uint32)[n:2 * n].cpu().numpy().astype(np.int64)
    flags = ps.user_dup.cpu().numpy()
    for b in range(nb):
        k_, v_ = keys[b * B:(b + 1) * B], vals[b * B:(b + 1) * B]
        ub = user[b * B:(b + 1) * B].astype(np.int64)
        assert np.array_equal(k_, np.sort(ub)), b
        assert np.array_equal(np.sort(v_), np.arange(b * B, (b + 1) * B)), b
        assert np.array_equal(user[v_].astype(np.int64), k_), b
        assert np.array_equal(flags[b * B:(b + 1) * B], (np.bincount(ub, minlength=NU)[ub] > 1).astype(np.uint8)), b


@pytest.mark.parametrize("n,batch", [(1, 1), (1000, 7), (70_001, 512), (300, 1000), (65_536, 1024)])
def test_hinge_auc_batches(n, batch):
    """Per-batch hinge sums / AUC counts of consecutive batches in one launch (evaluate()): each slot equals the oracle's
    batch value; the AUC counts are exact integers."""
    ops = _ops()
    rs = np.random.RandomState(n)
    pos, neg = rs.normal(0, 1, n).astype(np.float32), rs.normal(0, 1, n).astype(np.float32)
    neg[::5] = pos[::5]  # ties: pos > neg is false
    nb = -(-n // batch)
    ls = torch.zeros(nb, dtype=torch.float32, device=DEV)
    ac = torch.zeros(nb, dtype=torch.int32, device=DEV)
    ops.hinge_auc_batches(torch.from_numpy(pos).to(DEV), torch.from_numpy(neg).to(DEV), batch, ls, ac)
    ls, ac = ls.cpu().numpy(), ac.cpu().numpy()
    for b in range(nb):
        p, q = pos[b * batch:(b + 1) * batch], neg[b * batch:(b + 1) * batch]
        want = float(onets.hinge_loss(p, q))
        assert abs(ls[b] / p.size - want) < 1e-5 * max(1.0, want), b
        assert ac[b] == int((p > q).sum()), b


@pytest.mark.parametrize("n,k", [(1, 1), (37, 10), (4096, 10), (4097, 5), (100_000, 10), (100_000, 2048),
                                 (1_000_003, 100),
                                 # k > 2048 (full-sort path; the reference sorts everything for any top_k, model.py:447)
                                 (2049, 2049), (4096, 4096), (5000, 5000), (10_000, 3000), (100_000, 100_000),
                                 (1_000_003, 5000)])
def test_topk_bit_exact(n, k):
    ops = _ops()
    rs = np.random.RandomState(n % 1000)
    sc = rs.normal(0, 1, n).astype(np.float32)
    if n > 100:
        sc[rs.randint(0, n, 50)] = sc.max()  # ties at the top: index-ascending order must hold
        sc[5] = -0.0
        sc[6] = 0.0
    out = ops.topk(torch.from_numpy(sc).to(DEV), k)
    assert np.array_equal(out.cpu().numpy(), onets.topk(sc, k))


@pytest.mark.parametrize("net,D,M", [("fm", 64, 0), ("fm", 16, 2), ("linear", 32, 0), ("linear", 8, 1)])
def test_score_all_items(net, D, M):
    ops = _ops()
    NI = 777
    p, batch, _ = make_case(net, D, M, 16, NU=20, NI=NI, seed=2)
    sizes = [p[f"metadata.{m}.weight"].shape[0] for m in range(M)]
    rs = np.random.RandomState(1)
    im = np.stack([rs.randint(0, sizes[m], NI) for m in range(M)], axis=1).astype(np.int32) if M else None
    t, T, Bt, ids, err, keep = to_dev(net, p, batch, np.int64)
    tim = None if im is None else torch.from_numpy(im).to(DEV)
    sc = ops.score_all_items(net, T, 3, NI, DEV, tim)
    items = np.arange(NI)
    fwd = onets.fm_forward if net == "fm" else onets.linear_forward
    ref = fwd(p, np.full(NI, 3), items, None if im is None else im.astype(np.int64)).reshape(-1)
    assert rel_err(sc.cpu().numpy(), ref) < TOL
    # chunked == unchunked (reference tests/test_model_and_features.py:203-215)
    parts = [ops.score_all_items(net, T, 3, NI, DEV, tim, item0=a, n=min(100, NI - a)) for a in range(0, NI, 100)]
    assert torch.equal(torch.cat(parts), sc)
    assert np.array_equal(ops.topk(sc, 10).cpu().numpy(), onets.topk(ref, 10)) or rel_err(sc.cpu().numpy(), ref) > 0


# ------------------------------------------------------------------------------------------------- MLP kernels
GEMM_SHAPES = [(128, 128, 32), (256, 384, 512), (1000, 130, 77), (37, 5, 3), (1, 1, 1), (513, 257, 1029),
               (4096, 128, 384), (130, 1, 64), (64, 300, 2)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("tA,tB", [(0, 1), (0, 0), (1, 0), (1, 1)])
def test_gemm_f32_all_layouts(M, N, K, tA, tB):
    ops = _ops()
    rs = np.random.RandomState(M + N + K)
    A = rs.normal(0, 1, (K, M) if tA else (M, K)).astype(np.float32)
    Bm = rs.normal(0, 1, (N, K) if tB else (K, N)).astype(np.float32)
    bias = rs.normal(0, 1, N).astype(np.float32)
    C0 = rs.normal(0, 1, (M, N)).astype(np.float32)
    opA, opB = (A.T if tA else A).astype(np.float64), (Bm.T if tB else Bm).astype(np.float64)
    ref = 0.5 * (opA @ opB) + 2.0 * C0 + bias
    out = torch.from_numpy(C0.copy()).to(DEV)
    ops.gemm(tA, tB, torch.from_numpy(A).to(DEV), torch.from_numpy(Bm).to(DEV), out=out,
             bias=torch.from_numpy(bias).to(DEV), alpha=0.5, beta=2.0)
    assert rel_err(out.cpu().numpy(), ref) < 2e-6
    out2 = ops.gemm(tA, tB, torch.from_numpy(A).to(DEV), torch.from_numpy(Bm).to(DEV))
    assert rel_err(out2.cpu().numpy(), opA @ opB) < 2e-6


@pytest.mark.parametrize("M,N,K,stats", [(32768, 512, 160, True), (32768, 384, 96, False), (65536, 256, 32, True)])
def test_gemm_f32_nt_lds_dma_kernel(M, N, K, stats, tune):
    """fp32 NT GEMMs whose 256-row tiles fill the chip take gemm32_nt_glds_kernel (256 x 256 tiles, or 256 x 128 when N is
    only a multiple of 128): exact-FMA products, bias, per-128-row BatchNorm partials; == the register-staged kernel
    (knob GEMM32_NO_GLDS = 1) to fp32 summation accuracy."""
    ops = _ops()
    rs = np.random.RandomState(M % 97 + N)
    A = torch.from_numpy(rs.normal(0, 1, (M, K)).astype(np.float32)).to(DEV)
    Bm = torch.from_numpy(rs.normal(0, 1, (N, K)).astype(np.float32)).to(DEV)
    bias = torch.from_numpy(rs.normal(0, 1, N).astype(np.float32)).to(DEV)
    ref = A.double() @ Bm.double().T + bias.double()[None, :]
    part = torch.empty((M // 128, 2, N), dtype=torch.float32, device=DEV) if stats else None
    out = ops.gemm(False, True, A, Bm, bias=bias, bn_part=part)
    assert float((out.double() - ref).abs().max()) < 2e-5 * float(ref.abs().max())
    if stats:
        r3 = ref.reshape(M // 128, 128, N)
        assert rel_err(part[:, 0].cpu().numpy(), r3.mean(dim=1).cpu().numpy()) < 1e-5
        assert rel_err(part[:, 1].cpu().numpy(), ((r3 - r3.mean(dim=1, keepdim=True)) ** 2).sum(dim=1).cpu().numpy()) < 1e-5
    tune(GEMM32_NO_GLDS=1)
    out2 = ops.gemm(False, True, A, Bm, bias=bias)
    assert float((out - out2).abs().max()) < 2e-5 * float(ref.abs().max())


def test_gemm_split_k_wgrad_shape_and_strided_views():
    """dW = dy^T x with K = 2B rows (split-K path) and operands that are column-slices of wider buffers."""
    ops = _ops()
    rs = np.random.RandomState(0)
    rows = 20_000
    dy = rs.normal(0, 1, (rows, 96)).astype(np.float32)
    x = rs.normal(0, 1, (rows, 200)).astype(np.float32)
    tdy, tx = torch.from_numpy(dy).to(DEV), torch.from_numpy(x).to(DEV)
    out = ops.gemm(True, False, tdy, tx)
    assert rel_err(out.cpu().numpy(), dy.astype(np.float64).T @ x.astype(np.float64)) < 3e-6
    out_v = ops.gemm(True, False, tdy[:, 8:72], tx[:, 40:168])  # row stride != width, 16-byte aligned
    assert rel_err(out_v.cpu().numpy(), dy[:, 8:72].astype(np.float64).T @ x[:, 40:168].astype(np.float64)) < 3e-6
    out_u = ops.gemm(True, False, tdy[:, 3:70], tx[:, 1:150])   # unaligned views: scalar-load path
    assert rel_err(out_u.cpu().numpy(), dy[:, 3:70].astype(np.float64).T @ x[:, 1:150].astype(np.float64)) < 3e-6
    # interior-tile fast path with an uneven split-K (412 k-tiles over 42 splits of 10: the last split has 2)
    rows = 412 * 32
    dy = rs.normal(0, 1, (rows, 512)).astype(np.float32)
    x = rs.normal(0, 1, (rows, 384)).astype(np.float32)
    out_f = ops.gemm(True, False, torch.from_numpy(dy).to(DEV), torch.from_numpy(x).to(DEV))
    assert rel_err(out_f.cpu().numpy(), dy.astype(np.float64).T @ x.astype(np.float64)) < 3e-6


@pytest.mark.parametrize("tile", ["128", "256", "512", "512-regstage"])
@pytest.mark.parametrize("B,K,H", [(256, 128, 256), (512, 256, 512), (384, 1280, 768)])
def test_gemm_bf16_resident_tiles_and_fused_bn_statistics(tile, B, K, H, tune):
    """The workgroup tiles of the bf16-resident kernels (128x128, 256x128, 256x256 filled by the LDS-DMA [NT form] and
    256x256 staged through registers; forced through the knobs GEMM16_TILE / GEMM16_NO_GLDS) give the same product, bf16
    output and per-128-row BatchNorm partials."""
    ops = _ops()
    tune(GEMM16_TILE=int(tile.split("-")[0]), GEMM16_NO_GLDS=1 if tile.endswith("regstage") else 0)
    rs = np.random.RandomState(B + K)
    rows = 2 * B
    x = torch.from_numpy(rs.normal(0, 1, (rows, K)).astype(np.float32)).to(DEV).to(torch.bfloat16)
    w = torch.from_numpy(rs.normal(0, 1, (H, K)).astype(np.float32)).to(DEV).to(torch.bfloat16)
    bias = torch.from_numpy(rs.normal(0, 1, H).astype(np.float32)).to(DEV)
    ref = x.double().cpu().numpy() @ w.double().cpu().numpy().T + bias.cpu().numpy()[None, :]
    part = torch.empty((rows // 128, 2, H), dtype=torch.float32, device=DEV)
    y = ops.gemm_bf16in(False, x, w, bias=bias, bn_part=part)
    assert rel_err(y.cpu().numpy(), ref) < 2e-6
    r3 = ref.reshape(rows // 128, 128, H)
    assert rel_err(part[:, 0].cpu().numpy(), r3.mean(axis=1)) < 1e-5
    assert rel_err(part[:, 1].cpu().numpy(), ((r3 - r3.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)) < 1e-5
    y16 = ops.gemm_bf16in(False, x, w, bias=bias, out_bf16=True)
    assert torch.equal(y16, y.to(torch.bfloat16))
    out_t = ops.gemm_bf16in(True, x, x)  # (K,K) = x^T x, both operands one row per k
    assert rel_err(out_t.cpu().numpy(), x.double().cpu().numpy().T @ x.double().cpu().numpy()) < 2e-6


@pytest.mark.parametrize("M,N,K", [(256, 128, 64), (384, 256, 448), (128, 384, 64 * 37)])
def test_gemm_bf16_resident_nt_and_tn(M, N, K):
    """bf16 operands in HBM, fp32 accumulate: exact products of the bf16 values, so the fp64 product of the SAME rounded
    operands is matched to fp32 summation accuracy.  tn: both operands stored one row per k (ds_read_b64_tr_b16)."""
    ops = _ops()
    rs = np.random.RandomState(M + N + K)
    A = torch.from_numpy(rs.normal(0, 1, (M, K)).astype(np.float32)).to(DEV)
    Bm = torch.from_numpy(rs.normal(0, 1, (N, K)).astype(np.float32)).to(DEV)
    bias = torch.from_numpy(rs.normal(0, 1, N).astype(np.float32)).to(DEV)
    Ab, Bb = A.to(torch.bfloat16), Bm.to(torch.bfloat16)
    ref = Ab.double().cpu().numpy() @ Bb.double().cpu().numpy().T
    out = ops.gemm_bf16in(False, Ab, Bb, bias=bias)
    assert rel_err(out.cpu().numpy(), ref + bias.cpu().numpy()[None, :]) < 2e-6
    out_t = ops.gemm_bf16in(True, Ab.t().contiguous(), Bb.t().contiguous())  # (K,M), (K,N)
    assert rel_err(out_t.cpu().numpy(), ref) < 2e-6
    # weight images: bf16 copy + transposed copy, RNE like torch
    w = torch.from_numpy(rs.normal(0, 1, (70, 45)).astype(np.float32)).to(DEV)
    d, dt = torch.empty((70, 45), dtype=torch.bfloat16, device=DEV), torch.empty((45, 70), dtype=torch.bfloat16, device=DEV)
    ops.f32_to_bf16(w, d, dt)
    assert torch.equal(d, w.to(torch.bfloat16)) and torch.equal(dt, w.to(torch.bfloat16).t().contiguous())
    # ... of several matrices in one launch (every layer's images of an MLP step)
    ws = [torch.from_numpy(rs.normal(0, 1, sh).astype(np.float32)).to(DEV) for sh in ((70, 45), (128, 256), (33, 1), (5, 97))]
    ds = [torch.empty(w_.shape, dtype=torch.bfloat16, device=DEV) for w_ in ws]
    dts = [torch.empty(w_.shape[::-1], dtype=torch.bfloat16, device=DEV) for w_ in ws]
    dts[2] = None
    wi = ops.WeightImages(ws, ds, dts)
    wi.refresh()
    for w_, d_, dt_ in zip(ws, ds, dts):
        assert torch.equal(d_, w_.to(torch.bfloat16))
        assert dt_ is None or torch.equal(dt_, w_.to(torch.bfloat16).t().contiguous())
    ws[1].mul_(2.0)
    wi.refresh()
    assert torch.equal(ds[1], ws[1].to(torch.bfloat16))
    with pytest.raises(ValueError):
        ops.WeightImages(ws * 3, ds * 3, dts * 3)


@pytest.mark.parametrize("H,Kin,rows", [(256, 384, 64 * 300), (512, 1024, 64 * 257), (1024, 768, 8192)])
def test_gemm_bf16_resident_split_k_wgrad_shape(H, Kin, rows):
    """dW = dy^T x over many rows (split-K slabs).  (512, 1024) and (1024, 768) take the 256 x 256 tiles with an uneven
    last split (257 k-tiles); (256, 384) the 128-tile kernel."""
    ops = _ops()
    rs = np.random.RandomState(3)
    dy = torch.from_numpy(rs.normal(0, 1, (rows, H)).astype(np.float32)).to(DEV).to(torch.bfloat16)
    x = torch.from_numpy(rs.normal(0, 1, (rows, Kin)).astype(np.float32)).to(DEV).to(torch.bfloat16)
    out = ops.gemm_bf16in(True, dy, x)
    assert rel_err(out.cpu().numpy(), dy.double().cpu().numpy().T @ x.double().cpu().numpy()) < 3e-6
    # out = alpha * product + beta * out in place (the SGD step folded into the weight gradient): (alpha * sum) + beta * W
    # on the sums of the call above, bit for bit
    W = torch.from_numpy(rs.normal(0, 1, (H, Kin)).astype(np.float32)).to(DEV)
    W0 = W.clone()
    ops.gemm_bf16in(True, dy, x, out=W, alpha=-0.05, beta=1.0)
    assert torch.equal(W, W0 + (-0.05) * out)
    ops.gemm_bf16in(True, dy, x, out=W, alpha=0.5, beta=-2.0)
    assert torch.equal(W, 0.5 * out + (-2.0) * (W0 + (-0.05) * out))


def test_gemm_bf16_resident_alpha_beta_without_split_k():
    """The same epilogue inside the GEMM kernels (one k-split: short K, and the NT form)."""
    ops = _ops()
    rs = np.random.RandomState(4)
    for tn, (M, N, K) in ((True, (256, 256, 128)), (True, (128, 384, 64)), (False, (512, 256, 128)), (False, (128, 128, 64))):
        A = torch.from_numpy(rs.normal(0, 1, (K, M) if tn else (M, K)).astype(np.float32)).to(DEV).to(torch.bfloat16)
        Bm = torch.from_numpy(rs.normal(0, 1, (K, N) if tn else (N, K)).astype(np.float32)).to(DEV).to(torch.bfloat16)
        prod = ops.gemm_bf16in(tn, A, Bm)
        C0 = torch.from_numpy(rs.normal(0, 1, (M, N)).astype(np.float32)).to(DEV)
        C = C0.clone()
        ops.gemm_bf16in(tn, A, Bm, out=C, alpha=-0.3, beta=1.0)
        assert rel_err(C.cpu().numpy(), (C0.double() - 0.3 * prod.double()).cpu().numpy()) < 1e-6, (tn, M, N, K)
    with pytest.raises(ValueError):
        ops.gemm_bf16in(False, A, Bm, out_bf16=True, beta=1.0)


@pytest.mark.parametrize("D,M,B,n_cat", [(8, 0, 300, 0), (64, 1, 1000, 37), (256, 3, 4096, 1000), (128, 2, 777, 5000),
                                          (256, 3, 2000, 10_000)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("flags", [False, True])
def test_mlp_embed_sgd_update(D, M, B, n_cat, dt, flags):
    """trs_mlp_embed_sgd_update: every embedding table of an MLP step from d x0 in two launches — W[row] -= lr * (sum of
    the row's d x0 segments), the user's two passes merged, duplicate-free references (flags) as plain read-modify-writes,
    metadata tables by owner-computes LDS sums — against the float64 scatter-add of the same (bf16-rounded) d x0."""
    ops = _ops()
    rs = np.random.RandomState(D + M + B)
    NU, NI, lr = 500, 300, 0.37
    F = 2 + M
    user = rs.randint(0, NU, B).astype(np.int64)
    pos = (rs.zipf(1.5, B) % NI).astype(np.int64)   # hot items: duplicates inside the batch
    neg = rs.randint(0, NI, B).astype(np.int64)
    user[:5] = user[5:10]                            # duplicated users too
    pm = rs.randint(0, max(n_cat, 1), (B, M)).astype(np.int64)
    nm = rs.randint(0, max(n_cat, 1), (B, M)).astype(np.int64)
    if M:
        pm[:, 0] = np.minimum(pm[:, 0], n_cat - 1)
        pm[:3, 0], nm[:3, 0] = n_cat - 1, 0          # first / last category
    tabs = [rs.normal(0, 1, (n, D)).astype(np.float32) for n in [NU, NI] + [n_cat] * M]
    dx = rs.normal(0, 1, (2 * B, F * D + 8)).astype(np.float32)   # row stride wider than the F blocks
    d = lambda a: torch.from_numpy(a).to(DEV)
    tdx = d(dx)
    if dt == "bf16":
        tdx = tdx.to(torch.bfloat16)
        dx = tdx.float().cpu().numpy()
    want = [t.astype(np.float64) for t in tabs]
    np.add.at(want[0], user, -lr * (dx[:B, :D].astype(np.float64) + dx[B:, :D]))
    np.add.at(want[1], pos, -lr * dx[:B, D:2 * D].astype(np.float64))
    np.add.at(want[1], neg, -lr * dx[B:, D:2 * D].astype(np.float64))
    for m in range(M):
        np.add.at(want[2 + m], pm[:, m], -lr * dx[:B, (2 + m) * D:(3 + m) * D].astype(np.float64))
        np.add.at(want[2 + m], nm[:, m], -lr * dx[B:, (2 + m) * D:(3 + m) * D].astype(np.float64))
    ttabs = [d(t.copy()) for t in tabs]
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    T, keep = ops.make_tables(ttabs[0], ttabs[1], None, None, ttabs[2:], [])
    ids = [d(user), d(pos), d(neg)] + ([d(pm), d(nm)] if M else [None, None])
    Bt, keep2 = ops.make_batch(*ids, err)
    assert ops.mlp_embed_sgd_supported(T)
    ud = idp = None
    if flags:
        ud = d((np.bincount(user, minlength=NU)[user] > 1).astype(np.uint8))
        cnt = np.bincount(np.concatenate([pos, neg]), minlength=NI)
        idp = d(np.stack([cnt[pos] > 1, cnt[neg] > 1], 1).astype(np.uint8))
    ops.mlp_embed_sgd_update(T, Bt, tdx, lr, ud, idp)
    torch.cuda.synchronize()
    assert err.item() == 0
    for k, (got, w) in enumerate(zip(ttabs, want)):
        assert np.abs(got.cpu().numpy() - w).max() < 1e-5 * max(1.0, np.abs(w).max()) * 8, k
    # an id outside its table: skipped and flagged
    bad = d(np.full(B, NU + 3, dtype=np.int64))
    Bt2, keep3 = ops.make_batch(bad, ids[1], ids[2], ids[3], ids[4], err)
    before = ttabs[0].clone()
    ops.mlp_embed_sgd_update(T, Bt2, tdx, lr)
    torch.cuda.synchronize()
    assert err.item() == 1 and torch.equal(ttabs[0], before)


def test_mlp_embed_sgd_update_refuses_what_it_cannot_do():
    ops = _ops()
    big = torch.zeros((300_000, 256), device=DEV)
    small = torch.zeros((10, 256), device=DEV)
    T, keep = ops.make_tables(small, small, None, None, [big, big, big], [])
    assert not ops.mlp_embed_sgd_supported(T)       # 300 K categories x 3 columns: the per-table scatter's job
    T2, keep2 = ops.make_tables(torch.zeros((10, 6), device=DEV), torch.zeros((10, 6), device=DEV))
    assert not ops.mlp_embed_sgd_supported(T2)      # D % 4 != 0


@pytest.mark.parametrize("B", [300, 128 * 16 * 12 - 5, 128 * 16 * 30, 128 * 16 * 40 + 77])
def test_bn_statistics_finalise_kernels_agree(B, tune):
    """The finalise of the BatchNorm batch statistics: the kernel that keeps a thread's chunk partials in registers (up to
    8 / 16 / 32 chunks per thread) and the two-sweep kernel (longer chunk lists; forced by the knob BN_FINAL_TWO_SWEEPS = 1) add
    in the same order — bit-identical mean / variance / running statistics."""
    ops = _ops()
    rs = np.random.RandomState(B % 1000)
    H, passes = 40, 2
    y = torch.from_numpy((rs.normal(0, 1, (passes * B, H)) * rs.uniform(0.1, 3, H) + rs.normal(0, 5, H)).astype(np.float32)).to(DEV)
    dx = torch.from_numpy(rs.normal(0, 1, (passes * B, H)).astype(np.float32)).to(DEV)
    gam = torch.from_numpy(rs.uniform(0.5, 1.5, H).astype(np.float32)).to(DEV)
    bet = torch.from_numpy(rs.normal(0, 0.5, H).astype(np.float32)).to(DEV)
    rw = torch.from_numpy(rs.normal(0, 1, passes * B).astype(np.float32)).to(DEV)
    res = []
    for two in ("0", "1"):
        tune(BN_FINAL_TWO_SWEEPS=int(two))
        mean, var = torch.empty((passes, H), device=DEV), torch.empty((passes, H), device=DEV)
        rm, rv = torch.zeros(H, device=DEV), torch.ones(H, device=DEV)
        ops.bn_batch_stats(y, B, passes, 0.1, mean, var, rm, rv)
        # ... and the finalise kernels of the backward sums / column sums (both passes' partials in registers)
        dy, dg, db, dbias = torch.empty_like(y), torch.empty(H, device=DEV), torch.empty(H, device=DEV), torch.empty(H, device=DEV)
        ops.bn_relu_backward(y, dx, B, passes, True, mean, var, gam, bet, 1e-5, dy, dg, db, dy_colsum=dbias)
        cs = torch.empty(H, device=DEV)
        ops.colsum(y, cs, row_weight=rw, passes=passes)
        res.append((mean, var, rm, rv, dy, dg, db, dbias, cs))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    y64 = y.double().reshape(passes, B, H)
    assert rel_err(res[0][0].cpu().numpy(), y64.mean(1).cpu().numpy()) < 1e-6
    assert rel_err(res[0][1].cpu().numpy(), y64.var(1, unbiased=False).cpu().numpy()) < 1e-6


@pytest.mark.parametrize("B,H", [(64, 32), (1000, 130), (5000, 7), (256, 512), (300, 256), (97, 128)])
@pytest.mark.parametrize("passes", [1, 2])
def test_bn_stats_forward_backward(B, H, passes):
    ops = _ops()
    rs = np.random.RandomState(B + H)
    rows = B * passes
    y = (rs.normal(0, 1, (rows, H)) * rs.uniform(0.1, 3, H) + rs.normal(0, 5, H)).astype(np.float32)
    gamma, beta = rs.uniform(0.5, 1.5, H).astype(np.float32), rs.normal(0, 0.5, H).astype(np.float32)
    rm0, rv0 = rs.normal(0, 1, H).astype(np.float32), rs.uniform(0.5, 2, H).astype(np.float32)
    ty = torch.from_numpy(y).to(DEV)
    mean = torch.empty((passes, H), device=DEV)
    var = torch.empty((passes, H), device=DEV)
    rm, rv = torch.from_numpy(rm0.copy()).to(DEV), torch.from_numpy(rv0.copy()).to(DEV)
    ops.bn_batch_stats(ty, B, passes, 0.1, mean, var, rm, rv)
    y64 = y.astype(np.float64).reshape(passes, B, H)
    rmean, rvar = y64.mean(axis=1), y64.var(axis=1)
    assert rel_err(mean.cpu().numpy(), rmean) < 1e-6 and rel_err(var.cpu().numpy(), rvar) < 1e-6
    erm, erv = rm0.astype(np.float64), rv0.astype(np.float64)
    for p in range(passes):
        erm = 0.9 * erm + 0.1 * rmean[p]
        erv = 0.9 * erv + 0.1 * rvar[p] * B / max(B - 1, 1)
    assert rel_err(rm.cpu().numpy(), erm) < 1e-6 and rel_err(rv.cpu().numpy(), erv) < 1e-6
    tg, tb = torch.from_numpy(gamma).to(DEV), torch.from_numpy(beta).to(DEV)
    out = torch.empty_like(ty)
    ops.bn_relu_forward(ty, B, passes, True, passes, mean, var, tg, tb, 1e-5, out)
    # the running update riding in the forward launch == the one bn_batch_stats made above, bit for bit; same output
    rm2, rv2 = torch.from_numpy(rm0.copy()).to(DEV), torch.from_numpy(rv0.copy()).to(DEV)
    out2 = torch.empty_like(ty)
    nbt = torch.tensor(5, dtype=torch.int64, device=DEV)
    ops.bn_relu_forward(ty, B, passes, True, passes, mean, var, tg, tb, 1e-5, out2, momentum=0.1, running_mean=rm2,
                        running_var=rv2, tracked=nbt)
    assert torch.equal(rm2, rm) and torch.equal(rv2, rv) and torch.equal(out2, out)
    assert int(nbt.item()) == 5 + passes  # BatchNorm1d.num_batches_tracked rides along
    # the H -> 1 output layer from the same launch (H a power of two <= 256: a row sits in one wave) or by the row-dot
    # kernel behind it (wide / unaligned layers): scores = out . w + bias
    wv = torch.from_numpy(rs.normal(0, 1, H).astype(np.float32)).to(DEV)
    bv = torch.from_numpy(rs.normal(0, 1, 1).astype(np.float32)).to(DEV)
    sc = torch.full((rows,), float("nan"), device=DEV)
    out3 = torch.empty_like(ty)
    ops.bn_relu_forward(ty, B, passes, True, passes, mean, var, tg, tb, 1e-5, out3, dot=(wv, bv, sc))
    assert torch.equal(out3, out)
    assert rel_err(sc.cpu().numpy(), out.double().cpu().numpy() @ wv.double().cpu().numpy() + float(bv.item())) < 1e-6
    sc0 = torch.empty_like(sc)
    ops.rowdot(out, wv, bv, sc0)
    assert rel_err(sc.cpu().numpy(), sc0.cpu().numpy()) < 1e-6
    if passes == 2:  # eval-mode statistics (one shared set) cannot feed a running update
        with pytest.raises(RuntimeError, match="running update"):
            ops.bn_relu_forward(ty, B, passes, True, 1, mean, var, tg, tb, 1e-5, out2, momentum=0.1, running_mean=rm2,
                                running_var=rv2)
    xhat = (y64 - rmean[:, None, :]) / np.sqrt(rvar[:, None, :] + 1e-5)
    yhat = xhat * gamma + beta
    assert rel_err(out.cpu().numpy(), np.maximum(yhat, 0).reshape(rows, H)) < 1e-5  # fp32 (y - mean) with |mean| ~ 5 sigma
    # backward
    dx = rs.normal(0, 1, (rows, H)).astype(np.float32)
    tdx = torch.from_numpy(dx).to(DEV)
    dy, dg, db = torch.empty_like(ty), torch.empty(H, device=DEV), torch.empty(H, device=DEV)
    dbias = torch.empty(H, device=DEV)
    ops.bn_relu_backward(ty, tdx, B, passes, True, mean, var, tg, tb, 1e-5, dy, dg, db, dy_colsum=dbias)
    # column sums of dy (the Linear bias gradient under BatchNorm) are rounding noise around an exact 0
    assert np.abs(dbias.cpu().numpy() - dy.double().sum(0).cpu().numpy()).max() < 1e-4 * np.abs(dy.cpu().numpy()).max() * np.sqrt(rows)
    d = dx.astype(np.float64).reshape(passes, B, H) * (yhat > 0)
    s1, s2 = d.sum(axis=1, keepdims=True), (d * xhat).sum(axis=1, keepdims=True)
    ref_dy = gamma / np.sqrt(rvar[:, None, :] + 1e-5) * (d - s1 / B - xhat * s2 / B)
    assert rel_err(dy.cpu().numpy(), ref_dy.reshape(rows, H)) < 2e-5
    assert rel_err(dg.cpu().numpy(), s2.sum(axis=0).reshape(-1)) < 2e-5
    assert rel_err(db.cpu().numpy(), s1.sum(axis=0).reshape(-1)) < 2e-5
    if H % 4 == 0:  # outer-product form: dx[r][c] = g[r] * w[c] formed inside the kernels == the materialised dx
        g = rs.normal(0, 1, rows).astype(np.float32)
        w = rs.normal(0, 1, H).astype(np.float32)
        tgv, tw = torch.from_numpy(g).to(DEV), torch.from_numpy(w).to(DEV)
        dxo = torch.empty_like(ty)
        ops.outer(tgv, tw, dxo)
        dy_a, dg_a, db_a = torch.empty_like(ty), torch.empty(H, device=DEV), torch.empty(H, device=DEV)
        dy_b, dg_b, db_b = torch.empty_like(ty), torch.empty(H, device=DEV), torch.empty(H, device=DEV)
        ops.bn_relu_backward(ty, dxo, B, passes, True, mean, var, tg, tb, 1e-5, dy_a, dg_a, db_a)
        ops.bn_relu_backward(ty, None, B, passes, True, mean, var, tg, tb, 1e-5, dy_b, dg_b, db_b, outer=(tgv, tw))
        assert torch.equal(dy_a, dy_b) and torch.equal(dg_a, dg_b) and torch.equal(db_a, db_b)
        # ... and the output layer's weight gradient sum_r g[r] * relu(bn(y))[r] out of the same reduce pass == the weighted
        # column sums of the stored activations; everything else unchanged
        xw = torch.full((H,), float("nan"), device=DEV)
        dy_c, dg_c, db_c = torch.empty_like(ty), torch.empty(H, device=DEV), torch.empty(H, device=DEV)
        ops.bn_relu_backward(ty, None, B, passes, True, mean, var, tg, tb, 1e-5, dy_c, dg_c, db_c, outer=(tgv, tw), outer_xw=xw)
        assert torch.equal(dy_c, dy_b) and torch.equal(dg_c, dg_b) and torch.equal(db_c, db_b)
        ref_xw = (g.astype(np.float64)[:, None] * np.maximum(yhat, 0).reshape(rows, H)).sum(0)
        assert rel_err(xw.cpu().numpy(), ref_xw) < 2e-5
        xw2 = torch.empty(H, device=DEV)
        ops.colsum(out, xw2, row_weight=tgv, passes=passes)
        assert rel_err(xw.cpu().numpy(), xw2.cpu().numpy()) < 2e-5
        with pytest.raises(RuntimeError, match="outer_xw"):  # no BatchNorm: no reduce pass to ride in
            ops.bn_relu_backward(ty, None, B, passes, False, None, None, None, None, 1e-5, dy_c, None, None,
                                 outer=(tgv, tw), outer_xw=xw)
        # forward without a stored output: the dot alone, where the launch forms it
        if ops.bn_relu_forward_forms_dot(ty):
            sc2 = torch.empty_like(sc)
            ops.bn_relu_forward(ty, B, passes, True, passes, mean, var, tg, tb, 1e-5, None, dot=(wv, bv, sc2))
            assert torch.equal(sc2, sc)
        else:
            with pytest.raises(RuntimeError, match="out_dev"):
                ops.bn_relu_forward(ty, B, passes, True, passes, mean, var, tg, tb, 1e-5, None, dot=(wv, bv, sc))
        ops.bn_relu_backward(ty, None, B, passes, False, None, None, None, None, 1e-5, dy_b, None, None, outer=(tgv, tw))
        assert np.array_equal(dy_b.cpu().numpy(), dxo.cpu().numpy() * (y > 0))
    # no-BN variants
    ops.bn_relu_forward(ty, B, passes, False, 1, None, None, None, None, 1e-5, out)
    assert np.array_equal(out.cpu().numpy(), np.maximum(y, 0))
    ops.bn_relu_backward(ty, tdx, B, passes, False, None, None, None, None, 1e-5, dy, None, None, dy_colsum=dbias)
    assert np.array_equal(dy.cpu().numpy(), dx * (y > 0))
    assert rel_err(dbias.cpu().numpy(), (dx.astype(np.float64) * (y > 0)).sum(0)) < 2e-5
    if passes == 2:  # negative pass = exact negation of the positive one: the bias gradient cancels to an exact 0
        ty2, tdx2 = torch.cat([ty[:B], ty[:B]]), torch.cat([tdx[:B], -tdx[:B]])
        ops.bn_relu_backward(ty2, tdx2, B, 2, False, None, None, None, None, 1e-5, dy, None, None, dy_colsum=dbias)
        assert np.array_equal(dbias.cpu().numpy(), np.zeros(H, np.float32))


def test_colsum_rowdot_outer_gather():
    ops = _ops()
    rs = np.random.RandomState(1)
    rows, H = 3001, 77
    x = rs.normal(0, 1, (rows, H)).astype(np.float32)
    w = rs.normal(0, 1, rows).astype(np.float32)
    tx, tw = torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV)
    out = torch.empty(H, device=DEV)
    ops.colsum(tx, out)
    assert rel_err(out.cpu().numpy(), x.astype(np.float64).sum(0)) < 1e-6
    ops.colsum(tx, out, row_weight=tw)
    assert rel_err(out.cpu().numpy(), (x.astype(np.float64) * w[:, None]).sum(0)) < 1e-6
    wv, b = rs.normal(0, 1, H).astype(np.float32), np.float32(0.3)
    sc = torch.empty(rows, device=DEV)
    ops.rowdot(tx, torch.from_numpy(wv).to(DEV), torch.tensor([b], device=DEV), sc)
    assert rel_err(sc.cpu().numpy(), x.astype(np.float64) @ wv + b) < 1e-6
    dx = torch.empty_like(tx)
    ops.outer(tw, torch.from_numpy(wv).to(DEV), dx)
    assert np.array_equal(dx.cpu().numpy(), w[:, None] * wv[None, :])
    # gather-concat, both passes, metadata
    for D, M in ((8, 0), (16, 2), (10, 1)):
        p, batch, _ = make_case("fm", D, M, 50, seed=4)
        t, T, Bt, ids, err, keep = to_dev("fm", p, batch, np.int64)
        F = 2 + M
        xg = torch.empty((100, F * D), device=DEV)
        ops.mlp_gather_concat(T, Bt, 2, xg)
        for pas, ik, mk in ((0, "pos_item_id", "pos_metadata_id"), (1, "neg_item_id", "neg_metadata_id")):
            cols = [p["user.weight"][batch["user_id"]], p["item.weight"][batch[ik]]]
            cols += [p[f"metadata.{m}.weight"][batch[mk][:, m]] for m in range(M)]
            assert np.array_equal(xg[pas * 50:(pas + 1) * 50].cpu().numpy(), np.concatenate(cols, axis=1))


FAST_SGD_STEP = [("fm", 64), ("fm", 8), ("fm", 128), ("fm", 80), ("fm", 10), ("linear", 32), ("linear", 256), ("linear", 7),
                 ("fm", 512), ("fm", 1024), ("linear", 3), ("fm", 201), ("linear", 12), ("fm", 33)]


@pytest.mark.parametrize("net,D", FAST_SGD_STEP)
def test_fast_sgd_step_matches_oracle_and_generic_path(net, D):
    """csrc/fast_step.hip (3-kernel exact SGD step, ids given) vs the oracle and vs the generic staged path.  The last
    six widths are the row shapes (4,64,2), (4,64,4), (1,4,1), (1,64,4), (4,4,1) and (1,64,1) of csrc/score_kernels.h's
    table; with the widths before them every shape of the table is met (tests/test_gpu_row_shapes.py: every shape, ragged
    and full, on every path)."""
    check_fast_sgd_step(net, D)


@functools.lru_cache(maxsize=4)
def fast_sgd_step_case(net, D, lr=None):
    """The input of check_fast_sgd_step (no GPU): one batch of 777 on 90 users and 41 items, three steps on it."""
    def build(bump):
        B = 777
        p, batch, _ = make_case(net, D, 0, B, NU=90, NI=41, seed=D + 1000 * bump)
        return sens.StepCase(net, sens.condition_tables(net, p), [batch] * 3, lr_of(B, D, lr), D=D)
    return sens.conditioned(build, first=lr is not None)


def check_fast_sgd_step(net, D, first_stamp=1, prepare_scratch=None):
    """first_stamp / prepare_scratch(scratch, net, NU, NI, B, D): the step stamps and the state of the duplicate-detection
    scratch a long run arrives with (tests/test_gpu_long_run.py)."""
    ops = _ops()
    case = fast_sgd_step_case(net, D)
    p, batch, B, lr = case.p, case.batches[0], case.B, case.lr
    t, T, Bt, ids, err, keep = to_dev(net, p, batch, np.int32)
    gz = torch.empty((2, B), device=DEV)
    du = torch.empty((B, D), device=DEV)
    losses = torch.zeros(3, device=DEV)
    scratch = ops.train_scratch(90, 41, B, D, DEV) if D != 8 else None  # D == 8 exercises the all-atomic variant
    if prepare_scratch is not None:
        prepare_scratch(scratch, net, 90, 41, B, D)
    for step in range(3):
        ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, 1, lr, ids["user_id"], ids["pos_item_id"],
                            ids["neg_item_id"], gz, du, losses[step:step + 1], err, scratch, first_stamp + step)
    sens.assert_losses(case, losses.cpu().numpy())
    sens.criterion_for(case)(tables_to_host(t), case.ref, p)
    assert err.item() == 0
    # generic path from the same start: same result to rounding
    t2, T2, Bt2, ids2, err2, keep2 = to_dev(net, p, batch, np.int32)
    for step in range(3):
        ls = torch.zeros(1, device=DEV)
        _, _, gr, gl = ops.score_fwd_bwd(net, T2, Bt2, B, D, 0, DEV, ls, want_scores=False)
        ops.score_sgd_update(net, T2, Bt2, gr, gl, lr)
    for k in p:
        assert rel_err(t[k].cpu().numpy(), t2[k].cpu().numpy()) < 1e-6, k


RESIDENT_TOL = 1e-6  # fast path against generic path: the same sums in another order


@functools.lru_cache(maxsize=4)
def resident_stream_case(lr=None):
    """The input of test_fast_sgd_steps_from_resident_stream (no GPU): a stream of 5000 interactions, 5 batches of 512
    from epoch position 1024 as the device RNG derives them (oracle/loader.py restates it).  The criterion's bar is ten
    times tighter than TOL, so a tenth of the usual step size per triple meets the same ratio."""
    def build(bump):
        rs = np.random.RandomState(3 + 1000 * bump)
        N, NU, NI, D, B = 5000, 300, 77, 16, 512
        su, si = rs.randint(0, NU, N).astype(np.int32), rs.randint(0, NI, N).astype(np.int32)
        p, _, _ = make_case("fm", D, 0, 8, NU=NU, NI=NI, seed=1)
        key, seed_, n_steps = 0xFEEDBEEF12, 4242, 5
        batches = []
        for s_ in range(n_steps):
            t0 = 1024 + s_ * B
            out = oloader.device_batch(su, si, None, key, t0, B, NI, seed_, t0)
            batches.append(sens.batch_of(np.asarray(out["user"]), np.asarray(out["pos"]), np.asarray(out["neg"])))
        return sens.StepCase("fm", sens.condition_tables("fm", p), batches, max(0.1, sens.step_lr(B) * RESIDENT_TOL / TOL) if lr is None else lr,
                             tol=RESIDENT_TOL, su=su, si=si, NU=NU, NI=NI, D=D, key=key, seed_=seed_)
    return sens.conditioned(build, first=lr is not None)


def test_fast_sgd_steps_from_resident_stream():
    """The C step loop deriving its batches from the stream == batch_prepare + generic step, step by step."""
    ops = _ops()
    case = resident_stream_case()
    p, su, si, NU, NI, D, B, lr = case.p, case.su, case.si, case.NU, case.NI, case.D, case.B, case.lr
    dsu, dsi = torch.from_numpy(su).to(DEV), torch.from_numpy(si).to(DEV)
    key, seed_, n_steps = case.key, case.seed_, case.nb
    # fast: one C call for 5 steps starting at epoch position 1024
    ta = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in p.items()}
    Ta, keepa = ops.make_tables(ta["user.weight"], ta["item.weight"], ta["linear_user.weight"], ta["linear_item.weight"])
    bufs = [torch.empty(B, dtype=torch.int32, device=DEV) for _ in range(3)]
    gz, du = torch.empty((2, B), device=DEV), torch.empty((B, D), device=DEV)
    la = torch.zeros(n_steps, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.train_steps_sgd("fm", Ta, ops.interleave_stream(dsu, dsi), None, key, seed_, 1024, B, n_steps, lr, *bufs, gz, du, la, err,
                        ops.train_scratch(NU, NI, B, D, DEV), 7)
    # generic: batch_prepare + fwd_bwd + sgd_update per step
    tb = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in p.items()}
    Tb, keepb = ops.make_tables(tb["user.weight"], tb["item.weight"], tb["linear_user.weight"], tb["linear_item.weight"])
    lb = torch.zeros(n_steps, device=DEV)
    for s in range(n_steps):
        t0 = 1024 + s * B
        out = ops.batch_prepare(dsu, dsi, None, key, t0, B, NI, seed_, t0)
        for q, name in (("user", "user_id"), ("pos", "pos_item_id"), ("neg", "neg_item_id")):  # (the case's batches)
            assert np.array_equal(out[q].cpu().numpy().astype(np.int64), case.batches[s][name]), (s, q)
        Bt, kb = ops.make_batch(out["user"], out["pos"], out["neg"], None, None, err)
        _, _, gr, gl = ops.score_fwd_bwd("fm", Tb, Bt, B, D, 0, DEV, lb[s:s + 1], want_scores=False)
        ops.score_sgd_update("fm", Tb, Bt, gr, gl, lr)
    torch.cuda.synchronize()
    assert torch.equal(bufs[0], out["user"]) and torch.equal(bufs[1], out["pos"]) and torch.equal(bufs[2], out["neg"])
    assert np.allclose(la.cpu().numpy(), lb.cpu().numpy(), rtol=1e-6)
    sens.ValueCriterion(RESIDENT_TOL)(tables_to_host(ta), tables_to_host(tb), p)
    assert err.item() == 0


@pytest.mark.parametrize("M,N,K", [(256, 384, 512), (1000, 130, 77), (37, 5, 3), (513, 257, 1029), (4096, 128, 384)])
@pytest.mark.parametrize("tA,tB", [(0, 1), (0, 0), (1, 0), (1, 1)])
def test_gemm_bf16_inputs_fp32_accumulate(M, N, K, tA, tB):
    """bf16 GEMM == fp32 GEMM of the bf16-rounded operands (exact products, fp32 accumulation order aside)."""
    ops = _ops()
    rs = np.random.RandomState(M + N + K)
    A = rs.normal(0, 1, (K, M) if tA else (M, K)).astype(np.float32)
    Bm = rs.normal(0, 1, (N, K) if tB else (K, N)).astype(np.float32)
    bias = rs.normal(0, 1, N).astype(np.float32)
    tA_, tB_ = torch.from_numpy(A).to(DEV), torch.from_numpy(Bm).to(DEV)
    Ar = tA_.to(torch.bfloat16).float().cpu().numpy().astype(np.float64)   # RNE rounding, as v_cvt_pk_bf16_f32
    Br = tB_.to(torch.bfloat16).float().cpu().numpy().astype(np.float64)
    ref = (Ar.T if tA else Ar) @ (Br.T if tB else Br) + bias
    out = ops.gemm(tA, tB, tA_, tB_, bias=torch.from_numpy(bias).to(DEV), bf16=True)
    assert rel_err(out.cpu().numpy(), ref) < 3e-6
    full = (A.T if tA else A).astype(np.float64) @ (Bm.T if tB else Bm).astype(np.float64) + bias
    assert rel_err(out.cpu().numpy(), full) < 2e-2  # bf16 operand rounding


@pytest.mark.parametrize("B,passes,K,H", [(256, 2, 40, 96), (1000, 1, 77, 130), (128, 2, 384, 512), (333, 1, 16, 7)])
@pytest.mark.parametrize("bf16", [False, True])
def test_gemm_fused_bn_statistics(B, passes, K, H, bf16):
    """BatchNorm batch statistics from the GEMM epilogue (+ finalize) == the stand-alone statistics kernels."""
    ops = _ops()
    rs = np.random.RandomState(B + H)
    rows = B * passes
    x = torch.from_numpy(rs.normal(0, 1, (rows, K)).astype(np.float32)).to(DEV)
    W = torch.from_numpy(rs.normal(0, 1, (H, K)).astype(np.float32)).to(DEV)
    bias = torch.from_numpy(rs.normal(0, 3, H).astype(np.float32)).to(DEV)
    n_tiles = (rows + 127) // 128
    part = torch.empty((n_tiles, 2, H), device=DEV)
    y = ops.gemm(False, True, x, W, bias=bias, bf16=bf16, bn_part=part)
    y_plain = ops.gemm(False, True, x, W, bias=bias, bf16=bf16)
    assert rel_err(y.cpu().numpy(), y_plain.cpu().numpy()) < 1e-6  # (the plain call may split K: other summation order)
    m1, v1 = torch.empty((passes, H), device=DEV), torch.empty((passes, H), device=DEV)
    m2, v2 = torch.empty((passes, H), device=DEV), torch.empty((passes, H), device=DEV)
    rm1, rv1 = torch.zeros(H, device=DEV), torch.ones(H, device=DEV)
    rm2, rv2 = torch.zeros(H, device=DEV), torch.ones(H, device=DEV)
    ops.bn_stats_finalize(part, B, 128, H, passes, 0.1, m1, v1, rm1, rv1)
    ops.bn_batch_stats(y, B, passes, 0.1, m2, v2, rm2, rv2)
    y64 = y.cpu().numpy().astype(np.float64).reshape(passes, B, H)
    assert rel_err(m1.cpu().numpy(), y64.mean(axis=1)) < 1e-6 and rel_err(v1.cpu().numpy(), y64.var(axis=1)) < 2e-6
    assert rel_err(m1.cpu().numpy(), m2.cpu().numpy()) < 1e-6 and rel_err(v1.cpu().numpy(), v2.cpu().numpy()) < 2e-6
    assert rel_err(rm1.cpu().numpy(), rm2.cpu().numpy()) < 1e-6 and rel_err(rv1.cpu().numpy(), rv2.cpu().numpy()) < 2e-6


BIG_FLAG_MODE_BUMP = {("linear", 32, True): 1}  # the seed bumps of flag_mode_case's big form (0 otherwise)
FLAG_MODE = [("fm", 64, False), ("fm", 64, True), ("fm", 16, True), ("linear", 32, True), ("fm", 80, False), ("fm", 10, True),
             ("fm", 128, False)]


@pytest.mark.parametrize("net,D,skew", FLAG_MODE)
@pytest.mark.parametrize("n_users", [300, 3_000_000])
@pytest.mark.parametrize("one_launch", [False, True, "ordered"])
def test_flag_mode_matches_oracle(net, D, skew, n_users, one_launch, tune):
    """The sparse regime's step (trs_epoch_flags + K1 taking every lone reference + flagged_update_kernel): rows
    referenced once in the batch updated in place by K1, the flagged references added with float atomics afterwards — 3
    batches in one C call == oracle SGD steps.  n_users = 3M: more rows than bitmap bits, so the user flags are
    hashed (conservative) — flagged lone rows must still be exact; the 3M-row user tables hold random values outside the
    300 rows that occur, and every row no triple names must come back bit-identical.  Flags: exact where the table fits
    the bitmap.
    one_launch: the same step as ONE launch (trs_train_args.sync_dev): K1's workgroups count themselves in on the
    arrival counter after their last row read, wait for the whole grid and apply the flagged references themselves;
    the library reports the arrivals it scheduled (3 launches x grid), and a second call continues the counter.
    ordered: the presort also puts every batch's triples with a flagged reference first (trs_epoch_flags_ordered: the
    same multiset of triples, the same flags per triple, their count reported) and the one-launch step counts its
    workgroups in after those triples (trs_train_args.n_flagged_dev) instead of after its last one."""
    check_flag_mode(net, D, skew, n_users, one_launch, tune)


@functools.lru_cache(maxsize=4)
def flag_mode_case(net, D, skew, n_users, big=False, lr=None, bands=False):
    """The input of check_flag_mode (no GPU): 3 batches of 512 on 300 users that occur (at their places in a table of
    n_users rows) and 57 or 5000 items, one hot item under skew.  big (the ordered form on the 3M-row table): mostly lone
    references, 16 000 users and 20 000 items for batches of 2 048 — about 40 % of the triples carry a flag.
    bands (tests/test_gpu_large_offsets.py): the users that occur sit at large_tables.band_rows of the n_users-row table
    — every offset band and both sides of every boundary — and everything else (tables, triples, step size, and with
    them the conditioning and the written-down seed bump) is the 3M-row case's."""
    def build(bump):
        rs = np.random.RandomState(D + skew + 1000 * bump)
        NU, NI, B, nb = n_users, 57 if n_users == 300 else 5000, 512, 3
        NUS = 300  # users that occur
        if big:
            NUS, NI, B = 16000, 20000, 2048
        p, _, _ = make_case(net, D, 0, 8, NU=NUS, NI=NI, seed=2)
        if bands:
            rs.choice(3_000_000, NUS, replace=False)  # (drawn and dropped: the triples below stay the 3M-row case's)
        else:
            urows = np.sort(rs.choice(NU, NUS, replace=False)) if NU > 300 else np.arange(300)  # the users that occur
        u_small = rs.randint(0, NUS, nb * B)
        if bands:  # (users drawn by a triple take the boundary rows: the ids then name every band and boundary)
            urows = large_tables.band_places(u_small, NUS, NU, D, seed=D)
        i = rs.randint(0, NI, nb * B)
        j = rs.randint(0, NI, nb * B)
        if skew:
            i[rs.rand(nb * B) < 0.4] = 7
            j[rs.rand(nb * B) < 0.4] = 7
        return sens.StepCase(net, sens.condition_tables(net, p), sens.batches_of(u_small, i, j, B, nb), lr_of(B, D, lr), D=D, NU=NU, NI=NI, NUS=NUS,
                             urows=urows, u_small=u_small, i=i, j=j)
    # (big: 36 000 rows of tables — the seed is written down, and checked by tests/test_step_sensitivity_host.py)
    return sens.conditioned(build, first=lr is not None,
                            bump=BIG_FLAG_MODE_BUMP.get((net, D, skew), 0) if big and lr is None else None)


def check_flag_mode(net, D, skew, n_users, one_launch, tune, first_stamp=1, prepare_scratch=None, bands=False):
    ops = _ops()
    big = one_launch == "ordered" and n_users > 300
    if big:  # four iterations per wave: the workgroups count themselves in after iteration 2 of 4 (mid-loop)
        tune(K1_ITERS=4)
    case = flag_mode_case(net, D, skew, n_users, big, bands=bands)
    p, NU, NI, NUS, B, nb, lr = case.p, case.NU, case.NI, case.NUS, case.B, case.nb, case.lr
    urows, u_small, i, j = case.urows, case.u_small, case.i, case.j
    u = urows[u_small]
    lin = ("user_bias.weight", "item_bias.weight") if net == "linear" else ("linear_user.weight", "linear_item.weight")
    t = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in p.items()}
    named = np.unique(u)  # the user rows a triple names
    if bands:
        large_tables.assert_covers(named, NU, D)
    if NU > 300:  # full-size user tables holding the 300 small rows at their places, random rows everywhere else
        bigD = large_tables.fill(torch.empty((NU, D), device=DEV), seed=D)
        bigD[torch.from_numpy(urows).to(DEV)] = t["user.weight"]
        big1 = large_tables.fill(torch.empty((NU, 1), device=DEV), seed=D + 1)
        big1[torch.from_numpy(urows).to(DEV)] = t[lin[0]]
        t["user.weight"], t[lin[0]] = bigD, big1
        sums_before = {k: large_tables.row_checksums(t[k]) for k in ("user.weight", lin[0])}
    T, keep = ops.make_tables(t["user.weight"], t["item.weight"], t[lin[0]], t[lin[1]])
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ordered = one_launch == "ordered"
    ef = ops.EpochFlags(nb, B, NU, NI, DEV, ordered=ordered)
    ef.run(None, None, 0, 0, 0, err, given_ids=[torch.from_numpy(a.astype(np.int32)).to(DEV) for a in (u, i, j)])
    ids, udup, idup = ef.step_args(0)
    if ordered:  # every batch: a permutation of its triples, the flagged ones first, their number reported
        uo, io, jo = (t_[:nb * B].cpu().numpy().astype(np.int64) for t_ in ids)
        small_of = {int(r): k for k, r in enumerate(urows)}
        for b in range(nb):
            sl = slice(b * B, (b + 1) * B)
            a_, b_ = np.stack([u[sl], i[sl], j[sl]], 1), np.stack([uo[sl], io[sl], jo[sl]], 1)
            assert np.array_equal(a_[np.lexsort(a_.T)], b_[np.lexsort(b_.T)])
            anyf = (udup[sl].cpu().numpy() != 0) | (idup[sl].cpu().numpy() != 0).any(axis=1)
            nf = int(ef.n_flagged[b].item())
            assert nf == int(anyf.sum()) and anyf[:nf].all() and not anyf[nf:].any()
        u, i, j = uo, io, jo  # what the steps (and the oracle below) see
        u_small = np.array([small_of[int(x)] for x in u])
    run = case.oracle_on(sens.batches_of(u_small, i, j, B, nb)) if ordered else case.oracle()  # (ordered: as the steps see them)
    for b in range(nb):
        sl = slice(b * B, (b + 1) * B)
        ucnt = np.unique(u[sl], return_counts=True)
        want_u = np.array([dict(zip(ucnt[0], ucnt[1]))[x] > 1 for x in u[sl]])
        got_u = udup[sl].cpu().numpy().astype(bool)
        assert (got_u | ~want_u).all()  # never 0 for a shared row
        if NU <= 1 << 20:
            assert np.array_equal(got_u, want_u)
        cnt = np.bincount(np.concatenate([i[sl], j[sl]]), minlength=NI)
        want_i = np.stack([cnt[i[sl]] > 1, cnt[j[sl]] > 1], axis=1)
        assert np.array_equal(idup[sl].cpu().numpy().astype(bool), want_i)
    gz, du = torch.empty((2, B), device=DEV), torch.empty((B, D), device=DEV)
    losses = torch.zeros(nb, device=DEV)
    import ctypes
    sync = (torch.zeros(288, dtype=torch.int32, device=DEV), ctypes.c_uint32(0)) if one_launch else None
    scratch, ustage = ops.train_scratch(NU, NI, B, D, DEV), torch.empty((B, D), device=DEV)
    if prepare_scratch is not None:
        prepare_scratch(scratch, net, NU, NI, B, D)
    # (two C calls, 2 + 1 steps: the arrival counter carries over from call to call)
    ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, 2, lr, *ids, gz, du, losses, err, scratch, first_stamp, None,
                        user_dup=udup, item_dup=idup, ustage=ustage, sync=sync, n_flagged=ef.n_flagged_from(0))
    ids2, udup2, idup2 = ef.step_args(2)
    ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, 1, lr, *ids2, gz, du, losses[2:], err, scratch,
                        first_stamp + 2, None,
                        user_dup=udup2, item_dup=idup2, ustage=ustage, sync=sync, n_flagged=ef.n_flagged_from(2))
    torch.cuda.synchronize()
    if one_launch:  # every launch counted all its workgroups in, and the library knows how many it scheduled
        assert sync[1].value > 0 and sync[1].value % 3 == 0 and int(sync[0][0].item()) == sync[1].value
    sens.assert_losses(case, losses.cpu().numpy(), run)
    ut = torch.from_numpy(urows).to(DEV)
    got = {k: (t[k][ut] if (NU > 300 and k in ("user.weight", lin[0])) else t[k]).cpu().numpy() for k in run.after}
    sens.criterion_for(case)(got, run.after, p)
    if NU > 300:  # every row no triple names is bit-identical
        for k, before in sums_before.items():
            large_tables.assert_untouched(before, large_tables.row_checksums(t[k]), named, k)
    assert err.item() == 0


def test_one_launch_step_reports_flag_counts_of_another_origin(tune):
    """n_flagged_dev that does not describe the arrays it comes with (here: zeroed counts for batches that do hold
    flagged triples) is detected by the step — err bit 3 — instead of silently racing."""
    import ctypes
    ops = _ops()
    rs = np.random.RandomState(5)
    NU, NI, B, D = 4000, 5000, 2048, 64
    tune(K1_ITERS=4)
    p, _, _ = make_case("fm", D, 0, 8, NU=NU, NI=NI, seed=1)
    t = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in p.items()}
    T, keep = ops.make_tables(t["user.weight"], t["item.weight"], t["linear_user.weight"], t["linear_item.weight"])
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ef = ops.EpochFlags(1, B, NU, NI, DEV)
    ef.run(None, None, 0, 0, 0, err,
           given_ids=[torch.from_numpy(rs.randint(0, n, B).astype(np.int32)).to(DEV) for n in (NU, NI, NI)])
    assert 0 < int(ef.n_flagged[0].item()) < B
    ef.n_flagged.zero_()
    ids, udup, idup = ef.step_args(0)
    sync = (torch.zeros(288, dtype=torch.int32, device=DEV), ctypes.c_uint32(0))
    ops.train_steps_sgd("fm", T, None, None, 0, 0, 0, B, 1, 0.05, *ids, torch.empty((2, B), device=DEV),
                        torch.empty((B, D), device=DEV), torch.zeros(1, device=DEV), err,
                        ops.train_scratch(NU, NI, B, D, DEV), 1, None, user_dup=udup, item_dup=idup,
                        ustage=torch.empty((B, D), device=DEV), sync=sync, n_flagged=ef.n_flagged_from(0))
    torch.cuda.synchronize()
    assert sync[1].value > 0  # (the one-launch form ran)
    assert int(err.item()) & 8
    from torchrecsys_amd.collaborative._scorer import check_err_flag
    with pytest.raises(RuntimeError, match="n_flagged_dev"):
        check_err_flag(err, "step")


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 1000, 4097, 20000])
@pytest.mark.parametrize("dense", [False, True])
def test_flagged_first_order_any_batch_length(B, dense):
    """trs_epoch_flags_ordered on batches whose length is no multiple of anything (the partition works on 64-position
    cells and 1024-thread rounds): per batch the same multiset of triples as given, every triple with its own flags,
    the flagged ones first and counted.  dense: nearly every triple flagged; sparse: a few."""
    ops = _ops()
    rs = np.random.RandomState(B + dense)
    nb = 3
    NU, NI = (max(B // 2, 2), max(B // 3, 3)) if dense else (min(40 * B + 7, 1 << 20), min(60 * B + 11, 1 << 20))
    u, i, j = rs.randint(0, NU, nb * B), rs.randint(0, NI, nb * B), rs.randint(0, NI, nb * B)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ef = ops.EpochFlags(nb, B, NU, NI, DEV)
    ef.run(None, None, 0, 0, 0, err, given_ids=[torch.from_numpy(a.astype(np.int32)).to(DEV) for a in (u, i, j)])
    torch.cuda.synchronize()
    uo, io, jo = (t_[:nb * B].cpu().numpy().astype(np.int64) for t_ in ef.ids)
    ud, idp = ef.user_dup[:nb * B].cpu().numpy().astype(bool), ef.item_dup[:nb * B].cpu().numpy().astype(bool)
    for b in range(nb):
        sl = slice(b * B, (b + 1) * B)
        a_, b_ = np.stack([u[sl], i[sl], j[sl]], 1), np.stack([uo[sl], io[sl], jo[sl]], 1)
        assert np.array_equal(a_[np.lexsort(a_.T)], b_[np.lexsort(b_.T)])
        assert np.array_equal(ud[sl], np.bincount(uo[sl], minlength=NU)[uo[sl]] > 1)  # (tables fit the bitmap: exact)
        cnt = np.bincount(np.concatenate([io[sl], jo[sl]]), minlength=NI)
        assert np.array_equal(idp[sl], np.stack([cnt[io[sl]] > 1, cnt[jo[sl]] > 1], 1))
        anyf = ud[sl] | idp[sl].any(axis=1)
        nf = int(ef.n_flagged[b].item())
        assert nf == int(anyf.sum()) and anyf[:nf].all() and not anyf[nf:].any(), (b, nf, int(anyf.sum()))
    assert err.item() == 0


NO_SHARED_ROW = [("fm", 64), ("linear", 32), ("fm", 128)]


@functools.lru_cache(maxsize=4)
def no_shared_row_case(net, D, lr=None):
    """The input of test_flag_mode_ordered_batches_without_any_shared_row (no GPU): 2 batches of 2048 on 4096 users and
    8192 items, no row named twice in a batch."""
    def build(bump):
        NU, NI, B, nb = 4096, 8192, 2048, 2
        rs = np.random.RandomState(D + 1000 * bump)
        p, _, _ = make_case(net, D, 0, 8, NU=NU, NI=NI, seed=3)
        u = np.concatenate([rs.permutation(NU)[:B] for _ in range(nb)])
        it = [rs.permutation(NI) for _ in range(nb)]
        i, j = np.concatenate([x[:B] for x in it]), np.concatenate([x[B:2 * B] for x in it])
        return sens.StepCase(net, sens.condition_tables(net, p), sens.batches_of(u, i, j, B, nb), lr_of(B, D, lr), D=D, NU=NU, NI=NI, u=u, i=i, j=j)
    return sens.conditioned(build, first=lr is not None)


@pytest.mark.parametrize("net,D", NO_SHARED_ROW)
def test_flag_mode_ordered_batches_without_any_shared_row(net, D, tune):
    """Flagged-first order, edge: no row is named twice in a batch — n_flagged = 0, the one-launch step counts its
    workgroups in before their first iteration, no wave has anything to apply — 2 steps == oracle SGD steps; and the
    arrival counter still advances by the grid per launch."""
    import ctypes
    ops = _ops()
    tune(K1_ITERS=4)
    case = no_shared_row_case(net, D)
    p, NU, NI, B, nb, lr, u, i, j = case.p, case.NU, case.NI, case.B, case.nb, case.lr, case.u, case.i, case.j
    lin = ("user_bias.weight", "item_bias.weight") if net == "linear" else ("linear_user.weight", "linear_item.weight")
    t = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in p.items()}
    T, keep = ops.make_tables(t["user.weight"], t["item.weight"], t[lin[0]], t[lin[1]])
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ef = ops.EpochFlags(nb, B, NU, NI, DEV)
    ef.run(None, None, 0, 0, 0, err, given_ids=[torch.from_numpy(a.astype(np.int32)).to(DEV) for a in (u, i, j)])
    ids, udup, idup = ef.step_args(0)
    assert ef.n_flagged.tolist() == [0, 0] and int(udup.sum()) == 0 and int(idup.sum()) == 0
    for got, want in zip(ids, (u, i, j)):  # nothing to move: the batches are as given
        assert np.array_equal(got[:nb * B].cpu().numpy(), want)
    gz, du = torch.empty((2, B), device=DEV), torch.empty((B, D), device=DEV)
    losses = torch.zeros(nb, device=DEV)
    sync = (torch.zeros(288, dtype=torch.int32, device=DEV), ctypes.c_uint32(0))
    ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, nb, lr, *ids, gz, du, losses, err,
                        ops.train_scratch(NU, NI, B, D, DEV), 1, None, user_dup=udup, item_dup=idup,
                        ustage=torch.empty((B, D), device=DEV), sync=sync, n_flagged=ef.n_flagged_from(0))
    torch.cuda.synchronize()
    assert sync[1].value > 0 and sync[1].value % nb == 0 and int(sync[0][0].item()) == sync[1].value
    sens.assert_losses(case, losses.cpu().numpy())
    sens.criterion_for(case)(tables_to_host(t), case.ref, p)
    assert err.item() == 0


PRESORTED_ITEM = [("fm", 64, False), ("fm", 64, True), ("fm", 16, True), ("linear", 32, True), ("fm", 80, False), ("fm", 10, True)]


@pytest.mark.parametrize("net,D,skew", PRESORTED_ITEM)
@pytest.mark.parametrize("inline_user", [False, True, "items", "userflags"])
def test_presorted_item_update_matches_oracle(net, D, skew, inline_user):
    """trs_epoch_presort + the atomic-free per-run item update: 3 batches in one C call == oracle SGD steps.
    `skew`: one hot item takes 40 % of the references (runs cut at 64, pieces added atomically).
    inline_user "items": K1 also updates the item rows referenced once in the batch (item-duplicate flags) and the
    sorted runs only walk rows with several references.  "userflags": no user sort — user duplicates as flags of the
    LDS-bitmap kernel, the flagged users' gradients added with float atomics in the sorted-run launch (the dense regime's
    plain-SGD step)."""
    check_presorted_item_update(net, D, skew, inline_user)


@functools.lru_cache(maxsize=4)
def presorted_item_update_case(net, D, skew, lr=None):
    """The input of check_presorted_item_update (no GPU): 3 batches of 512 on 300 users and 57 items, one hot item under
    skew."""
    def build(bump):
        rs = np.random.RandomState(D + skew + 1000 * bump)
        NU, NI, B, nb = 300, 57, 512, 3
        p, _, _ = make_case(net, D, 0, 8, NU=NU, NI=NI, seed=2)
        u = rs.randint(0, NU, nb * B)
        i = rs.randint(0, NI, nb * B)
        j = rs.randint(0, NI, nb * B)
        if skew:
            i[rs.rand(nb * B) < 0.4] = 7
            j[rs.rand(nb * B) < 0.4] = 7
        return sens.StepCase(net, sens.condition_tables(net, p), sens.batches_of(u, i, j, B, nb), lr_of(B, D, lr), D=D, NU=NU, NI=NI, u=u, i=i, j=j)
    return sens.conditioned(build, first=lr is not None)


def check_presorted_item_update(net, D, skew, inline_user, first_stamp=1, prepare_scratch=None):
    ops = _ops()
    case = presorted_item_update_case(net, D, skew)
    p, NU, NI, B, nb, lr, u, i, j = case.p, case.NU, case.NI, case.B, case.nb, case.lr, case.u, case.i, case.j
    lin = ("user_bias.weight", "item_bias.weight") if net == "linear" else ("linear_user.weight", "linear_item.weight")
    t = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in p.items()}
    T, keep = ops.make_tables(t["user.weight"], t["item.weight"], t[lin[0]], t[lin[1]])
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ps = ops.EpochPresort(nb, B, NU, NI, DEV, user_sort=inline_user != "userflags")
    given = [torch.from_numpy(a.astype(np.int32)).to(DEV) for a in (u, i, j)]
    ps.run(None, None, 0, 0, 0, err, given_ids=given)
    ids, sk, sv, udup, usorted, idup = ps.step_args(0)
    assert (usorted[0] is None) == (inline_user == "userflags")
    gz, du = torch.empty((2, B), device=DEV), torch.empty((B, D), device=DEV)
    losses = torch.zeros(nb, device=DEV)
    # user-duplicate flags of the slice == "another triple of the same batch has this user"
    for b in range(nb):
        ub = u[b * B:(b + 1) * B]
        cnt = np.bincount(ub, minlength=NU)
        assert np.array_equal(udup[b * B:(b + 1) * B].cpu().numpy(), (cnt[ub] > 1).astype(np.uint8))
        # item-duplicate flags: {pos, neg} reference of a position shares its row with another reference of the batch
        cnt = np.bincount(np.concatenate([i[b * B:(b + 1) * B], j[b * B:(b + 1) * B]]), minlength=NI)
        want = np.stack([cnt[i[b * B:(b + 1) * B]] > 1, cnt[j[b * B:(b + 1) * B]] > 1], axis=1).astype(np.uint8)
        assert np.array_equal(idup[b * B:(b + 1) * B].cpu().numpy(), want)
    scratch = ops.train_scratch(NU, NI, B, D, DEV)
    if prepare_scratch is not None:
        prepare_scratch(scratch, net, NU, NI, B, D)
    if inline_user:
        ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, nb, lr, *ids, gz, du, losses, err,
                            scratch, first_stamp, None, sk, sv, ps.key_bytes, udup,
                            torch.empty((B, D), device=DEV), usorted,
                            item_dup=idup if inline_user == "items" else None)
    else:
        ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, nb, lr, *ids, gz, du, losses, err,
                            scratch, first_stamp, None, sk, sv, ps.key_bytes)
    torch.cuda.synchronize()
    sens.assert_losses(case, losses.cpu().numpy())
    sens.criterion_for(case)(tables_to_host(t), case.ref, p)
    assert err.item() == 0


@pytest.mark.parametrize("net,D,skew", [("fm", 64, False), ("fm", 64, True), ("linear", 32, True), ("fm", 10, True)])
@pytest.mark.parametrize("kind", ["sparse_adam", "adagrad"])
def test_presorted_adaptive_rules_match_the_oracle(net, D, skew, kind):
    """SparseAdam / Adagrad on the presorted two-launch step (users referenced once updated by K1, duplicated users
    and item rows by their sorted runs, cut runs through the gradient accumulator + cut_rows_apply_kernel): 4 batches
    in one C call == oracle steps on the coalesced gradients of the rows present in each batch."""
    check_presorted_adaptive_rules(net, D, skew, kind)


def check_presorted_adaptive_rules(net, D, skew, kind, first_stamp=1, prepare_scratch=None, bands=False):
    """Returns the number of cut runs the last step listed.  bands (tests/test_gpu_large_offsets.py): the same 300 users
    sit at large_tables.band_rows of user tables with n_rows_for(D) rows — parameters AND state, random everywhere else
    (the state non-negative, and zero on the rows that occur, as the oracle starts) — and every row no triple names
    must come back bit-identical."""
    from torchrecsys_amd import _lib
    from oracle.nets import touched_rows
    ops = _ops()
    rs = np.random.RandomState(D + skew)
    NU, NI, B, nb = 300, 57, 512, 4
    lr, b1, b2, eps, lr_decay = (0.01, 0.9, 0.999, 1e-8, 0.0) if kind == "sparse_adam" else (0.05, 0, 0, 1e-10, 0.02)
    p, _, _ = make_case(net, D, 0, 8, NU=NU, NI=NI, seed=2)
    u, i, j = rs.randint(0, NU, nb * B), rs.randint(0, NI, nb * B), rs.randint(0, NI, nb * B)
    if skew:
        i[rs.rand(nb * B) < 0.4] = 7
        j[rs.rand(nb * B) < 0.4] = 7
    lin = ("user_bias.weight", "item_bias.weight") if net == "linear" else ("linear_user.weight", "linear_item.weight")
    names = ["user.weight", "item.weight", lin[0], lin[1]]
    t = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in p.items()}
    s1 = {k: torch.zeros_like(t[k]) for k in names}
    s2 = {k: torch.zeros_like(t[k]) for k in names}
    u_small, large = u, ()
    if bands:
        NU = large_tables.n_rows_for(D)
        place = large_tables.band_places(u_small, 300, NU, D, seed=D + 1)  # small user j sits at row place[j]
        u = place[u_small]
        urows = np.unique(u)  # the rows a triple names: every other row stays as it is
        large_tables.assert_covers(urows, NU, D)
        ut, large = torch.from_numpy(place).to(DEV), (names[0], names[2])
        for n_, k in enumerate(large):
            w = t[k].shape[1]
            small = t[k]
            t[k] = large_tables.fill(torch.empty((NU, w), device=DEV), seed=10 * D + n_)
            t[k][ut] = small
            for m_, s_ in enumerate((s1, s2) if kind == "sparse_adam" else (s1,)):
                s_[k] = large_tables.fill(torch.empty((NU, w), device=DEV), seed=10 * D + 2 + 2 * m_ + n_).abs_()
                s_[k][ut] = 0.0
        watched = {(name, k): tab[k] for name, tab in (("table", t), ("state 1", s1), ("state 2", s2)) for k in large
                   if tab[k].shape[0] == NU}
        sums_before = {key: large_tables.row_checksums(v) for key, v in watched.items()}
    T, keep = ops.make_tables(*(t[k] for k in names))
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ps = ops.EpochPresort(nb, B, NU, NI, DEV)
    ps.run(None, None, 0, 0, 0, err, given_ids=[torch.from_numpy(a.astype(np.int32)).to(DEV) for a in (u, i, j)])
    ids, sk, sv, udup, usorted, idup = ps.step_args(0)
    gz, du = torch.empty((2, B), device=DEV), torch.empty((B, D), device=DEV)
    losses = torch.zeros(nb, device=DEV)
    gacc, gacc_lin = torch.zeros_like(t["item.weight"]), torch.zeros_like(t[lin[1]])
    cut_rows = torch.empty(2 * B // 64 + 64, dtype=torch.int32, device=DEV)
    cut_count = torch.zeros(2, dtype=torch.int32, device=DEV)
    o = _lib.TrsOpt()
    o.kind, o.lr, o.beta1, o.beta2, o.eps, o.lr_decay, o.step0 = (1 if kind == "sparse_adam" else 2), lr, b1, b2, eps, lr_decay, 0
    o.user_s1, o.item_s1, o.user_lin_s1, o.item_lin_s1 = (ops.ptr(s1[k]) for k in names)
    if kind == "sparse_adam":
        o.user_s2, o.item_s2, o.user_lin_s2, o.item_lin_s2 = (ops.ptr(s2[k]) for k in names)
    o.gacc, o.gacc_lin, o.cut_rows, o.cut_count = ops.ptr(gacc), ops.ptr(gacc_lin), ops.ptr(cut_rows), ops.ptr(cut_count)
    o.cut_capacity = cut_rows.numel()
    scratch = ops.train_scratch(NU, NI, B, D, DEV)
    if prepare_scratch is not None:
        prepare_scratch(scratch, net, NU, NI, B, D)
    ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, nb, lr, *ids, gz, du, losses, err,
                        scratch, first_stamp, None, sk, sv, ps.key_bytes, udup,
                        torch.empty((B, D), device=DEV), usorted, o)
    torch.cuda.synchronize()
    cuts_listed = int(cut_count.max().item())  # (the last step's list; the other parity's counter is reset by it)
    ref = {k: v.copy() for k, v in p.items()}
    r1 = {k: np.zeros_like(v) for k, v in p.items()}
    r2 = {k: np.zeros_like(v) for k, v in p.items()}
    for b in range(nb):
        batch = {"user_id": u_small[b * B:(b + 1) * B], "pos_item_id": i[b * B:(b + 1) * B], "neg_item_id": j[b * B:(b + 1) * B]}
        _, _, loss, grads = onets.train_forward_backward(net, ref, batch)
        rows = touched_rows(net, ref, batch)
        for k in names:
            if kind == "sparse_adam":
                ooptim.sparse_adam_rows(ref[k], grads[k], rows[k], r1[k], r2[k], b + 1, lr, b1, b2, eps)
            else:
                ooptim.adagrad_rows(ref[k], grads[k], rows[k], r1[k], b + 1, lr, lr_decay, eps)
        assert abs(losses[b].item() / B - float(loss)) <= 2 * TOL * max(abs(float(loss)), 1e-3)
    def rows_within(got, want, tol):
        """fraction of rows whose largest deviation is below tol * max|want|"""
        return float((np.abs(got - want).max(axis=1) <= tol * np.abs(want).max()).mean())

    for key, v in (watched.items() if bands else ()):  # rows no triple names: bit-identical, parameters and state
        large_tables.assert_untouched(sums_before.pop(key), large_tables.row_checksums(v), urows, " ".join(key))
    for tab in ((t, s1, s2) if bands else ()):       # the compacted rows of the large tables, for the criteria below
        for k in large:
            if tab[k].shape[0] == NU:
                tab[k] = tab[k][ut]
    for k in names:
        # Both rules divide by a norm of the row's own gradient history, so a coalesced gradient that cancels to rounding
        # noise (the skewed cases make a user meet the hot item as positive of one triple and negative of another) is
        # turned into a +-lr step of random sign — in torch too.  Such rows are rare: bulk criterion, like the golden
        # trajectories; every other row matches to fp32 summation order.
        need = 0.97 if skew else 1.0
        assert rows_within(t[k].cpu().numpy(), ref[k], 1e-3 if skew else 3 * TOL) >= need, k
        assert rows_within(s1[k].cpu().numpy(), r1[k], 1e-3) >= need, k
        if kind == "sparse_adam":
            assert rows_within(s2[k].cpu().numpy(), r2[k], 1e-3) >= need, k
        assert rel_err(t[k].cpu().numpy(), ref[k]) < 0.05, k
    assert float(gacc.abs().max()) == 0.0 and float(gacc_lin.abs().max()) == 0.0  # accumulator left clean
    assert err.item() == 0
    return cuts_listed


PRESORTED_META = [("fm", 64, 1, False), ("fm", 16, 3, True), ("linear", 32, 1, True), ("linear", 8, 2, False), ("fm", 10, 1, True)]
PRESORTED_META_FORMS = [(False, 512), (True, 512), (True, 509), (True, 3), ("hot", 2048)]


@pytest.mark.parametrize("net,D,M,skew", PRESORTED_META)
@pytest.mark.parametrize("meta_sorted,B", PRESORTED_META_FORMS)
def test_presorted_step_with_metadata_matches_oracle(net, D, M, skew, meta_sorted, B):
    """Metadata scorers on the presorted step (SGD): K1 = the scorer's staging mode (ids from the item -> metadata
    table, user update in place, FM: per-pass field sums staged), user / item rows through the sorted runs (FM: w +=
    sum(c*S) - sum(c)*w), metadata tables through the atomic scatter of the staged fields: 3 batches == oracle steps.
    "hot": 90 % of the items carry category 0 of the first column, batch 2048 — that row's run
    is ~3 700 references long and is cut into ~58 pieces of 64; FM's pieces subtract sum(c)*w with the w they loaded,
    which other pieces may already have touched (second order in the step size): held to the same 1e-5."""
    check_presorted_step_with_metadata(net, D, M, skew, meta_sorted, B)


@functools.lru_cache(maxsize=4)
def presorted_metadata_case(net, D, M, skew, hot, B, lr=None):
    """The input of check_presorted_step_with_metadata (no GPU): 3 batches of B on 300 users, 57 items and M metadata
    columns; hot: 90 % of the items in category 0 of the first column."""
    def build(bump):
        rs = np.random.RandomState(D + M + skew + 1000 * bump)
        NU, NI, nb = 300, 57, 3
        p, _, _ = make_case(net, D, M, 8, NU=NU, NI=NI, seed=2)
        sizes = [p[f"metadata.{m}.weight"].shape[0] for m in range(M)]
        item_meta = np.stack([rs.randint(0, sizes[m], NI) for m in range(M)], axis=1).astype(np.int32)
        if hot:
            item_meta[rs.rand(NI) < 0.9, 0] = 0
        u, i, j = rs.randint(0, NU, nb * B), rs.randint(0, NI, nb * B), rs.randint(0, NI, nb * B)
        if skew:
            i[rs.rand(nb * B) < 0.4] = 7
            j[rs.rand(nb * B) < 0.4] = 7
        return sens.StepCase(net, sens.condition_tables(net, p), sens.batches_of(u, i, j, B, nb, item_meta),
                             lr_of(B, D, lr, 0.5 if hot else 0.05, hot), D=D, M=M, NU=NU, NI=NI,
                             u=u, i=i, j=j, item_meta=item_meta, sizes=sizes)
    return sens.conditioned(build, first=lr is not None)


def check_presorted_step_with_metadata(net, D, M, skew, meta_sorted, B, first_stamp=1, prepare_scratch=None):
    from torchrecsys_amd import _lib
    ops = _ops()
    case = presorted_metadata_case(net, D, M, skew, meta_sorted == "hot", B)
    p, NU, NI, nb, lr, u, i, j = case.p, case.NU, case.NI, case.nb, case.lr, case.u, case.i, case.j
    item_meta, sizes = case.item_meta, case.sizes
    lin = ("user_bias.weight", "item_bias.weight") if net == "linear" else ("linear_user.weight", "linear_item.weight")
    t = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in p.items()}
    metas = [t[f"metadata.{m}.weight"] for m in range(M)]
    meta_lins = [t[f"linear_metadata.{m}.weight"] for m in range(M)] if net == "fm" else []
    T, keep = ops.make_tables(t["user.weight"], t["item.weight"], t[lin[0]], t[lin[1]], metas, meta_lins)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    tab = torch.from_numpy(item_meta).to(DEV)
    # meta_sorted: every metadata column's references grouped by row too (sorted runs instead of the atomic scatter)
    ps = ops.EpochPresort(nb, B, NU, NI, DEV, **(dict(item_meta=tab, n_meta=sizes) if meta_sorted else {}))
    ps.run(None, None, 0, 0, 0, err, given_ids=[torch.from_numpy(a.astype(np.int32)).to(DEV) for a in (u, i, j)])
    ids, sk, sv, udup, usorted, idup = ps.step_args(0)
    R = 3 + 2 * M
    gz, du = torch.empty((2, B), device=DEV), torch.empty((B, D), device=DEV)
    xstage = torch.empty((2 if net == "fm" else 1, B, D), device=DEV)
    grad_rows, grad_lin = torch.empty((R, B, D), device=DEV), torch.zeros((R, B), device=DEV)
    meta_ids = torch.empty((2, B, M), dtype=torch.int32, device=DEV)
    ms = _lib.TrsMetaStage()
    ms.item_meta_tab, ms.xstage, ms.meta_ids = ops.ptr(tab), ops.ptr(xstage), ops.ptr(meta_ids)
    ms.grad_rows, ms.grad_lin = ops.ptr(grad_rows), ops.ptr(grad_lin)
    lin_scratch = torch.zeros(max(sizes), device=DEV)
    if meta_sorted:
        for m, (k_, v_) in enumerate(ps.meta_step_args(0)):
            ms.sorted_keys[m], ms.sorted_vals[m] = k_, v_
        ms.lin_scratch = ops.ptr(lin_scratch)
        if D != 16:  # one case keeps the table look-up inside K1
            pm, nm = ps.meta_id_args(0)
            ms.pos_meta_ids, ms.neg_meta_ids = ops.ptr(pm), ops.ptr(nm)
    losses = torch.zeros(nb, device=DEV)
    scratch = ops.train_scratch(NU, NI, B, D, DEV)
    if prepare_scratch is not None:
        prepare_scratch(scratch, net, NU, NI, B, D)
    ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, nb, lr, *ids, gz, du, losses, err,
                        scratch, first_stamp, None, sk, sv, ps.key_bytes, udup,
                        torch.empty((B, D), device=DEV), usorted, None, ms)
    torch.cuda.synchronize()
    sens.assert_losses(case, losses.cpu().numpy())
    sens.criterion_for(case)(tables_to_host(t), case.ref, p)
    assert err.item() == 0


@pytest.mark.parametrize("net,D,M,skew", [("fm", 64, 1, False), ("fm", 32, 3, True), ("linear", 32, 2, False),
                                          ("linear", 64, 1, True), ("fm", 128, 2, False)])
@pytest.mark.parametrize("kind", ["sparse_adam", "adagrad"])
def test_presorted_adaptive_rules_with_metadata_match_the_oracle(net, D, M, skew, kind):
    """SparseAdam / Adagrad on the presorted step of a metadata scorer: the user rule inside the staging kernel, item
    and every metadata column through sorted runs on their COALESCED gradients (FM: sum(c*S) - sum(c)*w with the
    pre-update row w), each table with its own state, accumulator and cut-run list: 4 batches == oracle steps."""
    from torchrecsys_amd import _lib
    from oracle.nets import touched_rows
    ops = _ops()
    rs = np.random.RandomState(D + M + skew)
    NU, NI, B, nb = 300, 57, 512, 4
    lr, b1, b2, eps, lr_decay = (0.01, 0.9, 0.999, 1e-8, 0.0) if kind == "sparse_adam" else (0.05, 0, 0, 1e-10, 0.02)
    p, _, _ = make_case(net, D, M, 8, NU=NU, NI=NI, seed=2)
    sizes = [p[f"metadata.{m}.weight"].shape[0] for m in range(M)]
    item_meta = np.stack([rs.randint(0, sizes[m], NI) for m in range(M)], axis=1).astype(np.int32)
    u, i, j = rs.randint(0, NU, nb * B), rs.randint(0, NI, nb * B), rs.randint(0, NI, nb * B)
    if skew:
        i[rs.rand(nb * B) < 0.4] = 7
        j[rs.rand(nb * B) < 0.4] = 7
    lin = ("user_bias.weight", "item_bias.weight") if net == "linear" else ("linear_user.weight", "linear_item.weight")
    names = ["user.weight", "item.weight", lin[0], lin[1]]
    t = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in p.items()}
    metas = [t[f"metadata.{m}.weight"] for m in range(M)]
    meta_lins = [t[f"linear_metadata.{m}.weight"] for m in range(M)] if net == "fm" else []
    T, keep = ops.make_tables(t["user.weight"], t["item.weight"], t[lin[0]], t[lin[1]], metas, meta_lins)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    tab = torch.from_numpy(item_meta).to(DEV)
    ps = ops.EpochPresort(nb, B, NU, NI, DEV, item_meta=tab, n_meta=sizes)
    ps.run(None, None, 0, 0, 0, err, given_ids=[torch.from_numpy(a.astype(np.int32)).to(DEV) for a in (u, i, j)])
    ids, sk, sv, udup, usorted, idup = ps.step_args(0)
    gz, du = torch.empty((2, B), device=DEV), torch.empty((B, D), device=DEV)
    xstage = torch.empty((2 if net == "fm" else 1, B, D), device=DEV)
    ms = _lib.TrsMetaStage()
    ms.item_meta_tab, ms.xstage = ops.ptr(tab), ops.ptr(xstage)
    for m, (k_, v_) in enumerate(ps.meta_step_args(0)):
        ms.sorted_keys[m], ms.sorted_vals[m] = k_, v_
    lin_scratch = torch.zeros(max(sizes), device=DEV)
    ms.lin_scratch = ops.ptr(lin_scratch)
    pm, nm = ps.meta_id_args(0)
    ms.pos_meta_ids, ms.neg_meta_ids = ops.ptr(pm), ops.ptr(nm)
    s1 = {k: torch.zeros_like(v) for k, v in t.items()}
    s2 = {k: torch.zeros_like(v) for k, v in t.items()}
    gacc = {k: torch.zeros_like(v) for k, v in t.items()}
    cap = 2 * B // 64 + 64
    cut_rows = torch.empty((1 + M, cap), dtype=torch.int32, device=DEV)
    cut_count = torch.zeros((1 + M, 2), dtype=torch.int32, device=DEV)
    lin_state = [torch.zeros((3, sizes[m]), device=DEV) for m in range(M)]  # Linear: no 1-wide metadata tables
    o = _lib.TrsOpt()
    o.kind, o.lr, o.beta1, o.beta2, o.eps, o.lr_decay, o.step0 = (1 if kind == "sparse_adam" else 2), lr, b1, b2, eps, lr_decay, 0
    o.user_s1, o.item_s1, o.user_lin_s1, o.item_lin_s1 = (ops.ptr(s1[k]) for k in names)
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
    ops.train_steps_sgd(net, T, None, None, 0, 0, 0, B, nb, lr, *ids, gz, du, losses, err,
                        ops.train_scratch(NU, NI, B, D, DEV), 1, None, sk, sv, ps.key_bytes, udup,
                        torch.empty((B, D), device=DEV), usorted, o, ms)
    torch.cuda.synchronize()
    ref = {k: v.copy() for k, v in p.items()}
    r1 = {k: np.zeros_like(v) for k, v in p.items()}
    r2 = {k: np.zeros_like(v) for k, v in p.items()}
    for b in range(nb):
        sl = slice(b * B, (b + 1) * B)
        batch = {"user_id": u[sl], "pos_item_id": i[sl], "neg_item_id": j[sl],
                 "pos_metadata_id": item_meta[i[sl]].astype(np.int64), "neg_metadata_id": item_meta[j[sl]].astype(np.int64)}
        _, _, loss, grads = onets.train_forward_backward(net, ref, batch)
        rows = touched_rows(net, ref, batch)
        for k in ref:
            if kind == "sparse_adam":
                ooptim.sparse_adam_rows(ref[k], grads[k], rows[k], r1[k], r2[k], b + 1, lr, b1, b2, eps)
            else:
                ooptim.adagrad_rows(ref[k], grads[k], rows[k], r1[k], b + 1, lr, lr_decay, eps)
        assert abs(losses[b].item() / B - float(loss)) <= 2 * TOL * max(abs(float(loss)), 1e-3)

    def rows_within(got, want, tol):
        return float((np.abs(got - want).max(axis=1) <= tol * np.abs(want).max()).mean())

    for k in ref:
        # bulk criterion as in test_presorted_adaptive_rules_match_the_oracle: gradients that cancel to rounding noise
        # become +-lr steps of random sign under both rules (in torch too); the few-row metadata tables of the skewed
        # cases see more of them
        need = 0.9 if skew else (0.97 if k.startswith(("metadata", "linear_metadata")) else 1.0)
        assert rows_within(t[k].cpu().numpy(), ref[k], 1e-3) >= need, k
        assert rows_within(s1[k].cpu().numpy(), r1[k], 1e-3) >= need, k
        if kind == "sparse_adam":
            assert rows_within(s2[k].cpu().numpy(), r2[k], 1e-3) >= need, k
        assert rel_err(t[k].cpu().numpy(), ref[k]) < 0.05, k
        assert float(gacc[k].abs().max()) == 0.0, k  # accumulators left clean
    assert err.item() == 0


def test_presort_generates_the_same_batches_as_batch_prepare():
    ops = _ops()
    rs = np.random.RandomState(1)
    N, NU, NI, B, nb = 6000, 400, 91, 256, 4
    su = torch.from_numpy(rs.randint(0, NU, N).astype(np.int32)).to(DEV)
    si = torch.from_numpy(rs.randint(0, NI, N).astype(np.int32)).to(DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ps = ops.EpochPresort(nb, B, NU, NI, DEV)
    key, seed_ = 0xC0FFEE1234, 99
    ps.run(ops.interleave_stream(su, si), None, key, seed_, 512, err)
    torch.cuda.synchronize()
    for b in range(nb):
        out = ops.batch_prepare(su, si, None, key, 512 + b * B, B, NI, seed_, 512 + b * B)
        for k, arr in zip(("user", "pos", "neg"), ps.ids):
            assert torch.equal(arr[b * B:(b + 1) * B], out[k]), (k, b)
    # sorted references: per batch ascending item rows, a permutation of the batch's 2B references
    n = 2 * nb * B
    assert ps.key_bytes == 4  # keys = item rows, one sort segment per batch
    keys = ps.keys.view(torch.uint32)[n:].cpu().numpy().astype(np.int64)
    for b in range(nb):
        items = keys[2 * b * B:2 * (b + 1) * B]
        assert (np.diff(items) >= 0).all()
        exp = np.sort(np.concatenate([ps.ids[1][b * B:(b + 1) * B].cpu().numpy(), ps.ids[2][b * B:(b + 1) * B].cpu().numpy()]))
        assert np.array_equal(items, exp)


@pytest.mark.parametrize("bf16,D,M,N,B,passes,out16", [(False, 64, 1, 1024, 8192, 2, False), (False, 128, 0, 512, 16384, 2, False),
                                                       (True, 64, 1, 1024, 8192, 2, True), (True, 128, 2, 512, 16384, 2, False),
                                                       (True, 256, 0, 1024, 16384, 1, True)])
def test_gather_fused_first_layer_gemm_equals_gather_then_gemm(bf16, D, M, N, B, passes, out16):
    """trs_mlp_gather_gemm1_fwd (the "concat-GEMM": embedding gather inside the first layer's A-operand load, reference
    collaborative/mlp.py:93-107) == trs_mlp_gather_concat followed by the GEMM of the same family, BIT FOR BIT: y, the
    BatchNorm chunk partials, and the x0 image written as a by-product (fp32 / bf16 RNE).  Ids with duplicates, both
    passes, metadata columns with a stride; an id outside its table raises the error flag without touching memory
    outside the tables."""
    ops = _ops()
    g = torch.Generator(device=DEV)
    g.manual_seed(D + N + M)
    NU, NI, cats = 50_000, 20_000, [997, 31][:M]
    tabs = [torch.randn(NU, D, device=DEV, generator=g), torch.randn(NI, D, device=DEV, generator=g)] + \
           [torch.randn(c, D, device=DEV, generator=g) for c in cats]
    K = (2 + M) * D
    W = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    bias = torch.randn(N, device=DEV, generator=g)
    ids = {"user": torch.randint(0, NU, (B,), device=DEV, dtype=torch.int32, generator=g),
           "pos": torch.randint(0, NI, (B,), device=DEV, dtype=torch.int32, generator=g),
           "neg": torch.randint(0, NI, (B,), device=DEV, dtype=torch.int32, generator=g)}
    ids["user"][:100] = 7  # duplicates
    pm = nm = None
    if M:
        pm = torch.stack([torch.randint(0, c, (B,), device=DEV, dtype=torch.int32, generator=g) for c in cats], 1).contiguous()
        nm = torch.stack([torch.randint(0, c, (B,), device=DEV, dtype=torch.int32, generator=g) for c in cats], 1).contiguous()
    T, keep = ops.make_tables(tabs[0], tabs[1], None, None, tabs[2:], [])
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    Bt, keep2 = ops.make_batch(ids["user"], ids["pos"], ids["neg"] if passes == 2 else None, pm, nm if passes == 2 else None, err)
    rows = passes * B
    part_a = torch.zeros((rows // 128, 2, N), device=DEV)
    part_b = torch.zeros_like(part_a)
    if bf16:
        W16 = W.bfloat16()
        x_ref = torch.empty((rows, K), dtype=torch.bfloat16, device=DEV)
        ops.mlp_gather_concat(T, Bt, passes, x16=x_ref)
        y_ref = ops.gemm_bf16in(False, x_ref, W16, bias=bias, bn_part=part_a, out_bf16=out16)
        x_img = torch.zeros_like(x_ref)
        y = torch.zeros((rows, N), dtype=torch.bfloat16 if out16 else torch.float32, device=DEV)
        assert ops.mlp_gather_gemm1(T, Bt, passes, W16, bias, y, part_b, x_img)
    else:
        x_ref = torch.empty((rows, K), device=DEV)
        ops.mlp_gather_concat(T, Bt, passes, x_ref)
        y_ref = ops.gemm(False, True, x_ref, W, bias=bias, bn_part=part_a)
        x_img = torch.zeros_like(x_ref)
        y = torch.zeros((rows, N), device=DEV)
        assert ops.mlp_gather_gemm1(T, Bt, passes, W, bias, y, part_b, x_img)
    torch.cuda.synchronize()
    assert err.item() == 0
    # x0 itself against torch indexing (the gather the reference does with nn.Embedding + torch.cat)
    cols = [tabs[0][ids["user"].long()].repeat(passes, 1),
            torch.cat([tabs[1][ids["pos"].long()]] + ([tabs[1][ids["neg"].long()]] if passes == 2 else []))]
    for m in range(M):
        cols.append(torch.cat([tabs[2 + m][pm[:, m].long()]] + ([tabs[2 + m][nm[:, m].long()]] if passes == 2 else [])))
    want_x = torch.cat(cols, 1)
    assert torch.equal(x_img, want_x.to(x_img.dtype)) and torch.equal(x_img, x_ref)
    assert torch.equal(y, y_ref) and torch.equal(part_a, part_b)
    # without the image (eval): the same y
    y2 = torch.zeros_like(y)
    assert ops.mlp_gather_gemm1(T, Bt, passes, W16 if bf16 else W, bias, y2, None, None)
    assert torch.equal(y2, y)
    # shapes the fused kernels do not take are refused without a launch (False), not run wrong
    Bt_small, keep3 = ops.make_batch(ids["user"][:384], ids["pos"][:384], ids["neg"][:384] if passes == 2 else None,
                                     None if pm is None else pm[:384].contiguous(),
                                     None if (nm is None or passes == 1) else nm[:384].contiguous(), err)
    assert not ops.mlp_gather_gemm1(T, Bt_small, passes, W16 if bf16 else W, bias, y[:passes * 384], None, None)
    # an id outside its table: flagged, clamped (no fault)
    bad = ids["pos"].clone()
    bad[5] = NI + 3
    Bt_bad, keep4 = ops.make_batch(ids["user"], bad, ids["neg"] if passes == 2 else None, pm, nm if passes == 2 else None, err)
    assert ops.mlp_gather_gemm1(T, Bt_bad, passes, W16 if bf16 else W, bias, y2, None, None)
    torch.cuda.synchronize()
    assert err.item() == 1
