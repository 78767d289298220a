# -*- coding: utf-8 -*-
"""Score-aware hard-negative mining on the GPU (trs_batch_prepare_mined) against the numpy restatement
tests/mining_ref.py: bit-exact choices on exactly representable tables, float tables under the near-tie rule, the
K = 1 identity with the unmined loader, the sampler's rules, consistency with the scoring pass, fit() end to end with a
step-by-step replay, and the unmined paths left where they were."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

import mining_ref
from conftest import rel_err
from oracle import nets as onets
from oracle import optim as ooptim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5          # the project's fp32 tolerance (norm-wise relative)
NEAR_TIE_CAP = 1e-3  # largest share of triples whose fp32 choice may differ from the float64 arg-max (near-ties only)


def _ops():
    from torchrecsys_amd import ops
    return ops


def make_params(net, NU, NI, D, M, rs, exact):
    """exact: small integers — every product and partial sum of a score is exactly representable in fp32 (and ties are
    frequent); else N(0, 0.3)."""
    sizes = [5, 7][:M]
    draw = (lambda shape: rs.randint(-2, 3, shape)) if exact else (lambda shape: rs.normal(0, 0.3, shape))
    lin = ("user_bias.weight", "item_bias.weight") if net == "linear" else ("linear_user.weight", "linear_item.weight")
    p = {"user.weight": draw((NU, D)), "item.weight": draw((NI, D)), lin[0]: draw((NU, 1)), lin[1]: draw((NI, 1))}
    for m in range(M):
        p[f"metadata.{m}.weight"] = draw((sizes[m], D))
        if net == "fm":
            p[f"linear_metadata.{m}.weight"] = draw((sizes[m], 1))
    p = {k: v.astype(np.float32) for k, v in p.items()}
    item_meta = np.stack([rs.randint(0, sizes[m], NI) for m in range(M)], axis=1).astype(np.int32) if M else None
    return p, item_meta


def to_tables(net, p, M):
    ops = _ops()
    t = {k: torch.from_numpy(v).to(DEV) for k, v in p.items()}
    lin = ("user_bias.weight", "item_bias.weight") if net == "linear" else ("linear_user.weight", "linear_item.weight")
    metas = [t[f"metadata.{m}.weight"] for m in range(M)]
    meta_lins = [t[f"linear_metadata.{m}.weight"] for m in range(M)] if net == "fm" else []
    T, keep = ops.make_tables(t["user.weight"], t["item.weight"], t[lin[0]], t[lin[1]], metas, meta_lins)
    return T, (keep, t)


def make_stream(rs, NU, NI, N):
    """Interaction stream with forced repeats: a hot user and a hot item take a tenth of the rows each."""
    su, si = rs.randint(0, NU, N), rs.randint(0, NI, N)
    su[rs.rand(N) < 0.1] = 3
    si[rs.rand(N) < 0.1] = 7
    return su.astype(np.int32), si.astype(np.int32)


def samplers(su, si, NU, NI, k, options, K, top, max_tries=8, mine="hardest"):
    """(ops.Sampler, the restatement's dict) of the same options."""
    ops = _ops()
    su_d, si_d = torch.from_numpy(su).to(DEV), torch.from_numpy(si).to(DEV)
    seen = ops.Sampler.seen_csr(su_d, si_d, NU, NI) if options else None
    dev = ops.Sampler(k=k, popularity=options, seen=seen, stream_item=si_d, max_tries=max_tries, mine=mine,
                      candidates=K, top=top)
    ref = {"k": k, "max_tries": max_tries}
    if options:
        ref.update(popularity=True, seen=(seen[0].cpu().numpy(), seen[1].cpu().numpy()))
    return dev, ref, (su_d, si_d)


def mined_on_device(su_d, si_d, key, t0, B, NI, seed, net, T, sampler, item_meta):
    ops = _ops()
    im = None if item_meta is None else torch.from_numpy(item_meta).to(DEV)
    out = ops.batch_prepare_mined(su_d, si_d, key, t0, B, NI, seed, t0, net, T, sampler, im, return_chosen=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_near_ties(got_neg, ref, what=""):
    """The float rule of the issue: the mined ITEM is the float64 arg-max item, or the float64 gap between its score and
    the best is <= 1e-5 * max|z|.  Returns the number of triples that took the second branch; any other triple fails."""
    z, cand = ref["z"], ref["cand"]
    differ = np.nonzero(got_neg != ref["neg"])[0]
    if differ.size == 0:
        return 0
    is_cand = (cand[differ] == got_neg[differ, None])
    assert is_cand.any(axis=1).all(), f"{what}: a mined negative is not one of the triple's candidates"
    z_got = np.where(is_cand, z[differ], -np.inf).max(axis=1)
    gap = z[differ].max(axis=1) - z_got
    bound = TOL * np.abs(z).max()
    print(f"{what}: {differ.size} of {got_neg.size} triples differ from the float64 arg-max item, largest gap "
          f"{gap.max():.3e} (bound {bound:.3e})")
    assert (gap <= bound).all(), f"{what}: a mined negative is neither the arg-max item nor a near-tie"
    return int(differ.size)


# ------------------------------------------------------------------------------------------------ 1. exact arithmetic
@pytest.mark.parametrize("M", [0, 2])
@pytest.mark.parametrize("D", [16, 64, 100, 128])
@pytest.mark.parametrize("net", ["linear", "fm"])
def test_choice_is_bit_exact_on_exact_arithmetic(net, D, M):
    rs = np.random.RandomState(D + 7 * M + (net == "fm"))
    NU, NI, N, B = 50, 200, 3000, 2048
    p, item_meta = make_params(net, NU, NI, D, M, rs, exact=True)
    T, keep = to_tables(net, p, M)
    su, si = make_stream(rs, NU, NI, N)
    n_ties = 0
    for options in (False, True):
        for k in (1, 2):
            t0, key, seed = 517 * k, 0x1234ABCD5 + k, 99 + k
            for K in (1, 2, 8, 33, 64):
                cand = None
                for top in (1, 3):
                    if top > K:
                        continue
                    dev, ref_s, (su_d, si_d) = samplers(su, si, NU, NI, k, options, K, top)
                    got = mined_on_device(su_d, si_d, key, t0, B, NI, seed, net, T, dev, item_meta)
                    ref = mining_ref.mined_batch(su, si, key, t0, B, NI, seed, t0, net, p, K, top, ref_s, item_meta,
                                                 cand=cand)
                    cand = ref["cand"]
                    for name in ("user", "pos", "neg", "chosen") + (("pos_meta", "neg_meta") if M else ()):
                        assert np.array_equal(got[name], ref[name]), (name, options, k, K, top)
                    if K > 1:
                        zs = np.sort(ref["z"], axis=1)
                        n_ties += int((zs[:, -1] == zs[:, -2]).sum())
    assert n_ties > 0  # exact ties at the top occur: the index rule was exercised


@pytest.mark.parametrize("net,D,M", [("fm", 100, 2), ("linear", 16, 0), ("fm", 16, 2), ("linear", 128, 0)])
def test_ragged_batches_and_several_iterations_per_wave(net, D, M, tune):
    """B that is not a multiple of the triples a wave owns (64 / G: the last wave's spare lane groups load the batch's
    last position and write nothing), and a grid capped far below the batch so that every wave walks several
    iterations: ids, choice and metadata rows equal the restatement, and nothing is written beyond B."""
    ops = _ops()
    rs = np.random.RandomState(3 * D + M)
    NU, NI, N = 50, 200, 3000
    p, item_meta = make_params(net, NU, NI, D, M, rs, exact=True)
    T, keep = to_tables(net, p, M)
    su, si = make_stream(rs, NU, NI, N)
    im = None if item_meta is None else torch.from_numpy(item_meta).to(DEV)
    for B, cap in ((2047, None), (1, None), (2047, 3), (1531, 1)):
        if cap is not None:
            tune(GRID_CAP=cap)  # workgroups of the launch: 4 waves each
        for K, top, options in ((8, 1, False), (33, 3, True), (2, 1, True)):
            dev, ref_s, (su_d, si_d) = samplers(su, si, NU, NI, 1, options, K, top)
            names = ("user", "pos", "neg", "chosen") + (("pos_meta", "neg_meta") if M else ())
            out = {k: torch.full((B + 64,) + ((M,) if k.endswith("meta") else ()), -7, dtype=torch.int32, device=DEV)
                   for k in names}
            ops.batch_prepare_mined(su_d, si_d, 0x9A1B, 301, B, NI, 5, 301, net, T, dev, im, out=out, return_chosen=True)
            torch.cuda.synchronize()
            ref = mining_ref.mined_batch(su, si, 0x9A1B, 301, B, NI, 5, 301, net, p, K, top, ref_s, item_meta)
            for name in names:
                got = out[name].cpu().numpy()
                assert np.array_equal(got[:B], ref[name]), (name, B, cap, K, top)
                assert (got[B:] == -7).all(), (name, B, cap, "written beyond the batch")


# ------------------------------------------------------------------------------------------------ 2. float tables
@pytest.mark.parametrize("net,D,M,key", [("linear", 64, 0, 0), ("fm", 64, 0, 0x77AA1), ("linear", 128, 0, 0x5151),
                                         ("fm", 128, 0, 0), ("fm", 16, 0, 0), ("linear", 100, 2, 0), ("fm", 64, 2, 0)])
def test_float_tables_mine_the_float64_argmax_item(net, D, M, key):
    rs = np.random.RandomState(D + M)
    NU, NI, B, K = 20000, 5000, 65536, 8
    p, item_meta = make_params(net, NU, NI, D, M, rs, exact=False)
    T, keep = to_tables(net, p, M)
    su, si = make_stream(rs, NU, NI, B)
    dev, ref_s, (su_d, si_d) = samplers(su, si, NU, NI, 1, False, K, 1)
    got = mined_on_device(su_d, si_d, key, 0, B, NI, 31, net, T, dev, item_meta)
    ref = mining_ref.mined_batch(su, si, key, 0, B, NI, 31, 0, net, p, K, 1, ref_s, item_meta)
    assert np.array_equal(got["user"], ref["user"]) and np.array_equal(got["pos"], ref["pos"])
    n = check_near_ties(got["neg"], ref, f"{net} D={D} M={M}")
    assert n <= NEAR_TIE_CAP * B, n
    if M:
        assert np.array_equal(got["neg_meta"], item_meta[got["neg"]])
        assert np.array_equal(got["pos_meta"], item_meta[got["pos"]])
    cand_of_chosen = np.take_along_axis(ref["cand"], got["chosen"][:, None].astype(np.int64), axis=1)[:, 0]
    assert np.array_equal(cand_of_chosen, got["neg"])  # `chosen` indexes the candidate that was written


# ------------------------------------------------------------------------------------------------ 3. K = 1 identity
@pytest.mark.parametrize("net,M", [("fm", 2), ("linear", 0)])
@pytest.mark.parametrize("options,k", [(False, 1), (True, 1), (True, 2), (False, 2)])
def test_one_candidate_equals_batch_prepare_bit_for_bit(net, M, options, k):
    ops = _ops()
    rs = np.random.RandomState(11)
    NU, NI, N, B, D = 300, 400, 5000, 4096, 32
    p, item_meta = make_params(net, NU, NI, D, M, rs, exact=False)
    T, keep = to_tables(net, p, M)
    su, si = make_stream(rs, NU, NI, N)
    dev, _, (su_d, si_d) = samplers(su, si, NU, NI, k, options, 1, 1)
    plain, _, _ = samplers(su, si, NU, NI, k, options, 8, 1, mine=None)
    im = None if item_meta is None else torch.from_numpy(item_meta).to(DEV)
    for sampler in (plain, None) if (not options and k == 1) else (plain,):
        want = ops.batch_prepare(su_d, si_d, None, 0xFEED5, 700, B, NI, 5, 700, im, sampler=sampler)
        got = ops.batch_prepare_mined(su_d, si_d, 0xFEED5, 700, B, NI, 5, 700, net, T, dev, im, return_chosen=True)
        torch.cuda.synchronize()
        for name in want:
            assert torch.equal(got[name], want[name]), name
        assert int(got["chosen"].abs().max()) == 0


# ------------------------------------------------------------------------------------------------ 4. sampler rules
@pytest.mark.parametrize("top", [1, 4])
def test_sampler_rules_hold_for_the_mined_negative(top):
    rs = np.random.RandomState(4)
    NU, NI, N, B, D = 80, 500, 6000, 6000, 16
    p, _ = make_params("fm", NU, NI, D, 0, rs, exact=False)
    T, keep = to_tables("fm", p, 0)
    su, si = make_stream(rs, NU, NI, N)
    dev, _, (su_d, si_d) = samplers(su, si, NU, NI, 1, True, 16, top, max_tries=32)
    got = mined_on_device(su_d, si_d, 0x55, 0, B, NI, 9, "fm", T, dev, None)
    assert (got["neg"] != got["pos"]).all()
    seen = set((su.astype(np.int64) * NI + si).tolist())
    assert not any(int(u) * NI + int(j) in seen for u, j in zip(got["user"], got["neg"]))
    assert ((0 <= got["neg"]) & (got["neg"] < NI)).all() and ((0 <= got["chosen"]) & (got["chosen"] < 16)).all()


# ------------------------------------------------------------------------------------------------ 5. scoring pass
@pytest.mark.parametrize("net,D,M", [("linear", 64, 0), ("fm", 64, 0), ("fm", 128, 0), ("linear", 100, 2), ("fm", 16, 2)])
def test_mined_score_is_never_below_candidate_zero(net, D, M):
    """trs_score_forward on the mined batch and on the candidate-0 batch of the same tables: the mined negative's score is
    >= candidate 0's for EVERY triple, exactly (the miner ranks by the very value the pass computes; FM compares the
    sigmoid values, where equality may replace strict order) — hence the summed hinge loss can only grow."""
    ops = _ops()
    rs = np.random.RandomState(D + M)
    NU, NI, N, B = 3000, 2000, 40000, 32768
    p, item_meta = make_params(net, NU, NI, D, M, rs, exact=False)
    T, keep = to_tables(net, p, M)
    su, si = make_stream(rs, NU, NI, N)
    dev, _, (su_d, si_d) = samplers(su, si, NU, NI, 1, False, 8, 1)
    im = None if item_meta is None else torch.from_numpy(item_meta).to(DEV)
    mined = ops.batch_prepare_mined(su_d, si_d, 0xC0FFEE, 100, B, NI, 3, 100, net, T, dev, im)
    base = ops.batch_prepare(su_d, si_d, None, 0xC0FFEE, 100, B, NI, 3, 100, im, sampler=None)
    scores = []
    for ids in (mined, base):
        Bt, k2 = ops.make_batch(ids["user"], ids["pos"], ids["neg"], ids.get("pos_meta"), ids.get("neg_meta"), None)
        scores.append(ops.score_forward(net, T, Bt, B, DEV))
    (pm, nm), (pb, nb) = scores
    assert torch.equal(pm, pb)
    assert bool((nm >= nb).all())
    assert bool((nm > nb).any())
    hinge = lambda pos, neg: float(torch.clamp(neg - pos + 1, min=0).double().sum())  # noqa: E731
    assert hinge(pm, nm) >= hinge(pb, nb)


# ------------------------------------------------------------------------------------------------ 6. end to end
def _model(net_type, M, neg_sampling, seed=1, n_factors=16):
    from torchrecsys_amd.model import TorchRecSys
    rs = np.random.RandomState(4)
    n_u, n_i, n = 80, 500, 6000
    users = torch.from_numpy(np.concatenate([np.arange(n_u), rs.randint(0, n_u, n - n_u)]).astype(np.int64)).to(DEV)
    items = torch.from_numpy(np.concatenate([np.arange(n_i), rs.randint(0, n_i, n - n_i)]).astype(np.int64)).to(DEV)
    meta = torch.from_numpy(rs.randint(0, 6, (n_i, M)).astype(np.int64)).to(DEV) if M else None
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        return TorchRecSys.from_tensors(users, items, n_users=n_u, n_items=n_i, item_metadata=meta,
                                        metadata_names=[f"c{m}" for m in range(M)] if M else None,
                                        n_factors=n_factors, net_type=net_type, dynamic_neg_sampling=True, seed=seed,
                                        neg_sampling=neg_sampling)


def _rows_within(got, want, tol):
    return float((np.abs(got - want).max(axis=1) <= tol * np.abs(want).max()).mean())


@pytest.mark.parametrize("loss", ["hinge", "bpr"])
@pytest.mark.parametrize("opt_kind", ["sgd", "sparse_adam"])
@pytest.mark.parametrize("net_type,M", [("linear", 0), ("fm", 0), ("linear", 1), ("fm", 1)])
def test_fit_with_mining_and_step_by_step_replay(net_type, M, opt_kind, loss):
    from torchrecsys_amd._lib import LOSS_ID
    from oracle.nets import touched_rows
    ns = dict(mine="hardest", candidates=8, top=2, k=2)
    make_opt = (lambda m: torch.optim.SGD(m.parameters(), lr=0.1)) if opt_kind == "sgd" else \
        (lambda m: torch.optim.SparseAdam(list(m.parameters()), lr=0.01))
    model = _model(net_type, M, ns)
    opt = make_opt(model)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        model.fit(opt, epochs=3, batch_size=128, loss=loss)
        model.evaluate(batch_size=128)
    losses = [float(x) for x in re.findall(r"Training Loss: ([0-9.]+)", buf.getvalue())]
    print("training losses", losses)
    assert len(losses) == 3 and all(np.isfinite(losses))
    assert "Testing auc" in buf.getvalue()

    # replay: every step's ids against the restatement on the tables as they were, then the oracle's step with the
    # device's ids against the tables after the step
    model = _model(net_type, M, ns)
    opt = make_opt(model)
    B, steps = 256, 24  # 256 triples over 80 users: every batch repeats users and items
    runner = model.make_runner(opt, B)
    runner.trainer.loss_id = LOSS_ID[loss]
    model.net.train()
    runner.begin_epoch()
    st = model._device_stream("train")
    su, si = st["user"].cpu().numpy(), st["pos"].cpu().numpy()
    item_meta = None if st["item_meta"] is None else st["item_meta"].cpu().numpy()
    names = list(model.net.state_dict().keys())
    plist = dict(model.net.named_parameters())
    n_near, n_total = 0, 0
    for step in range(steps):
        before = {k: v.detach().cpu().numpy().copy() for k, v in model.net.state_dict().items()}
        state = {k: {s: (v.detach().cpu().numpy().copy() if torch.is_tensor(v) and v.dim() else float(v))
                     for s, v in opt.state[plist[k]].items()} for k in names if len(opt.state.get(plist[k], {}))}
        assert runner.run_steps(1) == 1
        torch.cuda.synchronize()
        ids = {k: v.cpu().numpy().astype(np.int64) for k, v in runner.prep_out.items()}
        ref = mining_ref.mined_batch(su, si, runner.shuffle_key, step * B, B, model.n_items, runner.sample_seed, step * B,
                                     net_type, before, 8, 2, {"k": 2, "max_tries": 8}, item_meta)
        assert np.array_equal(ids["user"], ref["user"]) and np.array_equal(ids["pos"], ref["pos"])
        # top = 2: the restatement's candidate of the drawn rank; a device choice that differs must be a near-tie of it
        differ = np.nonzero(ids["neg"] != ref["neg"])[0]
        for t in differ:
            zc = ref["z"][t][ref["cand"][t] == ids["neg"][t]]
            assert zc.size, "mined negative is not a candidate"
            assert abs(zc[0] - ref["z"][t][ref["chosen"][t]]) <= TOL * np.abs(ref["z"]).max()
        n_near += differ.size
        n_total += B
        batch = {"user_id": ids["user"], "pos_item_id": ids["pos"], "neg_item_id": ids["neg"]}
        if M:
            assert np.array_equal(ids["neg_meta"], item_meta[ids["neg"]])
            batch["pos_metadata_id"], batch["neg_metadata_id"] = ids["pos_meta"], ids["neg_meta"]
        want = {k: v.copy() for k, v in before.items()}
        _, _, oloss, grads = onets.train_forward_backward(net_type, want, batch, loss=loss)
        assert abs(runner.loss_sums[step].item() / B - float(oloss)) <= 5 * TOL * max(abs(float(oloss)), 1e-3)
        after = {k: v.detach().cpu().numpy() for k, v in model.net.state_dict().items()}
        if opt_kind == "sgd":
            ooptim.sgd_step(want, grads, 0.1)
            for k in names:
                assert rel_err(after[k], want[k]) < 5 * TOL, (step, k)
        else:
            rows = touched_rows(net_type, want, batch)
            for k in names:
                s = state.get(k, {})
                m1 = s.get("exp_avg", np.zeros_like(want[k]))
                m2 = s.get("exp_avg_sq", np.zeros_like(want[k]))
                ooptim.sparse_adam_rows(want[k], grads[k], rows[k], m1, m2, int(s.get("step", 0)) + 1, 0.01)
                # the bulk criterion of test_presorted_adaptive_rules_match_the_oracle for batches with repeated rows
                assert _rows_within(after[k], want[k], 1e-3) >= 0.97, (step, k)
                assert rel_err(after[k], want[k]) < 0.05, (step, k)
    print(f"replay: {n_near} of {n_total} triples chose a near-tie of the restatement's candidate")
    assert n_near <= NEAR_TIE_CAP * n_total
    runner.end_epoch()


# ------------------------------------------------------------------------------------------------ 7. nothing else moved
def test_unmined_runs_keep_their_paths_and_mining_leaves_them(monkeypatch):
    from torchrecsys_amd import ops
    from torchrecsys_amd.engine import SparseScorerTrainer
    calls = {"mined": 0, "sorted": 0, "stream": 0, "prepare": 0}

    def spy(obj, name, key):
        orig = getattr(obj, name)

        def wrapped(*a, **kw):
            calls[key] += 1
            return orig(*a, **kw)
        monkeypatch.setattr(obj, name, wrapped)

    spy(ops, "batch_prepare_mined", "mined")
    spy(ops, "batch_prepare", "prepare")
    spy(SparseScorerTrainer, "fast_sorted_steps", "sorted")
    spy(SparseScorerTrainer, "fast_stream_steps", "stream")

    def run(ns, steps=6):
        for key in calls:
            calls[key] = 0
        model = _model("fm", 0, ns)
        runner = model.make_runner(torch.optim.SGD(model.parameters(), lr=0.1), 128)
        model.net.train()
        runner.begin_epoch()
        assert runner.run_steps(steps) == steps
        runner.end_epoch()
        return dict(calls)

    c = run(None)
    assert c["mined"] == 0 and c["sorted"] > 0 and c["stream"] == 0 and c["prepare"] == 0
    c = run({"k": 2, "max_tries": 4})
    assert c["mined"] == 0 and c["sorted"] > 0
    monkeypatch.setenv("TRS_PRESORT_MIN_DENSITY", "1e9")  # no presort: the C step loop reads the resident stream
    c = run(None)
    assert c["mined"] == 0 and c["stream"] > 0 and c["sorted"] == 0 and c["prepare"] == 0
    c = run({"mine": "hardest"})
    assert c["mined"] == 6 and c["sorted"] == 0 and c["stream"] == 0 and c["prepare"] == 0
    monkeypatch.delenv("TRS_PRESORT_MIN_DENSITY")
    c = run({"mine": "hardest", "candidates": 4, "k": 2})
    assert c["mined"] == 6 and c["sorted"] == 0 and c["stream"] == 0 and c["prepare"] == 0
