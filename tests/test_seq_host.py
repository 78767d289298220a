# -*- coding: utf-8 -*-
"""The sequence model without a GPU: trs_seq_fwd_bwd / trs_seq_user_rows are declared, exported and bound and refuse bad
arguments on the host; fit_sequence / recommend_next / recommend_for_sequences / evaluate_next validate before any
device work; the shipped kernels use no scratch; the ordered CSR is what a pandas groupby gives; and the numpy
restatement (tests/seq_ref.py) is consistent with itself."""
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

import foldin_ref as base
import seq_ref as ref
from test_abi import _shipped_kernel_registers
from torchrecsys_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTO = _lib.PROTOTYPES["trs_seq_fwd_bwd"]  # this module is about that entry point


def _err():
    return _lib.load().trs_last_error().decode()


def test_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "trs.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in (("trs_seq_fwd_bwd", 18), ("trs_seq_user_rows", 11)):
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        assert len(_lib.PROTOTYPES[name][1]) == n_args
        decl = header[header.index(name + "("):]
        assert decl[:decl.index(")")].count(",") == n_args - 1
    assert int(re.search(r"#define TRS_SEQ_LMAX (\d+)", header).group(1)) == _lib.SEQ_LMAX == 16
    assert open(os.path.join(ROOT, "torchrecsys_amd", "csrc", "Makefile")).read().count("seq.hip") == 1


def test_entry_points_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    P = 0x1000  # never dereferenced

    def tables(**kw):
        T = _lib.TrsTables()
        T.user = T.item = T.user_lin = T.item_lin = P
        T.n_users, T.n_items, T.D, T.M = 40, 30, 16, 0
        for k, v in kw.items():
            setattr(T, k, v)
        return T

    def csr(off=P, items=P, n_rows=40):
        c = _lib.TrsCsr()
        c.off, c.items, c.n_rows = off, items, n_rows
        return c

    def fwd(T=tables(), ctx=P, seq=csr(), user=P, entry=P, neg=P, B=8, L=4, w=P, loss=1, loss_sum=P, gr=P, gl=P,
            cid=P):
        return lib.trs_seq_fwd_bwd(ctypes.byref(T) if T is not None else None, ctx,
                                   ctypes.byref(seq) if seq is not None else None, user, entry, neg, B, L, w, loss,
                                   0.125, loss_sum, None, gr, gl, cid, None, None)

    for kw, word in ((dict(T=None), "tables"), (dict(T=tables(user=None)), "NULL"), (dict(T=tables(item=None)), "NULL"),
                     (dict(T=tables(item_lin=None)), "NULL"), (dict(T=tables(user_lin=None)), "NULL"),
                     (dict(T=tables(M=1)), "metadata"), (dict(T=tables(D=0)), "D=0"), (dict(T=tables(D=1025)), "D=1025"),
                     (dict(T=tables(D=258)), "D=258"), (dict(ctx=None), "context"), (dict(seq=None), "CSR"),
                     (dict(seq=csr(off=None)), "CSR"), (dict(seq=csr(items=None)), "CSR"),
                     (dict(seq=csr(n_rows=0)), "CSR"), (dict(L=-1), "L=-1"), (dict(L=17), "L=17"),
                     (dict(w=None), "ctx_weight"), (dict(loss=2), "loss"), (dict(loss=3), "loss"), (dict(loss=-1), "loss"),
                     (dict(loss_sum=None), "loss_sum"), (dict(gr=None), "grad_rows"), (dict(gl=None), "grad_rows"),
                     (dict(cid=None), "ctx_ids_out"), (dict(B=-1), "batch"), (dict(user=None), "NULL"),
                     (dict(entry=None), "NULL"), (dict(neg=None), "NULL")):
        assert fwd(**kw) == -1, kw
        assert _err().startswith("trs_seq_fwd_bwd:") and word in _err(), (kw, _err())
    # nothing to do, nothing launched; forward only and L = 0 need no staging outputs; bad arguments are still bad
    assert fwd(B=0) == 0 and fwd(B=0, user=None, entry=None, neg=None) == 0
    assert fwd(B=0, gr=None, gl=None, cid=None) == 0 and fwd(B=0, L=0, w=None, cid=None) == 0
    assert fwd(B=0, L=17) == -1 and fwd(B=0, loss_sum=None) == -1

    def rows(T=tables(), ctx=P, seq=csr(n_rows=5), users=P, n=5, L=4, w=P, out=P, ld=16):
        return lib.trs_seq_user_rows(ctypes.byref(T) if T is not None else None, ctx,
                                     ctypes.byref(seq) if seq is not None else None, users, n, L, w, out, ld, None, None)

    for kw, word in ((dict(T=None), "tables"), (dict(T=tables(user=None)), "NULL"), (dict(T=tables(M=2)), "metadata"),
                     (dict(T=tables(D=1026)), "D=1026"), (dict(ctx=None), "context"), (dict(seq=None), "CSR"),
                     (dict(seq=csr(off=None, n_rows=5)), "CSR"), (dict(seq=csr(items=None, n_rows=5)), "item ids"),
                     (dict(seq=csr(n_rows=4)), "rows"), (dict(n=-1, seq=csr(n_rows=-1)), "CSR"), (dict(L=17), "L=17"),
                     (dict(w=None), "ctx_weight"), (dict(out=None), "out"), (dict(ld=15), "ld=15"),
                     (dict(ld=18), "ld=18")):
        assert rows(**kw) == -1, kw
        assert _err().startswith("trs_seq_user_rows:") and word in _err(), (kw, _err())
    assert rows(n=0, seq=csr(n_rows=0), out=None) == 0
    assert rows(n=0, seq=csr(n_rows=0), ld=8) == -1


def test_every_shipped_sequence_kernel_is_free_of_scratch(tmp_path):
    """One instance of seq_stage_kernel and of seq_rows_kernel per entry of TRS_ROW_SHAPES (12), none with scratch.
    Every instance stays within the 128 VGPRs of four waves per SIMD but the staging kernel of the widest shape
    (D > 512: 16 registers per row), which keeps three (DESIGN.md 4.18 lists the counts)."""
    found = _shipped_kernel_registers(tmp_path)
    for fam in ("seq_stage_kernel", "seq_rows_kernel"):
        seen = {n: v for n, v in found.items() if re.search(r"\d%sI" % fam, n)}
        assert len(seen) == 12, (fam, sorted(seen))
        for n, (vgpr, scratch) in seen.items():
            widest = "seq_stage_kernelILi4ELi64ELi4E" in n
            assert scratch == 0 and vgpr <= (168 if widest else 128), (n, vgpr, scratch)
    assert not [n for n in found if "seq_" in n and re.search(r"score_kernel|multineg_kernel|warp_kernel", n)]


# ------------------------------------------------------------------------------------------------ the ordered CSR
def _frame(seed=3, n=400, n_users=23, n_items=17):
    rs = np.random.RandomState(seed)
    return pd.DataFrame({"u": rs.randint(0, n_users, n), "i": rs.randint(0, n_items, n), "pos": np.arange(n),
                         "ts": rs.randint(0, 25, n)})  # few distinct timestamps: plenty of ties


def _groupby(df, by, n_users):
    g = df.sort_values(by, kind="stable").groupby("u")["i"].apply(list)
    return [g.get(u, []) for u in range(n_users)]


@pytest.mark.parametrize("with_ts", [False, True])
def test_ordered_csr_is_the_pandas_groupby(with_ts):
    from torchrecsys_amd.model import ordered_sequences, sequence_entries
    df = _frame()
    rs = np.random.RandomState(0)
    rows = rs.permutation(len(df))[:300]  # a split's train rows: a subset of the input, in permutation order
    tr = df.iloc[rows]
    ts = torch.from_numpy(df["ts"].to_numpy()) if with_ts else None
    off, ids = ordered_sequences(torch.from_numpy(tr["u"].to_numpy()), torch.from_numpy(tr["i"].to_numpy()),
                                 torch.from_numpy(rows.astype(np.int64)), 23, ts)
    want = _groupby(tr, ["ts", "pos"] if with_ts else ["pos"], 23)
    assert ids.dtype == torch.int32 and off.dtype == torch.int64 and int(off[-1]) == 300
    got = [ids[int(off[u]):int(off[u + 1])].tolist() for u in range(23)]
    assert got == want
    assert any(len(set(s)) < len(s) for s in got), "the frame must repeat items inside a sequence"
    if with_ts:
        assert got != _groupby(tr, ["pos"], 23), "the timestamps must change the order"
    # holdout_last: the last position of every user with at least two, nothing of the others
    entries, hu, hp = sequence_entries(off, True)
    lens = np.diff(off.numpy())
    assert hu.tolist() == [u for u in range(23) if lens[u] >= 2]
    assert hp.tolist() == [int(off[u + 1]) - 1 for u in hu.tolist()]
    assert sorted(entries.tolist() + hp.tolist()) == list(range(300)) and entries.numel() == 300 - hu.numel()
    e2, hu2, hp2 = sequence_entries(off, False)
    assert e2.tolist() == list(range(300)) and hu2.numel() == 0 and hp2.numel() == 0
    e_ref, u_ref, h_ref = ref.holdout(off.numpy())
    assert e_ref.tolist() == entries.tolist() and u_ref.tolist() == hu.tolist() and h_ref.tolist() == hp.tolist()


def test_train_rows_are_the_input_positions_of_the_split_for_both_front_doors():
    from torchrecsys_amd.model import TorchRecSys
    df = _frame(seed=5, n=200)
    with contextlib.redirect_stdout(io.StringIO()):
        a = TorchRecSys(df, "u", "i", n_factors=8, dynamic_neg_sampling=True)
        b = TorchRecSys.from_tensors(torch.from_numpy(df["u"].to_numpy()), torch.from_numpy(df["i"].to_numpy()),
                                     n_factors=8, dynamic_neg_sampling=True)
    for m in (a, b):
        rows = m.data_processor.train_rows()
        assert m.data_processor.n_input_rows == 200 and rows.numel() == 160 and rows.unique().numel() == 160
        assert not bool((rows[1:] > rows[:-1]).all()), "the split's order is a permutation, not ascending"
        assert torch.equal(m.data_processor.train_data["user_id"].long(), torch.from_numpy(df["u"].to_numpy())[rows])
        assert torch.equal(m.data_processor.train_data["pos_item_id"].long(), torch.from_numpy(df["i"].to_numpy())[rows])


# ------------------------------------------------------------------------------------------------ public arguments
def _model(net_type="linear", M=0, n_factors=8, **kw):
    return base.make_model(net_type, 40, 30, n_factors, M, seed=1, scale=0.3, **kw)


def test_public_calls_refuse_before_any_device_work(monkeypatch):
    from torchrecsys_amd import model as model_mod

    def no_device(*a, **kw):
        raise AssertionError("reached the device before validating the arguments")
    # (the models first: where a GPU is present their construction moves the net to it)
    others = [_model(kind) for kind in ("fm", "mlp", "ease")]
    with_meta, wide, too_wide, m = _model("linear", M=2), _model("linear", n_factors=258), _model(n_factors=260), _model()
    monkeypatch.setattr(model_mod, "_device", no_device)
    calls = (lambda m: m.fit_sequence(), lambda m: m.recommend_next([0]), lambda m: m.recommend_for_sequences([[1]]),
             lambda m: m.evaluate_next())
    for call in calls:
        for other in others:
            with pytest.raises(ValueError, match="linear"):
                call(other)
        with pytest.raises(ValueError, match="metadata"):
            call(with_meta)
        with pytest.raises(ValueError, match="n_factors"):
            call(wide)
    monkeypatch.setattr(model_mod.tdist, "world_info", lambda: (0, 2))
    for call in calls:
        with pytest.raises(NotImplementedError, match="world"):
            call(m)
    monkeypatch.undo()
    monkeypatch.setattr(model_mod, "_device", no_device)
    n_in = m.data_processor.n_input_rows
    for kw, word in ((dict(epochs=0), "epochs"), (dict(epochs=1.5), "epochs"), (dict(epochs=True), "epochs"),
                     (dict(lr=0), "lr"), (dict(lr=-0.1), "lr"), (dict(lr=float("nan")), "lr"), (dict(lr="1"), "lr"),
                     (dict(batch_size=0), "batch_size"), (dict(context=-1), "context"), (dict(context=17), "context"),
                     (dict(context=2.0), "context"), (dict(decay=0), "decay"), (dict(decay=float("inf")), "decay"),
                     (dict(loss="softmax"), "loss"), (dict(loss="warp"), "loss"), (dict(seed=-1), "seed"),
                     (dict(timestamps=np.zeros(n_in + 1)), "timestamps"), (dict(timestamps=np.zeros((n_in, 1))), "timestamps"),
                     (dict(timestamps=np.full(n_in, np.nan)), "timestamps")):
        with pytest.raises(ValueError, match=word):
            m.fit_sequence(**kw)
    with pytest.raises(AssertionError, match="reached the device"):  # valid arguments do go on to the device
        m.fit_sequence(epochs=1, timestamps=np.arange(n_in))
    for bad in (np.zeros(n_in + 1), np.zeros((n_in, 1)), np.full(n_in, np.inf)):
        with pytest.raises(ValueError, match="timestamps"):
            m.set_sequence_order(bad)
    with pytest.raises(ValueError, match="linear"):
        others[0].set_sequence_order()
    with pytest.raises(AssertionError, match="reached the device"):
        m.set_sequence_order(np.arange(n_in))
    # a model without C
    for call in calls[1:]:
        with pytest.raises(RuntimeError, match=r"call fit_sequence\(\) first"):
            call(m)
    with pytest.raises(ValueError, match="top_k"):
        m.recommend_next([0], top_k=129)
    with pytest.raises(ValueError, match="top_k"):
        m.recommend_for_sequences([[1]], top_k=129)
    with pytest.raises(ValueError, match="k must"):
        m.evaluate_next(k=0)
    with pytest.raises(ValueError, match="n_factors"):
        too_wide.recommend_next([0])
    # with C (as a loaded state_dict leaves it): ids are checked on the host, other slot weights are refused
    m.net.seq_context = torch.zeros((30, 8))
    m.net.seq_weights = torch.from_numpy(ref.weights(4, 0.7))
    with pytest.raises(IndexError):
        m.recommend_next([40])
    with pytest.raises(IndexError):
        m.recommend_for_sequences([[1, 30]])
    with pytest.raises(RuntimeError, match="holdout_last"):
        m.evaluate_next()
    for kw in (dict(context=3), dict(decay=0.5)):
        with pytest.raises(ValueError, match="slot weights"):
            m.fit_sequence(**kw)
    with pytest.raises(AssertionError, match="reached the device"):
        m.fit_sequence(context=4, decay=0.7)
    assert m.recommend_next([]).shape == (0, 10) and m.recommend_for_sequences([], top_k=3).shape == (0, 3)


def test_state_dict_carries_the_sequence_buffers_only_once_fitted():
    m = _model()
    assert not [k for k in m.net.state_dict() if k.startswith("seq_")]
    m.net.seq_context = torch.full((30, 8), 0.5)
    m.net.seq_weights = torch.from_numpy(ref.weights(3, 0.7))
    sd = m.net.state_dict()
    assert {"seq_context", "seq_weights"} <= set(sd)
    fresh = _model()
    fresh.net.load_state_dict(sd)
    assert torch.equal(fresh.net.seq_context.cpu(), m.net.seq_context.cpu())
    assert torch.equal(fresh.net.seq_weights.cpu(), m.net.seq_weights.cpu())
    bad = dict(sd, seq_context=torch.zeros((29, 8)))
    with pytest.raises(RuntimeError, match="size mismatch"):
        _model().net.load_state_dict(bad)


# ------------------------------------------------------------------------------------------------ the restatement
def test_weights_are_normalised_whatever_is_present():
    w = ref.weights(4, 0.7)
    assert w.dtype == np.float32 and abs(float(w.astype(np.float64).sum()) - 1) < 1e-6 and np.all(w[1:] < w[:-1])
    assert np.allclose(w[1:] / w[:-1], 0.7, rtol=1e-6) and ref.weights(0, 0.7).size == 0
    from torchrecsys_amd import ops
    for L, d in ((1, 0.7), (4, 0.7), (16, 0.3), (8, 1.0)):
        assert np.array_equal(ops.seq_weights(L, d).numpy(), ref.weights(L, d))


def test_restatement_gradients_are_the_derivatives_of_its_loss():
    """Central differences of the float64 batch loss against the staged rows, summed per table row (a row referenced by
    several triples, or as positive and context at once, collects every reference)."""
    off, ids = ref.make_sequences(12, 9, (1, 2, 5, 7), seed=2)
    T = {k: v.astype(np.float64) for k, v in ref.make_tables(12, 9, 5, seed=4).items()}
    rs = np.random.RandomState(6)
    entry = rs.randint(0, int(off[-1]), 20)
    user = (np.searchsorted(off, entry, side="right") - 1)
    neg = rs.randint(0, 9, 20)
    w = ref.weights(3, 0.7)
    for loss in ("bpr", "hinge"):
        gr, gl, cid, _, _ = ref.staged(T, off, ids, user, entry, neg, w, loss)
        pos = ids[entry]
        G = {k: np.zeros_like(v) for k, v in T.items()}
        np.add.at(G["U"], user, gr[0])
        np.add.at(G["V"], pos, gr[1])
        np.add.at(G["V"], neg, gr[2])
        np.add.at(G["b"], pos, gl[1])
        np.add.at(G["b"], neg, gl[2])
        for l in range(3):
            np.add.at(G["C"], cid[l], gr[3 + l])
        assert not gl[0].any()
        mean = lambda: ref.staged(T, off, ids, user, entry, neg, w, loss)[3] / 20
        for name, idx in (("U", (int(user[0]), 2)), ("V", (int(pos[1]), 0)), ("V", (int(neg[2]), 4)),
                          ("b", (int(pos[3]),)), ("C", (int(cid[0][np.argmax(entry - off[user])]), 1))):
            keep, h = T[name][idx], 1e-6
            T[name][idx] = keep + h
            up = mean()
            T[name][idx] = keep - h
            dn = mean()
            T[name][idx] = keep
            assert abs((up - dn) / (2 * h) - G[name][idx]) < 1e-7, (loss, name, idx)


def test_fast_step_is_the_step_and_the_planted_order_is_learned_by_the_restatement():
    off, ids = ref.make_sequences(12, 9, (1, 2, 5, 7), seed=2)
    rs = np.random.RandomState(8)
    entry = rs.randint(0, int(off[-1]), 33)
    user = np.searchsorted(off, entry, side="right") - 1
    neg = rs.randint(0, 9, 33)
    w = ref.weights(3, 0.7)
    for loss in ("bpr", "hinge"):
        A = {k: v.astype(np.float64) for k, v in ref.make_tables(12, 9, 5, seed=4).items()}
        Bt = {k: v.copy() for k, v in A.items()}
        ref.step(A, off, ids, user, entry, neg, w, loss, 0.5)
        ref.fast_step(Bt, off, ids, user, entry, neg, w, loss, 0.5)
        for k in A:
            assert np.allclose(A[k], Bt[k], rtol=0, atol=1e-13), (loss, k)


def test_the_restatement_learns_the_planted_order_and_meets_both_bars():
    """The two bars of tests/test_gpu_seq.py::test_learns_order are conditions the float64 restatement alone satisfies:
    three seeds reach the recorded hit_rate@10 (0.840, 0.837, 0.827 with context; 0.100, 0.097, 0.070 without), every
    one at least 0.8 x the lowest of the three and at least twice its own context-free value."""
    got = [ref.planted_fit(seed) for seed in (0, 1, 2)]
    for (hit, plain), want, want_plain in zip(got, ref.PLANTED_REF_HIT, ref.PLANTED_REF_HIT_NO_CONTEXT):
        assert abs(hit - want) < 6e-4 and abs(plain - want_plain) < 6e-4, got
        assert hit >= 0.8 * min(ref.PLANTED_REF_HIT) and hit >= 2 * plain, got
