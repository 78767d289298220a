# -*- coding: utf-8 -*-
"""LightGCN without a GPU: trs_lgcn_propagate / trs_lgcn_adam are declared, exported and bound and refuse bad arguments
on the host; fit_lightgcn validates before any device work; the shipped kernels use no scratch and stay within 128
VGPRs; the state_dict carries the buffers once fitted; and the numpy restatement (tests/lgcn_ref.py) agrees with the
paper's layer-mean definition and with itself."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import foldin_ref as base
import lgcn_ref as ref
from test_abi import _shipped_kernel_registers
from torchrecsys_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err():
    return _lib.load().trs_last_error().decode()


def test_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "trs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in (("trs_lgcn_propagate", 13), ("trs_lgcn_adam", 11)):
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        assert len(_lib.PROTOTYPES[name][1]) == n_args
        decl = code[code.index(name + "("):]
        assert decl[:decl.index(")")].count(",") == n_args - 1
        assert name in header[header.index("#define TRS_ABI_VERSION") - 1200:header.index("#define TRS_ABI_VERSION")]
    assert int(re.search(r"#define TRS_LGCN_SEG (\d+)", header).group(1)) == _lib.LGCN_SEG == ref.SEG == 512
    assert int(re.search(r"#define TRS_ABI_VERSION (\d+)", header).group(1)) == 6
    assert open(os.path.join(ROOT, "torchrecsys_amd", "csrc", "Makefile")).read().count("lgcn.hip") == 1


def test_entry_points_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    P = 0x1000  # never dereferenced
    Q = 0x2000

    def csr(off=P, items=P, n_rows=40):
        c = _lib.TrsCsr()
        c.off, c.items, c.n_rows = off, items, n_rows
        return c

    def prop(inp=P, n_in=30, D=16, nbr=csr(), dinv_out=P, dinv_in=P, add=P, scale=1.0, out=Q, n_out=40, accumulate=0):
        return lib.trs_lgcn_propagate(inp, n_in, D, ctypes.byref(nbr) if nbr is not None else None, dinv_out, dinv_in,
                                      add, scale, out, n_out, accumulate, None, None)

    for kw, word in ((dict(D=0), "D=0"), (dict(D=257), "D=257"), (dict(D=-4), "D=-4"),
                     (dict(scale=float("nan")), "scale"), (dict(scale=float("inf")), "scale"),
                     (dict(scale=-float("inf")), "scale"), (dict(accumulate=2), "accumulate"),
                     (dict(accumulate=-1), "accumulate"), (dict(n_out=-1, nbr=csr(n_rows=-1)), "negative"),
                     (dict(n_in=-1), "negative"), (dict(nbr=None), "CSR"), (dict(nbr=csr(n_rows=39)), "rows"),
                     (dict(nbr=csr(off=None)), "NULL"), (dict(nbr=csr(items=None)), "NULL"), (dict(inp=None), "NULL"),
                     (dict(dinv_out=None), "NULL"), (dict(dinv_in=None), "NULL"), (dict(out=None), "NULL"),
                     (dict(n_in=0), "n_in=0"), (dict(out=P), "aliases")):
        assert prop(**kw) == -1, kw
        assert _err().startswith("trs_lgcn_propagate:") and word in _err(), (kw, _err())
    # nothing to do, nothing launched (no array is needed then); bad arguments are still bad
    assert prop(n_out=0, nbr=csr(n_rows=0)) == 0
    assert prop(n_out=0, nbr=csr(off=None, items=None, n_rows=0), inp=None, dinv_out=None, dinv_in=None, out=None,
                add=None, n_in=0) == 0
    assert prop(n_out=0, nbr=csr(n_rows=0), D=300) == -1 and prop(n_out=0, nbr=csr(n_rows=1)) == -1

    def adam(p=P, g=P, m=P, v=P, n=64, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, t=1):
        return lib.trs_lgcn_adam(p, g, m, v, n, lr, b1, b2, eps, t, None)

    for kw, word in ((dict(n=-1), "negative"), (dict(t=0), "step_count"), (dict(lr=-1.0), "lr"),
                     (dict(lr=float("nan")), "lr"), (dict(b1=1.0), "betas"), (dict(b2=-0.1), "betas"),
                     (dict(eps=float("inf")), "eps"), (dict(p=None), "NULL"), (dict(g=None), "NULL"),
                     (dict(m=None), "NULL"), (dict(v=None), "NULL")):
        assert adam(**kw) == -1, kw
        assert _err().startswith("trs_lgcn_adam:") and word in _err(), (kw, _err())
    assert adam(n=0, p=None, g=None, m=None, v=None) == 0 and adam(n=0, t=0) == -1


def test_every_shipped_lgcn_kernel_is_free_of_scratch_and_within_128_registers(tmp_path):
    """Ten instances of lgcn_propagate_kernel (lane groups of 4 .. 64 lanes, 16-byte lanes and the scalar path) and two
    of lgcn_adam_kernel: none with scratch, every one within the 128 VGPRs of four waves per SIMD (DESIGN.md 4.19 lists
    the counts).  The 16-byte-lane instances of lane groups up to 32 lanes are the shapes D <= 128."""
    found = _shipped_kernel_registers(tmp_path)
    prop = {n: v for n, v in found.items() if re.search(r"\d+lgcn_propagate_kernelI", n)}
    adam = {n: v for n, v in found.items() if re.search(r"\d+lgcn_adam_kernelI", n)}
    assert len(prop) == 10 and len(adam) == 2, (sorted(prop), sorted(adam))
    for n, (vgpr, scratch) in {**prop, **adam}.items():
        assert scratch == 0 and vgpr <= 128, (n, vgpr, scratch)
    vec = [n for n in prop if re.search(r"ILi(4|8|16|32)ELb1E", n)]
    assert len(vec) == 4
    assert len({n for n in found if "lgcn" in n}) == 12


# ------------------------------------------------------------------------------------------------ public arguments
def _model(net_type="linear", M=0, n_factors=8, **kw):
    return base.make_model(net_type, 40, 30, n_factors, M, seed=1, scale=0.3, **kw)


def test_fit_lightgcn_refuses_before_any_device_work(monkeypatch):
    from torchrecsys_amd import model as model_mod

    def no_device(*a, **kw):
        raise AssertionError("reached the device before validating the arguments")
    # (the models first: where a GPU is present their construction moves the net to it)
    mlp, ease, with_meta, wide = _model("mlp"), _model("ease"), _model("linear", M=2), _model("fm", n_factors=260)
    one_item, m, fm = _model(), _model(), _model("fm")
    one_item.n_items = 1
    monkeypatch.setattr(model_mod, "_device", no_device)
    for other in (mlp, ease):
        with pytest.raises(ValueError, match="fit_lightgcn"):
            other.fit_lightgcn()
    with pytest.raises(ValueError, match="metadata"):
        with_meta.fit_lightgcn()
    with pytest.raises(ValueError, match="n_factors"):
        wide.fit_lightgcn()
    with pytest.raises(ValueError, match="n_items"):
        one_item.fit_lightgcn()
    monkeypatch.setattr(model_mod.tdist, "world_info", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="world"):
        m.fit_lightgcn()
    monkeypatch.undo()
    monkeypatch.setattr(model_mod, "_device", no_device)
    for kw, word in ((dict(epochs=0), "epochs"), (dict(epochs=1.5), "epochs"), (dict(epochs=True), "epochs"),
                     (dict(lr=0), "lr"), (dict(lr=-0.1), "lr"), (dict(lr=float("nan")), "lr"), (dict(lr="1"), "lr"),
                     (dict(lr=float("inf")), "lr"), (dict(batch_size=0), "batch_size"), (dict(layers=-1), "layers"),
                     (dict(layers=9), "layers"), (dict(layers=2.0), "layers"), (dict(optimizer="adagrad"), "optimizer"),
                     (dict(loss="softmax"), "loss"), (dict(loss="warp"), "loss"), (dict(l2=-1e-4), "l2"),
                     (dict(l2=float("nan")), "l2"), (dict(l2=None), "l2"), (dict(seed=-1), "seed"),
                     (dict(max_tries=0), "max_tries")):
        for model in (m, fm):
            with pytest.raises(ValueError, match=word):
                model.fit_lightgcn(**kw)
    for model in (m, fm):  # valid arguments do go on to the device
        with pytest.raises(AssertionError, match="reached the device"):
            model.fit_lightgcn(epochs=1, layers=0, l2=0, optimizer="sgd", loss="hinge")


def test_fit_lightgcn_refuses_when_the_device_has_too_little_free_memory(monkeypatch):
    """The count of table-pair-sized buffers the docstring states (4 with sgd, 6 with adam, one fewer once the base
    tables exist) times 4 * (n_users + n_items) * n_factors bytes: one byte less free raises, exactly that much goes on."""
    from torchrecsys_amd import model as model_mod
    from torchrecsys_amd.engine import LightGCNTrainer
    assert LightGCNTrainer.BUFFERS == {"sgd": 4, "adam": 6}
    pair = 4 * (40 + 30) * 8
    free = {}

    class Went(Exception):
        pass

    def went_on(*a, **kw):
        raise Went()
    monkeypatch.setattr(model_mod, "_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda dev=None: (free["bytes"], 1 << 40))
    for fitted in (False, True):
        m = _model()
        monkeypatch.setattr(m, "_als_csrs", went_on)  # the first thing after the check
        if fitted:
            m.net.lgcn_user_base, m.net.lgcn_item_base = torch.zeros((40, 8)), torch.zeros((30, 8))
            m.net.lgcn_layers = torch.tensor([3])
        for optimizer, count in (("sgd", 4), ("adam", 6)):
            need = (count - fitted) * pair
            free["bytes"] = need - 1
            with pytest.raises(RuntimeError, match=f"needs {count} buffers"):
                m.fit_lightgcn(optimizer=optimizer)
            free["bytes"] = need
            with pytest.raises(Went):
                m.fit_lightgcn(optimizer=optimizer)


def test_state_dict_carries_the_lgcn_buffers_only_once_fitted():
    for kind in ("linear", "fm"):
        m = _model(kind)
        assert not [k for k in m.net.state_dict() if k.startswith("lgcn_")]
        m.net.lgcn_user_base = torch.full((40, 8), 0.5)
        m.net.lgcn_item_base = torch.full((30, 8), 0.25)
        m.net.lgcn_layers = torch.tensor([3])
        sd = m.net.state_dict()
        assert {"lgcn_user_base", "lgcn_item_base", "lgcn_layers"} <= set(sd)
        fresh = _model(kind)
        fresh.net.load_state_dict(sd)
        for k in ("lgcn_user_base", "lgcn_item_base", "lgcn_layers"):
            assert torch.equal(getattr(fresh.net, k).cpu(), getattr(m.net, k).cpu())
        bad = dict(sd, lgcn_item_base=torch.zeros((29, 8)))
        with pytest.raises(RuntimeError, match="size mismatch"):
            _model(kind).net.load_state_dict(bad)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("layers", [0, 1, 2, 3, 8])
def test_horner_forward_is_the_layer_mean_definition(layers):
    graph = ref.make_graph(37, 29, 260, seed=layers)
    rs = np.random.RandomState(layers + 1)
    U, V = rs.standard_normal((37, 6)), rs.standard_normal((29, 6))
    fu, fv = ref.horner(U, V, graph, layers, 1.0 / (layers + 1), dtype=np.float64)
    wu, wv = ref.layer_mean(U, V, graph, layers)
    assert np.abs(fu - wu).max() < 1e-12 and np.abs(fv - wv).max() < 1e-12


def test_float32_loop_follows_the_segment_rule_and_float64():
    """A list longer than a segment is NOT one straight float32 sum, and both are the float64 sum to rounding."""
    rs = np.random.RandomState(2)
    n_in, D = 1400, 5
    inp, w = rs.standard_normal((n_in, D)).astype(np.float32), rs.uniform(0.1, 1, n_in).astype(np.float32)
    lens = np.array([0, 3, 512, 513, 1300])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate([rs.permutation(n_in)[:n] for n in lens]).astype(np.int32)
    s32, s64 = ref.neighbour_sums(inp, off, ids, w), ref.neighbour_sums(inp, off, ids, w, dtype=np.float64)
    assert s32.dtype == np.float32 and not s32[0].any() and np.abs(s32 - s64).max() < 1e-3
    for r in range(len(lens)):
        straight = np.zeros(D, np.float32)
        for c in ids[off[r]:off[r + 1]]:
            straight = straight + w[c] * inp[c]
        same = np.array_equal(straight, s32[r])
        assert same if lens[r] <= ref.SEG else np.abs(straight - s32[r]).max() < 1e-3
    # an id outside the table is skipped and keeps its place
    bad = ids.copy()
    bad[off[2] + 7] = n_in
    keep = np.delete(ids, off[2] + 7)
    off2 = off.copy()
    off2[3:] -= 1
    assert np.array_equal(ref.neighbour_sums(inp, off, bad, w)[2], ref.neighbour_sums(inp, off2, keep, w)[2])


def test_restatement_step_is_the_autograd_step_in_float64():
    """The Horner step with the hand-written backward equals torch autograd on the dense layer-mean form."""
    graph = ref.make_graph(31, 23, 200, seed=3)
    rs = np.random.RandomState(4)
    U0, V0 = 0.3 * rs.standard_normal((31, 6)), 0.3 * rs.standard_normal((23, 6))
    user, pos, neg = rs.randint(0, 31, 20), rs.randint(0, 23, 20), rs.randint(0, 23, 20)
    for optimizer, lr in (("sgd", 0.5), ("adam", 1e-2)):
        for loss in ("bpr", "hinge"):
            for layers in (0, 2):
                wu, wv, wl = ref.autograd_step(U0, V0, graph, layers, user, pos, neg, loss, lr, 0.05, optimizer)
                ru, rv, rl, _ = ref.step(U0, V0, graph, layers, user, pos, neg, loss, lr, 0.05, optimizer,
                                         dtype=np.float64)
                # (alpha and the step scale are the contract's float32 values in both; Adam divides by sqrt(v) + 1e-8)
                tol = 1e-9 if optimizer == "sgd" else 1e-6
                assert np.abs(ru - wu).max() < tol and np.abs(rv - wv).max() < tol and abs(rl - wl) < 1e-9, \
                    (optimizer, loss, layers, np.abs(ru - wu).max())
                assert np.abs(wu - U0).max() > 1e-4
