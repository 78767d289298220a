# -*- coding: utf-8 -*-
"""fold_in_items() / recommend_with_new_items() without a GPU: trs_fold_in_items is declared, exported and bound; its
arguments and the public methods' arguments are validated on the host before any device work; the history CSR and the
extended seen CSR are built correctly; the numpy restatement (tests/foldin_items_ref.py) takes the SGD step of the
stated loss (torch autograd) and has the properties the GPU tests rely on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import foldin_items_ref as ref
import foldin_ref as base
from torchrecsys_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "trs_fold_in_items"
PROTO = _lib.PROTOTYPES[NAME]  # this module is about that entry point: without its binding nothing here applies


def _err():
    return _lib.load().trs_last_error().decode()


def test_symbol_declared_exported_and_bound():
    lib = _lib.load()
    assert lib.trs_abi_version() == _lib.ABI_VERSION == 6  # added without touching a signature: no bump
    header = open(os.path.join(ROOT, "include", "trs.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint %s\s*\(" % NAME, header)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert len(PROTO[1]) == 26
    decl = header[header.index("int " + NAME):]
    assert decl[:decl.index(")")].count(",") == 25


def test_entry_point_rejects_bad_arguments_before_any_launch():
    lib = _lib.load()
    P = 0x1000  # never dereferenced
    fb, nb = lib.trs_item_fold_bytes(300, 24), lib.trs_item_fold_bytes(5, 24)
    hist = _lib.TrsCsr()
    hist.off, hist.items, hist.n_rows = P, P, 5
    empty = _lib.TrsCsr()
    empty.off, empty.items, empty.n_rows = P, P, 0
    seen = _lib.TrsCsr()
    seen.off, seen.items, seen.n_rows = P, P, 100
    inf, nan = float("inf"), float("nan")

    def tables(user=P, user_lin=P, n_users=100, D=24):
        T = _lib.TrsTables()
        T.user, T.user_lin, T.n_users, T.D = user, user_lin, n_users, D
        return T

    def call(net=0, T=tables(), fold=P, fold_bytes=fb, n_items=300, new=P, new_bytes=nb, h=hist, su=P, si=P, N=1000,
             sn=seen, loss=0, epochs=4, lr=0.05, l2=0.0, nu=1, seed=1, shuffle=1, reject=1, tries=8, V=P, b=P, ls=None,
             err=None):
        ref_ = ctypes.byref
        return lib.trs_fold_in_items(net, ref_(T) if T is not None else None, fold, fold_bytes, n_items, new, new_bytes,
                                     ref_(h) if h is not None else None, su, si, N, ref_(sn) if sn is not None else None,
                                     loss, epochs, lr, l2, nu, seed, shuffle, reject, tries, V, b, ls, err, None)
    for kw, word in ((dict(net=2), "net"), (dict(net=-1), "net"), (dict(T=None), "tables"),
                     (dict(T=tables(user=None)), "user table"), (dict(T=tables(user_lin=None)), "user table"),
                     (dict(T=tables(n_users=0)), "n_users"), (dict(T=tables(n_users=1 << 31)), "n_users"),
                     (dict(T=tables(D=0)), "D=0"), (dict(T=tables(D=_lib.RETRIEVE_DMAX + 1), fold_bytes=1 << 30), "D="),
                     (dict(fold=None), "fold buffer"), (dict(fold_bytes=fb - 4), "fold buffer too small"),
                     (dict(new=None), "new-item fold"), (dict(new_bytes=nb - 4), "new-item fold buffer too small"),
                     (dict(n_items=1), "n_items"), (dict(n_items=0), "n_items"), (dict(epochs=0), "epochs"),
                     (dict(epochs=1025), "epochs"), (dict(lr=0.0), "lr"), (dict(lr=-1.0), "lr"), (dict(lr=inf), "lr"),
                     (dict(lr=nan), "lr"), (dict(l2=-0.5), "l2"), (dict(l2=inf), "l2"), (dict(l2=nan), "l2"),
                     (dict(loss=2), "loss"), (dict(loss=3), "loss"), (dict(loss=-1), "loss"),
                     (dict(tries=-1), "max_tries"), (dict(tries=65), "max_tries"),
                     (dict(reject=1, tries=0), "reject_seen"), (dict(nu=-1), "negative_visits"),
                     (dict(nu=9), "negative_visits"), (dict(nu=1, N=0), "negative_visits"),
                     (dict(nu=2, su=None), "negative_visits"), (dict(nu=2, si=None), "negative_visits"),
                     (dict(N=-1), "n_stream"), (dict(h=None), "NULL"), (dict(V=None), "NULL"), (dict(b=None), "NULL")):
        assert call(**kw) == -1, kw
        assert _err().startswith(NAME + ":") and word in _err(), (kw, _err())
    for arr in ("off", "items"):
        for which in ("h", "sn"):
            bad = _lib.TrsCsr()
            bad.off, bad.items, bad.n_rows = P, P, 5
            setattr(bad, arr, None)
            assert call(**{which: bad}) == -1 and "NULL" in _err()
    # nothing to do, nothing launched: no new item (outputs and the new-item fold may then be NULL); bad arguments are
    # still bad.  Without negative visits no stream is needed, and the seen CSR is optional.
    assert call(h=empty) == 0
    assert call(h=empty, V=None, b=None, new=None, new_bytes=0) == 0
    assert call(h=empty, nu=0, su=None, si=None, N=0, sn=None) == 0
    assert call(h=empty, reject=0, tries=0) == 0
    assert call(h=empty, epochs=0) == -1 and "epochs" in _err()
    assert call(h=empty, nu=9) == -1 and "negative_visits" in _err()
    with _lib.tuning(FOLDIN_DEPTH=3):
        assert call() == -1 and "FOLDIN_DEPTH" in _err()


def test_the_three_key_schedules_never_meet():
    """key_e (seed + KEY_STEP), the sampler's tries (seed + k TRY_STEP) and the stream draws (seed + (1 + t) KEY_STEP +
    k TRY_STEP, t = 1..8) are distinct keys for every t and every try k < 64."""
    mask = ref.MASK64
    sampler = {(k * ref.TRY_STEP) & mask for k in range(64)}
    stream = [((1 + t) * ref.KEY_STEP + k * ref.TRY_STEP) & mask for t in range(1, 9) for k in range(64)]
    assert len(set(stream)) == len(stream)
    assert not sampler & set(stream) and ref.KEY_STEP & mask not in set(stream) | sampler


# ------------------------------------------------------------------------------------------------ public methods
N_USERS, N_ITEMS = 40, 30


def _model(net_type, M=0, n_factors=8, **kw):
    return ref.make_model(net_type, N_USERS, N_ITEMS, n_factors, M, seed=1, n_rows=400, scale=0.3, **kw)


def test_argument_errors_come_before_any_device_work(monkeypatch):
    from torchrecsys_amd import model as model_mod

    def no_device(*a, **kw):
        raise AssertionError("reached the device before validating the arguments")
    # the models first: where a GPU is present, building one moves its tables there
    m, mm, mlp, wide = _model("fm"), _model("linear", M=2), _model("mlp"), _model("linear", n_factors=257)
    monkeypatch.setattr(model_mod, "_device", no_device)
    with pytest.raises(ValueError, match="mlp"):
        mlp.fold_in_items([[0]])
    with pytest.raises(ValueError, match="mlp"):
        mlp.recommend_with_new_items([0], [100], np.zeros((1, 8)), np.zeros(1))
    with pytest.raises(ValueError, match="n_factors"):
        wide.fold_in_items([[0]])
    with pytest.raises(ValueError, match="n_factors"):
        wide.recommend_with_new_items([0], [100], np.zeros((1, 257)), np.zeros(1))
    f = m.fold_in_items
    for bad in (dict(epochs=0), dict(epochs=1025), dict(epochs=2.5), dict(lr=0), dict(lr=-1.0), dict(lr=float("inf")),
                dict(lr=float("nan")), dict(lr="fast"), dict(l2=-1e-3), dict(l2=float("nan")), dict(loss="warp"),
                dict(loss=None), dict(max_tries=-1), dict(max_tries=65), dict(max_tries=1.5),
                dict(reject_seen=True, max_tries=0), dict(seed=1.5), dict(negative_visits=-1), dict(negative_visits=9),
                dict(negative_visits=1.0), dict(negative_visits=True)):
        with pytest.raises(ValueError, match=list(bad)[0] if "reject_seen" not in bad else "reject_seen"):
            f([[0, 1]], **bad)
    with pytest.raises(IndexError, match="1000"):
        f([[0, 1], [2, 1000]])
    with pytest.raises(IndexError, match="-1"):
        f([[-1]])
    # metadata: required exactly when the model uses it, (n, M) integers inside their tables
    with pytest.raises(ValueError, match="no metadata"):
        f([[0]], metadata=[[1]])
    with pytest.raises(ValueError, match="required"):
        mm.fold_in_items([[0]])
    for bad in ([[1]], [[1, 2], [3, 4]], [[0.5, 1.0]], [1, 2]):
        with pytest.raises(ValueError, match="metadata must be"):
            mm.fold_in_items([[0]], metadata=bad)
    with pytest.raises(IndexError, match="metadata id 5 of column 1"):
        mm.fold_in_items([[0], [1]], metadata=[[0, 4], [4, 5]])
    with pytest.raises(IndexError, match="metadata id -1 of column 0"):
        mm.fold_in_items([[0]], metadata=[[-1, 0]])
    with pytest.raises(AssertionError, match="reached the device"):  # valid arguments get as far as the device
        f([[0, 1], [], [5, 5, 3]])
    with pytest.raises(AssertionError, match="reached the device"):
        mm.fold_in_items([np.array([0, 1]), (2,)], metadata=np.array([[0, 4], [4, 0]]), reject_seen=False, max_tries=0,
                         loss="bpr", l2=0.25, seed=-3, shuffle=False, negative_visits=0)
    # empty calls need no device
    V, b = m.fold_in_items([])
    assert V.shape == (0, 8) and b.shape == (0,) and V.dtype == b.dtype == torch.float32
    V, b, ls = m.fold_in_items([], epochs=3, return_loss=True)
    assert ls.shape == (3, 0) and ls.dtype == torch.float32
    V, b = mm.fold_in_items([], metadata=np.zeros((0, 2), dtype=np.int64))
    assert V.shape == (0, 8)

    r = m.recommend_with_new_items
    V1, b1 = np.zeros((2, 8), dtype=np.float32), np.zeros(2, dtype=np.float32)
    with pytest.raises(ValueError, match="top_k"):
        r([0], [100, 101], V1, b1, top_k=_lib.RETRIEVE_KMAX + 1)
    with pytest.raises(ValueError, match="distinct"):
        r([0], [100, 100], V1, b1)
    with pytest.raises(ValueError, match="item id 29 is an item of the model"):
        r([0], [100, 29], V1, b1)
    with pytest.raises(ValueError, match="V must be"):
        r([0], [100, 101], V1[:1], b1)
    with pytest.raises(ValueError, match="V must be"):
        r([0], [100, 101], V1, b1[:1])
    with pytest.raises(ValueError, match="V must be"):
        r([0], [100, 101], np.zeros((2, 7)), b1)
    with pytest.raises(ValueError, match="histories for 2 new items"):
        r([0], [100, 101], V1, b1, histories=[[0]])
    with pytest.raises(IndexError, match="77"):
        r([0], [100, 101], V1, b1, histories=[[0], [77]])
    with pytest.raises(IndexError, match="40"):
        r([40], [100, 101], V1, b1)
    with pytest.raises(ValueError, match="no metadata"):
        r([0], [100, 101], V1, b1, metadata=[[0], [1]])
    with pytest.raises(ValueError, match="required"):
        mm.recommend_with_new_items([0], [100, 101], V1, b1)
    with pytest.raises(IndexError, match="metadata id 9"):
        mm.recommend_with_new_items([0], [100, 101], V1, b1, metadata=[[0, 0], [9, 0]])
    with pytest.raises(AssertionError, match="reached the device"):
        r([0, 3], [100, 101], V1, b1, histories=[[0], [1, 2]])
    with pytest.raises(AssertionError, match="reached the device"):
        r([0, 3], [], np.zeros((0, 8)), np.zeros(0))
    ids, sc = r([], [100, 101], V1, b1, top_k=4, return_scores=True)
    assert ids.shape == (0, 4) and sc.shape == (0, 4) and ids.dtype == torch.int64
    assert r([1, 2], [100, 101], V1, b1, top_k=0).shape == (2, 0)


def test_remapped_item_ids_of_the_model_are_not_new():
    from torchrecsys_amd.model import TorchRecSys
    import contextlib
    import io
    rs = np.random.RandomState(1)
    uu, ii = rs.randint(0, 20, 200), rs.randint(0, 10, 200)
    with contextlib.redirect_stdout(io.StringIO()):
        m = TorchRecSys.from_tensors(torch.from_numpy(uu * 7 + 3), torch.from_numpy(ii * 5 + 11), n_factors=8,
                                     net_type="linear", remap_ids=True)
    V, b = np.zeros((1, 8), dtype=np.float32), np.zeros(1, dtype=np.float32)
    known = int(m.data_processor.item_index[2])
    with pytest.raises(ValueError, match="item id %d is an item of the model" % known):
        m.recommend_with_new_items([3], [known], V, b)
    with pytest.raises(IndexError, match="4"):  # 4 is not one of the original user ids 7 k + 3
        m.fold_in_items([[3, 4]])
    off, users, rank = m._history_csr([[10, 3, 10]], side="user")
    assert users.tolist() == [0, 1]  # dense rows of the original ids 3 and 10


def test_user_history_csr_is_sorted_distinct_and_longest_first():
    m = _model("linear")
    hs = [[5, 3, 5, 9], [], [7], [2, 1, 0, 1, 39, 4], [4, 4]]  # user 39 exists, item 39 does not
    off, users, rank = m._history_csr(hs, side="user")
    assert off.dtype == np.int64 and users.dtype == np.int32 and off[0] == 0 and off[-1] == users.size
    lens = np.diff(off)
    assert np.all(lens[:-1] >= lens[1:])  # longest first
    for r, h in enumerate(base.clean(hs)):
        assert np.array_equal(users[off[rank[r]]:off[rank[r] + 1]], h)
    assert sorted(rank.tolist()) == list(range(5))
    with pytest.raises(IndexError, match="39"):
        m._history_csr(hs)  # the item side is unchanged: 39 is outside the catalogue


def test_extended_seen_csr_appends_the_new_rows_in_order():
    from torchrecsys_amd.model import TorchRecSys
    rs = np.random.RandomState(3)
    n_users, n_items = 12, 9
    su, si = rs.randint(0, n_users, 40), rs.randint(0, n_items, 40)
    su[su == 7] = 6  # user 7 has seen nothing
    off, items = ref.seen_csr(su, si, n_users)
    hists = [np.array([0, 7, 11]), np.zeros(0, dtype=np.int64), np.array([7]), np.array([3, 0, 5, 11])]
    hoff = np.concatenate([[0], np.cumsum([h.size for h in hists])])
    eo, ei = TorchRecSys._extended_seen_csr(off, items, hoff, np.concatenate(hists), n_items)
    assert eo.dtype == np.int64 and ei.dtype == np.int32 and eo.size == n_users + 1 and eo[-1] == ei.size
    for u in range(n_users):
        want = sorted(set(si[su == u].tolist()) | {n_items + j for j, h in enumerate(hists) if u in h})
        assert ei[eo[u]:eo[u + 1]].tolist() == want, u
    assert ei[eo[7]:eo[8]].tolist() == [n_items, n_items + 2]
    eo2, ei2 = TorchRecSys._extended_seen_csr(off, items, np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.int64), n_items)
    assert np.array_equal(eo2, off) and np.array_equal(ei2, items)


# ------------------------------------------------------------------------------------------------ the reference
def _autograd_case(net, M, loss, rs):
    D, n_users, n_items, lr, l2 = 5, 7, 6, 0.05, 0.125
    U, a = 0.5 * rs.randn(n_users, D), 0.5 * rs.randn(n_users)
    I, il = 0.5 * rs.randn(n_items, D), 0.5 * rs.randn(n_items)
    metas, mlins = [0.5 * rs.randn(4, D) for _ in range(M)], [0.5 * rs.randn(4) for _ in range(M)]
    tab = rs.randint(0, 4, (n_items, M))
    new_meta = rs.randint(0, 4, M)
    su, si = rs.randint(0, n_users, 20), rs.randint(0, n_items, 20)

    def logit(user, row, lin, meta_ids):
        """The scorer's own statement: Linear <U_u, item + sum meta> + biases; FM: linear terms + every pair of the
        features {user, item, meta_0, ..}."""
        feats = [torch.as_tensor(U[user]), row] + [torch.as_tensor(metas[j][meta_ids[j]]) for j in range(M)]
        if net == "linear":
            return (feats[0] * sum(feats[1:])).sum() + a[user] + lin
        z = a[user] + lin + sum(mlins[j][meta_ids[j]] for j in range(M))
        for i in range(len(feats)):
            for j in range(i + 1, len(feats)):
                z = z + (feats[i] * feats[j]).sum()
        return z

    def pair(pos, neg):
        sp, sn = (torch.sigmoid(pos), torch.sigmoid(neg)) if net == "fm" else (pos, neg)
        return torch.clamp(sn - sp + 1, min=0) if loss == "hinge" else torch.nn.functional.softplus(sn - sp)

    # the folded form the rule is stated on
    S = I + sum(metas[j][tab[:, j]] for j in range(M)) if M else I.copy()
    T = sum(metas[j][new_meta[j]] for j in range(M)) if M else np.zeros(D)
    if net == "linear":
        c, kappa = il.copy(), 0.0
    else:
        c = il + sum(mlins[j][tab[:, j]] for j in range(M)) + 0.5 * (
            (S * S).sum(1) - (I * I).sum(1) - sum((metas[j][tab[:, j]] ** 2).sum(1) for j in range(M)))
        kappa = sum(mlins[j][new_meta[j]] for j in range(M)) + 0.5 * (
            (T * T).sum() - sum((metas[j][new_meta[j]] ** 2).sum() for j in range(M)))
    hist = np.array([3])
    kw = dict(nu=1, seed=4, shuffle=False, reject_seen=True, max_tries=8)
    got = ref.fold_in(U, a, S, c, T[None, :], np.array([kappa]), [hist], su, si, ref.seen_csr(su, si, n_users), net,
                      loss, 1, lr, l2, **kw)
    users, others, positive = ref.schedule(hist, n_items, su, si, ref.seen_csr(su, si, n_users), 1, 1, 4, False, True, 8)[0]
    assert positive.tolist() == [True, False] and users[0] == 3 and users[1] not in hist
    v = torch.zeros(D, dtype=torch.float64, requires_grad=True)
    beta = torch.zeros((), dtype=torch.float64, requires_grad=True)
    total = 0.0
    for u, o, is_pos in zip(users, others, positive):
        znew = logit(u, v, beta, new_meta)
        zold = logit(u, torch.as_tensor(I[o]), il[o], tab[o])
        L = pair(znew, zold) if is_pos else pair(zold, znew)
        assert float(L.detach()) > 0  # an active visit: the hinge passes a gradient
        gv, gb = torch.autograd.grad(L, (v, beta))
        with torch.no_grad():
            v -= lr * (gv + l2 * v)
            beta -= lr * (gb + l2 * beta)
        total += float(L.detach())
    assert np.abs(got["V"][0] - v.detach().numpy()).max() < 1e-13, (net, M, loss)
    assert abs(got["b"][0] - float(beta.detach())) < 1e-13 and abs(got["loss"][0, 0] - total / 2) < 1e-13
    assert np.abs(got["V"][0]).max() > 1e-3 and got["b"][0] != 0  # both visits moved the state


@pytest.mark.parametrize("M", [0, 2])
@pytest.mark.parametrize("net", ["linear", "fm"])
def test_the_reference_takes_the_sgd_step_of_the_stated_loss(net, M):
    rs = np.random.RandomState(10 + M)
    for loss in ("hinge", "bpr"):
        _autograd_case(net, M, loss, rs)


def _small():
    rs = np.random.RandomState(2)
    n_users, n_items, D = 50, 20, 16
    U, a = rs.randint(-3, 4, (n_users, D)).astype(np.float64), rs.randint(-3, 4, n_users).astype(np.float64)
    S, c = rs.randint(-3, 4, (n_items, D)).astype(np.float64), rs.randint(-3, 4, n_items).astype(np.float64)
    su, si = rs.randint(0, n_users, 300), rs.randint(0, n_items, 300)
    lens = [0, 1, 2, 7, 33, 48, 49, 50]
    hs = [np.sort(rs.choice(n_users, size=n, replace=False)).astype(np.int64) for n in lens]
    T, kappa = rs.randint(-2, 3, (len(hs), D)).astype(np.float64), rs.randint(-2, 3, len(hs)).astype(np.float64)
    return U, a, S, c, T, kappa, hs, su, si, ref.seen_csr(su, si, n_users)


def test_schedule_visits_every_user_once_and_rejects_what_it_should():
    U, a, S, c, T, kappa, hs, su, si, seen = _small()
    n_items = S.shape[0]
    pairs = set(zip(su.tolist(), si.tolist()))
    for shuffle in (False, True):
        for h in hs:
            for nu in (0, 2):
                sched = ref.schedule(h, n_items, su, si, seen, 3, nu, 9, shuffle, True, 64)
                for users, others, positive in sched:
                    assert users.size == h.size * (1 + nu) and positive.reshape(-1, 1 + nu)[:, 0].all()
                    assert sorted(users[positive].tolist()) == h.tolist()  # every user of the history once per epoch
                    if not shuffle:
                        assert np.array_equal(users[positive], h)
                    assert np.all((others >= 0) & (others < n_items))
                    # t == 0: never an item the user has in train, where one is left (64 tries; every user here has
                    # seen at most 14 of the 20 items: a miss has probability (14/20)^64 < 2e-10 per draw)
                    assert not any((u, o) in pairs for u, o in zip(users[positive], others[positive]))
                    # t >= 1: a train interaction, never of a user of the history unless nearly all users are in it
                    assert all((u, o) in pairs for u, o in zip(users[~positive], others[~positive]))
                    if h.size <= 33:
                        assert not np.isin(users[~positive], h).any()
    # without rejection: the plain draws, whatever max_tries
    h = hs[4]
    a0 = ref.schedule(h, n_items, su, si, None, 2, 2, 9, True, False, 0)
    a8 = ref.schedule(h, n_items, su, si, seen, 2, 2, 9, True, False, 8)
    for x, y in zip(a0, a8):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
    # the whole user base in the history: the last candidate is kept, still a train row
    full = ref.schedule(hs[7], n_items, su, si, seen, 1, 1, 9, True, True, 8)[0]
    assert np.isin(full[0][~full[2]], hs[7]).all()


def test_an_item_folds_in_the_same_alone_or_among_others():
    U, a, S, c, T, kappa, hs, su, si, seen = _small()
    for net, loss in (("linear", "hinge"), ("fm", "bpr")):
        kw = dict(nu=2, seed=5, shuffle=True, reject_seen=True, max_tries=8)
        both = ref.fold_in(U, a, S, c, T, kappa, hs, su, si, seen, net, loss, 3, 2.0 ** -6, 0.0, **kw)
        rev = ref.fold_in(U, a, S, c, T[::-1], kappa[::-1], hs[::-1], su, si, seen, net, loss, 3, 2.0 ** -6, 0.0, **kw)
        for i, h in enumerate(hs):
            one = ref.fold_in(U, a, S, c, T[i:i + 1], kappa[i:i + 1], [h], su, si, seen, net, loss, 3, 2.0 ** -6, 0.0, **kw)
            assert np.array_equal(one["V"][0], both["V"][i]) and one["b"][0] == both["b"][i]
            assert np.array_equal(one["loss"][:, 0], both["loss"][:, i])
            j = len(hs) - 1 - i
            assert np.array_equal(rev["V"][j], both["V"][i]) and rev["b"][j] == both["b"][i]
        assert not both["V"][0].any() and both["b"][0] == 0 and not both["loss"][:, 0].any()  # the empty history
    lin = ref.fold_in(U, a, S, c, T, kappa, hs, su, si, seen, "linear", "hinge", 3, 2.0 ** -6, 0.0, nu=1, seed=5,
                      require_exact=True)
    assert lin["bound"] < 2.0 ** 24 and 0 < lin["active"] < lin["visits"] and 0 < lin["active_pos"] < lin["visits_pos"]
    # fp32 restatements in two summation orders stay close to float64 (the GPU test's tolerance is measured this way)
    rs = np.random.RandomState(3)
    f = np.float32
    U3, a3, S3, c3 = [(0.3 * rs.randn(*x.shape)).astype(f) for x in (U, a, S, c)]
    T3, k3 = (0.3 * rs.randn(*T.shape)).astype(f), (0.3 * rs.randn(*kappa.shape)).astype(f)
    want = ref.fold_in(U3, a3, S3, c3, T3, k3, hs, su, si, seen, "fm", "bpr", 3, 0.05, 0.125, nu=1, seed=1)
    for order in ("asc", "desc"):
        g = ref.fold_in(U3, a3, S3, c3, T3, k3, hs, su, si, seen, "fm", "bpr", 3, 0.05, 0.125, nu=1, seed=1, dtype=f,
                        order=order)
        assert g["V"].dtype == f and np.abs(g["V"] - want["V"]).max() < 1e-5
        assert np.abs(g["loss"] - want["loss"]).max() < 1e-5 and np.abs(g["b"] - want["b"]).max() < 1e-5


def _planted_ranks(V, b, U, S, users, k=10):
    """For each user: is the new item (score <U_u, v> + b) among the top k of the catalogue extended by it?"""
    z = np.concatenate([U[users] @ S.T, (U[users] @ V + b)[:, None]], axis=1)
    order = np.argsort(-z, axis=1, kind="stable")[:, :k]
    return (order == S.shape[0]).any(axis=1)


def test_planted_case_learns_the_planted_direction_and_negative_visits_hold_the_bias_down():
    U, S, hist, plus, minus = ref.planted()
    n_users, n_items = U.shape[0], S.shape[0]
    rs = np.random.RandomState(0)
    su, si = rs.randint(0, n_users, 3000), rs.randint(0, n_items, 3000)
    seen = ref.seen_csr(su, si, n_users)
    z = np.zeros
    out = {}
    for nu in (0, 1):
        out[nu] = ref.fold_in(U, z(n_users), S, z(n_items), z((1, U.shape[1])), z(1), [hist], su, si, seen, "linear",
                              "hinge", 8, 0.05, 0.0, nu=nu, seed=0)
        V, b = out[nu]["V"][0], out[nu]["b"][0]
        assert V[0] > 0 and _planted_ranks(V, b, U, S, plus).all() and not _planted_ranks(V, b, U, S, minus).any(), nu
    assert out[1]["b"][0] < out[0]["b"][0]
