# -*- coding: utf-8 -*-
"""The two table-indexing kernels of the sequence model (trs_seq_fwd_bwd, trs_seq_user_rows) at row offsets beyond 32
bits, after the pattern of tests/test_gpu_large_offsets.py: ids from large_tables.band_rows (every band, both sides of
every boundary, row 0 and the last row), the table under test filled with device-generated values everywhere, the
float64 restatement (tests/seq_ref.py) on the COMPACTED rows, and test_gpu_seq's own criteria.  Neither kernel writes
a table.  Two sides: the user table large (U: one table of 8.6 GB), and the item side large (V and C are indexed by
the same ids: two tables).  A handful of triples (24 rows name the 16 band rows)."""
import numpy as np
import pytest
import torch

import large_tables as lt
import seq_ref as ref
import test_gpu_seq as SQ

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = 3


def _ops():
    from torchrecsys_amd import ops
    return ops


def _case(side, D, seed):
    """Large tables of one side, the small ones of the other, sequences over the 16 band rows, and the compacted
    float32 tables of the restatement."""
    N = lt.n_rows_for(D)
    rows = lt.band_rows(N, D, 2, seed=seed)
    n = rows.size
    off_s, ids_s = ref.make_sequences(n, n, (1, 2, 5, 7), seed=seed + 1)  # small ids: positions in `rows`
    ids_s[:n] = np.arange(n)  # every band row occurs as an item
    small = ref.make_tables(n, n, D, seed=seed + 2)
    n_users, n_items = (N, n) if side == "user" else (n, N)
    tabs = {}
    for name, large in (("U", side == "user"), ("V", side == "item"), ("C", side == "item")):
        if large:
            tabs[name] = lt.fill(torch.empty((N, D), device=DEV), seed=seed + len(tabs))
            small[name] = lt.gather_small(tabs[name], rows)
        else:
            tabs[name] = torch.from_numpy(small[name]).to(DEV)
    b = torch.zeros((n_items, 1), device=DEV)
    place = torch.as_tensor(rows, device=DEV) if side == "item" else torch.arange(n, device=DEV)
    b[place, 0] = torch.from_numpy(small["b"]).to(DEV)
    # the CSR over the real ids: users at `rows` (user side) or 0..n-1; items mapped through `rows` on the item side
    lens = torch.zeros(n_users, dtype=torch.int64, device=DEV)
    lens[torch.as_tensor(rows, device=DEV) if side == "user" else torch.arange(n, device=DEV)] = \
        torch.from_numpy(np.diff(off_s)).to(DEV)
    off = torch.zeros(n_users + 1, dtype=torch.int64, device=DEV)
    off[1:] = torch.cumsum(lens, 0)
    ids_real = rows[ids_s] if side == "item" else ids_s
    T, keep = _ops().make_tables(tabs["U"], tabs["V"], torch.zeros((n_users, 1), device=DEV), b)
    return dict(N=N, rows=rows, n=n, off_s=off_s, ids_s=ids_s, small=small, T=T, keep=(keep, tabs), C=tabs["C"],
                seq=(off, SQ.dev(ids_real, np.int32)), side=side)


@pytest.mark.parametrize("side,D", [("user", 64), ("item", 64), ("item", 10)])
def test_sequence_kernels_on_large_tables(side, D):
    ops = _ops()
    c = _case(side, D, seed=D + (7 if side == "user" else 3))
    n, rows, off_s, ids_s = c["n"], c["rows"], c["off_s"], c["ids_s"]
    rs = np.random.RandomState(5)
    entry = np.concatenate([off_s[:-1], rs.randint(0, int(off_s[-1]), 8)]).astype(np.int64)  # every user once, then more
    user = (np.searchsorted(off_s, entry, side="right") - 1).astype(np.int64)
    neg = rs.randint(0, n - 1, entry.size)
    neg = neg + (neg >= ids_s[entry])
    big_u = rows[user] if side == "user" else user
    big_i = (lambda a: rows[a]) if side == "item" else (lambda a: a)
    lt.assert_covers(big_u if side == "user" else np.concatenate([big_i(ids_s), big_i(neg)]), c["N"], D)
    w = ref.weights(L, 0.7)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    for loss in ("bpr", "hinge"):
        want, tol_r, tol_l, tol_loss = SQ.measured_tolerance(c["small"], off_s, ids_s, user, entry, neg, w, loss)
        loss_sum = torch.zeros(1, device=DEV)
        gr, gl, cid = ops.seq_fwd_bwd(c["T"], c["C"], c["seq"], SQ.dev(big_u, np.int32), SQ.dev(entry, np.int64),
                                      SQ.dev(big_i(neg), np.int32), SQ.dev(w, np.float32), SQ._loss_id(loss), loss_sum,
                                      err_flag=err)
        torch.cuda.synchronize()
        assert np.abs(gr.cpu().numpy() - want[0]).max() <= tol_r and np.abs(gl.cpu().numpy() - want[1]).max() <= tol_l
        assert abs(loss_sum.item() - want[3]) <= max(tol_loss, 1e-6 * want[3])
        k = entry - off_s[user]
        present = np.arange(L)[:, None] < k[None, :]
        assert np.array_equal(cid.cpu().numpy(), np.where(present, big_i(want[2]), 0))
    # the query rows of the same users' whole sequences, bit for bit against the float32 loop on the compacted tables
    users = np.arange(n, dtype=np.int64)
    sub = (SQ.dev(off_s, np.int64), SQ.dev(big_i(ids_s), np.int32))
    out = ops.seq_user_rows(c["T"], c["C"], sub, SQ.dev(rows[users] if side == "user" else users, np.int64),
                            SQ.dev(w, np.float32), err_flag=err).cpu().numpy()
    assert np.array_equal(out.view(np.int32), ref.user_rows(c["small"], off_s, ids_s, users, w).view(np.int32))
    assert err.item() == 0
