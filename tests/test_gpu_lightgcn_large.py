# -*- coding: utf-8 -*-
"""trs_lgcn_propagate at row offsets beyond 32 bits, after the pattern of tests/test_gpu_seq_large.py: ids from
large_tables.band_rows (every band, both sides of every boundary, row 0 and the last row), the tables under test filled
with device-generated values everywhere, and the float32 loop of the rule (tests/lgcn_ref.py) on the COMPACTED rows,
bit for bit.  Two sides: the gathered side large (in_rows: one table of 8.6 GB, with its dinv_in), and the written side
large (out_rows and add_rows: two tables, the CSR and dinv_out one entry per row; accumulate, so that out_rows is read
and written there)."""
import numpy as np
import pytest
import torch

import large_tables as lt
import lgcn_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENS = (1, 2, 5, 7, 16, 3, 0, 9)


def _ops():
    from torchrecsys_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _small_lists(n_rows, n_in, seed):
    """CSR of n_rows short lists into n_in rows that names every one of them."""
    rs = np.random.RandomState(seed)
    lens = np.array([LENS[r % len(LENS)] for r in range(n_rows)])
    lens[0] = n_in
    off = np.zeros(n_rows + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    ids = np.concatenate([rs.permutation(n_in)[:n] for n in lens]).astype(np.int32)
    return off, ids


@pytest.mark.parametrize("D", [64, 10])
def test_gathered_side_beyond_32_bit_offsets(D):
    ops = _ops()
    N = lt.n_rows_for(D)
    rows = lt.band_rows(N, D, 2, seed=D)
    n, n_out = rows.size, 21
    off, ids_s = _small_lists(n_out, n, seed=D + 1)
    lt.assert_covers(rows[ids_s], N, D)
    inp = lt.fill(torch.empty((N, D), device=DEV), seed=D + 2)
    g = torch.Generator(device=DEV)
    g.manual_seed(D + 3)
    dinv_in = torch.empty(N, device=DEV).uniform_(0.05, 1.0, generator=g)
    rs = np.random.RandomState(D + 4)
    add = rs.standard_normal((n_out, D)).astype(np.float32)
    dinv_out = rs.uniform(0.05, 1.0, n_out).astype(np.float32)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.empty((n_out, D), device=DEV)
    ops.lgcn_propagate(inp, (dev(off), dev(rows[ids_s].astype(np.int32))), dev(dinv_out), dinv_in, out, add=dev(add),
                       scale=0.25, err_flag=err)
    want = ref.propagate(lt.gather_small(inp, rows), (off, ids_s), dinv_out,
                         dinv_in[torch.as_tensor(rows, device=DEV)].cpu().numpy(), add=add, scale=0.25)
    assert err.item() == 0 and np.array_equal(bits(out.cpu().numpy()), bits(want))


@pytest.mark.parametrize("D", [64, 10])
def test_written_side_beyond_32_bit_offsets(D):
    ops = _ops()
    N = lt.n_rows_for(D)
    rows = lt.band_rows(N, D, 2, seed=D + 10)
    lt.assert_covers(rows, N, D)
    n, n_in = rows.size, 40
    off_s, ids = _small_lists(n, n_in, seed=D + 11)
    rs = np.random.RandomState(D + 12)
    inp = rs.standard_normal((n_in, D)).astype(np.float32)
    dinv_in = rs.uniform(0.05, 1.0, n_in).astype(np.float32)
    # the CSR over all N rows: the band rows carry the lists (in ascending row order, as `rows` is sorted), every other
    # row is empty and is still written: out + scale * add
    where = torch.as_tensor(rows, device=DEV)
    lens = torch.zeros(N, dtype=torch.int64, device=DEV)
    lens[where] = dev(np.diff(off_s))
    off = torch.zeros(N + 1, dtype=torch.int64, device=DEV)
    off[1:] = torch.cumsum(lens, 0)
    del lens
    add = lt.fill(torch.empty((N, D), device=DEV), seed=D + 13)
    out = lt.fill(torch.empty((N, D), device=DEV), seed=D + 14)
    g = torch.Generator(device=DEV)
    g.manual_seed(D + 15)
    dinv_out = torch.empty(N, device=DEV).uniform_(0.05, 1.0, generator=g)
    others = np.setdiff1d(np.unique(np.random.RandomState(D + 16).randint(0, N, 500)), rows)
    look = np.concatenate([rows, others])  # compacted: the band rows, then rows with an empty list from all over
    off_c = np.concatenate([off_s, np.full(others.size, off_s[-1])])
    small = {k: lt.gather_small(t, look) for k, t in (("add", add), ("out", out))}
    d_small = dinv_out[torch.as_tensor(look, device=DEV)].cpu().numpy()
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.lgcn_propagate(dev(inp), (off, dev(ids)), dinv_out, dev(dinv_in), out, add=add, scale=0.25, accumulate=True,
                       err_flag=err)
    want = ref.propagate(inp, (off_c, ids), d_small, dinv_in, add=small["add"], scale=0.25, out=small["out"],
                         accumulate=True)
    got = lt.gather_small(out, look)
    assert err.item() == 0 and np.array_equal(bits(got), bits(want))
    assert not np.array_equal(got[:n], small["out"][:n] + np.float32(0.25) * small["add"][:n])  # the lists did count
