# -*- coding: utf-8 -*-
"""Counters that outlive a step, host side (no GPU): the stamps SparseScorerTrainer._stamps hands to the duplicate-
detection scratch, RowState.next_id of the coalescing row optimisers, and trs_train_steps_sgd's refusal of stamps that
are zero or would wrap (argument checks that run before anything touches the device).  The kernels at those values:
tests/test_gpu_long_run.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from torchrecsys_amd import _lib, ops
from torchrecsys_amd.engine import RowState, SparseScorerTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 0xFFFFFFF0
P = 0x1000  # a non-NULL "device pointer": validation never dereferences it


def _stub(kind, stamp):
    """A trainer with nothing but what _stamps touches; scratch and counters on the CPU."""
    tr = SparseScorerTrainer.__new__(SparseScorerTrainer)
    tr.fast_kind, tr.stamp = kind, stamp
    tr.scratch = torch.ones(64, dtype=torch.int64)
    if kind != "sgd":
        tr.cut_count = torch.ones((2, 2), dtype=torch.int32)
    return tr


@pytest.mark.parametrize("kind", ["sgd", "sparse_adam", "adagrad"])
@pytest.mark.parametrize("start", [1, LIMIT - 700, LIMIT - 2, 0x7FFFFFF0])
def test_stamps_never_zero_never_at_the_limit_consecutive_and_reset_cleanly(kind, start):
    rs = np.random.RandomState(start % 1000)
    tr = _stub(kind, start)
    sizes = [1, 64, 1, 7, 512, 64, 64, 2, 1, 1, 333] + rs.randint(1, 600, 40).tolist()
    prev_end, resets = start, 0  # the stamp after the previous call's last one
    for n in sizes:
        tr.scratch.fill_(1)  # marks of earlier steps
        if kind != "sgd":
            tr.cut_count.fill_(3)  # a list the previous step left behind
        first = tr._stamps(n)
        assert first != 0 and 0 < first and first + n < LIMIT and first + n - 1 <= 0xFFFFFFFF
        if first == prev_end:  # no reset: the range follows the previous one, nothing was cleared
            assert int(tr.scratch.min()) == 1
            assert kind == "sgd" or int(tr.cut_count.min()) == 3
            # (so the parity the cut-run counters alternate by goes on from the previous call's last stamp)
        else:  # a reset: back to 1 on a zeroed scratch, and both cut-run counters empty whatever parity comes next
            resets += 1
            assert first == 1 and prev_end + n >= LIMIT
            assert int(tr.scratch.abs().max()) == 0
            assert kind == "sgd" or int(tr.cut_count.abs().max()) == 0
        assert tr.stamp == first + n
        prev_end = first + n
    assert resets == (1 if start >= LIMIT - 700 else 0)


def test_stamps_restart_exactly_at_the_limit():
    tr = _stub("sgd", LIMIT - 10)
    assert tr._stamps(9) == LIMIT - 10 and tr.stamp == LIMIT - 1  # first + n = LIMIT - 1: the last range before the limit
    tr = _stub("sgd", LIMIT - 10)
    assert tr._stamps(10) == 1 and tr.stamp == 11 and int(tr.scratch.abs().max()) == 0  # first + n would be LIMIT


def test_every_stamp_the_trainer_hands_out_is_one_the_library_accepts():
    """_stamps stops 15 short of the C guard (first_stamp + n_steps < 0xFFFFFFFF)."""
    tr = _stub("sgd", LIMIT - 65)
    first = tr._stamps(64)
    assert first + 64 == LIMIT - 1 < 0xFFFFFFFF


def test_next_id_never_zero_never_int32_max_and_zeroes_the_stamps_exactly_at_the_restart():
    rs = RowState(torch.nn.Parameter(torch.zeros(5, 3)))
    assert rs.stamp.dtype == torch.int32 and rs.step_id == 0
    assert [rs.next_id() for _ in range(3)] == [1, 2, 3]
    rs.step_id = 2 ** 31 - 5
    top = 2 ** 31 - 1
    seen = []
    for _ in range(8):
        rs.stamp.fill_(7)  # marks of the steps before
        before = rs.step_id
        sid = rs.next_id()
        seen.append(sid)
        assert sid != 0 and 0 < sid < top  # fits the kernel's int32, and never the value a zeroed stamp holds
        if sid == before + 1:
            assert int(rs.stamp.min()) == 7  # no restart: the stamps are left alone
        else:
            assert sid == 1 and before == top - 1 and int(rs.stamp.abs().max()) == 0
    assert seen == [top - 3, top - 2, top - 1, 1, 2, 3, 4, 5]


# ------------------------------------------------------------------------------------------- the C guard on the stamps
def _args(first_stamp, n_steps, scratch=P):
    T = _lib.TrsTables()
    T.user = T.item = T.user_lin = T.item_lin = P
    T.n_users, T.n_items, T.D, T.M = 10, 10, 8, 0
    a = _lib.TrsTrainArgs()
    a.net, a.n_steps, a.tables, a.batch, a.lr = ops.NET_ID["fm"], n_steps, C.pointer(T), 16, 0.05
    a.first_stamp = first_stamp
    a.user_buf_dev = a.pos_buf_dev = a.neg_buf_dev = a.gz_buf_dev = a.du_buf_dev = a.loss_sums_dev = P
    a.scratch_dev = scratch
    return a, T


@pytest.mark.parametrize("first_stamp,n_steps", [(0, 3), (0, 0), (0xFFFFFFFF - 3, 3), (0xFFFFFFFF, 0),
                                                 (0xFFFFFFFE, 1), (0xFFFFFFFF - 64, 64)])
def test_stamps_that_are_zero_or_reach_the_end_are_refused_before_the_device_is_touched(first_stamp, n_steps):
    lib = _lib.load()
    a, keep = _args(first_stamp, n_steps)
    rc = lib.trs_train_steps_sgd(C.byref(a), None)
    assert rc < 0
    msg = lib.trs_last_error().decode()
    assert "stamps must be non-zero and must not wrap" in msg
    with pytest.raises(_lib.TrsError, match="stamps"):
        _lib.check(rc, "trs_train_steps_sgd")


def test_the_guard_accepts_the_largest_stamps_and_anything_without_a_scratch():
    """(n_steps = 0: the checks run, no step is launched — FitRunner.touch_host_path relies on the same)"""
    lib = _lib.load()
    for first_stamp, scratch in ((0xFFFFFFFE, P), (1, P), (0x80000000, P), (0, None), (0xFFFFFFFF, None)):
        a, keep = _args(first_stamp, 0, scratch)
        assert lib.trs_train_steps_sgd(C.byref(a), None) == 0, hex(first_stamp)


def test_rebase_threshold_of_the_arrival_counter_is_declared():
    """TRS_SYNC_REBASE: far enough below 2^31 that no two values on sync_dev are ever a sign bit apart, whatever the
    grid (at most 4096 workgroups per launch)."""
    hdr = open(os.path.join(ROOT, "include", "trs.h")).read()
    rebase = int(re.search(r"#define TRS_SYNC_REBASE (0x[0-9a-fA-F]+)u", hdr).group(1), 16)
    words = int(re.search(r"#define TRS_SYNC_WORDS (\d+)", hdr).group(1))
    assert rebase == 1 << 30 and rebase + 4096 < 1 << 31
    assert words == 288 >= 32 * 8 + 1  # the counter's line + eight flag lines of 32 words
