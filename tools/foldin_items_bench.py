# -*- coding: utf-8 -*-
"""Fold-in of unseen items (csrc/foldin.hip: fold_in_items_kernel; TorchRecSys.fold_in_items) at c2- and c4-like shapes,
CUDA events around the launch, with trs_fold_in_users in the same session as the yardstick.

  c2: 1 000 000 users x 100 000 items, D = 64, 65 536 new items    c4: 10 000 000 users x 1 000 000 items, D = 128,
  32 768 new items; 10 000 000 synthetic train rows (uniform users and items) for the negative visits and the seen CSR.
  history lengths log-normal (median 20, sigma 1), capped at --caps (1 000 and 100), at least 1; E = 8 epochs; shuffle
  and reject_seen on (max_tries 8); items handed over longest history first, as fold_in_items does.  The yardstick
  folds in as many new USERS with item histories of the same lengths against the same catalogue fold.

One JSON line per (case, net, cap, negative_visits, FOLDIN_DEPTH): ms per launch (median and minimum over the
repetitions, one warm-up call first), visits (E n_h (1 + nu) summed over the items) per second, the algorithmic byte
rate — (D + Dp + 2) 4 bytes per visit: the user row, the catalogue fold row and the two constants a visit reads — the
yardstick's ms and visits per second, and `per_visit_vs_users` = the yardstick's visits per second over this kernel's
(1.0 = a visit costs what a visit of the user fold-in costs; the user fold-in reads 2 (Dp + 1) 4 bytes per visit).
A launch cannot end before its longest chain of n_h (1 + nu) E sequential visits has (`longest_history`).
Usage: python tools/foldin_items_bench.py [--cases c2,c4] [--nets fm] [--depths 4,1] [--nus 0,1] [--caps 1000,100]
                                          [--reps 7]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchrecsys_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"
CASES = {"c2": (1_000_000, 100_000, 64, 65_536), "c4": (10_000_000, 1_000_000, 128, 32_768)}
N_STREAM = 10_000_000
E = 8


def histories(n_ids, n_new, seed, cap):
    """(offsets int64, ids int32) CSR on the GPU, rows sorted and distinct, longest first; and the entry count."""
    rs = np.random.RandomState(seed)
    lens = np.clip(np.rint(rs.lognormal(np.log(20.0), 1.0, n_new)), 1, cap).astype(np.int64)
    lens = np.sort(lens)[::-1]
    rows = np.repeat(np.arange(n_new, dtype=np.int64), lens)
    key = np.unique(rows * n_ids + rs.randint(0, n_ids, rows.size))  # a repeated draw shortens its row by one
    rows, ids = key // n_ids, (key % n_ids).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_new))]).astype(np.int64)
    return torch.from_numpy(off).to(DEV), torch.from_numpy(ids).to(DEV), int(ids.size)


def times(fn, reps):
    fn()  # warm-up (allocations)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def run_case(name, nets, depths, nus, caps, reps):
    n_users, n_items, D, n_new = CASES[name]
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    user = (torch.randn(n_users, D, device=DEV, generator=g) * 0.1).contiguous()
    user_lin = (torch.randn(n_users, 1, device=DEV, generator=g) * 0.1).contiguous()
    item = (torch.randn(n_items, D, device=DEV, generator=g) * 0.1).contiguous()
    item_lin = (torch.randn(n_items, 1, device=DEV, generator=g) * 0.1).contiguous()
    T, keep = ops.make_tables(user, item, user_lin, item_lin)
    su = torch.randint(0, n_users, (N_STREAM,), device=DEV, generator=g, dtype=torch.int32)
    si = torch.randint(0, n_items, (N_STREAM,), device=DEV, generator=g, dtype=torch.int32)
    seen = ops.Sampler.seen_csr(su, si, n_users, n_items)
    Dp = max(16, 1 << (D - 1).bit_length())
    new_fold = torch.zeros(_lib.load().trs_item_fold_bytes(n_new, D), dtype=torch.uint8, device=DEV)  # no metadata
    for cap in caps:
        ioff, iusers, innz = histories(n_users, n_new, 2, cap)   # new items: histories of users
        uoff, uitems, unnz = histories(n_items, n_new, 2, cap)   # the yardstick: new users, histories of items
        longest = int((ioff[1:] - ioff[:-1]).max())
        for net in nets:
            fold = ops.item_fold(net, T, n_items, D, DEV)

            def users_fold_in():
                return ops.fold_in_users(net, fold, n_items, D, (uoff, uitems), "hinge", E, 0.05, 0.0, 0, True, True, 8)

            for depth in depths:
                with _lib.tuning(FOLDIN_DEPTH=depth):
                    tu = times(users_fold_in, reps)
                    ums = statistics.median(tu)
                    u_rate = unnz * E / (ums * 1e-3)
                    for nu in nus:
                        def items_fold_in():
                            return ops.fold_in_items(net, T, fold, n_items, new_fold, (ioff, iusers), su, si, seen,
                                                     "hinge", E, 0.05, 0.0, nu, 0, True, True, 8)
                        t = times(items_fold_in, reps)
                        ms = statistics.median(t)
                        visits = innz * E * (1 + nu)
                        rate = visits / (ms * 1e-3)
                        print(json.dumps({
                            "case": name, "net": net, "n_users": n_users, "n_items": n_items, "D": D, "n_new": n_new,
                            "epochs": E, "cap": cap, "negative_visits": nu, "history_users": innz,
                            "longest_history": longest, "foldin_depth": depth, "fold_in_items_ms": round(ms, 3),
                            "fold_in_items_ms_min": round(min(t), 3), "visits_per_s": round(rate),
                            "algorithmic_TB_per_s": round(rate * (D + Dp + 2) * 4 / 1e12, 3),
                            "fold_in_users_ms": round(ums, 3), "fold_in_users_visits_per_s": round(u_rate),
                            "per_visit_vs_users": round(u_rate / rate, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,c4")
    ap.add_argument("--nets", default="fm")
    ap.add_argument("--depths", default="4,1")
    ap.add_argument("--nus", default="0,1")
    ap.add_argument("--caps", default="1000,100", help="longest history (a launch lasts as long as its longest chain)")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    ints = lambda s: [int(x) for x in s.split(",")]
    for name in a.cases.split(","):
        run_case(name, a.nets.split(","), ints(a.depths), ints(a.nus), ints(a.caps), a.reps)


if __name__ == "__main__":
    main()
