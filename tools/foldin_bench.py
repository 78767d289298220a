# -*- coding: utf-8 -*-
"""Fold-in of unseen users (csrc/foldin.hip: fold_in_kernel; TorchRecSys.fold_in_users / recommend_for_histories) at
c2- and c4-like shapes, CUDA events around the fold-in launch and around fold-in + top-k.

  c2: 100 000 items, D = 64, 65 536 new users        c4: 1 000 000 items, D = 128, 32 768 new users
  history lengths log-normal (median 20, sigma 1), capped at 1 000, at least 1; E = 8 epochs; shuffle and reject_seen on
  (max_tries 8); users handed over longest history first, as fold_in_users does.

One JSON line per (case, net, FOLDIN_DEPTH): ms per launch (median and minimum over the repetitions, one warm-up call
first), visits per second, the algorithmic byte rate — 2 (Dp + 1) 4 bytes per visit, the two item rows and constants a
visit reads — and its ratio to 5.5 TB/s, the rate at which random whole rows of a large table gather into registers on
an MI355X (a yardstick: the kernel also derives every visit's schedule), and ms of fold-in + top-10 with the histories
excluded.
FOLDIN_DEPTH = 1 is the loop with only the next visit requested ahead; the default is 4.
--cap N caps the history lengths at N instead of 1 000: per-visit SGD is sequential per user, so a launch cannot end
before its longest history has (the lines carry `longest_history`).
Usage: python tools/foldin_bench.py [--cases c2,c4] [--nets linear,fm] [--depths 4,1,2,8] [--reps 7] [--cap 1000]"""
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
GATHER_TBS = 5.5
CHUNK = 65_536  # TorchRecSys.RECOMMEND_CHUNK
CASES = {"c2": (100_000, 64, 65_536), "c4": (1_000_000, 128, 32_768)}
E = 8


def histories(n_items, n_new, seed, cap):
    """(offsets int64, items int32) CSR on the GPU, rows sorted and distinct, longest first; and the visit count."""
    rs = np.random.RandomState(seed)
    lens = np.clip(np.rint(rs.lognormal(np.log(20.0), 1.0, n_new)), 1, cap).astype(np.int64)
    lens = np.sort(lens)[::-1]
    rows = np.repeat(np.arange(n_new, dtype=np.int64), lens)
    key = np.unique(rows * n_items + rs.randint(0, n_items, rows.size))  # a repeated draw shortens its row by one
    rows, items = key // n_items, (key % n_items).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_new))]).astype(np.int64)
    return torch.from_numpy(off).to(DEV), torch.from_numpy(items).to(DEV), int(items.size)


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


def run_case(name, nets, depths, reps, cap):
    n_items, D, n_new = CASES[name]
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    item = (torch.randn(n_items, D, device=DEV, generator=g) * 0.1).contiguous()
    item_lin = (torch.randn(n_items, 1, device=DEV, generator=g) * 0.1).contiguous()
    user = torch.zeros(1, D, device=DEV)
    T, keep = ops.make_tables(user, item, torch.zeros(1, 1, device=DEV), item_lin)
    off, items, nnz = histories(n_items, n_new, 2, cap)
    longest = int((off[1:] - off[:-1]).max())
    Dp = max(16, 1 << (D - 1).bit_length())
    users = torch.arange(n_new, device=DEV, dtype=torch.int64)
    for net in nets:
        fold = ops.item_fold(net, T, n_items, D, DEV)

        def fold_in():
            return ops.fold_in_users(net, fold, n_items, D, (off, items), "hinge", E, 0.05, 0.0, 0, True, True, 8)

        def both():
            U, b, _ = fold_in()
            Tq, kq = ops.make_tables(U, item, b.view(-1, 1), item_lin)
            for s in range(0, n_new, CHUNK):
                ops.retrieve_topk(net, Tq, fold, users[s:s + CHUNK], 10, (off, items))

        for depth in depths:
            with _lib.tuning(FOLDIN_DEPTH=depth):
                t = times(fold_in, reps)
                tb = times(both, max(reps // 2, 2))
            ms = statistics.median(t)
            visits = nnz * E
            byte_rate = visits * 2 * (Dp + 1) * 4 / (ms * 1e-3) / 1e12
            print(json.dumps({"case": name, "net": net, "n_items": n_items, "D": D, "n_new": n_new, "epochs": E,
                              "history_items": nnz, "longest_history": longest, "foldin_depth": depth, "fold_in_ms": round(ms, 3),
                              "fold_in_ms_min": round(min(t), 3), "visits_per_s": round(visits / (ms * 1e-3)),
                              "algorithmic_TB_per_s": round(byte_rate, 3),
                              "ratio_to_register_gather_5.5TBs": round(byte_rate / GATHER_TBS, 3),
                              "fold_in_plus_top10_ms": round(statistics.median(tb), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,c4")
    ap.add_argument("--nets", default="linear,fm")
    ap.add_argument("--depths", default="4,1,2,8")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cap", type=int, default=1000, help="longest history (a launch lasts as long as its longest user)")
    a = ap.parse_args()
    for name in a.cases.split(","):
        run_case(name, a.nets.split(","), [int(d) for d in a.depths.split(",")], a.reps, a.cap)


if __name__ == "__main__":
    main()
