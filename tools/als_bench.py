# -*- coding: utf-8 -*-
"""Implicit ALS (csrc/als.hip: trs_als_gram + trs_als_solve; TorchRecSys.fit_als) at c2- and c4-like shapes, CUDA events
around the two launches of a half-sweep.

  c2: 1 000 000 users x 100 000 items, D = 64        c4: 10 000 000 users x 1 000 000 items, D = 128
  history lengths log-normal (median 20, sigma 1), capped at 1 000, at least 1, items uniform; the distinct pairs are the
  training data (ops.Sampler.seen_csr, as fit_als builds them), tables 0.1 * randn.

One JSON line per (case, side): ms of the half-sweep (Gram matrix of the frozen table + the solve of every row; median
and minimum over the repetitions, one warm-up first) and of its two launches, the algorithmic bytes — (1 + cg_steps)
passes over the neighbour rows, nnz * D * 4 bytes each, plus G — their rate over the half-sweep, and its ratio to 5.5
TB/s, the rate at which random whole rows of a large table gather into registers on an MI355X (tools/foldin_bench.py's
yardstick; the kernel also multiplies by G once per pass).  Every repetition starts from the same tables.
The user-side line also carries what trs_fold_in_users takes for ONE epoch over the same CSR in the same session
(Linear, hinge, shuffle and reject_seen on): per-visit SGD reads two item rows per pair once, ALS one row per pair
1 + cg_steps times.
Usage: python tools/als_bench.py [--cases c2,c4] [--cg-steps 3] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchrecsys_amd import ops  # noqa: E402

DEV = "cuda:0"
GATHER_TBS = 5.5
CASES = {"c2": (1_000_000, 100_000, 64), "c4": (10_000_000, 1_000_000, 128)}
LAMBDA, ALPHA = 0.1, 10.0


def pairs(n_users, n_items, seed):
    """(user, item) int32 streams on the GPU: log-normal history lengths, uniform items (repeats collapse later)."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    lens = torch.empty(n_users, device=DEV).log_normal_(mean=float(torch.log(torch.tensor(20.0))), std=1.0, generator=g)
    lens = lens.round().clamp_(1, 1000).long()
    user = torch.repeat_interleave(torch.arange(n_users, device=DEV, dtype=torch.int32), lens)
    item = torch.randint(0, n_items, (user.numel(),), device=DEV, generator=g, dtype=torch.int32)
    return user, item


def times(fn, reps, before=None):
    """Event times of fn() in ms; before() (restoring the start values) runs outside the events."""
    def prepare():
        if before is not None:
            before()
        torch.cuda.synchronize()
    prepare()
    fn()  # warm-up (allocations, code objects)
    out = []
    for _ in range(reps):
        prepare()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def run_case(name, cg_steps, reps):
    n_users, n_items, D = CASES[name]
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    X0 = (torch.randn(n_users, D, device=DEV, generator=g) * 0.1).contiguous()
    Y0 = (torch.randn(n_items, D, device=DEV, generator=g) * 0.1).contiguous()
    user, item = pairs(n_users, n_items, 2)
    by_user = ops.Sampler.seen_csr(user, item, n_users, n_items)
    by_item = ops.Sampler.seen_csr(item, user, n_items, n_users)
    del user, item
    nnz = int(by_user[1].numel())
    work = torch.empty_like(X0)
    for side, rows0, other, nbr in (("user", X0, Y0, by_user), ("item", Y0, X0, by_item)):
        rows = work[:rows0.shape[0]]
        state = {}

        def gram():
            state["G"] = ops.als_gram(other)

        def solve():
            ops.als_solve(other, state["G"], nbr, LAMBDA, ALPHA, cg_steps, rows)

        def half_sweep():
            gram()
            solve()

        def restore():  # every repetition from the same start values
            rows.copy_(rows0)

        t_gram = times(gram, reps)
        t_half = times(half_sweep, reps, restore)
        t_solve = times(solve, reps, restore)
        ms = statistics.median(t_half)
        nbytes = (1 + cg_steps) * nnz * D * 4 + D * D * 4
        rate = nbytes / (ms * 1e-3) / 1e12
        longest = int((nbr[0][1:] - nbr[0][:-1]).max())
        line = {"case": name, "side": side, "n_rows": int(rows0.shape[0]), "n_other": int(other.shape[0]), "D": D,
                "pairs": nnz, "longest_list": longest, "cg_steps": cg_steps, "half_sweep_ms": round(ms, 3),
                "half_sweep_ms_min": round(min(t_half), 3), "gram_ms": round(statistics.median(t_gram), 3),
                "solve_ms": round(statistics.median(t_solve), 3), "algorithmic_GB": round(nbytes / 1e9, 3),
                "algorithmic_TB_per_s": round(rate, 3), "ratio_to_register_gather_5.5TBs": round(rate / GATHER_TBS, 3)}
        if side == "user":
            T, keep = ops.make_tables(torch.zeros(1, D, device=DEV), Y0, torch.zeros(1, 1, device=DEV),
                                      torch.zeros(n_items, 1, device=DEV))
            fold = ops.item_fold("linear", T, n_items, D, DEV)
            t_fold = times(lambda: ops.fold_in_users("linear", fold, n_items, D, by_user, "hinge", 1, 0.05, 0.0, 0, True,
                                                     True, 8), reps)
            line["fold_in_users_one_epoch_ms"] = round(statistics.median(t_fold), 3)
            del fold
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,c4")
    ap.add_argument("--cg-steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for name in a.cases.split(","):
        run_case(name, a.cg_steps, a.reps)


if __name__ == "__main__":
    main()
