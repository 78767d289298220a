# -*- coding: utf-8 -*-
"""LightGCN (csrc/lgcn.hip: trs_lgcn_propagate + trs_lgcn_adam; TorchRecSys.fit_lightgcn) at c2- and c4-like shapes,
device events around every launch, the median of the repetitions after one warm-up.

  c2: 1 000 000 users x 100 000 items, D = 64        c4: 10 000 000 users x 1 000 000 items, D = 128
  history lengths log-normal (median 20, sigma 1), capped at 1 000 ("lognormal") or at 100 ("capped100": the same
  rate question without the skew), at least 1, items uniform; the distinct pairs are the graph (ops.Sampler.seen_csr,
  as fit_lightgcn builds it), tables 0.1 * randn.

One JSON line per (case, histories, side): ms of ONE trs_lgcn_propagate launch over that side's CSR (add given, scale
0.25), its algorithmic bytes — one pass over the neighbour rows, nnz * D * 4 — and their rate; beside it the yardstick
of the same session: trs_als_solve at cg_steps = 3 on the same CSR makes four passes over the same neighbour rows, so
its time / 4 is what one pass costs the existing kernel.  A propagate launch does strictly less per row and should take
no longer.  ALS's four passes are not alike, though: a row's second to fourth pass re-read the neighbour rows its first
pass has just fetched.  cg_steps = 1 (two passes) beside cg_steps = 3 separates them: a later pass costs (t3 - t1) / 2,
the first one t1 minus that, and propagate — always a first pass — is also held against that figure.
Then one line per (case, histories) with the rest of a step at batch 16 384: zeroing G plus the two scatter launches,
the two trs_lgcn_adam launches, and a whole LightGCNTrainer step (Adam, bpr, l2) for layers = 1 and 3.
Usage: python tools/lightgcn_bench.py [--cases c2,c4] [--reps 3] [--out profiles/lightgcn_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchrecsys_amd import _lib, ops  # noqa: E402
from torchrecsys_amd.collaborative.linear import Linear  # noqa: E402
from torchrecsys_amd.engine import LightGCNTrainer  # noqa: E402

DEV = "cuda:0"
CASES = {"c2": (1_000_000, 100_000, 64), "c4": (10_000_000, 1_000_000, 128)}
BATCH = 16384


def pairs(n_users, n_items, cap, seed):
    """(user, item) int32 streams on the GPU: log-normal history lengths capped at `cap`, uniform items."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    lens = torch.empty(n_users, device=DEV).log_normal_(mean=float(torch.log(torch.tensor(20.0))), std=1.0, generator=g)
    lens = lens.round().clamp_(1, cap).long()
    user = torch.repeat_interleave(torch.arange(n_users, device=DEV, dtype=torch.int32), lens)
    item = torch.randint(0, n_items, (user.numel(),), device=DEV, generator=g, dtype=torch.int32)
    return user, item


def times(fn, reps, before=None):
    """Median event time of fn() in ms, after one warm-up; before() (restoring start values) runs outside the events."""
    def prepare():
        if before is not None:
            before()
        torch.cuda.synchronize()
    prepare()
    fn()
    out = []
    for _ in range(reps):
        prepare()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def run_case(name, hist, cap, reps, emit):
    n_users, n_items, D = CASES[name]
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    with torch.device(DEV):  # (the tables are created where they live: no host copy of 5 GB)
        net = Linear(n_users, n_items, {}, D, use_metadata=False)
    U0 = (torch.randn(n_users, D, device=DEV, generator=g) * 0.1).contiguous()
    V0 = (torch.randn(n_items, D, device=DEV, generator=g) * 0.1).contiguous()
    user, item = pairs(n_users, n_items, cap, 2)
    by_user = ops.Sampler.seen_csr(user, item, n_users, n_items)
    by_item = ops.Sampler.seen_csr(item, user, n_items, n_users)
    nnz = int(by_user[1].numel())
    du, di = ops.lgcn_dinv(by_user[0]), ops.lgcn_dinv(by_item[0])
    work = torch.empty_like(U0)
    for side, out_rows, inp, nbr, d_out, d_in in (("user", U0, V0, by_user, du, di), ("item", V0, U0, by_item, di, du)):
        out = work[:out_rows.shape[0]]
        ms = times(lambda: ops.lgcn_propagate(inp, nbr, d_out, d_in, out, add=out_rows, scale=0.25), reps)
        G = ops.als_gram(inp)
        als, als1 = (times(lambda: ops.als_solve(inp, G, nbr, 0.1, 10.0, cg, out), reps, lambda: out.copy_(out_rows))
                     for cg in (3, 1))
        later = (als - als1) / 2  # cg_steps 3 against 1: two more passes over rows the set-up and first step just read
        nbytes = nnz * D * 4
        emit({"case": name, "histories": hist, "side": side, "n_rows": int(out_rows.shape[0]), "n_in": int(inp.shape[0]),
              "D": D, "pairs": nnz, "longest_list": int((nbr[0][1:] - nbr[0][:-1]).max()),
              "propagate_ms": round(ms, 3), "algorithmic_GB": round(nbytes / 1e9, 3),
              "algorithmic_TB_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3), "als_solve_cg3_ms": round(als, 3),
              "als_per_pass_ms": round(als / 4, 3), "propagate_over_als_pass": round(ms / (als / 4), 3),
              "als_solve_cg1_ms": round(als1, 3), "als_later_pass_ms": round(later, 3),
              "als_first_pass_ms": round(als1 - later, 3), "propagate_over_als_first_pass": round(ms / (als1 - later), 3)})
    del work
    line = {"case": name, "histories": hist, "D": D, "pairs": nnz, "batch": BATCH}
    n = int(user.numel())
    for layers in (1, 3):
        tr = LightGCNTrainer(net, (U0.clone(), V0.clone()), (by_user, by_item), layers, BATCH, 1e-3, _lib.LOSS_ID["bpr"],
                             "adam", 1e-4)
        tr.forward()
        loss = torch.zeros(1, device=DEV)
        state = {"s": 0}

        def step():
            s = state["s"]
            state["s"] = (s + BATCH) % (n - BATCH)
            ids = ops.batch_prepare(user, item, None, 12345, s, BATCH, n_items, 777, s,
                                    sampler=ops.Sampler(seen=by_user, max_tries=8))
            tr.lgcn_step(ids["user"], ids["pos"], ids["neg"], loss)

        with torch.no_grad():
            line[f"step_layers{layers}_ms"] = round(times(step, reps), 3)
            if layers == 1:
                ids = ops.batch_prepare(user, item, None, 12345, 0, BATCH, n_items, 777, 0)
                items2 = torch.cat([ids["pos"], ids["neg"]])
                rows = torch.randn(2 * BATCH, D, device=DEV)

                def g_fill():
                    tr.g_user.zero_()
                    tr.g_item.zero_()
                    ops.rows_scatter_add(tr.g_user, ids["user"], rows[:BATCH], 1.0, ld=D)
                    ops.rows_scatter_add(tr.g_item, items2, rows, 1.0, ld=D)

                def adam():
                    ops.lgcn_adam(tr.base_user, tr.g_user, tr.moments[0], tr.moments[1], 1e-3, 0.9, 0.999, 1e-8, 1)
                    ops.lgcn_adam(tr.base_item, tr.g_item, tr.moments[2], tr.moments[3], 1e-3, 0.9, 0.999, 1e-8, 1)

                line["g_zero_scatter_ms"] = round(times(g_fill, reps), 3)
                ms = times(adam, reps)
                line["adam_two_tables_ms"] = round(ms, 3)
                line["adam_TB_per_s"] = round(7 * 4 * (n_users + n_items) * D / (ms * 1e-3) / 1e12, 3)
        tr.check_errors()
        del tr
    emit(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,c4")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "lightgcn_bench.jsonl"))
    a = ap.parse_args()
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    for name in a.cases.split(","):
        for hist, cap in (("lognormal", 1000), ("capped100", 100)):
            run_case(name, hist, cap, a.reps, emit)
            torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
