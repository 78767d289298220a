# -*- coding: utf-8 -*-
"""Exact ranks (csrc/retrieve.hip rank_values_kernel / rank_count_kernel, TorchRecSys.rank_items / evaluate_ranks) at
the c2 and c4 shapes, beside the fused top-k on the same users, fold and seen CSR.

  c2: FM, 1M users x 100K items, D = 64      c4: FM, 10M users x 1M items, D = 128
  4 096 query users with 1 and with 4 targets each (sorted, distinct, seeded), seen masking from 100M seeded interactions

One JSON line per (case, targets per user): device-event ms, median and minimum of 7 after one warm-up call, of
  keys_ms     the target-key launch alone            (knob RANKS_STAGES = 1)
  count_ms    the counting launch alone              (RANKS_STAGES = 2, the keys of the call before still in the workspace)
  call_ms     trs_item_ranks as callers see it: the 8-byte read-back of the target count and both launches
  topk_ms     trs_retrieve_topk at k = 10 on the same users (its tile launch and its merge)
the three legs alternating within each repetition; count_over_topk = count_ms / topk_ms (medians); TFLOP/s of the
counting launch = 2 * rows * n_items * D over count_ms and its share of the 157.3 TF fp32 matrix peak (the launch is
matrix-bound at D >= 64: one row of 32 x 32 x 2 MFMAs per 8 factors, whatever the epilogue).
Usage: python tools/ranks_bench.py [--legs c2,c4] [--out profiles/ranks_bench_c2_c4.jsonl]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchrecsys_amd import _lib, ops  # noqa: E402
from retrieval_bench import DEV, PEAK_TF, seen_csr, tables  # noqa: E402

REPS = 7


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def leg(name, T, seen, users, fold, n_items, D, per_user, n_inter, out):
    lib = _lib.load()
    n_q = users.numel()
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    # per_user distinct targets per query: a random start plus distinct strides, sorted
    start = torch.randint(0, n_items // per_user, (n_q, 1), device=DEV, generator=g)
    items = (start + torch.arange(per_user, device=DEV)[None, :] * (n_items // per_user)).sort(1).values
    items = items.reshape(-1).to(torch.int32).contiguous()
    off = torch.arange(n_q + 1, device=DEV, dtype=torch.int64) * per_user
    n_t = n_q * per_user
    ranks = torch.empty(n_t, dtype=torch.int64, device=DEV)
    ws_bytes = lib.trs_item_ranks_workspace_bytes(n_q, n_t)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    ct, cs = ops.csr(off, items), ops.csr(*seen)

    def item_ranks():
        _lib.check(lib.trs_item_ranks(ops.NET_ID["fm"], C.byref(T), _lib.ptr(fold), fold.numel(), _lib.ptr(users), n_q,
                                      C.byref(ct), C.byref(cs), _lib.ptr(ranks), None, _lib.ptr(ws), ws_bytes,
                                      ops._stream()), "trs_item_ranks")

    def staged(stages):
        with _lib.tuning(RANKS_STAGES=stages):
            item_ranks()

    def topk():
        ops.retrieve_topk("fm", T, fold, users, 10, seen)

    item_ranks()  # warm-up; leaves the keys in the workspace for the counting launch alone
    want = ranks.clone()
    topk()
    torch.cuda.synchronize()
    t = {"keys": [], "count": [], "call": [], "topk": []}
    for _ in range(REPS):
        t["keys"].append(timed(lambda: staged(1)))
        t["count"].append(timed(lambda: staged(2)))
        t["call"].append(timed(item_ranks))
        t["topk"].append(timed(topk))
    assert torch.equal(ranks, want), "trs_item_ranks is not deterministic"
    med = {k: statistics.median(v) for k, v in t.items()}
    tf = 2.0 * n_t * n_items * D / (med["count"] * 1e-3) / 1e12
    rec = {"leg": name, "n_q": n_q, "targets_per_user": per_user, "rows": n_t, "n_items": n_items, "D": D,
           "seen_interactions": n_inter}
    for k in t:
        rec[f"{k}_ms"] = round(med[k], 3)
        rec[f"{k}_ms_min"] = round(min(t[k]), 3)
    rec.update({"count_over_topk": round(med["count"] / med["topk"], 3), "count_tflops": round(tf, 2),
                "count_fraction_of_fp32_peak": round(tf / PEAK_TF, 3),
                "mean_rank": round(float(want.double().mean()), 1)})
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="c2,c4")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.out and os.path.exists(a.out):
        os.remove(a.out)
    for name, n_users, n_items, D in (("c2", 1_000_000, 100_000, 64), ("c4", 10_000_000, 1_000_000, 128)):
        if name in a.legs.split(","):
            n_q, n_inter = 4096, 100_000_000
            T, keep = tables(n_users, n_items, D, 1)
            seen = seen_csr(n_users, n_items, n_inter, 2)
            users = torch.arange(n_q, device=DEV, dtype=torch.int64) * (n_users // n_q)
            fold = ops.item_fold("fm", T, n_items, D, DEV)
            for per_user in (1, 4):
                leg(f"{name}_t{per_user}", T, seen, users, fold, n_items, D, per_user, n_inter, a.out)
            del T, keep, seen, fold


if __name__ == "__main__":
    main()
