# -*- coding: utf-8 -*-
"""Batched top-k retrieval (csrc/retrieve.hip, TorchRecSys.recommend) at the c2 and c4 shapes.

  c2: FM, 1M users x 100K items, D = 64, all users, k in {10, 100}, seen masking from a random train split of 100M
      interactions (seeded)
  c4: FM, 10M users x 1M items, D = 128, 262 144 users, k = 10, seen masking from 100M interactions
  context: the per-user path predict_many() takes (trs_score_all_items + trs_topk per user) on 4 096 c2 users

Prints one JSON line per leg: ms (fold + top-k kernels, CUDA events, one warm-up call first), TFLOP/s of
2 * n_q * n_items * D over that time and its fraction of the 157.3 TF fp32 matrix peak, and the bytes of the folded item
matrix the user tiles stream (n_q / 32 * n_items_pad * Dp * 4).  Usage: python tools/retrieval_bench.py [--legs c2,c4,pm]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchrecsys_amd import ops  # noqa: E402

PEAK_TF = 157.3
DEV = "cuda:0"


def tables(n_users, n_items, D, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    r = lambda *s: (torch.randn(*s, device=DEV, generator=g) * 0.1).contiguous()
    keep = [r(n_users, D), r(n_items, D), r(n_users, 1), r(n_items, 1)]
    T, k2 = ops.make_tables(*keep)
    return T, keep + [k2]


def seen_csr(n_users, n_items, n_inter, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    u = torch.randint(0, n_users, (n_inter,), device=DEV, dtype=torch.int32, generator=g)
    i = torch.randint(0, n_items, (n_inter,), device=DEV, dtype=torch.int32, generator=g)
    return ops.Sampler.seen_csr(u, i, n_users, n_items)


def retrieval_leg(name, n_users, n_items, D, n_q, k, n_inter, chunk=65_536, reps=1):
    T, keep = tables(n_users, n_items, D, 1)
    seen = seen_csr(n_users, n_items, n_inter, 2)
    users = torch.arange(n_q, device=DEV, dtype=torch.int64) * (n_users // n_q)

    def run():
        fold = ops.item_fold("fm", T, n_items, D, DEV)
        for s in range(0, n_q, chunk):
            ops.retrieve_topk("fm", T, fold, users[s:s + chunk], k, seen)

    run()  # warm-up (workspace allocations)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    flop = 2.0 * n_q * n_items * D
    dp = ops._lib.load().trs_item_fold_bytes(n_items, D) // (((n_items + 127) // 128) * 128) // 4 - 1
    item_bytes = ((n_q + 31) // 32) * ((n_items + 127) // 128 * 128) * dp * 4
    tf = flop / (ms * 1e-3) / 1e12
    print(json.dumps({"leg": name, "n_q": n_q, "n_items": n_items, "D": D, "k": k, "seen_interactions": n_inter,
                      "ms": round(ms, 3), "tflops": round(tf, 2), "fraction_of_fp32_peak": round(tf / PEAK_TF, 3),
                      "item_matrix_bytes_streamed": item_bytes}), flush=True)


def predict_many_leg(n_q=4096, k=10):
    n_users, n_items, D = 1_000_000, 100_000, 64
    T, keep = tables(n_users, n_items, D, 1)
    users = (torch.arange(n_q) * (n_users // n_q)).tolist()
    out = torch.empty((n_q, k), dtype=torch.int64, device=DEV)

    def run():  # what predict_many() does per user: one score row, one top-k
        for r, u in enumerate(users):
            out[r] = ops.topk(ops.score_all_items("fm", T, u, n_items, DEV), k)

    run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    tf = 2.0 * n_q * n_items * D / (ms * 1e-3) / 1e12
    print(json.dumps({"leg": "c2_predict_many_path", "n_q": n_q, "n_items": n_items, "D": D, "k": k, "seen": False,
                      "ms": round(ms, 3), "tflops": round(tf, 3), "fraction_of_fp32_peak": round(tf / PEAK_TF, 4)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="c2,c4,pm")
    legs = ap.parse_args().legs.split(",")
    if "c2" in legs:
        for k in (10, 100):
            retrieval_leg(f"c2_k{k}", 1_000_000, 100_000, 64, 1_000_000, k, 100_000_000)
    if "c4" in legs:
        retrieval_leg("c4_k10", 10_000_000, 1_000_000, 128, 262_144, 10, 100_000_000)
    if "pm" in legs:
        predict_many_leg()


if __name__ == "__main__":
    main()
