# -*- coding: utf-8 -*-
"""Nearest-neighbour search (csrc/retrieve.hip: neighbour_fold_kernel + the fused top-k with the query's own row
excluded; TorchRecSys.similar_items / similar_users) at the c2 and c4 shapes.

  c2_items: every item of a 100 000 x 64 catalogue against the catalogue, k in {10, 100}, dot and cosine
  c4_items: every item of a 1 000 000 x 128 catalogue, k in {10, 100}, dot and cosine
  c2_users: 262 144 users of a 1 000 000 x 64 user table against the table, k = 10, cosine
  for comparison, same machine and session:
    retrieve  trs_retrieve_topk (no seen CSR) on the same n_q x n_items x Dp x k with a user table of n_q rows: the same
              kernel without the exclusion path
    fold      item_fold_kernel (Linear, no metadata) on the same rows: it moves the same bytes once

Prints one JSON line per leg: ms of fold + top-k + merge (CUDA events, one warm-up call first), ms of the fold alone,
TFLOP/s of 2 * n_q * n_rows * D over the whole time and its fraction of the 157.3 TF fp32 matrix peak; the comparison
legs add the ratio to the matching neighbour leg.  Usage: python tools/neighbours_bench.py [--legs c2,c4,users]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchrecsys_amd import ops  # noqa: E402

PEAK_TF = 157.3
DEV = "cuda:0"
CHUNK = 65_536  # TorchRecSys.RECOMMEND_CHUNK


def rows(n, D, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return (torch.randn(n, D, device=DEV, generator=g) * 0.1).contiguous()


def timed(fn, reps):
    fn()  # warm-up (allocations)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def line(leg, n_q, n_rows, D, k, ms, **more):
    tf = 2.0 * n_q * n_rows * D / (ms * 1e-3) / 1e12
    out = {"leg": leg, "n_q": n_q, "n_rows": n_rows, "D": D, "k": k, "ms": round(ms, 3), "tflops": round(tf, 2),
           "fraction_of_fp32_peak": round(tf / PEAK_TF, 3)}
    out.update(more)
    print(json.dumps(out), flush=True)


def neighbour_legs(name, X, n_q, ks, metrics, reps, compare=True):
    n_rows, D = X.shape
    queries = torch.arange(n_q, device=DEV, dtype=torch.int64) * (n_rows // n_q)

    def search(fold, k):
        for s in range(0, n_q, CHUNK):
            ops.neighbours_topk(fold, n_rows, D, queries[s:s + CHUNK], k)

    fold_ms = {m: timed(lambda: ops.neighbour_fold(X, n_rows, D, m == "cosine"), max(reps, 5)) for m in metrics}
    got = {}
    for k in ks:
        for m in metrics:
            ms = timed(lambda: search(ops.neighbour_fold(X, n_rows, D, m == "cosine"), k), reps)
            got.setdefault(k, (m, ms))
            line(f"{name}_{m}_k{k}", n_q, n_rows, D, k, ms, metric=m, fold_ms=round(fold_ms[m], 4))
    if not compare:
        return
    # the same kernel without the exclusion path: the query rows as a user table of n_q rows, constants zero
    U = X if n_q == n_rows else X[queries].contiguous()
    zu = torch.zeros(U.shape[0], 1, device=DEV)
    zi = torch.zeros(n_rows, 1, device=DEV)
    T, keep = ops.make_tables(U, X, zu, zi)
    users = torch.arange(n_q, device=DEV, dtype=torch.int64)
    ifold_ms = timed(lambda: ops.item_fold("linear", T, n_rows, D, DEV), max(reps, 5))
    for m in metrics:
        line(f"{name}_item_fold", 0, n_rows, D, 0, ifold_ms, compared_with=f"{name}_{m} fold",
             neighbour_fold_over_item_fold=round(fold_ms[m] / ifold_ms, 3))
    for k in ks:
        def run():
            fold = ops.item_fold("linear", T, n_rows, D, DEV)
            for s in range(0, n_q, CHUNK):
                ops.retrieve_topk("linear", T, fold, users[s:s + CHUNK], k)
        ms = timed(run, reps)
        line(f"{name}_retrieve_k{k}", n_q, n_rows, D, k, ms, seen=False, compared_with=f"{name}_{got[k][0]}_k{k}",
             neighbours_over_retrieve=round(got[k][1] / ms, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="c2,c4,users")
    legs = ap.parse_args().legs.split(",")
    if "c2" in legs:
        neighbour_legs("c2_items", rows(100_000, 64, 1), 100_000, (10, 100), ("dot", "cosine"), reps=5)
    if "c4" in legs:
        neighbour_legs("c4_items", rows(1_000_000, 128, 2), 1_000_000, (10, 100), ("dot", "cosine"), reps=1)
    if "users" in legs:
        neighbour_legs("c2_users", rows(1_000_000, 64, 3), 262_144, (10,), ("cosine",), reps=2)


if __name__ == "__main__":
    main()
