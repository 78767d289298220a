# -*- coding: utf-8 -*-
"""MMR re-ranking (csrc/rerank.hip mmr_rerank_kernel, TorchRecSys.recommend_diverse) at the c2 and c4 shapes, beside the
fused top-k that produces its candidate pool.

  c2: FM, 1M users x 100K items, D = 64      c4: FM, 10M users x 1M items, D = 128
  4 096 and 65 536 query users, pool N = 128, k in {10, 50}, lambda = 0.3, cosine rows, no seen CSR

One JSON line per (case, users, k): device-event ms, median and minimum of 7 after one warm-up call, of
  rerank_ms   the trs_mmr_rerank launch alone (pool, neighbour fold and outputs already on the device)
  pool_ms     trs_retrieve_topk at k = N on the same users (its tile launch and its merge): what the pool cost
  nfold_ms    trs_neighbour_fold of the item side (once per recommend_diverse call, whatever the number of users)
the legs alternating within each repetition; rerank_over_pool = rerank_ms / pool_ms (medians); per user the rerank is
k - 1 steps of N * Dp multiply-adds: gfma_per_s = n_q * (k - 1) * N * Dp / rerank_ms; moved_share = the share of list
positions that differ from the pool's first k.
Usage: python tools/mmr_bench.py [--legs c2,c4] [--out profiles/mmr_bench_c2_c4.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchrecsys_amd import ops  # noqa: E402
from retrieval_bench import DEV, tables  # noqa: E402

REPS = 7
N = 128
LAMBDA = 0.3


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def leg(name, T, keep, fold, n_users, n_items, D, n_q, out):
    users = torch.arange(n_q, device=DEV, dtype=torch.int64) * (n_users // n_q)
    item_rows = keep[1]

    def pool():
        return ops.retrieve_topk("fm", T, fold, users, N)

    def nfold():
        return ops.neighbour_fold(item_rows, n_items, D, True)

    pids, pscores, _ = pool()  # warm-up; the pool the rerank legs read
    nf = nfold()
    Dp = ops.fold_rows(nf, n_items).shape[1]
    for k in (10, 50):
        def rerank():
            return ops.mmr_rerank(nf, n_items, D, pids, pscores, k, LAMBDA)

        want = rerank()[0].clone()  # warm-up
        torch.cuda.synchronize()
        t = {"rerank": [], "pool": [], "nfold": []}
        for _ in range(REPS):
            t["rerank"].append(timed(rerank))
            t["pool"].append(timed(pool))
            t["nfold"].append(timed(nfold))
        assert torch.equal(rerank()[0], want), "trs_mmr_rerank is not deterministic"
        med = {x: statistics.median(v) for x, v in t.items()}
        rec = {"leg": f"{name}_q{n_q}_k{k}", "n_q": n_q, "n_items": n_items, "D": D, "Dp": Dp, "N": N, "k": k,
               "lambda": LAMBDA}
        for x in t:
            rec[f"{x}_ms"] = round(med[x], 3)
            rec[f"{x}_ms_min"] = round(min(t[x]), 3)
        rec.update({"rerank_over_pool": round(med["rerank"] / med["pool"], 4),
                    "gfma_per_s": round(n_q * (k - 1) * N * Dp / (med["rerank"] * 1e-3) / 1e9, 1),
                    "moved_share": round(float((want != pids[:, :k]).float().mean()), 3)})
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
            T, keep = tables(n_users, n_items, D, 1)
            fold = ops.item_fold("fm", T, n_items, D, DEV)
            for n_q in (4096, 65_536):
                leg(name, T, keep, fold, n_users, n_items, D, n_q, a.out)
            del T, keep, fold


if __name__ == "__main__":
    main()
