# -*- coding: utf-8 -*-
"""Item kNN (csrc/knn.hip; TorchRecSys.fit_itemknn): 1 000 000 users, history lengths log-normal (median 20, sigma 1),
capped at 1 000, at least 1, items uniform (the data of tools/ease_bench.py); K = 100, cosine, no shrinkage.

One JSON line per size, device events, median (and minimum) of the repetitions after one warm-up:
  build_ms                      trs_knn_build over the two CSRs of the distinct pairs: one LDS integer add per ordered
                                pair of a user's items (pairs_of_items), the same increments trs_ease_gram performs
  ease_gram_ms / build_over_gram
                                at n_items <= TRS_EASE_NMAX: trs_ease_gram on the same CSR in the same session (fp64
                                atomics into an n^2 matrix in memory) and the ratio build_ms / ease_gram_ms.  The
                                yardstick is a ratio <= 1.0; it is reported whichever way it falls.
  count_ms_folded_to_one_tile / tiles_ms
                                beyond one column tile, the two terms of the build apart: the same pairs with the item
                                ids folded into ONE tile (id mod TRS_KNN_TILE; folded_pairs_of_items increments, a few
                                less than pairs_of_items where two of a user's items fold together) run the same kernel
                                without a tile loop: no segment search, no cursor, one selection pass per item.  That is
                                the counting term; tiles_ms = build_ms - it is what the tile loop adds (finding every
                                user's segment of every tile, the barriers and the selection pass per tile).
  scores_ms                     trs_knn_scores for 4 096 users (the first of the CSR), with the bytes it writes as a
                                fraction of the 8 TB/s HBM peak; beside it ease_scores_ms where EASE runs (a B of ones:
                                the time does not depend on the values)
Usage: python tools/itemknn_bench.py [--sizes 16384,24576,100000,1000000] [--reps 3] [--out profiles/itemknn_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchrecsys_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"
HBM_TBS = 8.0
N_USERS, N_SCORE_USERS, K, KIND = 1_000_000, 4096, 100, "cosine"


def pairs(n_users, n_items, seed):
    """(user, item) int32 streams on the GPU: log-normal history lengths, uniform items (repeats collapse later)."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    lens = torch.empty(n_users, device=DEV).log_normal_(mean=float(torch.log(torch.tensor(20.0))), std=1.0, generator=g)
    lens = lens.round().clamp_(1, 1000).long()
    user = torch.repeat_interleave(torch.arange(n_users, device=DEV, dtype=torch.int32), lens)
    item = torch.randint(0, n_items, (user.numel(),), device=DEV, generator=g, dtype=torch.int32)
    return user, item


def times(fn, reps):
    """Event times of fn() in ms after one warm-up."""
    out = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r:
            out.append(e0.elapsed_time(e1))
    return out


def med(ts):
    return round(statistics.median(ts), 3)


def run_size(n, reps):
    user, item = pairs(N_USERS, n, 2)
    seen = ops.Sampler.seen_csr(user, item, N_USERS, n)
    inv = ops.Sampler.seen_csr(item, user, n, N_USERS)
    lens = seen[0][1:] - seen[0][:-1]
    deg = inv[0][1:] - inv[0][:-1]
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    tiles = -(-n // _lib.KNN_TILE)
    line = {"n_items": n, "n_users": N_USERS, "K": K, "similarity": KIND, "column_tiles": tiles,
            "pairs": int(seen[1].numel()), "pairs_of_items": int((lens * lens).sum()),
            "longest_history": int(lens.max()), "most_users_of_an_item": int(deg.max()),
            "items_with_more_users_than_threads": int((deg > 512).sum())}

    t = times(lambda: ops.knn_build(seen, inv, n, KIND, 0.0, K, err), reps)
    line["build_ms"], line["build_ms_min"] = med(t), round(min(t), 3)
    ids, w = ops.knn_build(seen, inv, n, KIND, 0.0, K, err)
    line["neighbour_slots_filled"] = round(float((ids >= 0).float().mean()), 4)

    if n <= _lib.EASE_NMAX:
        t = times(lambda: ops.ease_gram(seen, n, 500.0, err), reps)
        line["ease_gram_ms"], line["ease_gram_ms_min"] = med(t), round(min(t), 3)
        line["build_over_gram"] = round(line["build_ms"] / line["ease_gram_ms"], 4)
        torch.cuda.empty_cache()

    if tiles > 1:  # the same pairs with the item ids folded into one column tile: the counting term alone
        nf = _lib.KNN_TILE
        seen_f = ops.Sampler.seen_csr(user, item % nf, N_USERS, nf)
        inv_f = ops.Sampler.seen_csr(item % nf, user, nf, N_USERS)
        lf = seen_f[0][1:] - seen_f[0][:-1]
        t = times(lambda: ops.knn_build(seen_f, inv_f, nf, KIND, 0.0, K, err), reps)
        line["count_ms_folded_to_one_tile"] = med(t)
        line["folded_pairs_of_items"] = int((lf * lf).sum())
        line["tiles_ms"] = round(line["build_ms"] - line["count_ms_folded_to_one_tile"], 3)
        del seen_f, inv_f
    del user, item

    rows = torch.arange(N_SCORE_USERS, dtype=torch.int64, device=DEV)
    t = times(lambda: ops.knn_scores(ids, w, seen, rows), reps)
    nbytes = N_SCORE_USERS * n * 4
    line["scores_users"] = N_SCORE_USERS
    line["scores_ms"], line["scores_ms_min"] = med(t), round(min(t), 3)
    line["scores_written_GB"] = round(nbytes / 1e9, 3)
    line["scores_fraction_of_8TBs_hbm_peak"] = round(nbytes / (statistics.median(t) * 1e-3) / 1e12 / HBM_TBS, 3)
    if n <= _lib.EASE_NMAX:
        B = torch.ones((n, n), dtype=torch.float32, device=DEV)
        t = times(lambda: ops.ease_scores(B, seen, rows), reps)
        line["ease_scores_ms"] = med(t)
        del B
    assert int(err.item()) == 0
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16384,24576,100000,1000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for n in (int(v) for v in a.sizes.split(",")):
        line = json.dumps(run_size(n, a.reps))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
