# -*- coding: utf-8 -*-
"""EASE (csrc/ease.hip; TorchRecSys.fit_ease) at n_items in {4 096, 16 384, 24 576}: 1 000 000 users, history lengths
log-normal (median 20, sigma 1), capped at 1 000, at least 1, items uniform; the distinct pairs are the training data
(ops.Sampler.seen_csr, as fit_ease takes them), lambda = 500.

One JSON line per size, device events, median (and minimum) of the repetitions after one warm-up:
  gram_ms                       trs_ease_gram: one fp64 atomic add per ordered pair of a user's items (pairs_of_items)
  factor_ms / triangular_inverse_ms / product_ms
                                the three phases of trs_ease_invert, each alone (knob EASE_STAGES = 1 / 2 / 4 on the
                                same matrix and workspace, in this order: together one inversion), nbar^3 / 3 flop
                                each, with the achieved TFLOP/s and its fraction of the fp64 matrix peak.  That peak,
                                78.6 TFLOP/s, is the datasheet's figure: nobody has measured it on this project's machines.
  invert_ms                     the whole call (EASE_STAGES = 7)
  weights_ms                    trs_ease_weights
  residual_max_abs_AP_minus_I   max |A P - I| over the padded matrices, the product in fp64 by torch.matmul (the
                                vendor's GEMM, used by this tool only): the one place where offsets beyond 4 GiB (fp64
                                from n = 16 384 on, B at 24 576 is 2.4 GB) are exercised
  scores_ms                     trs_ease_scores for 4 096 users (the first of the CSR), with its algorithmic bytes (the
                                rows of B their histories list, plus the rows written) as a fraction of the 8 TB/s HBM peak
  topk_ms_per_row               trs_topk on one score row: what the generic path of recommend() adds per user
The n = 4 096 line also carries numpy.linalg.inv on the same A on the CPU threads the process may use, once.
Usage: python tools/ease_bench.py [--sizes 4096,16384,24576] [--reps 3] [--out profiles/ease_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchrecsys_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"
FP64_MATRIX_TFLOPS = 78.6  # datasheet, not measured here
HBM_TBS = 8.0
N_USERS, N_SCORE_USERS, LAMBDA = 1_000_000, 4096, 500.0


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
    """Event times of fn() in ms after one warm-up; before() runs outside the events."""
    out = []
    for r in range(reps + 1):
        if before is not None:
            before()
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
    del user, item
    lens = seen[0][1:] - seen[0][:-1]
    nbar = ops.ease_padded(n)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    line = {"n_items": n, "nbar": nbar, "n_users": N_USERS, "pairs": int(seen[1].numel()),
            "pairs_of_items": int((lens * lens).sum()), "longest_history": int(lens.max()), "lambda": LAMBDA}

    t = times(lambda: ops.ease_gram(seen, n, LAMBDA, err), reps)
    line["gram_ms"], line["gram_ms_min"] = med(t), round(min(t), 3)
    A0 = ops.ease_gram(seen, n, LAMBDA, err)
    A = torch.empty_like(A0)
    ws = torch.empty(_lib.load().trs_ease_invert_workspace_bytes(n), dtype=torch.uint8, device=DEV)

    phase = {1: [], 2: [], 4: []}
    for r in range(reps + 1):  # the three phases in order on the same buffers: one inversion per repetition
        A.copy_(A0)
        for stages in (1, 2, 4):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with _lib.tuning(EASE_STAGES=stages):
                e0.record()
                ops.ease_invert(A, err, ws)
                e1.record()
            torch.cuda.synchronize()
            if r:
                phase[stages].append(e0.elapsed_time(e1))
    flop = nbar ** 3 / 3.0
    for stages, name in ((1, "factor"), (2, "triangular_inverse"), (4, "product")):
        ms = statistics.median(phase[stages])
        tf = flop / (ms * 1e-3) / 1e12
        line[f"{name}_ms"] = round(ms, 3)
        line[f"{name}_TFLOPs"] = round(tf, 2)
        line[f"{name}_fraction_of_datasheet_fp64_matrix_peak_78.6"] = round(tf / FP64_MATRIX_TFLOPS, 3)
    t = times(lambda: ops.ease_invert(A, err, ws), reps, before=lambda: A.copy_(A0))
    line["invert_ms"], line["invert_ms_min"] = med(t), round(min(t), 3)
    tf = 3 * flop / (statistics.median(t) * 1e-3) / 1e12
    line["invert_TFLOPs"] = round(tf, 2)
    line["invert_fraction_of_datasheet_fp64_matrix_peak_78.6"] = round(tf / FP64_MATRIX_TFLOPS, 3)
    assert int(err.item()) == 0, "a pivot was not positive"

    R = torch.matmul(A0, A)  # A holds P
    R.diagonal().sub_(1.0)
    line["residual_max_abs_AP_minus_I"] = float(R.abs().max())
    line["asymmetry_max_abs_P_minus_Pt"] = float((A - A.t()).abs().max())
    del R

    if n == 4096:  # the CPU baseline, once
        a = A0[:n, :n].cpu().numpy()
        t0 = time.perf_counter()
        p = np.linalg.inv(a)
        line["numpy_inv_s"] = round(time.perf_counter() - t0, 3)
        line["numpy_inv_threads"] = int(os.environ.get("OMP_NUM_THREADS", 0)) or torch.get_num_threads()
        line["max_abs_P_minus_numpy"] = float(np.abs(A[:n, :n].cpu().numpy() - p).max())
        del a, p

    t = times(lambda: ops.ease_weights(A, n), reps)
    line["weights_ms"] = med(t)
    B = ops.ease_weights(A, n)
    del A, A0, ws

    rows = torch.arange(N_SCORE_USERS, dtype=torch.int64, device=DEV)
    t = times(lambda: ops.ease_scores(B, seen, rows), reps)
    nbytes = (int(lens[:N_SCORE_USERS].sum()) + N_SCORE_USERS) * n * 4
    line["scores_users"] = N_SCORE_USERS
    line["scores_ms"], line["scores_ms_min"] = med(t), round(min(t), 3)
    line["scores_algorithmic_GB"] = round(nbytes / 1e9, 3)
    line["scores_fraction_of_8TBs_hbm_peak"] = round(nbytes / (statistics.median(t) * 1e-3) / 1e12 / HBM_TBS, 3)
    out = ops.ease_scores(B, seen, rows[:16])
    t = times(lambda: [ops.topk(out[r], 10) for r in range(16)], reps)
    line["topk_ms_per_row"] = round(statistics.median(t) / 16, 4)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,24576")
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
