# -*- coding: utf-8 -*-
"""One in-batch softmax training step (fit(loss='softmax'): csrc/softmax.hip + trs_gemm_f32) at table shapes of the
benchmark configurations.

  c2: FM, 1M users x 100K items, D = 64        c4: FM, 10M users x 1M items, D = 128
  B in {4 096, 16 384, 65 536}, plain SGD, log-Q correction on, one batch of uniform ids (seeded)

Prints one JSON line per leg: ms per step (CUDA events around --steps steps after one warm-up step), ms of the staged
loss + gradients alone (ops.InBatchSoftmax) and of the three GEMMs of it alone (the same calls on the same buffers),
TFLOP/s of 6 * B^2 * Dp GEMM flops over the GEMM time and its fraction of the 155 TF fp32 matrix peak, logit bytes
(5 passes of B^2 * 4: GEMM write, rows kernel read + write, two GEMM reads) per second of the staged part.
Usage: python tools/softmax_bench.py [--legs c2,c4] [--batches 4096,16384,65536] [--steps 5]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchrecsys_amd import ops  # noqa: E402

PEAK_TF = 155.0
DEV = "cuda:0"
SHAPES = {"c2": (1_000_000, 100_000, 64), "c4": (10_000_000, 1_000_000, 128)}


def timed(fn, steps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def leg(name, B, steps):
    from torchrecsys_amd.collaborative.fm import FM
    from torchrecsys_amd.engine import SparseScorerTrainer
    NU, NI, D = SHAPES[name]
    g = torch.Generator(device=DEV)
    g.manual_seed(B)
    net = FM(1, 1, {}, D, use_metadata=False)  # tables drawn on the device (a host init of c4 takes minutes)
    for mod, n, w in ((net.user, NU, D), (net.item, NI, D), (net.linear_user, NU, 1), (net.linear_item, NI, 1)):
        mod.weight = torch.nn.Parameter(torch.randn(n, w, device=DEV, generator=g) * 0.1)
    ids = {k: torch.randint(0, n, (B,), device=DEV, dtype=torch.int32, generator=g)
           for k, n in (("user", NU), ("pos", NI))}
    ids["neg"] = ids["pos"]
    logq = torch.full((NI,), -float(torch.log(torch.tensor(float(NI)))), device=DEV)
    tr = SparseScorerTrainer(net, torch.optim.SGD(net.parameters(), lr=0.01), B)
    tr.softmax = (0.1, logq)
    loss = torch.zeros(1, device=DEV)
    step_ms = timed(lambda: tr.softmax_step(ids, loss), steps)
    sm = tr._sm
    Bt, keep = ops.make_batch(ids["user"], ids["pos"], None, None, None, tr.err)
    T = net.tables()
    gr = tr._sm_rows[:2 * B * D].view(2, B, D)
    gl = tr._sm_lin[:2 * B].view(2, B)
    core_ms = timed(lambda: sm(net.NET, T, Bt, 0.1, logq, loss, gr, gl), steps)
    Q, K, dQ, dK = sm._mats(B)
    R = sm.chunk_rows(B)
    Dp = sm.Dp

    def gemms():
        for r0 in range(0, B, R):
            n = min(R, B - r0)
            Z = sm.z[:n * B].view(n, B)
            ops.gemm(0, 1, Q[r0:r0 + n, :Dp], K[:, :Dp], out=Z)
            ops.gemm(0, 0, Z, K[:, :Dp], out=dQ[r0:r0 + n, :Dp])
            ops.gemm(1, 0, Z, Q[r0:r0 + n], out=dK, beta=0.0 if r0 == 0 else 1.0)
    gemm_ms = timed(gemms, steps)
    tr.check_errors()
    flops = 6.0 * B * B * Dp
    logit_bytes = 5.0 * B * B * 4
    return {"leg": name, "B": B, "D": D, "chunk_rows": R, "step_ms": round(step_ms, 4),
            "loss_and_grads_ms": round(core_ms, 4), "gemm_ms": round(gemm_ms, 4),
            "gemm_tflops": round(flops / gemm_ms / 1e9, 2), "gemm_frac_peak": round(flops / gemm_ms / 1e9 / PEAK_TF, 3),
            "rest_ms": round(core_ms - gemm_ms, 4), "logit_gb_per_s": round(logit_bytes / core_ms / 1e6, 1),
            "loss": loss.item()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--legs", default="c2,c4")
    ap.add_argument("--batches", default="4096,16384,65536")
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    for name in a.legs.split(","):
        for B in (int(x) for x in a.batches.split(",")):
            print(json.dumps(leg(name, B, a.steps)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
