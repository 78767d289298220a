# -*- coding: utf-8 -*-
"""Training on K sampled negatives per positive (fit(n_negatives=K) / fit(loss='sampled_softmax'): csrc/multineg.hip,
trs_batch_prepare_multi + trs_score_multi_fwd_bwd) at the table shapes of the benchmark configurations, FM scorer, no
metadata, uniform random interaction stream (seeded).

  c2: 1M users x 100K items, D = 64, B = 65 536        c4: 10M users x 1M items, D = 128, B = 32 768

Per shape, one JSON line per leg:
  launch   the staging kernel alone for K in --ks and both loss families (sampled softmax, mean of K hinge pairs), next
           to the yardstick — trs_score_fwd_bwd (one negative) on the same tables, the same epoch positions and B —
           timed in one process with the legs alternating, one pair of device events around every launch after warm-up,
           fresh epoch positions every repetition; the ids of every leg are prepared outside the timed interval.  us per
           launch (median), algorithmic bytes per second and share of the 8 TB/s HBM peak:
             multi  8 + 4 K + (2 + K) (4D+4) read + (2 + K) (4D+4) written per row,
             pair   16 + 3 (4D+4) read + 3 (4D+4) written,
           and `rate_vs_pair` = the kernel's byte rate over the yardstick's (target >= 0.8 at K = 8).  The prepare
           launch (trs_batch_prepare_multi) is timed the same way, on its own line.
  step     --steps whole training steps, plain SGD, K = 8: prepare launch + staging kernel + per-table row updates for
           both loss families, next to the per-step-loop hinge step (trs_batch_prepare + the step) and the mined step
           (trs_batch_prepare_mined, 8 candidates + the step); us per step from device events around the window.
Usage: python tools/multineg_bench.py [--legs c2,c4] [--ks 4,8,16] [--reps 40] [--steps 200]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchrecsys_amd import _lib, ops  # noqa: E402

PEAK_GBS = 8000.0
DEV = "cuda:0"
SHAPES = {"c2": (1_000_000, 100_000, 64, 65536), "c4": (10_000_000, 1_000_000, 128, 32768)}
WINDOWS = 64  # distinct batches of epoch positions in the stream
FAMILIES = {"sampled_softmax": _lib.LOSS_SAMPLED_SOFTMAX, "hinge": _lib.LOSS_ID["hinge"]}


def multi_bytes(D, K):
    return 8 + 4 * K + 2 * (2 + K) * (4 * D + 4)


def pair_bytes(D):
    return 16 + 6 * (4 * D + 4)


def build(name):
    from torchrecsys_amd.collaborative.fm import FM
    NU, NI, D, B = SHAPES[name]
    g = torch.Generator(device=DEV)
    g.manual_seed(B)
    net = FM(1, 1, {}, D, use_metadata=False)  # tables drawn on the device (a host init of c4 takes minutes)
    for mod, n, w in ((net.user, NU, D), (net.item, NI, D), (net.linear_user, NU, 1), (net.linear_item, NI, 1)):
        mod.weight = torch.nn.Parameter(torch.randn(n, w, device=DEV, generator=g) * 0.1)
    net.n_users, net.n_items = NU, NI
    N = WINDOWS * B
    su = torch.randint(0, NU, (N,), device=DEV, dtype=torch.int32, generator=g)
    si = torch.randint(0, NI, (N,), device=DEV, dtype=torch.int32, generator=g)
    return net, su, si


def launch_legs(name, net, su, si, Ks, reps):
    NU, NI, D, B = SHAPES[name]
    T = net.tables()
    key, seed, tau = 0x5EED1234, 77, 0.5
    Kmax = max(Ks)
    F = ops.multineg_fields(Kmax, 0)
    gr = torch.empty(F * B * D, dtype=torch.float32, device=DEV)
    gl = torch.empty(F * B, dtype=torch.float32, device=DEV)
    pgr = torch.empty((3, B, D), dtype=torch.float32, device=DEV)
    pgl = torch.empty((3, B), dtype=torch.float32, device=DEV)
    loss = torch.zeros(1, device=DEV)
    ids = {K: None for K in Ks}
    legs = [(K, fam) for K in Ks for fam in FAMILIES]

    def prepare(K, t0):
        ids[K] = ops.batch_prepare_multi(su, si, key, t0, B, NI, seed, t0, K, out=ids[K])

    def multi(K, fam):
        Fk = ops.multineg_fields(K, 0)
        ops.score_multi_fwd_bwd("fm", T, ids[K]["user"], ids[K]["items"], None, FAMILIES[fam], tau, loss, None,
                                gr[:Fk * B * D].view(Fk, B, D), gl[:Fk * B].view(Fk, B))

    def pair():
        i = ids[Ks[0]]
        Bt, keep = ops.make_batch(i["user"], i["pos"], i["neg"])
        ops.score_fwd_bwd("fm", T, Bt, B, D, 0, DEV, loss, None, want_scores=False, grad_rows=pgr, grad_lin=pgl)

    def timed(fn, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(*a)
        e1.record()
        return e0, e1

    for w in range(3):  # warm-up: every kernel of the timed window
        for K in Ks:
            prepare(K, w * B)
        for K, fam in legs:
            multi(K, fam)
        pair()
    torch.cuda.synchronize()
    ev = {leg: [] for leg in legs + ["pair"] + [("prepare", K) for K in Ks]}
    for r in range(reps):
        t0 = ((r + 3) % WINDOWS) * B
        for K in Ks:
            ev[("prepare", K)].append(timed(prepare, K, t0))
        for leg in legs + ["pair"]:
            ev[leg].append(timed(pair) if leg == "pair" else timed(multi, *leg))
    torch.cuda.synchronize()
    us = {leg: [1e3 * a.elapsed_time(b) for a, b in v] for leg, v in ev.items()}
    p_us = statistics.median(us["pair"])
    p_rate = pair_bytes(D) * B / p_us / 1e3  # GB/s
    out = [{"leg": name, "kind": "pair", "B": B, "D": D, "us": round(p_us, 2), "us_min": round(min(us["pair"]), 2),
            "bytes_per_row": pair_bytes(D), "gb_per_s": round(p_rate, 1), "frac_hbm_peak": round(p_rate / PEAK_GBS, 3)}]
    for K, fam in legs:
        m_us = statistics.median(us[(K, fam)])
        rate = multi_bytes(D, K) * B / m_us / 1e3
        out.append({"leg": name, "kind": "multi", "loss": fam, "K": K, "B": B, "D": D, "us": round(m_us, 2),
                    "us_min": round(min(us[(K, fam)]), 2), "bytes_per_row": multi_bytes(D, K),
                    "gb_per_s": round(rate, 1), "frac_hbm_peak": round(rate / PEAK_GBS, 3),
                    "rate_vs_pair": round(rate / p_rate, 3)})
    for K in Ks:
        q = us[("prepare", K)]
        out.append({"leg": name, "kind": "prepare", "K": K, "B": B, "us": round(statistics.median(q), 2),
                    "us_min": round(min(q), 2)})
    return out


def step_legs(name, net, su, si, steps, K=8):
    from torchrecsys_amd.engine import SparseScorerTrainer
    NU, NI, D, B = SHAPES[name]
    tr = SparseScorerTrainer(net, torch.optim.SGD(net.parameters(), lr=0.01), B)
    miner = ops.Sampler(mine="hardest", candidates=K)
    loss = torch.zeros(1, device=DEV)
    key, seed = 0x5EED1234, 78
    state = {"multi": None, "pair": None}

    def run(kind, n):
        for s in range(n):
            t0 = (s % WINDOWS) * B
            if kind in FAMILIES:
                tr.multineg = (K, FAMILIES[kind], 0.5)
                ids = state["multi"] = ops.batch_prepare_multi(su, si, key, t0, B, NI, seed, t0, K, out=state["multi"])
                tr.multineg_step(ids, loss)
                continue
            if kind == "mined":
                ids = ops.batch_prepare_mined(su, si, key, t0, B, NI, seed, t0, "fm", net.tables(), miner,
                                              out=state["pair"])
            else:
                ids = ops.batch_prepare(su, si, None, key, t0, B, NI, seed, t0, out=state["pair"])
            state["pair"] = ids
            tr.step(ids, loss)

    kinds = list(FAMILIES) + ["mined", "hinge_one_negative"]
    res = {k: [] for k in kinds}
    for kind in kinds + kinds:  # alternating windows
        run(kind, 8)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(kind, steps)
        e1.record()
        torch.cuda.synchronize()
        res[kind].append(1e3 * e0.elapsed_time(e1) / steps)
    tr.check_errors()
    return [{"leg": name, "kind": "step", "B": B, "D": D, "K": K, "steps": steps,
             "step_us": {k: round(min(v), 2) for k, v in res.items()},
             "windows_us": {k: [round(x, 2) for x in v] for k, v in res.items()}}]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--legs", default="c2,c4")
    ap.add_argument("--ks", default="4,8,16")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--steps", type=int, default=200, help="0: skip the whole-step legs")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multineg_bench.py measures on the MI355X: no GPU found")
    Ks = [int(x) for x in a.ks.split(",")]
    for name in a.legs.split(","):
        net, su, si = build(name)
        for line in launch_legs(name, net, su, si, Ks, a.reps):
            print(json.dumps(line), flush=True)
        if a.steps > 0:
            for line in step_legs(name, net, su, si, a.steps):
                print(json.dumps(line), flush=True)
        del net, su, si
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
