# -*- coding: utf-8 -*-
"""WARP (fit(loss='warp'): csrc/multineg.hip warp_kernel, trs_score_warp_fwd_bwd) at the table shapes of the benchmark
configurations, FM scorer, no metadata, seeded.

  c2: 1M users x 100K items, D = 64, B = 65 536        c4: 10M users x 1M items, D = 128, B = 32 768

Two regimes bound the kernel's early exit.  The tables are at their initialisation (N(0, 0.1)) but for the 1-wide term of
the even items, raised by 100; positives are even items, candidates odd ones, both uniform over the whole table.  Then
z(u,p) - z(u,c) is about 100 for every pair, and the margin alone picks the regime:
  all_violate   margin 200: every row violates at c_0 — a wave reads one round and stages its three fields;
  no_violator   margin 1: no candidate violates — a wave reads all K candidates and stages zeros.
Per shape, one JSON line per leg:
  launch   warp_kernel alone for K in --ks in both regimes, next to its yardsticks on the same tables and the same id
           blocks: trs_score_multi_fwd_bwd with the hinge at the same K (reads the same rows, stages 2 + K fields) and
           trs_score_fwd_bwd on (user, positive, c_0) (the K = 1 pair kernel).  One process, the legs alternating, one
           pair of device events around every launch after warm-up, a fresh id block every repetition, ids prepared
           outside the timed interval.  us per launch: median, minimum, quartiles.  `vs_multi_hinge_us` is the no-violator
           median minus the yardstick's; `yardstick_iqr_us` the spread (interquartile range) of the yardstick's own
           repetitions in this run, the margin the expectation "no slower than the yardstick" is allowed.
  step     --steps whole K = 8 SGD steps (the prepare launch + warp_kernel + the fused row update) in both regimes, next
           to the K = 8 steps of DESIGN 4.8 (mean of hinge pairs, sampled softmax), the mined step of 4.7 (8 candidates)
           and the per-step-loop hinge step; us per step from device events around the window.  The WARP and K-negative
           steps train on the prepared id blocks above (their prepare launch runs too, into a buffer of its own).
Usage: python tools/warp_bench.py [--legs c2,c4] [--ks 4,8,16] [--reps 40] [--steps 200] [--out FILE.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchrecsys_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"
SHAPES = {"c2": (1_000_000, 100_000, 64, 65536), "c4": (10_000_000, 1_000_000, 128, 32768)}
WINDOWS = 16  # distinct id blocks per K
REGIMES = {"all_violate": 200.0, "no_violator": 1.0}  # margin
HINGE = _lib.LOSS_ID["hinge"]


def build(name):
    from torchrecsys_amd.collaborative.fm import FM
    NU, NI, D, B = SHAPES[name]
    g = torch.Generator(device=DEV)
    g.manual_seed(B)
    net = FM(1, 1, {}, D, use_metadata=False)  # tables drawn on the device (a host init of c4 takes minutes)
    for mod, n, w in ((net.user, NU, D), (net.item, NI, D), (net.linear_user, NU, 1), (net.linear_item, NI, 1)):
        mod.weight = torch.nn.Parameter(torch.randn(n, w, device=DEV, generator=g) * 0.1)
    with torch.no_grad():
        net.linear_item.weight[0::2] += 100.0  # the even items outrank every odd one
    net.n_users, net.n_items = NU, NI
    return net, g


def id_blocks(name, K, g):
    """WINDOWS id blocks in batch_prepare_multi's layout: positives even, candidates odd, uniform over the table."""
    NU, NI, D, B = SHAPES[name]
    out = []
    for _ in range(WINDOWS):
        user = torch.randint(0, NU, (B,), device=DEV, dtype=torch.int32, generator=g)
        items = torch.randint(0, NI // 2, (1 + K, B), device=DEV, dtype=torch.int32, generator=g) * 2
        items[1:] += 1
        out.append({"user": user, "items": items, "pos": items[0], "neg": items[1]})
    return out


def quart(v):
    q = statistics.quantiles(v, n=4)
    return {"us": round(statistics.median(v), 2), "us_min": round(min(v), 2), "us_q1": round(q[0], 2),
            "us_q3": round(q[2], 2)}


def launch_legs(name, net, g, Ks, reps):
    NU, NI, D, B = SHAPES[name]
    T = net.tables()
    Kmax = max(Ks)
    F = ops.multineg_fields(Kmax, 0)
    gr = torch.empty(F * B * D, dtype=torch.float32, device=DEV)
    gl = torch.empty(F * B, dtype=torch.float32, device=DEV)
    pgr = torch.empty((3, B, D), dtype=torch.float32, device=DEV)
    pgl = torch.empty((3, B), dtype=torch.float32, device=DEV)
    neg = torch.empty(B, dtype=torch.int32, device=DEV)
    loss = torch.zeros(1, device=DEV)
    blocks = {K: id_blocks(name, K, g) for K in Ks}
    weights = {K: ops.warp_rank_weights(NI, K, "log", DEV) for K in Ks}

    def warp(K, regime, w):
        i = blocks[K][w]
        ops.score_warp_fwd_bwd("fm", T, i["user"], i["items"], None, REGIMES[regime], weights[K], loss, None, neg, None,
                               None, pgr, pgl, want_trials=False)

    def multi(K, w):
        i = blocks[K][w]
        Fk = ops.multineg_fields(K, 0)
        ops.score_multi_fwd_bwd("fm", T, i["user"], i["items"], None, HINGE, 1.0, loss, None,
                                gr[:Fk * B * D].view(Fk, B, D), gl[:Fk * B].view(Fk, B))

    def pair(K, w):
        i = blocks[K][w]
        Bt, keep = ops.make_batch(i["user"], i["pos"], i["neg"])
        ops.score_fwd_bwd("fm", T, Bt, B, D, 0, DEV, loss, None, want_scores=False, grad_rows=pgr, grad_lin=pgl)

    legs = [(fn, K) for K in Ks for fn in ("all_violate", "no_violator", "multi_hinge", "pair")]

    def run(leg, w):
        fn, K = leg
        if fn in REGIMES:
            warp(K, fn, w)
        elif fn == "multi_hinge":
            multi(K, w)
        else:
            pair(K, w)

    def timed(leg, w):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(leg, w)
        e1.record()
        return e0, e1

    # the regimes are what they claim: trials all 1 / all 0
    for K in Ks:
        for regime, want in (("all_violate", 1), ("no_violator", 0)):
            i = blocks[K][0]
            tr = ops.score_warp_fwd_bwd("fm", T, i["user"], i["items"], None, REGIMES[regime], weights[K], loss,
                                        forward_only=True)[2]
            assert bool((tr == want).all()), (name, K, regime)
    for w in range(3):  # warm-up: every kernel of the timed window
        for leg in legs:
            run(leg, w)
    torch.cuda.synchronize()
    ev = {leg: [] for leg in legs}
    for r in range(reps):
        for leg in legs:
            ev[leg].append(timed(leg, (r + 3) % WINDOWS))
    torch.cuda.synchronize()
    us = {leg: [1e3 * a.elapsed_time(b) for a, b in v] for leg, v in ev.items()}
    out = []
    for K in Ks:
        y, p = quart(us[("multi_hinge", K)]), quart(us[("pair", K)])
        out.append({"leg": name, "kind": "yardstick_multi_hinge", "K": K, "B": B, "D": D, **y,
                    "yardstick_iqr_us": round(y["us_q3"] - y["us_q1"], 2)})
        out.append({"leg": name, "kind": "yardstick_pair", "K": 1, "ids_of_K": K, "B": B, "D": D, **p})
        for regime in REGIMES:
            q = quart(us[(regime, K)])
            line = {"leg": name, "kind": "warp", "regime": regime, "K": K, "B": B, "D": D, **q,
                    "vs_multi_hinge_us": round(q["us"] - y["us"], 2), "vs_pair_us": round(q["us"] - p["us"], 2)}
            if regime == "no_violator":
                line["yardstick_iqr_us"] = round(y["us_q3"] - y["us_q1"], 2)
                line["no_slower_than_yardstick_within_its_spread"] = bool(q["us"] <= y["us"] + y["us_q3"] - y["us_q1"])
            out.append(line)
    return out


def step_legs(name, net, g, steps, K=8):
    from torchrecsys_amd.engine import SparseScorerTrainer
    NU, NI, D, B = SHAPES[name]
    tr = SparseScorerTrainer(net, torch.optim.SGD(net.parameters(), lr=1e-4), B)
    miner = ops.Sampler(mine="hardest", candidates=K)
    loss = torch.zeros(1, device=DEV)
    key, seed = 0x5EED1234, 78
    N = WINDOWS * B
    su = torch.randint(0, NU, (N,), device=DEV, dtype=torch.int32, generator=g)
    si = torch.randint(0, NI // 2, (N,), device=DEV, dtype=torch.int32, generator=g) * 2
    blocks = id_blocks(name, K, g)
    weights = ops.warp_rank_weights(NI, K, "log", DEV)
    state = {"multi": None, "pair": None}
    families = {"multi_hinge": HINGE, "sampled_softmax": _lib.LOSS_SAMPLED_SOFTMAX}

    def run(kind, n):
        for s in range(n):
            t0 = (s % WINDOWS) * B
            if kind in REGIMES or kind in families:
                state["multi"] = ops.batch_prepare_multi(su, si, key, t0, B, NI, seed, t0, K, out=state["multi"])
                ids = blocks[s % WINDOWS]
                if kind in REGIMES:
                    tr.warp = (K, REGIMES[kind], weights)
                    tr.warp_step(ids, loss)
                else:
                    tr.multineg = (K, families[kind], 0.5)
                    tr.multineg_step(ids, loss)
                continue
            if kind == "mined":
                ids = ops.batch_prepare_mined(su, si, key, t0, B, NI, seed, t0, "fm", net.tables(), miner,
                                              out=state["pair"])
            else:
                ids = ops.batch_prepare(su, si, None, key, t0, B, NI, seed, t0, out=state["pair"])
            state["pair"] = ids
            tr.step(ids, loss)

    kinds = ["warp_" + r for r in REGIMES] + list(families) + ["mined", "hinge_one_negative"]
    res = {k: [] for k in kinds}
    for kind in kinds + kinds:  # alternating windows
        k_ = kind[5:] if kind.startswith("warp_") else kind
        run(k_, 8)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(k_, steps)
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
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("warp_bench.py measures on the MI355X: no GPU found")
    Ks = [int(x) for x in a.ks.split(",")]

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")

    for name in a.legs.split(","):
        net, g = build(name)
        for line in launch_legs(name, net, g, Ks, a.reps):
            emit(line)
        if a.steps > 0:
            for line in step_legs(name, net, g, a.steps):
                emit(line)
        del net
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
