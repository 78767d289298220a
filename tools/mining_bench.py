# -*- coding: utf-8 -*-
"""Score-aware hard-negative mining (neg_sampling={'mine': 'hardest'}: csrc/mine.hip, trs_batch_prepare_mined) at the
table shapes of the benchmark configurations, FM scorer, no metadata, uniform random interaction stream (seeded).

  c2: 1M users x 100K items, D = 64, B = 65 536        c4: 10M users x 1M items, D = 128, B = 32 768

Per shape, one JSON line per leg:
  launch   the mining launch alone for K in --ks, next to the yardstick — the north-star scoring pass
           (trs_score_forward) on the same tables, the same epoch positions and B — timed in one process with the legs
           alternating, one pair of device events around every launch after warm-up, fresh epoch positions every
           repetition.  us per launch (median), algorithmic bytes per second and share of the 8 TB/s HBM peak:
             mining  8 + (4D+4) + K (1+M) (4D+4) + 4 K M + 12 bytes per triple,    pass  16 + 3 (4D+4) + 8,
           and `rate_vs_pass` = the mining launch's byte rate over the pass's (target >= 0.8).  top = 1; one more
           leg, K = 8 with top = 2, shows what the rank selection and the second draw of the chosen candidate cost.
  step     --steps whole training steps, plain SGD: mined (mining launch + the step, K = 8) and, for what leaving the
           slice-ahead path costs by itself, the same per-step loop unmined (trs_batch_prepare + the step); us per step
           from device events around the window.  The unmined step on its own fast path is bench.py's figure.
Usage: python tools/mining_bench.py [--legs c2,c4] [--ks 4,8,16] [--reps 40] [--steps 200]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchrecsys_amd import ops  # noqa: E402

PEAK_GBS = 8000.0
DEV = "cuda:0"
SHAPES = {"c2": (1_000_000, 100_000, 64, 65536), "c4": (10_000_000, 1_000_000, 128, 32768)}
WINDOWS = 64  # distinct batches of epoch positions in the stream


def mine_bytes(D, K, M=0):
    return 8 + (4 * D + 4) + K * (1 + M) * (4 * D + 4) + 4 * K * M + 12


def pass_bytes(D, R=3):
    return 16 + R * (4 * D + 4) + 8


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
    samplers = {K: ops.Sampler(mine="hardest", candidates=K) for K in Ks}
    samplers["8top2"] = ops.Sampler(mine="hardest", candidates=8, top=2)
    Ks = list(Ks) + ["8top2"]
    outs = {K: None for K in Ks}
    key, seed = 0x5EED1234, 77
    pos = torch.empty(B, device=DEV)
    neg = torch.empty(B, device=DEV)
    lib = ops._lib.load()
    import ctypes as C

    def mined(K, t0):
        outs[K] = ops.batch_prepare_mined(su, si, key, t0, B, NI, seed, t0, "fm", T, samplers[K], out=outs[K])

    base = None

    def prepare(t0):
        nonlocal base
        base = ops.batch_prepare(su, si, None, key, t0, B, NI, seed, t0, out=base)
        return ops.make_batch(base["user"], base["pos"], base["neg"])

    def score(Bt):
        ops.check(lib.trs_score_forward(ops.NET_ID["fm"], C.byref(T), C.byref(Bt), ops.ptr(pos), ops.ptr(neg),
                                        ops._stream()), "trs_score_forward")

    for w in range(3):  # warm-up: every kernel of the timed window
        for K in Ks:
            mined(K, w * B)
        Bt, keep = prepare(w * B)
        score(Bt)
    torch.cuda.synchronize()
    ev = {leg: [] for leg in list(Ks) + ["pass"]}
    for r in range(reps):
        t0 = ((r + 3) % WINDOWS) * B
        Bt, keep = prepare(t0)  # untimed: the pass's ids
        for leg in list(Ks) + ["pass"]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            score(Bt) if leg == "pass" else mined(leg, t0)
            e1.record()
            ev[leg].append((e0, e1))
    torch.cuda.synchronize()
    us = {leg: [1e3 * a.elapsed_time(b) for a, b in v] for leg, v in ev.items()}
    p_us = statistics.median(us["pass"])
    p_rate = pass_bytes(D) * B / p_us / 1e3  # GB/s
    out = [{"leg": name, "kind": "pass", "B": B, "D": D, "us": round(p_us, 2), "us_min": round(min(us["pass"]), 2),
            "bytes_per_triple": pass_bytes(D), "gb_per_s": round(p_rate, 1), "frac_hbm_peak": round(p_rate / PEAK_GBS, 3)}]
    for leg in Ks:
        K, top = (8, 2) if leg == "8top2" else (leg, 1)
        m_us = statistics.median(us[leg])
        rate = mine_bytes(D, K) * B / m_us / 1e3
        out.append({"leg": name, "kind": "mine", "K": K, "top": top, "B": B, "D": D, "us": round(m_us, 2),
                    "us_min": round(min(us[leg]), 2), "bytes_per_triple": mine_bytes(D, K), "gb_per_s": round(rate, 1),
                    "frac_hbm_peak": round(rate / PEAK_GBS, 3), "rate_vs_pass": round(rate / p_rate, 3)})
    return out


def step_legs(name, net, su, si, steps, K=8):
    from torchrecsys_amd.engine import SparseScorerTrainer
    NU, NI, D, B = SHAPES[name]
    tr = SparseScorerTrainer(net, torch.optim.SGD(net.parameters(), lr=0.01), B)
    sampler = ops.Sampler(mine="hardest", candidates=K)
    loss = torch.zeros(1, device=DEV)
    key, seed = 0x5EED1234, 78
    state = {"out": None}

    def run(mining, n):
        for s in range(n):
            t0 = (s % WINDOWS) * B
            if mining:
                ids = ops.batch_prepare_mined(su, si, key, t0, B, NI, seed, t0, "fm", net.tables(), sampler,
                                              out=state["out"])
            else:
                ids = ops.batch_prepare(su, si, None, key, t0, B, NI, seed, t0, out=state["out"])
            state["out"] = ids
            tr.step(ids, loss)

    res = []
    for mining in (True, False, True, False):  # alternating windows
        run(mining, 8)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(mining, steps)
        e1.record()
        torch.cuda.synchronize()
        res.append((mining, 1e3 * e0.elapsed_time(e1) / steps))
    tr.check_errors()
    m = min(v for k, v in res if k)
    u = min(v for k, v in res if not k)
    return [{"leg": name, "kind": "step", "B": B, "D": D, "K": K, "steps": steps, "mined_step_us": round(m, 2),
             "unmined_per_step_loop_us": round(u, 2), "windows_us": [[int(k), round(v, 2)] for k, v in res]}]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--legs", default="c2,c4")
    ap.add_argument("--ks", default="4,8,16")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--steps", type=int, default=200, help="0: skip the whole-step legs")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mining_bench.py measures on the MI355X: no GPU found")
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
