# -*- coding: utf-8 -*-
"""fit(l2=...) (csrc/l2.hip, trs_stage_add_l2) at the table shapes of the benchmark configurations, FM
scorer, no metadata, bench.py's synthetic interaction stream (seeded).

  c2: 1M users x 100K items, D = 64, B = 65 536        c4: 10M users x 1M items, D = 128, B = 32 768

Per shape, one JSON line per leg:
  launch   trs_stage_add_l2 alone for S = 2 (a pair's buffer) and S = 9 (eight sampled negatives), all three
           coefficients non-zero, next to the staging kernel that fills the same buffer from the same rows
           (trs_score_fwd_bwd / trs_score_multi_fwd_bwd with the sampled softmax): one process, the legs alternating, one
           pair of device events around every launch after warm-up, fresh epoch positions every repetition, the ids
           prepared outside the timed interval.  us per launch (median), algorithmic bytes per second and share of the
           8 TB/s HBM peak.  Bytes per reference of the l2 launch: the id, one gathered table row and its 1-wide entry,
           the staged row and its 1-wide entry read and written — 4 + 3 (4D + 4); a row of the batch has 1 + S references.
  step     --steps whole steps, plain SGD, from device events around the window (alternating windows, the best of two):
             per_step              today's per-step loop: trs_batch_prepare + the one-launch step
             per_step_staged       the staged step a run with l2 takes, coefficients 0 (no l2 launch)
             per_step_staged_l2    the same with the l2 launch
             multineg_k8, multineg_k8_l2   sampled softmax over 8 negatives without / with the l2 launch
             presorted             FitRunner.run_steps on the presorted path (slices of 64 batches, prefetched as in a
                                   fit): what a run without l2 takes, i.e. the cost of leaving that path
Writes its lines to profiles/l2_bench_c2_c4.jsonl (--out) as well as to stdout.
Usage: python tools/l2_bench.py [--legs c2,c4] [--reps 40] [--steps 192]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from torchrecsys_amd import _lib, ops  # noqa: E402

PEAK_GBS = 8000.0
DEV = "cuda:0"
LAM = (0.05, 0.02, 0.01)
SLOTS = (2, 9)


def l2_bytes(D, S):
    return (1 + S) * (4 + 3 * (4 * D + 4))


def stage_bytes(D, S):
    """The staging kernels' model of tools/multineg_bench.py: ids + 1 + S rows read + 1 + S rows written."""
    return 4 * (1 + S) + 2 * (1 + S) * (4 * D + 4)


def build(name, extra):
    import bench
    cfg = bench.CONFIGS[name]
    model = bench.build_model(name, cfg["n_users"] + extra, torch.device(DEV))
    return model, cfg


def timed(fn, *a):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(*a)
    e1.record()
    return e0, e1


def launch_legs(name, model, cfg, reps):
    D, B, NI = cfg["D"], cfg["B"], cfg["n_items"]
    st = model._device_stream("train")
    T = model.net.tables()
    windows = st["user"].numel() // B
    key, seed, tau = 0x5EED1234, 77, 0.5
    bufs, ids = {}, {S: None for S in SLOTS}
    for S in SLOTS:
        F = 1 + S
        bufs[S] = (torch.empty((F, B, D), dtype=torch.float32, device=DEV),
                   torch.empty((F, B), dtype=torch.float32, device=DEV))
    loss = torch.zeros(1, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    coefs = [lam / B for lam in LAM]

    def prepare(S, t0):
        ids[S] = ops.batch_prepare_multi(st["user"], st["pos"], key, t0, B, NI, seed, t0, S - 1, out=ids[S])

    def stage(S):
        i, (gr, gl) = ids[S], bufs[S]
        if S == 2:
            Bt, keep = ops.make_batch(i["user"], i["pos"], i["neg"])
            ops.score_fwd_bwd("fm", T, Bt, B, D, 0, DEV, loss, None, want_scores=False, grad_rows=gr, grad_lin=gl)
        else:
            ops.score_multi_fwd_bwd("fm", T, i["user"], i["items"], None, _lib.LOSS_SAMPLED_SOFTMAX, tau, loss, None,
                                    gr, gl)

    def l2(S):
        i, (gr, gl) = ids[S], bufs[S]
        ops.stage_add_l2("fm", T, i["user"], i["items"], None, coefs, gr, gl, err)

    legs = [(kind, S) for S in SLOTS for kind in ("stage", "l2")]
    for w in range(3):  # warm-up: every kernel of the timed window
        for S in SLOTS:
            prepare(S, w * B)
            stage(S)
            l2(S)
    torch.cuda.synchronize()
    ev = {leg: [] for leg in legs}
    for r in range(reps):
        t0 = ((r + 3) % windows) * B
        for S in SLOTS:
            prepare(S, t0)
        for kind, S in legs:  # (the l2 launch follows the staging kernel of the same rows, as in a step)
            ev[(kind, S)].append(timed(stage if kind == "stage" else l2, S))
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    out = []
    for kind, S in legs:
        us = [1e3 * a.elapsed_time(b) for a, b in ev[(kind, S)]]
        med = statistics.median(us)
        nbytes = (l2_bytes if kind == "l2" else stage_bytes)(D, S)
        rate = nbytes * B / med / 1e3  # GB/s
        out.append({"leg": name, "kind": "launch", "what": "stage_add_l2" if kind == "l2" else
                    ("score_fwd_bwd" if S == 2 else "score_multi_fwd_bwd"), "S": S, "B": B, "D": D,
                    "us": round(med, 2), "us_min": round(min(us), 2), "bytes_per_row": nbytes,
                    "bytes_per_reference": nbytes // (1 + S), "gb_per_s": round(rate, 1),
                    "frac_hbm_peak": round(rate / PEAK_GBS, 3)})
    return out


def step_legs(name, model, cfg, steps):
    from torchrecsys_amd.engine import SparseScorerTrainer
    D, B, NI = cfg["D"], cfg["B"], cfg["n_items"]
    SparseScorerTrainer.SLICE_BATCHES = 64
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    runner = model.make_runner(opt, B)
    model.net.train()
    tr = runner.trainer
    st = model._device_stream("train")
    windows = st["user"].numel() // B
    full = runner.n_train // B
    loss = torch.zeros(1, device=DEV)
    key, seed, K = 0x5EED1234, 78, 8
    state = {"pair": None, "multi": None, "started": False}

    def run(kind, n):
        if kind == "presorted":
            tr.l2, tr.multineg = None, None
            done = 0
            while done < n:
                if not state["started"] or runner.next_batch >= full:
                    if state["started"]:
                        runner.end_epoch()
                    runner.begin_epoch()
                    state["started"] = True
                done += runner.run_steps(min(n - done, full - runner.next_batch))
            return
        tr.l2 = {"per_step": None, "per_step_staged": (0.0, 0.0, 0.0), "multineg_k8": None}.get(kind, LAM)
        for s in range(n):
            t0 = (s % windows) * B
            if kind.startswith("multineg"):
                tr.multineg = (K, _lib.LOSS_SAMPLED_SOFTMAX, 0.5)
                ids = state["multi"] = ops.batch_prepare_multi(st["user"], st["pos"], key, t0, B, NI, seed, t0, K,
                                                               out=state["multi"])
                tr.multineg_step(ids, loss)
            else:
                ids = state["pair"] = ops.batch_prepare(st["user"], st["pos"], None, key, t0, B, NI, seed, t0,
                                                        out=state["pair"])
                tr.step(ids, loss)

    kinds = ["per_step", "per_step_staged", "per_step_staged_l2", "multineg_k8", "multineg_k8_l2", "presorted"]
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
    return [{"leg": name, "kind": "step", "B": B, "D": D, "steps": steps, "l2": list(LAM),
             "step_us": {k: round(min(v), 2) for k, v in res.items()},
             "windows_us": {k: [round(x, 2) for x in v] for k, v in res.items()}}]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--legs", default="c2,c4")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--steps", type=int, default=192, help="0: skip the whole-step legs")
    ap.add_argument("--extra", type=int, default=24_000_000, help="interactions beyond one per user in the stream")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l2_bench_c2_c4.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("l2_bench.py measures on the MI355X: no GPU found")
    lines = []
    for name in a.legs.split(","):
        model, cfg = build(name, a.extra)
        for line in launch_legs(name, model, cfg, a.reps):
            print(json.dumps(line), flush=True)
            lines.append(line)
        if a.steps > 0:
            for line in step_legs(name, model, cfg, a.steps):
                print(json.dumps(line), flush=True)
                lines.append(line)
        del model
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
