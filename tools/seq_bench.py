# -*- coding: utf-8 -*-
"""The sequence model's step (fit_sequence: csrc/seq.hip, trs_seq_fwd_bwd + the staged tail) at the table shapes of the
benchmark configurations, Linear scorer, no metadata, uniform random sequences of 32 items per user (seeded).

  c2: 1M users x 100K items, D = 64, B = 65 536        c4: 10M users x 1M items, D = 128, B = 32 768

Per shape and context length L in --ls, one JSON line (appended to --out, default profiles/seq_bench.jsonl):
  stage_us   the staging launch alone (trs_seq_fwd_bwd), device events around the launch, the median of --reps after one
             warm-up, fresh triples every repetition; `stage_gb_per_s` its algorithmic byte rate —
               (3 + L) rows read and (3 + L) rows staged per triple, 16 + 4 L bytes of ids, 8 of 1-wide terms read
               and 12 staged: 2 (3 + L) 4D + 36 + 4 L bytes;
  pair_us    trs_score_fwd_bwd(TRS_NET_LINEAR) on the same (user, positive, negative) rows in the same session, timed
             the same way (16 + 6 (4D + 4) bytes per row), and `rate_vs_pair` = the staging kernel's byte rate over it;
  step_us    a whole step (gather of the positives, trs_sample_neg, the staging launch, four trs_rows_scatter_add),
             and `scatter_us` = the four scatters alone on the staged buffer.
Usage: python tools/seq_bench.py [--legs c2,c4] [--ls 1,4,8] [--reps 3] [--out profiles/seq_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from torchrecsys_amd import _lib, ops  # noqa: E402
from torchrecsys_amd.engine import SequenceTrainer  # noqa: E402

PEAK_GBS = 8000.0
DEV = "cuda:0"
SHAPES = {"c2": (1_000_000, 100_000, 64, 65536), "c4": (10_000_000, 1_000_000, 128, 32768)}
SEQ_LEN = 32
WINDOWS = 8  # distinct batches of triples


def seq_bytes(D, L):
    return 2 * (3 + L) * 4 * D + 36 + 4 * L


def pair_bytes(D):
    return 16 + 6 * (4 * D + 4)


def build(name):
    from torchrecsys_amd.collaborative.linear import Linear
    NU, NI, D, B = SHAPES[name]
    g = torch.Generator(device=DEV)
    g.manual_seed(B)
    net = Linear(1, 1, {}, D, use_metadata=False)  # tables drawn on the device (a host init of c4 takes minutes)
    for mod, n, w in ((net.user, NU, D), (net.item, NI, D), (net.user_bias, NU, 1), (net.item_bias, NI, 1)):
        mod.weight = torch.nn.Parameter(torch.randn(n, w, device=DEV, generator=g) * 0.1)
    net.n_users, net.n_items = NU, NI
    C = torch.randn(NI, D, device=DEV, generator=g) * 0.1
    off = torch.arange(NU + 1, dtype=torch.int64, device=DEV) * SEQ_LEN
    ids = torch.randint(0, NI, (NU * SEQ_LEN,), device=DEV, dtype=torch.int32, generator=g)
    entry = torch.randint(0, NU * SEQ_LEN, (WINDOWS * B,), device=DEV, dtype=torch.int64, generator=g)
    user = (entry // SEQ_LEN).to(torch.int32)
    return net, C, (off, ids), user, entry


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def median_us(fn, reps):
    """fn(r) timed by device events: one warm-up, then the median of `reps`."""
    fn(0)
    torch.cuda.synchronize()
    ev = [timed(lambda: fn(r + 1)) for r in range(reps)]
    torch.cuda.synchronize()
    return statistics.median(1e3 * a.elapsed_time(b) for a, b in ev)


def leg(name, net, C, seq, user, entry, L, reps):
    NU, NI, D, B = SHAPES[name]
    T = net.tables()
    w = ops.seq_weights(L, 0.7, DEV)
    tr = SequenceTrainer(net, C, w, seq, B, 0.01, _lib.LOSS_ID["bpr"])
    loss = torch.zeros(1, device=DEV)
    gr = tr.grad_rows.view(3 + L, B, D)
    gl = tr.grad_lin.view(3, B)
    cid = tr.ctx_ids[:L * B].view(L, B)
    pgr = torch.empty((3, B, D), dtype=torch.float32, device=DEV)
    pgl = torch.empty((3, B), dtype=torch.float32, device=DEV)
    win = lambda r: slice((r % WINDOWS) * B, (r % WINDOWS + 1) * B)
    pos = [seq[1][entry[win(r)]] for r in range(WINDOWS)]
    neg = [ops.sample_neg(pos[r], NI, 77, r * B) for r in range(WINDOWS)]

    def stage(r):
        s = win(r)
        ops.seq_fwd_bwd(T, C, seq, user[s], entry[s], neg[r % WINDOWS], w, tr.loss_id, loss, None, gr, gl, cid, tr.err)

    def pair(r):
        Bt, keep = ops.make_batch(user[win(r)], pos[r % WINDOWS], neg[r % WINDOWS])
        ops.score_fwd_bwd("linear", T, Bt, B, D, 0, DEV, loss, None, want_scores=False, grad_rows=pgr, grad_lin=pgl)

    def scatter(r):
        s = win(r)
        items = torch.cat([pos[r % WINDOWS], neg[r % WINDOWS]])
        ops.rows_scatter_add(tr.user, user[s], gr[0], -tr.lr, ld=D)
        ops.rows_scatter_add(tr.item, items, gr[1:3].view(2 * B, D), -tr.lr, ld=D)
        ops.rows_scatter_add(tr.item_lin, items, gl[1:3].view(2 * B, 1), -tr.lr, ld=1)
        if L:
            ops.rows_scatter_add(C, cid.view(-1), gr[3:].view(L * B, D), -tr.lr, ld=D)

    def step(r):
        s = win(r)
        tr.seq_step(user[s], entry[s], loss, 77, r * B)

    st, pr = median_us(stage, reps), median_us(pair, reps)
    sc, sp = median_us(scatter, reps), median_us(step, reps)
    tr.check_errors()
    rate, prate = seq_bytes(D, L) * B / st / 1e3, pair_bytes(D) * B / pr / 1e3
    return {"leg": name, "B": B, "D": D, "L": L, "stage_us": round(st, 2), "bytes_per_row": seq_bytes(D, L),
            "stage_gb_per_s": round(rate, 1), "frac_hbm_peak": round(rate / PEAK_GBS, 3), "pair_us": round(pr, 2),
            "pair_gb_per_s": round(prate, 1), "rate_vs_pair": round(rate / prate, 3), "scatter_us": round(sc, 2),
            "step_us": round(sp, 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--legs", default="c2,c4")
    ap.add_argument("--ls", default="1,4,8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seq_bench.py measures on the MI355X: no GPU found")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        for name in a.legs.split(","):
            net, C, seq, user, entry = build(name)
            for L in (int(x) for x in a.ls.split(",")):
                line = json.dumps(leg(name, net, C, seq, user, entry, L, a.reps))
                print(line, flush=True)
                out.write(line + "\n")
            del net, C, seq, user, entry
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
