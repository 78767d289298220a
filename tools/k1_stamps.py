# -*- coding: utf-8 -*-
"""Where the time of the one-launch flag-mode step (fwd_stage_kernel<..., INL 3>) goes, per workgroup: a DIAGNOSTIC build
(`make -C torchrecsys_amd/csrc EXTRA=-DTRS_K1_STAMPS`) stamps s_memrealtime at the kernel's start, the end of the main
loop, the end of the grid-wide wait, the end of the deferred atomics and the in-loop look into the (otherwise unused) gz buffer; this script
runs c4-shaped steps and prints the distribution over the 512 workgroups of the last step.  Not for the product build."""
import contextlib
import io
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

dev = torch.device("cuda", 0)
model = bench.build_model("c4", 20_000_000, dev)
opt = torch.optim.SGD(model.parameters(), lr=1e-2)
from torchrecsys_amd.engine import SparseScorerTrainer  # noqa: E402
SparseScorerTrainer.SLICE_BATCHES = 64
r = model.make_runner(opt, 32768)
model.net.train()
r.begin_epoch()
for rep in range(6):
    r.run_steps(9)
    torch.cuda.synchronize()
    st = r.trainer.gz.view(torch.int64).reshape(-1)[:8 * 512].reshape(512, 8).cpu().numpy().astype(np.float64) * 0.01  # us
    t0 = st[:, 0].min()
    q = lambda a: "min %.1f  p50 %.1f  p90 %.1f  max %.1f" % (a.min(), np.median(a), np.percentile(a, 90), a.max())
    print(f"rep {rep}: start {q(st[:, 0] - t0)} | main loop end {q(st[:, 1] - t0)} | wait end {q(st[:, 2] - t0)} | "
          f"deferred end {q(st[:, 3] - t0)}")
    il = st[st[:, 4] > 0]  # workgroups whose wave 0 issued its in-loop look (K1_APPLY_IN_LOOP; wave 0 had references)
    if len(il):
        print(f"rep {rep}: in-loop apply issued ({len(il)} workgroups) {q(il[:, 4] - t0)} | their main loop end "
              f"{q(il[:, 1] - t0)} | their deferred end {q(il[:, 3] - t0)}")
