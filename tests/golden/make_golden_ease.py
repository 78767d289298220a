# -*- coding: utf-8 -*-
"""Generates tests/golden/g5_ease.npz by RUNNING THE REAL REFERENCE's EASE class (as make_golden.py does for the other
fixtures; run only where the reference is installed, it never travels to the GPU box):

    cd <repo> && PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ease.py

The fixture holds DATA only: the (user, item) pairs (uint8: both sides are below 256) of one duplicate-free data set of
150 users x 65 items, lambda, and the reference's outputs `b` (float64 item-item weights) and `pred` (scores of all
users), each stored as its eight byte planes (ease_ref.byte_planes: the same 64 bits per value, but sign and exponent
bytes lie together and compress, which keeps the file under 100 KB).  No reference source is stored.
The pairs are tests/ease_ref.histories(150, 65, SEED); SEED is the first one for which at most 10 % of the users have two
values closer than 1e-6 among their six largest reference scores (those users are left out of the order comparison of
tests/test_gpu_ease.py) and the last user has an item (scipy sizes the matrix by the largest index).
"""
import os
import sys
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ease_ref  # noqa: E402

from torchrecsys.collaborative.ease import EASE  # noqa: E402

NU, NI, LAMBDA = 150, 65, 0.5


def near_ties(pred, top=6, gap=1e-6):
    s = -np.sort(-pred, axis=1)[:, :top]
    return int(((s[:, :-1] - s[:, 1:]) < gap).any(axis=1).sum())


def run(seed):
    lists = ease_ref.histories(NU, NI, seed)
    users = np.repeat(np.arange(NU), [len(v) for v in lists])
    items = np.concatenate(lists)
    df = pd.DataFrame({"user_id": users, "item_id": items, "product": items, "action": np.ones(len(items))})
    model = EASE(types.SimpleNamespace(dataset=df), split_train_test=False)
    model.fit(lambda_=LAMBDA)
    return lists, users, items, np.asarray(model.b, dtype=np.float64), np.asarray(model.pred, dtype=np.float64)


if __name__ == "__main__":
    for seed in range(100):
        lists, users, items, b, pred = run(seed)
        if len(lists[-1]) and pred.shape == (NU, NI) and near_ties(pred) <= NU // 10:
            break
    else:
        raise SystemExit("no seed found")
    out = os.path.join(HERE, "g5_ease.npz")
    np.savez_compressed(out, seed=np.int64(seed), n_users=np.int64(NU), n_items=np.int64(NI), lam=np.float64(LAMBDA),
                        users=users.astype(np.uint8), items=items.astype(np.uint8), b_planes=ease_ref.byte_planes(b),
                        pred_planes=ease_ref.byte_planes(pred))
    print("seed %d: %d pairs, %d users with near ties in their top 6, %d bytes"
          % (seed, len(items), near_ties(pred), os.path.getsize(out)))
