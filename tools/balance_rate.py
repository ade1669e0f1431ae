#!/usr/bin/env python
"""What a balanced epoch costs: the rate of TrainerSet.fit_data with and without `balance` on the same windows.

    python tools/balance_rate.py [--tree DIR] [--balance 100] [--h 45 --w 80 --batch 4 --frames 2003 --epochs 4]

One seeded recording of `frames` frames, three in four nearly empty, every overlapping window of it, shuffled and mirrored;
one warm-up epoch, then `epochs` epochs under a wall clock that ends in a device synchronise.  --tree DIR imports cova_amd from
another checkout (a build of the parent commit, which has no `balance`), so that the arms can alternate on one box as separate
processes; the line's "tree" repeats the argument.  One JSON line.  A run without a GPU fails."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--balance", type=int)
ap.add_argument("--h", type=int, default=45)
ap.add_argument("--w", type=int, default=80)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--frames", type=int, default=2003)
ap.add_argument("--epochs", type=int, default=4)
a = ap.parse_args()
sys.path.insert(0, a.tree)

import numpy as np  # noqa: E402

from cova_amd import train as T  # noqa: E402
from cova_amd.elements import Context  # noqa: E402

h, w, f = a.h, a.w, a.frames
rng = np.random.default_rng(0)
frames = rng.integers(0, 9, (f, h, w, 4), dtype=np.uint8)
dens = np.array([0.005, 0.005, 0.005, 0.1])[rng.integers(0, 4, f)]
gt = (rng.random((f, h, w)) < dens[:, None, None]).astype(np.uint8)
ctx = Context(0)
data = T.TrainData(ctx, h, w, f)
table = T.windows([data.append(frames, gt)], "overlap")
tr = T.Trainer(ctx, h, w, max_batch=a.batch, weights_flat=T.init_weights(0), seed=0)
kw = dict(shuffle=True, flip="xy", data_seed=1)
if a.balance is not None:
    kw["balance"] = a.balance
tr.fit_data(data, table, epochs=1, batch=a.batch, **kw)
ctx.sync()
t0 = time.perf_counter()
tr.fit_data(data, table, epochs=1 + a.epochs, batch=a.batch, start_epoch=1, **kw)
ctx.sync()
dt = time.perf_counter() - t0
print(json.dumps({"tool": "fit_data_rate", "tree": a.tree, "balance": a.balance, "grid": [h, w], "batch": a.batch, "windows": len(table),
                  "epochs": a.epochs, "seconds": round(dt, 4), "samples_per_s": round(a.epochs * len(table) / dt, 1)}))
tr.close()
data.close()
ctx.close()
