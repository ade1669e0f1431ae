#!/usr/bin/env python
"""What training from a resident data set costs on one GPU, against the path that existed before it.

    python tools/train_data_cost.py [--settings 45x80x4,68x120x64 --frames 259 --epochs 2 --reps 3]

Per setting HxWxB: `frames` seeded frames of one recording, every overlapping window of it (frames - 3 samples), in canonical
order, batches of B.  Two routes in the same process, alternating, `reps` times each after one warm-up epoch of each:
  fit       TrainerSet.fit on the materialised stacks (host arrays; every step slices and uploads B * 17 h w bytes),
  fit_data  TrainerSet.fit_data on the same windows in the same order (every step uploads B * 24 bytes of table),
wall clock around `epochs` epochs (each step ends in a synchronise), as samples per second: median and min .. max of the
repeats.  The two routes' final weights are compared for equality.  Then the gather launch alone: B samples into a device buffer,
100 launches under covahip_profile_* (HIP events around each), microseconds per launch.  One JSON line per setting.  A run
without a GPU fails: there is nothing to fall back to."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from cova_amd import train as T  # noqa: E402
from cova_amd.elements import Context  # noqa: E402


def measure(ctx, h, w, batch, n_frames, epochs, reps):
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 9, (n_frames, h, w, 4), dtype=np.uint8)
    gt = rng.integers(0, 2, (n_frames, h, w), dtype=np.uint8)
    data = T.TrainData(ctx, h, w, n_frames)
    table = T.windows([data.append(frames, gt)], "overlap")
    samples = T.plain_samples(table)
    n = len(samples)
    stacks = np.ascontiguousarray(frames[samples["frame"]].reshape(n, 4 * h, w, 4))
    labels = np.ascontiguousarray(gt[samples["label"]])
    flat = T.init_weights(0)
    trainers = {name: T.Trainer(ctx, h, w, max_batch=batch, weights_flat=flat, seed=0) for name in ("fit", "fit_data")}
    runs = {"fit": lambda tr, ep: tr.fit((stacks, labels), epochs=ep, batch=batch),
            "fit_data": lambda tr, ep: tr.fit_data(data, table, epochs=ep, batch=batch)}
    rates = {name: [] for name in runs}
    for name, run in runs.items():
        run(trainers[name], 1)                                             # warm-up: code objects, first launches
    for _ in range(reps):
        for name, run in runs.items():
            t0 = time.perf_counter()
            run(trainers[name], epochs)
            rates[name].append(epochs * n / (time.perf_counter() - t0))
    same = trainers["fit"].weights_bytes() == trainers["fit_data"].weights_bytes()
    # the gather launch alone
    d_stack, d_gt = ctx.malloc(batch * 16 * h * w), ctx.malloc(batch * h * w)
    data.gather_device(samples[:batch], d_stack, d_gt)
    ctx.profile(True, only="train_data_gather")
    for i in range(100):
        at = (i * batch) % max(1, n - batch)
        data.gather_device(samples[at:at + batch], d_stack, d_gt)
    ctx.sync()
    ms, launches = ctx.profile_read()["train_data_gather"]
    ctx.profile(False)
    ctx.free(d_stack)
    ctx.free(d_gt)
    for tr in trainers.values():
        tr.close()
    data.close()
    out = {"h": h, "w": w, "batch": batch, "windows": n, "epochs": epochs, "reps": reps, "weights_equal": same,
           "gather_us_per_launch": 1e3 * ms / launches, "gather_bytes_written": batch * 17 * h * w,
           "resident_bytes_per_frame": 3 * h * w, "appended_bytes_per_frame": 5 * h * w}
    for name, r in rates.items():
        out[name + "_samples_per_s"] = {"median": statistics.median(r), "min": min(r), "max": max(r)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default="45x80x4,68x120x64", help="HxWxB[,HxWxB...]")
    ap.add_argument("--frames", type=int, default=259)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    ctx = Context(0)
    for setting in a.settings.split(","):
        h, w, b = (int(v) for v in setting.split("x"))
        out = measure(ctx, h, w, b, a.frames, a.epochs, a.reps)
        print(json.dumps(out), flush=True)
        if not out["weights_equal"]:
            sys.exit(f"{setting}: the two routes ended on different weights; their rates do not compare")
    ctx.close()


if __name__ == "__main__":
    main()
