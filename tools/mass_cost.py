#!/usr/bin/env python
"""What the per-frame label mass costs on one GPU: covahip_train_data_label_mass against the route that existed before it.

    python tools/mass_cost.py [--h 68 --w 120 --frames 262144 --reps 20 --host-frames 2048]

Workload: a resident data set of `frames` frames (a seeded block of 4096 frames of uneven label density, appended from device
memory until the set is full: 2.1 GB of label bytes at the defaults, eight times the Infinity Cache), one mass call over all of
them into a device buffer.  Three forms, each warmed up and then `reps` calls between HIP events:
  plain    no keep map;
  keep     a seeded keep map that ignores a third of the grid;
and, under covahip_profile_* in a run of its own, the kernel alone (train_data_mass), so that the call's fixed cost shows.
Per form: microseconds per call (median and min .. max over the reps, each rep one call) and GB/s of label bytes read
(frames * h * w over the time).  hbm_share is that rate over the 8.0 TB/s the card's HBM3E is specified at.
  host     what the tree offered before: TrainData.gather of one sample per frame (its stacks come along: 17 bytes cross the
           bus per macroblock) and (labels != 0) & keep counted in numpy, wall clock, over the first `host-frames` frames only;
           reported per frame and scaled to `frames`.
The device masses of those frames are compared with numpy's.  One JSON line.  A run without a GPU fails: there is nothing to
fall back to."""
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

HBM_SPEC = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h", type=int, default=68)
    ap.add_argument("--w", type=int, default=120)
    ap.add_argument("--frames", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-frames", type=int, default=2048)
    a = ap.parse_args()
    h, w, n = a.h, a.w, a.frames
    block_n = min(4096, n)
    ctx = Context(0)
    rng = np.random.default_rng(0)
    dens = np.array([0.002, 0.01, 0.05, 0.3])[rng.integers(0, 4, block_n)]
    block_gt = (rng.random((block_n, h, w)) < dens[:, None, None]).astype(np.uint8)
    block = rng.integers(0, 9, (block_n, h, w, 4), dtype=np.uint8)
    keep = (rng.random((h, w)) > 1 / 3).astype(np.uint8)
    data = T.TrainData(ctx, h, w, n)
    d_fr, d_gt, d_mass = ctx.malloc(block.nbytes), ctx.malloc(block_gt.nbytes), ctx.malloc(n * 4)
    ctx.h2d(d_fr, block)
    ctx.h2d(d_gt, block_gt)
    for at in range(0, n, block_n):
        data.append_device(d_fr, d_gt, min(block_n, n - at))
    ctx.free(d_fr)
    ctx.free(d_gt)

    def timed(kp):
        data.label_mass_device(d_mass, 0, n, kp)               # warm-up: code object, the keep table
        us = []
        for _ in range(a.reps):
            ctx.timer_start(0)
            data.label_mass_device(d_mass, 0, n, kp)
            ctx.timer_stop(0)
            us.append(ctx.timer_ms(0) * 1e3)
        return us

    def kernel_us(kp):
        ctx.profile(True)
        for _ in range(a.reps):
            data.label_mass_device(d_mass, 0, n, kp)
        ctx.sync()
        prof = ctx.profile_read()
        ctx.profile(False)
        ms, launches = prof["train_data_mass"][:2]
        return ms * 1e3 / launches

    nbytes = n * h * w
    out = {"tool": "mass_cost", "device": ctx.info()["name"], "grid": [h, w], "frames": n, "label_bytes": nbytes, "reps": a.reps}
    for name, kp in (("plain", None), ("keep", keep)):
        us = timed(kp)
        med, k_us = statistics.median(us), kernel_us(kp)
        out[name] = {"call_us_median": round(med, 1), "call_us_min": round(min(us), 1), "call_us_max": round(max(us), 1),
                     "call_gb_s": round(nbytes / med / 1e3, 1), "kernel_us": round(k_us, 1), "kernel_gb_s": round(nbytes / k_us / 1e3, 1),
                     "hbm_share": round(nbytes / (k_us * 1e-6) / HBM_SPEC, 3)}
    m = min(a.host_frames, n)
    samples = np.zeros(m, T.SAMPLE)
    samples["frame"] = np.arange(m)[:, None]
    samples["label"] = np.arange(m)
    t0 = time.perf_counter()
    _, lab = data.gather(samples)
    host = ((lab != 0) & (keep != 0)[None]).reshape(m, -1).sum(axis=1)
    host_s = time.perf_counter() - t0
    same = bool((data.label_mass(0, m, keep) == host).all()) and bool(
        (data.label_mass(0, m) == (block_gt[np.arange(m) % block_n] != 0).reshape(m, -1).sum(axis=1)).all())
    out["host"] = {"frames": m, "us_per_frame": round(host_s / m * 1e6, 2), "scaled_ms": round(host_s / m * n * 1e3, 1),
                   "over_keep_call": round(host_s / m * n * 1e6 / out["keep"]["call_us_median"], 1)}
    out["routes_agree"] = same
    print(json.dumps(out))
    ctx.free(d_mass)
    data.close()
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
