#!/usr/bin/env python
"""What the per-macroblock heat costs on one GPU: covahip_post_heat_* against the route that existed before it.

    python tools/heat_cost.py [--h 68 --w 120 --samples 4096 --thresholds 16 --batch 256 --reps 5]

Workload: device-resident logits and labels of `samples` samples (seeded tests/sweep_ref.smooth_field), `thresholds` thresholds.
Two routes, in the same process on the same GPU:
  heat   covahip_post_heat_begin, one covahip_post_heat_add per `batch` samples, covahip_post_heat_end, between HIP events (a
         warm-up bracket, then `reps` brackets: median and spread); the kernel's share from covahip_profile_* in a profiled
         bracket of its own; and the same with one add for all samples;
  host   logits and labels to the host, then per threshold (logits > th).sum(0) and ((logits > th) & (gt != 0)).sum(0) in numpy:
         wall clock, one run.
The two routes' tables are compared for equality.  One JSON line.  A run without a GPU fails: there is nothing to fall back to."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from cova_amd import calibrate as cal  # noqa: E402
from cova_amd.elements import Context  # noqa: E402
from tests.sweep_ref import smooth_field  # noqa: E402


def host_route(ctx, d_logits, d_gt, n, h, w, th):
    """The workaround: everything after the forward on the host."""
    logits, gt = np.empty((n, h, w), np.float32), np.empty((n, h, w), np.uint8)
    ctx.d2h(logits, d_logits)
    ctx.d2h(gt, d_gt)
    g = gt != 0
    fire, both = np.zeros((len(th), h, w), np.int64), np.zeros((len(th), h, w), np.int64)
    for t in range(len(th)):
        m = logits > th[t]
        fire[t] = m.sum(0)
        both[t] = (m & g).sum(0)
    return fire, both, g.sum(0, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h", type=int, default=68)
    ap.add_argument("--w", type=int, default=120)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--thresholds", type=int, default=16)
    ap.add_argument("--batch", type=int, default=256, help="samples per covahip_post_heat_add")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    h, w, n = a.h, a.w, a.samples
    ctx = Context(0)
    rng = np.random.default_rng(0)
    th = np.linspace(-1.5, 1.5, a.thresholds).astype(np.float32)
    d_logits, d_gt = ctx.malloc(n * h * w * 4), ctx.malloc(n * h * w)
    for s0 in range(0, n, 256):                            # every block of samples is drawn fresh
        b = min(256, n - s0)
        ctx.h2d(d_logits + s0 * h * w * 4, smooth_field(rng, b, h, w, 7))
        ctx.h2d(d_gt + s0 * h * w, (smooth_field(rng, b, h, w, 7) > 1.0).astype(np.uint8))

    def run(step):
        t = cal.heat_begin(ctx, h, w, th)
        for s0 in range(0, n, step):
            cal.heat_add_device(ctx, d_logits + s0 * h * w * 4, d_gt + s0 * h * w, min(step, n - s0))
        return cal.heat_end(ctx, h, w, t)

    def timed(step):
        run(step)                                          # warm-up: code object, the table
        ms = []
        for _ in range(a.reps):
            ctx.timer_start(0)
            res = run(step)
            ctx.timer_stop(0)
            ms.append(ctx.timer_ms(0))
        return ms, res

    ms, res = timed(a.batch)
    ms_one, res_one = timed(n)
    ctx.profile(True)
    run(a.batch)
    ctx.sync()
    prof = ctx.profile_read()
    ctx.profile(False)
    t0 = time.perf_counter()
    fire, both, gtf = host_route(ctx, d_logits, d_gt, n, h, w, th)
    host_ms = (time.perf_counter() - t0) * 1e3
    same = all(np.array_equal(x, r[k]) for r in (res, res_one) for x, k in ((fire, "fire"), (both, "both"), (gtf, "gt"))) and res["samples"] == n
    med = statistics.median(ms)
    r3 = lambda v: [round(x, 3) for x in v]
    print(json.dumps({"tool": "heat_cost", "device": ctx.info()["name"], "grid": [h, w], "samples": n, "thresholds": a.thresholds,
                      "batch": a.batch, "heat_ms_median": round(med, 3), "heat_ms_min": round(min(ms), 3), "heat_ms_max": round(max(ms), 3),
                      "heat_ms_all": r3(ms), "one_add_ms_median": round(statistics.median(ms_one), 3), "one_add_ms_all": r3(ms_one),
                      "kernels_ms": {k: round(v[0], 3) for k, v in sorted(prof.items())},
                      "kernel_launches": {k: v[1] for k, v in sorted(prof.items())},
                      "bytes_read": n * h * w * 5, "host_route_ms": round(host_ms, 1), "host_over_heat": round(host_ms / med, 1),
                      "routes_agree": bool(same)}))
    ctx.free(d_logits)
    ctx.free(d_gt)
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
