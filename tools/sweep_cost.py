#!/usr/bin/env python
"""What a calibration sweep costs on one GPU: covahip_post_sweep against the route that existed before it.

    python tools/sweep_cost.py [--h 68 --w 120 --samples 4096 --thresholds 16 --reps 5] [--host-samples N]

Workload: device-resident logits and labels of `samples` samples (seeded smooth fields), `thresholds` thresholds x the six
default areas.  Two routes, in the same process on the same GPU:
  sweep  covahip_post_sweep between HIP events (a warm-up call, then `reps` calls: median and spread), plus the share of each of
         its kernels from covahip_profile_* in a profiled call of its own;
  host   logits and labels to the host, numpy thresholding, one covahip_bboxcc call per threshold (host masks), numpy box
         matching per (sample, threshold, area): wall clock.  With --host-samples N it runs on the first N samples only and is
         scaled to `samples` linearly (every step of it is per sample); the two routes' tables are compared on those samples.
One JSON line.  A run without a GPU fails: there is nothing to fall back to."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from cova_amd import calibrate as cal  # noqa: E402
from cova_amd.elements import BboxCc, Context  # noqa: E402


def field(rng, n, h, w, k=7):
    x = rng.standard_normal((n, h + k - 1, w + k - 1), dtype=np.float32)
    acc = np.zeros((n, h, w), np.float32)
    for dy in range(k):
        for dx in range(k):
            acc += x[:, dy:dy + h, dx:dx + w]
    return acc / acc.std()


def hits(P, G, num, den):
    f = lambda B, k: B[k].astype(np.int64)
    iw = np.minimum.outer(f(P, "left") + f(P, "width"), f(G, "left") + f(G, "width")) - np.maximum.outer(f(P, "left"), f(G, "left"))
    ih = np.minimum.outer(f(P, "top") + f(P, "height"), f(G, "top") + f(G, "height")) - np.maximum.outer(f(P, "top"), f(G, "top"))
    inter = np.where((iw > 0) & (ih > 0), iw * ih, 0)
    union = np.add.outer(f(P, "width") * f(P, "height"), f(G, "width") * f(G, "height")) - inter
    return (inter > 0) & (inter * den >= num * union)


def host_route(ctx, d_logits, d_gt, n, h, w, th, areas, max_boxes=256, iou=(1, 10)):
    """The workaround: everything after the forward on the host, bboxcc once per threshold."""
    cc1 = BboxCc(ctx, int(areas[0]), max_boxes)
    ccg = BboxCc(ctx, 1, max_boxes)
    logits, gt = np.empty((n, h, w), np.float32), np.empty((n, h, w), np.uint8)
    ctx.d2h(logits, d_logits)
    ctx.d2h(gt, d_gt)
    g_mask = gt != 0
    gb, gc = ccg.regionprops(g_mask.astype(np.uint8))
    T, A = len(th), len(areas)
    pixel, cells = np.zeros((T, 3), np.int64), np.zeros((T, A, 3), np.int64)
    for t in range(T):
        m = logits > th[t]
        tp = int((m & g_mask).sum())
        pixel[t] = (tp, int(m.sum()) - tp, int(g_mask.sum()) - tp)
        pb, pc = cc1.regionprops(m.astype(np.uint8))
        for s in range(n):
            P, G = pb[s, :min(pc[s], max_boxes)], gb[s, :min(gc[s], max_boxes)]
            H = hits(P, G, *iou)
            for a in range(A):
                sel = P["area_px"] >= areas[a]
                cells[t, a] += (int(sel.sum()), int(H[sel].any(axis=1).sum()), int(H[sel].any(axis=0).sum()))
    return pixel, cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h", type=int, default=68)
    ap.add_argument("--w", type=int, default=120)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--thresholds", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-samples", type=int, default=0, help="samples the host route runs on (0: all)")
    a = ap.parse_args()
    h, w, n = a.h, a.w, a.samples
    ctx = Context(0)
    rng = np.random.default_rng(0)
    th = np.linspace(-1.5, 1.5, a.thresholds).astype(np.float32)
    areas = list(cal.DEFAULT_AREAS)
    d_logits, d_gt = ctx.malloc(n * h * w * 4), ctx.malloc(n * h * w)
    step = 256
    for s0 in range(0, n, step):                           # every block of samples is drawn fresh
        b = min(step, n - s0)
        lg = field(rng, b, h, w)
        gt = (field(rng, b, h, w) > 1.0).astype(np.uint8)
        L_off, G_off = s0 * h * w * 4, s0 * h * w
        ctx.h2d(d_logits + L_off, lg)
        ctx.h2d(d_gt + G_off, gt)

    def run(count=n):
        return cal.sweep_device(ctx, d_logits, d_gt, count, h, w, th, areas)

    run()                                                  # warm-up: code objects, scratch, the bboxcc plan's statistics
    ms = []
    for _ in range(a.reps):
        ctx.timer_start(0)
        res = run()
        ctx.timer_stop(0)
        ms.append(ctx.timer_ms(0))
    ctx.profile(True)
    run()
    ctx.sync()
    prof = ctx.profile_read()
    ctx.profile(False)
    hs = min(a.host_samples, n) if a.host_samples > 0 else n
    t0 = time.perf_counter()
    pixel, cells = host_route(ctx, d_logits, d_gt, hs, h, w, th, areas)
    host_s = time.perf_counter() - t0
    sub = run(hs)
    same = bool(np.array_equal(pixel, sub["pixel"]) and np.array_equal(cells[..., 0], sub["pred"]) and
                np.array_equal(cells[..., 1], sub["pred_true"]) and np.array_equal(cells[..., 2], sub["gt_found"]))
    med = statistics.median(ms)
    host_ms = host_s * 1e3 * n / hs
    print(json.dumps({"tool": "sweep_cost", "device": ctx.info()["name"], "grid": [h, w], "samples": n, "thresholds": a.thresholds,
                      "areas": areas, "sweep_ms_median": round(med, 3), "sweep_ms_min": round(min(ms), 3), "sweep_ms_max": round(max(ms), 3),
                      "sweep_ms_all": [round(v, 3) for v in ms], "pred_boxes": int(res["pred"][:, 0].sum()), "truncated": int(res["truncated"].sum()),
                      "kernels_ms": {k: round(v[0], 3) for k, v in sorted(prof.items())},
                      "kernel_launches": {k: v[1] for k, v in sorted(prof.items())},
                      "host_route_samples": hs, "host_route_s_measured": round(host_s, 3), "host_route_ms_scaled": round(host_ms, 1),
                      "host_over_sweep": round(host_ms / med, 1), "routes_agree_on_subset": same}))
    ctx.free(d_logits)
    ctx.free(d_gt)
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
