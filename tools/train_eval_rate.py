#!/usr/bin/env python
"""What a held-out evaluation costs beside a training step: ms per chunk of covahip_train_eval (one chunk = max_batch samples
per model) next to ms per covahip_train_step of the same batch, solo, and one covahip_train_eval_set over K models next to K
solo evaluations one after the other.

    python tools/train_eval_rate.py [--h-mb 45 --w-mb 80 --batches 4,64 --models 8 --set-batch 4 --steps 30 --warmup 5 --repeats 3]

Device-pointer calls (the read-back of the results included).  The sides alternate, `--repeats` times each: the spread of a
side's rows is the box's noise.  One JSON line per configuration.  `--only eval` with `--steps N --warmup 0 --repeats 1` runs N
evaluation chunks and nothing else (a profiling run: the kernel trace then holds N chunks' launches)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from cova_amd import synth, train as T  # noqa: E402
from cova_amd.elements import Context  # noqa: E402


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()                      # every call ends in a stream synchronise (the result read-back)
    return 1e3 * (time.perf_counter() - t0) / steps


def device_data(ctx, n, h, w):
    stack = synth.stacked_batch(n, h, w, seed=3, streams=min(n, 8))
    gt = synth.random_masks(n, h, w, 0.2, seed=3)
    d_stack, d_gt = ctx.malloc(stack.nbytes), ctx.malloc(gt.nbytes)
    ctx.h2d(d_stack, stack)
    ctx.h2d(d_gt, gt)
    return d_stack, d_gt, stack.nbytes // n, gt.nbytes // n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h-mb", type=int, default=45)
    ap.add_argument("--w-mb", type=int, default=80)
    ap.add_argument("--batches", default="4,64", help="solo: eval chunk against training step at these batches")
    ap.add_argument("--models", type=int, default=8, help="set: one eval of K models against K solo evals (0: skip)")
    ap.add_argument("--set-batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=("eval",), help="time the evaluation side alone")
    a = ap.parse_args()
    h, w = a.h_mb, a.w_mb
    ctx = Context(0)
    med = lambda v: round(float(np.median(v)), 3)   # noqa: E731
    for b in (int(x) for x in a.batches.split(",") if x):
        d_stack, d_gt, _, _ = device_data(ctx, b, h, w)
        tr = T.Trainer(ctx, h, w, max_batch=b, weights_flat=T.init_weights(0), seed=0)
        ev_ms, st_ms = [], []
        for _ in range(a.repeats):
            ev_ms.append(timed(lambda: tr.evaluate_device(d_stack, d_gt, b), a.warmup, a.steps))
            if not a.only:
                st_ms.append(timed(lambda: tr.step_device(d_stack, d_gt, b), a.warmup, a.steps))
        rec = {"h_mb": h, "w_mb": w, "batch": b, "models": 1, "eval_ms_per_chunk": [round(v, 3) for v in ev_ms], "eval_ms": med(ev_ms)}
        if st_ms:
            rec.update(step_ms_per_step=[round(v, 3) for v in st_ms], step_ms=med(st_ms),
                       eval_over_step=round(float(np.median(ev_ms) / np.median(st_ms)), 3))
        print(json.dumps(rec), flush=True)
        tr.close()
        ctx.free(d_stack)
        ctx.free(d_gt)
    k, b = a.models, a.set_batch
    if k > 0:
        d_stack, d_gt, per_stack, per_gt = device_data(ctx, k * b, h, w)
        flats = [T.init_weights(m) for m in range(k)]
        ts = T.TrainerSet(ctx, h, w, weights=flats, seeds=list(range(k)), max_batch=b)
        solos = [] if a.only else [T.Trainer(ctx, h, w, max_batch=b, weights_flat=flats[m], seed=m) for m in range(k)]

        def solo_evals():
            for m, tr in enumerate(solos):
                tr.evaluate_device(d_stack + m * b * per_stack, d_gt + m * b * per_gt, b)

        set_ms, solo_ms = [], []
        for _ in range(a.repeats):
            set_ms.append(timed(lambda: ts.evaluate_device(d_stack, d_gt, [b] * k), a.warmup, a.steps))
            if solos:
                solo_ms.append(timed(solo_evals, a.warmup, a.steps))
        rec = {"h_mb": h, "w_mb": w, "batch": b, "models": k, "set_eval_ms_per_chunk": [round(v, 3) for v in set_ms], "set_eval_ms": med(set_ms)}
        if solo_ms:
            rec.update(solo_eval_ms_per_k_chunks=[round(v, 3) for v in solo_ms], solo_eval_ms=med(solo_ms),
                       solo_over_set=round(float(np.median(solo_ms) / np.median(set_ms)), 3))
        print(json.dumps(rec), flush=True)
        ts.close()
        for tr in solos:
            tr.close()
        ctx.free(d_stack)
        ctx.free(d_gt)
    ctx.close()


if __name__ == "__main__":
    main()
