#!/usr/bin/env python
"""Training sets against solo trainers on one GPU: samples/s of one covahip_train_step_set over K models beside K
covahip_train_step calls on K solo trainers, one after the other in the same process.

    python tools/train_set_rate.py [--h-mb 45 --w-mb 80 --batch 4 --models 1,2,4,8,16 --steps 30 --warmup 5 --repeats 3]

Device-pointer steps (the loss read-back included).  The two sides alternate, `--repeats` times per K: the spread of a side's
rows is the box's noise.  One JSON line per K.  `--only set|solo` runs one side alone (a profiling run).  `--freeze GROUPS` /
`--freeze-bn` put both sides under a training plan, `--math exact|matrix` in that arithmetic (cova_amd.train's flags of the same
names)."""
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
        fn()                      # every step ends in a stream synchronise (the loss read-back)
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h-mb", type=int, default=45)
    ap.add_argument("--w-mb", type=int, default=80)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--models", default="1,2,4,8,16")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=("set", "solo"))
    ap.add_argument("--freeze", default="")
    ap.add_argument("--freeze-bn", action="store_true")
    ap.add_argument("--math", choices=T.MATH_MODES, default="exact")
    a = ap.parse_args()
    h, w, b = a.h_mb, a.w_mb, a.batch
    plan = {"freeze": a.freeze, "bn_inference": "all" if a.freeze_bn else ()}
    ctx = Context(0)
    for k in (int(x) for x in a.models.split(",")):
        stack = synth.stacked_batch(k * b, h, w, seed=3, streams=min(k * b, 8))
        gt = synth.random_masks(k * b, h, w, 0.2, seed=3)
        d_stack, d_gt = ctx.malloc(stack.nbytes), ctx.malloc(gt.nbytes)
        ctx.h2d(d_stack, stack)
        ctx.h2d(d_gt, gt)
        flats = [T.init_weights(m) for m in range(k)]
        ts = T.TrainerSet(ctx, h, w, weights=flats, seeds=list(range(k)), max_batch=b, **plan) if a.only != "solo" else None
        solos = [T.Trainer(ctx, h, w, max_batch=b, weights_flat=flats[m], seed=m, **plan) for m in range(k)] if a.only != "set" else []
        for tr in ([ts] if ts else []) + solos:
            tr.set_math(a.math)
        per_stack, per_gt = stack.nbytes // (k * b), gt.nbytes // (k * b)

        def solo_step():
            for m, tr in enumerate(solos):
                tr.step_device(d_stack + m * b * per_stack, d_gt + m * b * per_gt, b)

        set_ms, solo_ms = [], []
        for _ in range(a.repeats):
            if ts:
                set_ms.append(timed(lambda: ts.step_device(d_stack, d_gt, [b] * k), a.warmup, a.steps))
            if solos:
                solo_ms.append(timed(solo_step, a.warmup, a.steps))
        rec = {"h_mb": h, "w_mb": w, "batch": b, "models": k, "steps": a.steps, "math": a.math, **T.plan_names(*T.plan_bits(**plan))}
        if set_ms:
            rec.update(set_ms_per_step=[round(v, 3) for v in set_ms], set_samples_per_s=round(1e3 * k * b / min(set_ms)))
        if solo_ms:
            rec.update(solo_ms_per_k_steps=[round(v, 3) for v in solo_ms], solo_samples_per_s=round(1e3 * k * b / min(solo_ms)))
        if set_ms and solo_ms:
            rec["solo_over_set"] = round(float(np.median(solo_ms) / np.median(set_ms)), 3)
        print(json.dumps(rec), flush=True)
        if ts:
            ts.close()
        for tr in solos:
            tr.close()
        ctx.free(d_stack)
        ctx.free(d_gt)
    ctx.close()


if __name__ == "__main__":
    main()
