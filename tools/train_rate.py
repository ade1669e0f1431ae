#!/usr/bin/env python
"""BlobNet training throughput on one GPU: samples/s of covahip_train_step at a given geometry and batch sizes.

    python tools/train_rate.py [--h-mb 45 --w-mb 80 --batches 4,64 --steps 30 --warmup 5 --freeze encoder --freeze-bn --math matrix]

--freeze GROUPS / --freeze-bn time the step under a training plan, --math exact|matrix in that arithmetic (cova_amd.train's flags
of the same names).
Host-pointer steps (the input copy and the loss read-back included), as Trainer.fit runs them; one JSON line per batch size.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from cova_amd import synth, train as T  # noqa: E402
from cova_amd.elements import Context  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h-mb", type=int, default=45)
    ap.add_argument("--w-mb", type=int, default=80)
    ap.add_argument("--batches", default="4,64")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--freeze", default="")
    ap.add_argument("--freeze-bn", action="store_true")
    ap.add_argument("--math", choices=T.MATH_MODES, default="exact")
    a = ap.parse_args()
    h, w = a.h_mb, a.w_mb
    plan = {"freeze": a.freeze, "bn_inference": "all" if a.freeze_bn else ()}
    ctx = Context(0)
    for b in (int(x) for x in a.batches.split(",")):
        stack = synth.stacked_batch(b, h, w, seed=3, streams=min(b, 8))
        gt = synth.random_masks(b, h, w, 0.2, seed=3)
        tr = T.Trainer(ctx, h, w, max_batch=b, seed=0, **plan)
        tr.set_math(a.math)
        for _ in range(a.warmup):
            tr.step(stack, gt)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            tr.step(stack, gt)
        dt = time.perf_counter() - t0
        tr_plan = tr.plan
        tr.close()
        print(json.dumps({"h_mb": h, "w_mb": w, "batch": b, "steps": a.steps, **tr_plan, "math": a.math, "ms_per_step": 1e3 * dt / a.steps,
                          "samples_per_s": b * a.steps / dt}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
