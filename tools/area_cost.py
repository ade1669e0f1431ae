"""What a per-model area threshold (covahip_blobnet_set_area) costs a step: 68x120, b = 256, carrier-frame device entry, one lane
and three lanes.

Two cases, each as alternating arms on the same box, in the same process and on the same loaded model, five repeats of each arm,
every repeat bracketed by HIP events like bench.py's steady-state leg:
  one model,  no area set            -- the default path: must be the kernels of a build without the feature;
  8 models round robin, no area set  against  the same set with an area on ONE model (the POST = true tail for every stack).
Models and inputs are the benchmark's kind (blob_like weights on synthetic streams of moving objects).  Prints one JSON line per
(case, lanes): the step times of the arms, their spread over the repeats, the boxes per frame and the kernels the profile saw.

`--arms default` runs the arms without an area only: that is what a build without covahip_blobnet_set_area can run, for an A/B
of two builds on one box (run the two trees' copies of this file alternately)."""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from cova_amd import _lib as L                      # noqa: E402
from cova_amd import synth                           # noqa: E402
from cova_amd import weights as W                   # noqa: E402
from cova_amd.elements import BlobNetInfer, Context  # noqa: E402

H, WD, B, STEPS, WARMUP, REPEATS, MAXB = 68, 120, 256, 200, 30, 5, 2048
AREA_MODEL, AREA = 3, 8


def streams_table(b, n_streams=8):
    rows, owner, base = [], [], 0
    per = [b // n_streams + (1 if s < b % n_streams else 0) for s in range(n_streams)]
    for s, n in enumerate(per):
        rows += [[base + i + 3, base + i + 2, base + i + 1, base + i] for i in range(n)]
        owner += [s] * n
        base += n + 3
    return np.array(rows, np.int32), np.array(owner), base


def step_us(ctx, net, dfr, nf, tab, ids, outs):
    def steps(n):
        for _ in range(n):
            net.filter_frames_device(dfr, nf, tab, B, 1, outs[0], outs[1], MAXB, outs[2], model_ids=ids)
    steps(WARMUP)
    ctx.sync()
    ctx.timer_start(0)
    steps(STEPS)
    ctx.timer_stop(0)
    us = ctx.timer_ms(0) * 1e3 / STEPS
    counts = np.empty(B, np.int32)
    ctx.d2h(counts, outs[1])
    return us, float(counts.mean())


def kernels(ctx, net, dfr, nf, tab, ids, outs):
    ctx.profile(True)
    try:
        net.filter_frames_device(dfr, nf, tab, B, 1, outs[0], outs[1], MAXB, outs[2], model_ids=ids)
        ctx.sync()
        return {k: v[1] for k, v in sorted(ctx.profile_read().items())}
    finally:
        ctx.profile(False)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--arms", nargs="+", default=["default", "area"], choices=["default", "area"])
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    models = [W.blob_like(7 + k) for k in range(8)]
    tab, owner, nf = streams_table(B)
    per = np.bincount(owner)
    fr = np.concatenate([synth.carrier_frames(int(n) + 3, H, WD, seed=0xC07A + s) for s, n in enumerate(per)])
    assert fr.shape[0] == nf
    ctx = Context(0)
    dfr = ctx.malloc(fr.nbytes)
    ctx.h2d(dfr, fr)
    outs = (ctx.malloc(B * MAXB * L.BOX_DTYPE.itemsize), ctx.malloc(B * 4), ctx.malloc(B * H * WD))
    for k, lanes in ((1, 1), (1, 3), (8, 1), (8, 3)):
        ctx.set_lanes(lanes)
        net = BlobNetInfer(ctx, models[:k] if k > 1 else models[0], H, WD, max_batch=B)
        ids = (owner % k).astype(np.uint8) if k > 1 else None
        arms = [x for x in a.arms if x == "default" or k > 1]
        t = {x: [] for x in arms}
        boxes, names = {}, {}
        for _ in range(REPEATS):
            for arm in arms:
                if "area" in a.arms:
                    net.set_area(AREA_MODEL if k > 1 else 0, AREA if arm == "area" else 0)
                us, boxes[arm] = step_us(ctx, net, dfr, nf, tab, ids, outs)
                t[arm].append(us)
        for arm in arms:
            if "area" in a.arms:
                net.set_area(AREA_MODEL if k > 1 else 0, AREA if arm == "area" else 0)
            names[arm] = kernels(ctx, net, dfr, nf, tab, ids, outs)
        out = {"tag": a.tag, "models": k, "lanes": lanes}
        for arm in arms:
            v = np.array(t[arm])
            out[arm] = {"us": [round(x, 2) for x in v], "median": round(float(np.median(v)), 2), "spread": round(float(v.max() - v.min()), 2),
                        "boxes_per_frame": round(boxes[arm], 2), "kernels": names[arm]}
        if len(arms) == 2:
            out["diff_us"] = round(out["area"]["median"] - out["default"]["median"], 2)
        print(json.dumps(out), flush=True)
    ctx.sync()
    for d in (dfr,) + outs:
        ctx.free(d)
    ctx.close()


if __name__ == "__main__":
    main()
