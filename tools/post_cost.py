"""What per-model post-processing (covahip_blobnet_set_post) costs a step: 68x120, b = 256, carrier-frame device entry, one lane and
three lanes, one model and a mixed batch of four.

Models and inputs are the benchmark's kind: blob_like weights on synthetic streams of moving objects, so the default mask holds
connected blobs and bboxcc has its usual work in both arms.  The post arm's threshold (p > 0.5001) and keep map (Bernoulli(0.9))
still change the mask, hence the work behind it: every line reports the boxes per frame of both arms beside the times.

The default settings (the kernels without post-processing) alternate with that threshold plus keep map on every
model, on the same box, in the same process and on the same loaded model; five repeats of each, every repeat bracketed by HIP
events like bench.py's steady-state leg.  Prints one JSON line per case: both step times, their spread over the repeats and the
difference."""
import json
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from cova_amd import _lib as L                      # noqa: E402
from cova_amd import synth                           # noqa: E402
from cova_amd import weights as W                   # noqa: E402
from cova_amd.elements import BlobNetInfer, Context  # noqa: E402

H, WD, B, STEPS, WARMUP, REPEATS, MAXB = 68, 120, 256, 200, 30, 5, 2048


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


def main():
    models = [W.blob_like(7 + k) for k in range(4)]
    tab, owner, nf = streams_table(B)
    per = np.bincount(owner)
    fr = np.concatenate([synth.carrier_frames(int(n) + 3, H, WD, seed=0xC07A + s) for s, n in enumerate(per)])
    assert fr.shape[0] == nf
    keeps = [(np.random.default_rng(k).random((H, WD)) < 0.9).astype(np.uint8) for k in range(4)]
    ctx = Context(0)
    dfr = ctx.malloc(fr.nbytes)
    ctx.h2d(dfr, fr)
    outs = (ctx.malloc(B * MAXB * L.BOX_DTYPE.itemsize), ctx.malloc(B * 4), ctx.malloc(B * H * WD))
    for k, lanes in ((1, 1), (1, 3), (4, 1), (4, 3)):
        ctx.set_lanes(lanes)
        net = BlobNetInfer(ctx, models[:k] if k > 1 else models[0], H, WD, max_batch=B)
        ids = (owner % k).astype(np.uint8) if k > 1 else None
        t = {"default": [], "post": []}
        boxes = {}
        for _ in range(REPEATS):
            for m in range(k):
                net.reset_post(m)
            us, boxes["default"] = step_us(ctx, net, dfr, nf, tab, ids, outs)
            t["default"].append(us)
            for m in range(k):
                net.set_post(m, prob_thresh=0.5001, keep=keeps[m])
            us, boxes["post"] = step_us(ctx, net, dfr, nf, tab, ids, outs)
            t["post"].append(us)
        d, p = np.array(t["default"]), np.array(t["post"])
        print(json.dumps({"models": k, "lanes": lanes, "default_us": [round(x, 2) for x in d], "post_us": [round(x, 2) for x in p],
                          "default_median": round(float(np.median(d)), 2), "post_median": round(float(np.median(p)), 2),
                          "default_spread": round(float(d.max() - d.min()), 2), "post_spread": round(float(p.max() - p.min()), 2),
                          "diff_us": round(float(np.median(p) - np.median(d)), 2),
                          "boxes_per_frame_default": round(boxes["default"], 2), "boxes_per_frame_post": round(boxes["post"], 2)}), flush=True)
    ctx.sync()
    for d in (dfr,) + outs:
        ctx.free(d)
    ctx.close()


if __name__ == "__main__":
    main()
