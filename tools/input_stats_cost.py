#!/usr/bin/env python
"""What the input monitor (covahip_monitor_set_inputs, covahip_train_data_record_stats) costs on one GPU.

    python tools/input_stats_cost.py [--parts attached alone train] [--frames 262144] [--reps 10]

attached  the filter step at 68x120, b = 256, three lanes, carrier-frame device entry on resident inputs as tools/monitor_cost.py
          builds them, monitor attached with every = 1: inputs off against inputs on (and no monitor at all), alternating within
          a repeat in one process, microseconds per step between HIP events, median and spread over the repeats; the two input
          kernels' own time from the per-kernel profile.  The yardstick is `off - none`, what the attached monitor itself costs.
alone     covahip_monitor_add_inputs on 4,096 packed samples of 68x120 in device memory, with sparse (2 % non-zero) and with uniform
          random records: microseconds per call and per kernel, GB/s of record bytes and the share of the HBM's 8.0 TB/s.  Both
          contents beside each other: the dominant bin is the design risk.
train     covahip_train_data_record_stats over a resident set of `frames` frames (a seeded block of 4,096 frames appended until the
          set is full: 2.14 GB of labels plus 4.28 GB of records at the defaults) against covahip_train_data_label_mass on the same
          set, which reads a third of the bytes; and the same counts through TrainData.gather and numpy over the first
          `host-frames` frames, wall clock, scaled to the set.  The two routes' counts are compared.
train_odd the same at 67x119, a quarter of the frames: h * w is odd, frames start on odd records, and the kernel reads a record
          at a time instead of 16 bytes (label_mass peels to alignment and keeps its 16-byte loads).
alone also measures the sparse records 2 bytes and 1 byte past the allocation: a record at a time, and byte-wise.
One JSON line per part.  A run without a GPU fails: there is nothing to fall back to."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from cova_amd import _lib as L  # noqa: E402
from cova_amd import monitor as mon  # noqa: E402
from cova_amd import train as T  # noqa: E402
from cova_amd.elements import BlobNetInfer, Context, pack_frames  # noqa: E402

HBM_SPEC = 8.0e12
H, WD, B, LANES, STEPS, WARMUP, MAXB = 68, 120, 256, 3, 300, 60, 2048


def spread(v):
    v = np.asarray(v, np.float64)
    return {"us": [round(float(x), 2) for x in v], "median": round(float(np.median(v)), 2), "spread": round(float(v.max() - v.min()), 2)}


def kernels(ctx, run, names):
    """{name: microseconds per launch} of the profiled kernels `names` over run()."""
    ctx.profile(True)
    run()
    ctx.sync()
    prof = ctx.profile_read()
    ctx.profile(False)
    return {k: round(prof[k][0] * 1e3 / max(1, prof[k][1]), 2) for k in names if k in prof}


def part_attached(ctx, reps):
    from tools.monitor_cost import streams_table
    from cova_amd import synth
    from cova_amd import weights as W
    tab, owner, nf = streams_table(B)
    per = np.bincount(owner)
    fr = np.concatenate([synth.carrier_frames(int(n) + 3, H, WD, seed=0xC07A + s) for s, n in enumerate(per)])
    ctx.set_lanes(LANES)
    dfr = ctx.malloc(fr.nbytes)
    ctx.h2d(dfr, fr)
    outs = [(ctx.malloc(B * MAXB * L.BOX_DTYPE.itemsize), ctx.malloc(B * 4), ctx.malloc(B * H * WD)) for _ in range(LANES)]
    net = BlobNetInfer(ctx, W.blob_like(7), H, WD, max_batch=B)

    def steps(n):
        for i in range(n):
            o = outs[i % LANES]
            net.filter_frames_device(dfr, nf, tab, B, 1, o[0], o[1], MAXB, o[2])

    def enter(state):
        if state != "none":
            net.monitor_begin(every=1)
            net.monitor_set_inputs(state == "on")

    def leave(state):
        if state != "none":
            net.monitor_end()

    states = ("none", "off", "on")
    t = {s: [] for s in states}
    for _ in range(reps):
        for state in states:
            enter(state)
            steps(WARMUP)
            ctx.sync()
            ctx.timer_start(0)
            steps(STEPS)
            ctx.timer_stop(0)
            t[state].append(ctx.timer_ms(0) * 1e3 / STEPS)
            leave(state)
    out = {"part": "attached", "grid": [H, WD], "batch": B, "lanes": LANES, "steps": STEPS, **{s: spread(t[s]) for s in states}}
    out["monitor_us"] = round(out["off"]["median"] - out["none"]["median"], 2)
    out["inputs_us"] = round(out["on"]["median"] - out["off"]["median"], 2)
    enter("on")
    out["kernel_us"] = kernels(ctx, lambda: steps(64), ("monitor_count", "input_count", "input_finish"))
    snap = net.monitor_read_inputs()
    out["in_frames"], out["moving_share"] = int(snap["in_frames"].sum()), round(float(mon.input_report(snap, 0)["moving_share"]), 4)
    leave("on")
    ctx.set_lanes(1)
    for d in [dfr] + [p for o in outs for p in o]:
        ctx.free(d)
    return out


def part_alone(ctx, reps, n=4096):
    rng = np.random.default_rng(1)
    out = {"part": "alone", "grid": [H, WD], "samples": n, "record_bytes": n * H * WD * 2}
    mon.begin(ctx, H, WD, 1, 0)
    mon.set_inputs(ctx, True)
    base = ctx.malloc((n + 3) * H * WD * 2 + 16)
    # sparse_off2 / sparse_off1: the same records 2 bytes and 1 byte past the allocation -- a record at a time, and byte-wise
    for name, shift in (("sparse", 0), ("uniform", 0), ("sparse_off2", 2), ("sparse_off1", 1)):
        rec = rng.integers(0, 512, (n + 3, H, WD)).astype(np.uint16)
        if name != "uniform":
            rec[rng.random(rec.shape) >= 0.02] = 0
        d = base + shift
        ctx.h2d(d, rec)
        run = lambda: mon.add_inputs_device(ctx, d, "packed", n + 3, None, n)
        run()
        us = []
        for _ in range(reps):
            ctx.timer_start(0)
            run()
            ctx.timer_stop(0)
            us.append(ctx.timer_ms(0) * 1e3)
        k = kernels(ctx, lambda: [run() for _ in range(reps)], ("input_count", "input_finish"))
        got = mon.read_inputs(ctx, reset=True)
        r = rec[3:].astype(np.int64)
        agree = bool((got["hist"][0] == np.bincount(r.ravel(), minlength=512) * (2 * reps + 1)).all() and
                     (got["moving"][0] == ((r & 0x1F8) != 0).sum(axis=0) * (2 * reps + 1)).all())
        k_us = k["input_count"] + k["input_finish"]
        out[name] = {"call": spread(us), "kernel_us": k, "kernel_gb_s": round(out["record_bytes"] / k_us / 1e3, 1),
                     "hbm_share": round(out["record_bytes"] / (k_us * 1e-6) / HBM_SPEC, 3), "agree": agree}
    ctx.free(base)
    mon.end(ctx)
    return out


def part_train(ctx, reps, n, host_frames, h=H, w=WD):
    block_n = min(4096, n)
    rng = np.random.default_rng(0)
    dens = np.array([0.002, 0.01, 0.05, 0.3])[rng.integers(0, 4, block_n)]
    block_gt = (rng.random((block_n, h, w)) < dens[:, None, None]).astype(np.uint8)
    block = np.zeros((block_n, h, w, 4), np.uint8)                      # records as a camera sends them: 2 % non-zero
    hit = rng.random((block_n, h, w)) < 0.02
    block[hit, :3] = rng.integers(0, 9, (int(hit.sum()), 3), dtype=np.uint8)
    data = T.TrainData(ctx, h, w, n)
    d_fr, d_gt, d_mass = ctx.malloc(block.nbytes), ctx.malloc(block_gt.nbytes), ctx.malloc(n * 4)
    ctx.h2d(d_fr, block)
    ctx.h2d(d_gt, block_gt)
    for at in range(0, n, block_n):
        data.append_device(d_fr, d_gt, min(block_n, n - at))
    ctx.free(d_fr)
    ctx.free(d_gt)
    nbytes = n * h * w
    out = {"part": "train" if (h * w) % 8 == 0 else "train_odd", "grid": [h, w], "frames": n, "label_bytes": nbytes, "record_bytes": 2 * nbytes}

    def timed(run):
        run()
        us = []
        for _ in range(reps):
            ctx.timer_start(0)
            run()
            ctx.timer_stop(0)
            us.append(ctx.timer_ms(0) * 1e3)
        return us

    us = timed(lambda: data.record_stats())
    k = kernels(ctx, lambda: data.record_stats(), ("input_count", "input_finish"))
    per_call = {name: round(v * -(-n // 16384), 1) for name, v in k.items()}     # (microseconds per launch x launches of a call)
    k_us = sum(per_call.values())
    out["record_stats"] = {"call": spread(us), "kernels_us_per_call": per_call, "kernel_gb_s": round(3 * nbytes / k_us / 1e3, 1),
                           "hbm_share": round(3 * nbytes / (k_us * 1e-6) / HBM_SPEC, 3)}
    us = timed(lambda: data.label_mass_device(d_mass, 0, n, None))
    out["label_mass"] = {"call": spread(us), "call_gb_s": round(nbytes / statistics.median(us) / 1e3, 1)}
    out["over_label_mass"] = round(out["record_stats"]["call"]["median"] / out["label_mass"]["call"]["median"], 2)
    m = min(host_frames, n)
    samples = np.zeros(m, T.SAMPLE)
    samples["frame"] = np.arange(m)[:, None]
    samples["label"] = np.arange(m)
    t0 = time.perf_counter()
    stack, lab = data.gather(samples)
    fr = stack[:, :h]
    r = fr[..., 0].astype(np.int64) | fr[..., 1].astype(np.int64) << 3 | fr[..., 2].astype(np.int64) << 6
    host = {"hist": np.bincount(r.ravel(), minlength=512), "hist_set": np.bincount(r[lab != 0], minlength=512),
            "moving": ((r & 0x1F8) != 0).sum(axis=0), "still_frames": int((r.reshape(m, -1) == 0).all(axis=1).sum()),
            "intra_frames": int(((r & 7) >= 5).reshape(m, -1).all(axis=1).sum())}
    host_s = time.perf_counter() - t0
    dev = data.record_stats(0, m)
    out["host"] = {"frames": m, "us_per_frame": round(host_s / m * 1e6, 2), "scaled_ms": round(host_s / m * n * 1e3, 1),
                   "over_call": round(host_s / m * n * 1e6 / out["record_stats"]["call"]["median"], 1)}
    out["routes_agree"] = all(np.array_equal(np.asarray(dev[k_]), np.asarray(host[k_])) for k_ in host)
    ctx.free(d_mass)
    data.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parts", nargs="+", default=["attached", "alone", "train", "train_odd"],
                    choices=["attached", "alone", "train", "train_odd"])
    ap.add_argument("--frames", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-frames", type=int, default=1024)
    a = ap.parse_args()
    ctx = Context(0)
    ok = True
    for part in a.parts:
        out = {"attached": lambda: part_attached(ctx, min(a.reps, 5)), "alone": lambda: part_alone(ctx, a.reps),
               "train": lambda: part_train(ctx, a.reps, a.frames, a.host_frames),
               "train_odd": lambda: part_train(ctx, a.reps, a.frames // 4, a.host_frames, 67, 119)}[part]()
        out["device"] = ctx.info()["name"]
        ok = ok and out.get("routes_agree", True) and all(v["agree"] for v in out.values() if isinstance(v, dict) and "agree" in v)
        print(json.dumps(out), flush=True)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
