#!/usr/bin/env python
"""What the label-alignment counts cost on one GPU: covahip_train_data_align against the label mass over the same frames and
against the route that existed before it.

    python tools/align_cost.py [--h 68 --w 120 --frames 262144 --shift 8 --reps 10 --host-frames 1024]

Workload: a resident data set of `frames` frames (a seeded block of 4096 frames of uneven label density and sparse motion,
appended from device memory until the set is full: 2.1 GB of label bytes and 4.3 GB of records at the defaults), taken as ONE
recording; one align call over all of it at S = `shift` into device buffers.  Forms, each warmed up and then `reps` calls
between HIP events, alternating with the label-mass call so that both see the same machine:
  align       min_mv = 1, no keep map;
  align_keep  a seeded keep map that ignores a third of the grid;
  mass        covahip_train_data_label_mass over the same frames (plain and keep): what ONE pass over the label bytes costs.
and, under covahip_profile_* in a run of its own, the kernels alone (train_data_align, train_data_mass).
Per form: microseconds per call (median and min .. max over the reps) and GB/s over the bytes the counts need: 3 * h * w * frames
for align (two of records, one of labels), h * w * frames for the mass.  over_mass = align call / mass call; re-reading the
label bytes once per shift would cost 2 S + 1 mass calls, and the records on top.
  host        what the tree offered before: TrainData.gather of one sample per frame and the same counts in numpy, one boolean
              pass per shift, wall clock, over the first `host-frames` frames only; reported per frame and scaled to `frames`.
The device counts of those frames are compared with numpy's.  One JSON line.  A run without a GPU fails: there is nothing to
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


def host_counts(frames, gt, S, keep):
    """The counts of one recording in numpy: frames u8 [n][h][w][4] (fields already clipped), min_mv = 1."""
    n = len(gt)
    mv = (np.maximum(frames[..., 1], frames[..., 2]) >= 1) & (keep != 0)[None]
    st = (gt != 0) & (keep != 0)[None]
    mv, st = mv.reshape(n, -1), st.reshape(n, -1)
    both = np.zeros((n, 2 * S + 1), np.uint32)
    for j in range(2 * S + 1):
        s = j - S
        a, b = max(0, -s), min(n, n - s)
        if a < b:
            both[a:b, j] = (mv[a:b] & st[a + s:b + s]).sum(axis=1)
    return both, mv.sum(axis=1).astype(np.uint32), st.sum(axis=1).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h", type=int, default=68)
    ap.add_argument("--w", type=int, default=120)
    ap.add_argument("--frames", type=int, default=262144)
    ap.add_argument("--shift", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-frames", type=int, default=1024)
    a = ap.parse_args()
    h, w, n, S = a.h, a.w, a.frames, a.shift
    wide = 2 * S + 1
    block_n = min(4096, n)
    ctx = Context(0)
    rng = np.random.default_rng(0)
    dens = np.array([0.002, 0.01, 0.05, 0.3])[rng.integers(0, 4, block_n)]
    block_gt = (rng.random((block_n, h, w)) < dens[:, None, None]).astype(np.uint8)
    block = rng.integers(0, 9, (block_n, h, w, 4), dtype=np.uint8)
    block[..., 1:3] *= (rng.random((block_n, h, w)) < dens[:, None, None])[..., None]   # vectors on as many macroblocks as labels
    keep = (rng.random((h, w)) > 1 / 3).astype(np.uint8)
    data = T.TrainData(ctx, h, w, n)
    d_fr, d_gt = ctx.malloc(block.nbytes), ctx.malloc(block_gt.nbytes)
    d_both, d_mov, d_lab, d_mass = ctx.malloc(n * wide * 4), ctx.malloc(n * 4), ctx.malloc(n * 4), ctx.malloc(n * 4)
    ctx.h2d(d_fr, block)
    ctx.h2d(d_gt, block_gt)
    for at in range(0, n, block_n):
        data.append_device(d_fr, d_gt, min(block_n, n - at))
    ctx.free(d_fr)
    ctx.free(d_gt)

    def align(kp):
        data.align_device(d_both, d_mov, d_lab, 0, n, S, keep=kp)

    def mass(kp):
        data.label_mass_device(d_mass, 0, n, kp)

    def timed(kp):
        """(align us, mass us) per rep, the two calls alternating."""
        align(kp)                                               # warm-up: code objects, the keep table
        mass(kp)
        us = ([], [])
        for _ in range(a.reps):
            for q, call in enumerate((align, mass)):
                ctx.timer_start(0)
                call(kp)
                ctx.timer_stop(0)
                us[q].append(ctx.timer_ms(0) * 1e3)
        return us

    def kernel_us(kp):
        ctx.profile(True)
        for _ in range(a.reps):
            align(kp)
            mass(kp)
        ctx.sync()
        prof = ctx.profile_read()
        ctx.profile(False)
        return [prof[k][0] * 1e3 / prof[k][1] for k in ("train_data_align", "train_data_mass")]

    def form(us, k_us, nbytes):
        med = statistics.median(us)
        return {"call_us_median": round(med, 1), "call_us_min": round(min(us), 1), "call_us_max": round(max(us), 1),
                "call_gb_s": round(nbytes / med / 1e3, 1), "kernel_us": round(k_us, 1), "kernel_gb_s": round(nbytes / k_us / 1e3, 1),
                "hbm_share": round(nbytes / (k_us * 1e-6) / HBM_SPEC, 3)}

    mb = n * h * w
    out = {"tool": "align_cost", "device": ctx.info()["name"], "grid": [h, w], "frames": n, "max_shift": S, "align_bytes": 3 * mb,
           "label_bytes": mb, "reps": a.reps}
    for name, kp in (("", None), ("_keep", keep)):
        (us_a, us_m), (k_a, k_m) = timed(kp), kernel_us(kp)
        out["align" + name], out["mass" + name] = form(us_a, k_a, 3 * mb), form(us_m, k_m, mb)
        out["align" + name]["over_mass"] = round(statistics.median(us_a) / statistics.median(us_m), 2)
        out["align" + name]["kernel_over_mass"] = round(k_a / k_m, 2)
    out["mass_calls_of_a_reread"] = wide
    m = min(a.host_frames, n)
    samples = np.zeros(m, T.SAMPLE)
    samples["frame"] = np.arange(m)[:, None]
    samples["label"] = np.arange(m)
    t0 = time.perf_counter()
    stack, lab = data.gather(samples)
    host = host_counts(stack[:, :h], lab, S, keep)
    host_s = time.perf_counter() - t0
    got = data.align(0, m, S, keep=keep)
    same = all(bool((g == x).all()) for g, x in zip(got, host))
    out["host"] = {"frames": m, "us_per_frame": round(host_s / m * 1e6, 2), "scaled_ms": round(host_s / m * n * 1e3, 1),
                   "over_keep_call": round(host_s / m * n * 1e6 / out["align_keep"]["call_us_median"], 1)}
    out["routes_agree"] = same
    print(json.dumps(out))
    for p in (d_both, d_mov, d_lab, d_mass):
        ctx.free(p)
    data.close()
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
