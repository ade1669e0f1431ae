#!/usr/bin/env python
"""MoG label throughput on one GPU: working frames per second of covahip_mog_apply at several stream counts.

    python tools/mog_rate.py [--streams 1,8,64 --sizes 1280x720,640x360 --frames 1024 --reps 3] [--oracle-frames 3]
    python tools/mog_rate.py --grid macroblock --sizes 1920x1080 --frames 256      (960x540 working frames, 68x120 labels)
    python tools/mog_rate.py --grid macroblock --sizes 3840x2160,2560x1440 --frames 64 --min-frames 2   (the banded kernels)
    python tools/mog_rate.py --format nv12 --sizes 1280x720      (covahip_mog_apply_yuv on tight NV12 frames; also i420)
    python tools/mog_rate.py --general --sizes 1920x1080,1280x960 --frames 64 --min-frames 2 --reps 5
                                 (covahip_mog_create_any's kernels: any even size, beside the table's kernels where a size has both)
    python tools/mog_rate.py --grid macroblock --sizes 2560x1440 --labels corner,cover:1,count --no-host
                                 (the label modes side by side: one labeller each, timed call by call in turn)
    python tools/mog_rate.py --sizes 1280x720 --streams 4 --frames 256 --shadows off,drop,keep --no-host
                                 (shadow detection side by side: one labeller per mode, in the same turn-by-turn loop)
    python tools/mog_rate.py --sizes 1280x720 --streams 4 --frames 256 --frozen off,on --no-host
                                 (frozen labelling beside learning: one labeller each; the frozen one learns the warm-up call first)
    python tools/mog_rate.py --grid macroblock --sizes 1280x720,3840x2160 --streams 1 --frames 8 --background --no-host
                                 (covahip_mog_background to device memory: ms per call beside the bytes it moves)

Two cases per (source size, streams), one JSON line each:
  device   frames and labels in device memory, the call timed with HIP events (both kernels and the per-call setup);
  host     frames from (pageable) host memory, wall clock of the call: the H2D copy and the label read-back included.
Each call advances every stream by frames / streams frames, so the model is read and written once per call.  The line also has
each kernel's share of the device call (HIP-event brackets, covahip_profile_*).  --oracle-frames > 0 adds a line with the numpy
oracle's (tests/mog_ref.py) frames/s on this machine's CPU.  --format nv12 | i420 labels the same clip, converted once with a
numpy forward transform (BT.601, limited range), from tight 4:2:0 frames of 1.5 bytes per pixel; every line says its format.
--general (macroblock grid) times the general kernels ("device_general": MogLabeler(force_general=True)) at any admitted size;
at a size the table has too, the table's labeller ("device") is timed in the same process on the same frames, call by call in
turn, so the two lines compare.  --labels lists label modes (corner, cover[:N], count): every device case is timed once per mode
("device[cover:1]"), in the same turn-by-turn loop.  --shadows lists shadow modes (off, drop[:TAU], keep[:TAU]) the same way
("device[drop]"; with both lists every pair is a case); a line of a mode other than off has a "shadows" key and the clip's mean
share of shadow and foreground pixels per frame, which is what the shadow test's cost depends on.  --frozen lists off and / or on:
"device[frozen]" is a labeller that learned the warm-up call and was frozen then (covahip_mog_set_frozen), timed in the same
loop.  --background adds a line per (size, streams) with the time of covahip_mog_background of all streams into device memory,
the bytes of model it reads at most (101 per pixel) and the bytes it writes (3 per pixel).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from cova_amd import mog  # noqa: E402
from cova_amd.elements import Context  # noqa: E402


def clip(n, w, h, seed=0):
    """n distinct BGR frames: a textured background with noise and a moving block."""
    rng = np.random.default_rng(seed)
    base = rng.integers(30, 200, (h // 8, w // 8, 3)).repeat(8, 0).repeat(8, 1).astype(np.int16)
    out = np.empty((n, h, w, 3), np.uint8)
    for t in range(n):
        f = base + rng.integers(-3, 4, base.shape, dtype=np.int16)
        x = (t * w // 16) % (w - w // 8)
        f[h // 3:h // 3 + h // 6, x:x + w // 8] = (250, 40, 90)
        out[t] = np.clip(f, 0, 255).astype(np.uint8)
    return out


def to_yuv420(bgr, fmt):
    """u8 [n][h][w][3] -> u8 [n][h * w * 3 / 2]: tight NV12 or I420 frames of the same scene (BT.601, limited range, chroma as the
    mean of the 2x2 block)."""
    f = bgr.astype(np.float32)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    cb, cr = (b - y) * (0.564 * 224 / 255), (r - y) * (0.713 * 224 / 255)
    y = 16 + y * (219 / 255)

    def sub(c):
        return 128 + (c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2]) / 4

    q = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)   # noqa: E731
    n = bgr.shape[0]
    yq, uq, vq = q(y).reshape(n, -1), q(sub(cb)), q(sub(cr))
    chroma = np.stack([uq, vq], -1).reshape(n, -1) if fmt == "nv12" else np.concatenate([uq.reshape(n, -1), vq.reshape(n, -1)], 1)
    return np.concatenate([yq, chroma], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,8,64")
    ap.add_argument("--sizes", default="1280x720,640x360")
    ap.add_argument("--grid", choices=sorted(mog.GRIDS), default="reference")
    ap.add_argument("--format", choices=("bgr24",) + tuple(mog.FORMATS), default="bgr24",
                    help="bgr24: covahip_mog_apply; nv12, i420: covahip_mog_apply_yuv on the same clip as tight 4:2:0 frames")
    ap.add_argument("--frames", type=int, default=1024, help="working frames per call (all streams)")
    ap.add_argument("--min-frames", type=int, default=8, help="frames per stream and call at least (4K frames are 24.9 MB each)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--oracle-frames", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--general", action="store_true", help="the general kernels (any even size of 256 .. 4096; implies --grid macroblock)")
    ap.add_argument("--labels", default="corner", help="label modes to time, comma-separated: corner, cover[:N], count")
    ap.add_argument("--shadows", default="off", help="shadow modes to time, comma-separated: off, drop[:TAU], keep[:TAU]")
    ap.add_argument("--frozen", default="off", help="off, on or both, comma-separated: time learning and / or frozen labellers")
    ap.add_argument("--background", action="store_true", help="also time covahip_mog_background (all streams, device memory)")
    a = ap.parse_args()
    if not set(a.frozen.split(",")) <= {"off", "on"}:
        ap.error("--frozen takes off, on or off,on")
    try:
        label_modes = [(t, mog.parse_labels(t)) for t in a.labels.split(",")]
        shadow_modes = [(t, mog.parse_shadows(t)) for t in a.shadows.split(",")]
    except argparse.ArgumentTypeError as e:
        ap.error(str(e))
    if a.general:
        a.grid = "macroblock"
    parse_size = mog.parse_any_size if a.general else mog.parse_size
    for size in a.sizes.split(","):
        if not a.general and parse_size(size) not in mog.GRID_SIZES[a.grid]:
            ap.error(f"--sizes {size} needs --grid macroblock")
    ctx = Context(0)
    for size in a.sizes.split(","):
        w, h = parse_size(size)
        pool = clip(8, w, h)
        yuv = a.format != "bgr24"
        if yuv:
            pool = to_yuv420(pool, a.format)
        for S in (int(s) for s in a.streams.split(",")):
            F = max(a.min_frames, a.frames // S)
            frames = np.empty((F, S, w * h * 3 // 2) if yuv else (F, S, h, w, 3), np.uint8)
            lay = mog.yuv_tight(w, h, a.format, streams=S) if yuv else None
            for f in range(F):
                frames[f] = pool[(f + np.arange(S)) % len(pool)]
            labels = np.zeros((F, S) + (mog.label_dims_any(w, h) if a.general else mog.label_dims(w, h, a.grid)), np.uint8)
            # the labellers timed on the device, call by call in turn; the host case is the last one's
            cases = {}
            for lt, lm in label_modes:
                for st, sm in shadow_modes:
                    for fz in a.frozen.split(","):
                        tags = [t for t, plain in ((lt, "corner"), (st, "off"), ("frozen" if fz == "on" else "", "")) if t != plain]
                        tag = f"[{','.join(tags)}]" if tags else ""
                        if not a.general or (w, h) in mog.GRID_SIZES[a.grid]:
                            cases["device" + tag] = mog.MogLabeler(ctx, w, h, streams=S, grid=a.grid, labels=lm, shadows=sm)
                        if a.general:
                            cases["device_general" + tag] = mog.MogLabeler(ctx, w, h, streams=S, grid=a.grid, force_general=True,
                                                                           labels=lm, shadows=sm)
            d_f, d_l = ctx.malloc(frames.nbytes), ctx.malloc(labels.nbytes)
            ctx.h2d(d_f, frames)

            def apply_device(m):
                if yuv:
                    m.apply_yuv_device(d_f, lay, F, d_l)
                else:
                    m.apply_device(d_f, F, d_l)

            def apply_host():
                if yuv:
                    m.apply_yuv(frames, lay, F, labels=labels)
                else:
                    m.apply(frames, labels=labels)

            for case, m in cases.items():
                apply_device(m)                              # warm-up (buffers, code objects)
                if "frozen" in case:                         # from here on against the model of the warm-up call
                    m.set_frozen(True)
                    apply_device(m)
            ms = {case: [] for case in cases}
            for _ in range(a.reps):
                for case, m in cases.items():
                    ctx.timer_start(0)
                    apply_device(m)
                    ctx.timer_stop(0)
                    ms[case].append(ctx.timer_ms(0))
            for case, m in cases.items():
                ctx.profile(True)
                apply_device(m)
                prof = ctx.profile_read()
                ctx.profile(False)
                tot = sum(v[0] for k, v in prof.items() if k.startswith("mog_"))
                med = statistics.median(ms[case])
                rec = {"case": case, "format": a.format, "src": size, "grid": a.grid, "streams": S, "frames_per_stream": F,
                       "ms_per_call": round(med, 3), "frames_per_s": round(F * S / med * 1e3, 1), "ms_all": [round(x, 3) for x in ms[case]],
                       "kernel_ms": {k: round(v[0], 3) for k, v in prof.items() if k.startswith("mog_")},
                       "kernel_share_of_call": round(tot / med, 3) if med > 0 else None}
                if m.shadows is not None:
                    sh, fg = m.shadow_counts()
                    npix = m.work_w * m.work_h
                    rec.update(shadows=f"{m.shadows[0]}:{m.shadows[1]:g}", shadow_share=round(float(sh.mean()) / npix, 5),
                               foreground_share=round(float(fg.mean()) / npix, 5))
                print(json.dumps(rec), flush=True)
            m = list(cases.values())[-1]
            if a.background:
                npix = m.work_w * m.work_h
                d_b = ctx.malloc(S * npix * 3)
                bg = []
                for i in range(a.reps + 1):                  # (the first call loads the code object)
                    ctx.timer_start(0)
                    mog.L.check(m._lib.covahip_mog_background(m.handle, -1, d_b, S * npix * 3, mog.L.MEM_DEVICE), "covahip_mog_background")
                    ctx.timer_stop(0)
                    bg.append(ctx.timer_ms(0))
                ctx.free(d_b)
                med = statistics.median(bg[1:])
                print(json.dumps({"case": "background_general" if m.general else "background", "src": size, "grid": a.grid, "streams": S,
                                  "work": f"{m.work_w}x{m.work_h}", "ms_per_call": round(med, 4), "read_mb_at_most": round(S * npix * 101 / 1e6, 2),
                                  "write_mb": round(S * npix * 3 / 1e6, 2), "gb_per_s_at_most": round(S * npix * 104 / med / 1e6, 1),
                                  "ms_all": [round(x, 4) for x in bg[1:]]}), flush=True)
            ctx.free(d_f)
            ctx.free(d_l)
            if not a.no_host:
                apply_host()
                wall = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    apply_host()
                    wall.append((time.perf_counter() - t0) * 1e3)
                med = statistics.median(wall)
                print(json.dumps({"case": "host_general" if m.general else "host", "format": a.format, "src": size, "grid": a.grid, "streams": S, "frames_per_stream": F, "ms_per_call": round(med, 3),
                                  "frames_per_s": round(F * S / med * 1e3, 1), "in_gb_per_s": round(frames.nbytes / med / 1e6, 2),
                                  "ms_all": [round(x, 3) for x in wall]}), flush=True)
            for m in cases.values():
                m.close()
            del frames
    ctx.close()
    if a.oracle_frames > 0:
        from tests import mog_ref as R
        vid = clip(a.oracle_frames + 1, 1280, 720)
        mdl = R.Mog2()
        R.post(mdl.apply(R.resize_bgr(vid[0])))
        t0 = time.perf_counter()
        for f in vid[1:]:
            R.post(mdl.apply(R.resize_bgr(f)))
        dt = time.perf_counter() - t0
        print(json.dumps({"case": "oracle_cpu", "src": "1280x720", "frames": a.oracle_frames,
                          "frames_per_s": round(a.oracle_frames / dt, 2)}), flush=True)


if __name__ == "__main__":
    main()
