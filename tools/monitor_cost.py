"""What the serving monitor (covahip_monitor_*) costs a step: 68x120, b = 256, carrier-frame device entry on resident inputs as
bench.py builds them, three lanes, with one model and with 8 models round robin.

Three states, each measured as microseconds per step between HIP events, five repeats after a warm-up, median and spread:
  none      no monitor open            -- the launch sequence of a build without the feature;
  attach1   attached, every = 1        -- one monitor launch behind every batch;
  attach16  attached, every = 16.
The states alternate within a repeat, in one process and on one loaded model.  For the attached states the monitor kernel's own
time comes from the per-kernel profile (covahip_profile_*, events around the launch).  Prints one JSON line per model count.

`--lib PATH --states none` runs state `none` on another build of the library -- one without the monitor's symbols too (the parent
commit's): run this tree's and that one alternately on the same box, tools/ab.sh style, and compare the two `none` columns."""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from cova_amd import _lib as L                      # noqa: E402

H, WD, B, LANES, STEPS, WARMUP, REPEATS, MAXB = 68, 120, 256, 3, 300, 60, 5, 2048
EVERY = {"none": 0, "attach1": 1, "attach16": 16}


def streams_table(b, n_streams=8):
    rows, owner, base = [], [], 0
    per = [b // n_streams + (1 if s < b % n_streams else 0) for s in range(n_streams)]
    for s, n in enumerate(per):
        rows += [[base + i + 3, base + i + 2, base + i + 1, base + i] for i in range(n)]
        owner += [s] * n
        base += n + 3
    return np.array(rows, np.int32), np.array(owner), base


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--states", nargs="+", default=list(EVERY), choices=list(EVERY))
    ap.add_argument("--lib", help="another build of libcovahip.so (it may lack the monitor: --states none)")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if a.lib:
        L.LIB_PATH = a.lib
        if a.states == ["none"]:        # a build from before the monitor binds without its symbols
            for table in (L.PROTOTYPES, L.DEV_PROTOTYPES):
                for name in [n for n in table if "monitor" in n]:
                    del table[name]
    from cova_amd import synth
    from cova_amd import weights as W
    from cova_amd.elements import BlobNetInfer, Context

    models = [W.blob_like(7 + k) for k in range(8)]
    tab, owner, nf = streams_table(B)
    per = np.bincount(owner)
    fr = np.concatenate([synth.carrier_frames(int(n) + 3, H, WD, seed=0xC07A + s) for s, n in enumerate(per)])
    assert fr.shape[0] == nf
    ctx = Context(0)
    ctx.set_lanes(LANES)
    dfr = ctx.malloc(fr.nbytes)
    ctx.h2d(dfr, fr)
    # every lane writes its own outputs (two filter calls in flight must not share them)
    outs = [(ctx.malloc(B * MAXB * L.BOX_DTYPE.itemsize), ctx.malloc(B * 4), ctx.malloc(B * H * WD)) for _ in range(LANES)]

    def steps(net, ids, n):
        for i in range(n):
            o = outs[i % LANES]
            net.filter_frames_device(dfr, nf, tab, B, 1, o[0], o[1], MAXB, o[2], model_ids=ids)

    def enter(net, state):
        if EVERY[state]:
            net.monitor_begin(every=EVERY[state])

    def leave(net, state):
        if EVERY[state]:
            snap = net.monitor_read()
            net.monitor_end()
            return snap
        return None

    for k in (1, 8):
        net = BlobNetInfer(ctx, models[:k] if k > 1 else models[0], H, WD, max_batch=B)
        ids = (owner % k).astype(np.uint8) if k > 1 else None
        t = {s: [] for s in a.states}
        for _ in range(REPEATS):
            for state in a.states:
                enter(net, state)
                steps(net, ids, WARMUP)
                ctx.sync()
                ctx.timer_start(0)
                steps(net, ids, STEPS)
                ctx.timer_stop(0)
                t[state].append(ctx.timer_ms(0) * 1e3 / STEPS)
                leave(net, state)
        out = {"tag": a.tag, "lib": a.lib or "tree", "models": k, "lanes": LANES, "batch": B}
        for state in a.states:
            v = np.array(t[state])
            out[state] = {"us": [round(float(x), 2) for x in v], "median": round(float(np.median(v)), 2),
                          "spread": round(float(v.max() - v.min()), 2)}
            if EVERY[state]:                       # the kernel's own time, and that the counters moved
                enter(net, state)
                ctx.profile(True, only="monitor_count")
                steps(net, ids, 64)
                ctx.sync()
                ms, launches = ctx.profile_read().get("monitor_count", (0.0, 0))
                ctx.profile(False)
                snap = leave(net, state)
                out[state].update(kernel_us=round(ms * 1e3 / max(1, launches), 2), kernel_launches=launches,
                                  batches_counted=snap["batches_counted"], frames=int(snap["frames"].sum()),
                                  boxes_per_frame=round(float(snap["boxes"].sum()) / max(1, int(snap["frames"].sum())), 2))
        if "none" in a.states:
            for state in a.states:
                if state != "none":
                    out[state]["diff_us"] = round(out[state]["median"] - out["none"]["median"], 2)
        print(json.dumps(out), flush=True)
    ctx.sync()
    for d in [dfr] + [p for o in outs for p in o]:
        ctx.free(d)
    ctx.close()


if __name__ == "__main__":
    main()
