"""Step time of a model set (covahip_blobnet_load_set) on the carrier-frame device entry: 68x120, b = 256, three lanes.

K = 1 by load and by load_set; K = 2, 8, 32 with the stacks' models in contiguous runs and round robin; and the per-model-context
alternative (K contexts, b = 256 / K each).  Prints one JSON line per case."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from cova_amd import _lib as L                      # noqa: E402
from cova_amd import weights as W                   # noqa: E402
from cova_amd.elements import BlobNetInfer, Context  # noqa: E402

H, WD, B, LANES, STEPS, MAXB = 68, 120, 256, 3, 300, 2048
REPEATS = 2   # the cases alternate, twice: the spread of one case's two rows is the box's noise


def streams_table(b, n_streams=8):
    rows, owner, base = [], [], 0
    per = [b // n_streams + (1 if s < b % n_streams else 0) for s in range(n_streams)]
    for s, n in enumerate(per):
        rows += [[base + i + 3, base + i + 2, base + i + 1, base + i] for i in range(n)]
        owner += [s] * n
        base += n + 3
    return np.array(rows, np.int32), np.array(owner), base


def run(ctxs_nets_ids, steps=STEPS):
    """ctxs_nets_ids: [(ctx, net, table, n_frames, d_frames, ids, outs)]; one step = one call of every entry."""
    for _ in range(30):
        for c, net, tab, nf, dfr, ids, o in ctxs_nets_ids:
            net.filter_frames_device(dfr, nf, tab, tab.shape[0], 1, o[0], o[1], MAXB, o[2], model_ids=ids)
    for c, *_ in ctxs_nets_ids:
        c.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        for c, net, tab, nf, dfr, ids, o in ctxs_nets_ids:
            net.filter_frames_device(dfr, nf, tab, tab.shape[0], 1, o[0], o[1], MAXB, o[2], model_ids=ids)
    for c, *_ in ctxs_nets_ids:
        c.sync()
    return (time.perf_counter() - t0) / steps * 1e6


def setup(ctx, models, b, ids, n_streams=8, interleave=False):
    """ids(owner) -> the model of every stack from its stream; interleave: the streams' stacks round robin in the batch (what a
    batching element produces), else each stream's stacks in one run."""
    tab, owner, nf = streams_table(b, n_streams)
    if interleave:
        order = np.lexsort((owner, np.concatenate([np.arange(np.sum(owner == s)) for s in range(n_streams)])))
        tab, owner = tab[order], owner[order]
    rng = np.random.default_rng(0)
    fr = np.zeros((nf, H, WD, 4), np.uint8)
    fr[..., 0] = rng.integers(0, 8, (nf, H, WD))
    fr[..., 1:3] = rng.integers(0, 9, (nf, H, WD, 2))
    dfr = ctx.malloc(fr.nbytes)
    ctx.h2d(dfr, fr)
    outs = (ctx.malloc(b * MAXB * L.BOX_DTYPE.itemsize), ctx.malloc(b * 4), ctx.malloc(b * H * WD))
    net = BlobNetInfer(ctx, models, H, WD, max_batch=b)
    return net, tab, nf, dfr, None if ids is None else ids(owner), outs


def main():
    models = [W.random_init(100 + k, fg_bias=-1.0) for k in range(32)]
    ctx = Context(0)
    ctx.set_lanes(LANES)
    cases = [("K=1 load", models[0], None, 8, False), ("K=1 load_set", [models[0]], lambda o: np.zeros(len(o), np.uint8), 8, False)]
    for k in (2, 8, 32):
        # max(8, K) streams, stream s on model s % K; the streams' stacks in runs (contiguous) or interleaved (round robin)
        for inter in (False, True):
            cases.append((f"K={k} {'round-robin' if inter else 'contiguous'}", models[:k],
                          lambda o, k=k: (o % k).astype(np.uint8), max(8, k), inter))
    only = sys.argv[1].split(",") if len(sys.argv) > 1 else None     # e.g. "K=1 load,K=8 round-robin" (a profiling run)
    for name, ms, ids, ns, inter in [c for c in cases if only is None or c[0] in only] * REPEATS:
        net, tab, nf, dfr, idv, outs = setup(ctx, ms, B, ids, ns, inter)
        us = run([(ctx, net, tab, nf, dfr, idv, outs)])
        print(json.dumps({"case": name, "us_per_step": round(us, 1), "frames_per_s": round(B / us * 1e6)}), flush=True)
        ctx.sync()
        for d in (dfr,) + outs:
            ctx.free(d)
    ctx.close()
    if only is not None:
        return
    for k in (2, 8):   # the per-model-context alternative: K contexts of one model each, b = 256 / K each
        entries = []
        for i in range(k):
            c = Context(0)
            c.set_lanes(LANES)
            net, tab, nf, dfr, idv, outs = setup(c, models[i], B // k, None)
            entries.append((c, net, tab, nf, dfr, idv, outs))
        for _ in range(REPEATS):
            us = run(entries)
            print(json.dumps({"case": f"{k} contexts x b={B // k}", "us_per_step": round(us, 1), "frames_per_s": round(B / us * 1e6)}), flush=True)
        for c, *_ in entries:
            c.close()


if __name__ == "__main__":
    main()
