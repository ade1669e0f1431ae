"""Calibrate a camera's mask threshold and area threshold: score the deployed forward's logits against labels on the GPU.

covahip_post_sweep (include/covahip.h, "Calibration") counts, for T mask thresholds x A area thresholds in one pass, the pixels
and the boxes that serving would emit at each setting and how they meet the labelled objects.  This module marshals that call
(sweep / sweep_device / add), picks the operating point (choose), and keeps it in a small JSON sidecar (save_post / load_post)
whose values go to BlobNetInfer.set_post and to the cc-threshold of bboxcc / cova.

    python -m cova_amd.calibrate --weights blobnet.cvhw -o post.json RECORDS...

runs the records through BlobNetInfer (the fp16 forward the threshold will be applied to), sweeps every batch with the logits
left on the device, prints the table and the choice.

The ignore region can be measured too.  covahip_post_heat_* ("Ignore region from heat") count per macroblock how often the
forward and the labels fire over all samples (heat_begin / heat_add_device / heat_end, heat, add_heat); ignore_from_heat marks
the macroblocks that fire in at least a given share of the samples -- a burned-in clock, not a vehicle -- and rects_from_keep
turns the keep map into the pixel rectangles the sidecar, load_post and pad-ignore-rects take.  --auto-ignore RATE does all of
it before the sweep.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys

import numpy as np

from . import _lib as L
from .elements import BlobNetInfer, keep_from_rects

DEFAULT_PROBS = tuple(round(0.05 * k, 2) for k in range(1, 20))      # 0.05 ... 0.95, 0.5 among them
DEFAULT_AREAS = (1, 2, 4, 8, 16, 30)


def logit_thresholds(thresholds=None, prob_thresholds=None) -> np.ndarray:
    """The float32 logit thresholds of a sweep, ascending: `thresholds` as given, or probabilities converted with the logit
    function of BlobNetInfer.set_post (post_logit_thresh)."""
    if (thresholds is None) == (prob_thresholds is None):
        raise ValueError("give thresholds or prob_thresholds, not both")
    if prob_thresholds is not None:
        vals = [BlobNetInfer.post_logit_thresh(prob_thresh=p) for p in prob_thresholds]
    else:
        vals = [BlobNetInfer.post_logit_thresh(logit_thresh=t) for t in thresholds]
    out = np.asarray(vals, dtype=np.float32)
    if out.ndim != 1 or out.size == 0 or not np.isfinite(out).all() or (np.diff(out) <= 0).any():
        raise ValueError("thresholds must be finite and strictly ascending")
    return out


def _iou(iou):
    num, den = (int(iou[0]), int(iou[1])) if isinstance(iou, (tuple, list)) else _fraction(float(iou))
    if not 1 <= num <= den:
        raise ValueError(f"iou must be a fraction in (0, 1], got {iou!r}")
    return num, den


def _fraction(x: float):
    """A decimal IoU such as 0.1 as the exact fraction the hit rule takes (1 / 10)."""
    from fractions import Fraction
    f = Fraction(repr(x)).limit_denominator(10000)
    return f.numerator, f.denominator


def sweep_device(ctx, d_logits, d_gt, n, h, w, thresholds=None, areas=DEFAULT_AREAS, *, prob_thresholds=None, keep=None,
                 gt_area=1, iou=(1, 10), max_boxes=256, chunk=0, mem_kind=L.MEM_DEVICE) -> dict:
    """covahip_post_sweep on n samples: logits f32 [n][h][w] and labels u8 [n][h][w] as device pointers.  Returns the tables
    pixel i64 [T][3] (tp, fp, fn), pred / pred_true / gt_found i64 [T][A], truncated i64 [T], the scalars samples, gt_objects,
    gt_truncated, and the sweep's grid (logit_thresh, area_thresh, gt_area, iou, max_boxes, h, w)."""
    th = logit_thresholds(thresholds, prob_thresholds)
    ar = np.ascontiguousarray(areas, dtype=np.int32)
    num, den = _iou(iou)
    cfg = L.SweepCfg(h, w, th.size, th.ctypes.data, ar.size, ar.ctypes.data, int(gt_area), num, den, int(max_boxes), None, int(chunk))
    if keep is not None:
        keep = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
        if keep.shape != (h, w):
            raise ValueError(f"keep must be [{h}][{w}], got {keep.shape}")
        cfg.keep = keep.ctypes.data
    pixel = np.zeros((th.size, 3), np.int64)
    cells = np.zeros((th.size, ar.size, 3), np.int64)
    trunc = np.zeros(th.size, np.int64)
    res = L.SweepResult()
    L.check(L.lib().covahip_post_sweep(ctx.handle, C.byref(cfg), d_logits, d_gt, n, mem_kind, pixel.ctypes.data, cells.ctypes.data,
                                       trunc.ctypes.data, C.byref(res)), "covahip_post_sweep", ctx.handle)
    return {"pixel": pixel, "pred": cells[..., 0].copy(), "pred_true": cells[..., 1].copy(), "gt_found": cells[..., 2].copy(),
            "truncated": trunc, "samples": int(res.samples), "gt_objects": int(res.gt_objects), "gt_truncated": int(res.gt_truncated),
            "logit_thresh": th, "area_thresh": ar, "gt_area": int(gt_area), "iou": (num, den), "max_boxes": int(max_boxes),
            "h": int(h), "w": int(w)}


def sweep(ctx, logits, gt, thresholds=None, areas=DEFAULT_AREAS, **kw) -> dict:
    """sweep_device on host arrays: logits f32 [n][h][w], gt u8 [n][h][w]."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    gt = np.ascontiguousarray(gt, dtype=np.uint8)
    if logits.ndim != 3 or gt.shape != logits.shape:
        raise ValueError(f"logits [n][h][w] and gt of the same shape expected, got {logits.shape} and {gt.shape}")
    n, h, w = logits.shape
    return sweep_device(ctx, logits.ctypes.data, gt.ctypes.data, n, h, w, thresholds, areas, mem_kind=L.MEM_HOST, **kw)


# ------------------------------------------------------------------------------------------------------------------ heat
def heat_begin(ctx, h, w, thresholds=None, *, prob_thresholds=None) -> np.ndarray:
    """covahip_post_heat_begin: opens a heat of grid [h][w] on ctx (zeroed counters; an open one starts over).  -> the float32
    logit thresholds."""
    th = logit_thresholds(thresholds, prob_thresholds)
    cfg = L.HeatCfg(int(h), int(w), th.size, th.ctypes.data)
    L.check(L.lib().covahip_post_heat_begin(ctx.handle, C.byref(cfg)), "covahip_post_heat_begin", ctx.handle)
    return th


def heat_add_device(ctx, d_logits, d_gt, n, mem_kind=L.MEM_DEVICE) -> None:
    """covahip_post_heat_add: n samples, logits f32 [n][h][w] and labels u8 [n][h][w] as device pointers.  Synchronous."""
    L.check(L.lib().covahip_post_heat_add(ctx.handle, d_logits, d_gt, int(n), mem_kind), "covahip_post_heat_add", ctx.handle)


def heat_set_stage(ctx, nbytes: int = 0) -> None:
    """Developer switch (include/covahip_dev.h): device bytes of host samples staged per piece of a heat_add, 0 = the default."""
    L.check(L.lib().covahip_dev_heat_set_stage(ctx.handle, int(nbytes)), "covahip_dev_heat_set_stage")


def heat_end(ctx, h, w, th) -> dict:
    """covahip_post_heat_end: reads the open heat of grid [h][w] with thresholds th out and closes it.  -> fire, both i64
    [T][h][w], gt i64 [h][w], samples, logit_thresh."""
    th = np.asarray(th, np.float32)
    fire, both = np.zeros((th.size, h, w), np.int64), np.zeros((th.size, h, w), np.int64)
    gtf = np.zeros((h, w), np.int64)
    samples = C.c_int64()
    L.check(L.lib().covahip_post_heat_end(ctx.handle, fire.ctypes.data, both.ctypes.data, gtf.ctypes.data, C.byref(samples)),
            "covahip_post_heat_end", ctx.handle)
    return {"fire": fire, "both": both, "gt": gtf, "samples": int(samples.value), "logit_thresh": th}


def heat(ctx, logits, gt, thresholds=None, *, prob_thresholds=None) -> dict:
    """The heat of host arrays: logits f32 [n][h][w], gt u8 [n][h][w]."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    gt = np.ascontiguousarray(gt, dtype=np.uint8)
    if logits.ndim != 3 or gt.shape != logits.shape:
        raise ValueError(f"logits [n][h][w] and gt of the same shape expected, got {logits.shape} and {gt.shape}")
    n, h, w = logits.shape
    th = heat_begin(ctx, h, w, thresholds, prob_thresholds=prob_thresholds)
    heat_add_device(ctx, logits.ctypes.data, gt.ctypes.data, n, L.MEM_HOST)
    return heat_end(ctx, h, w, th)


def add_heat(a: dict, b: dict) -> dict:
    """The heat of both sample sets together.  Raises when the grids or the thresholds differ."""
    if a["fire"].shape != b["fire"].shape or not np.array_equal(a["logit_thresh"], b["logit_thresh"]):
        raise ValueError("heats of different grids or thresholds cannot be added")
    out = dict(a)
    for k in ("fire", "both", "gt", "samples"):
        out[k] = a[k] + b[k]
    return out


def ignore_from_heat(heat: dict, rate, *, at=0, source="either", dilate=0, max_share=0.25) -> np.ndarray:
    """The keep map u8 [h][w] that ignores the persistent macroblocks of a heat.  With rate = num / den (an exact fraction, as
    the hit rule's IoU), a macroblock is hot when fire[at] * den >= num * samples (source "pred"), when gt * den >= num *
    samples ("labels"), or when either holds ("either"); dilate grows the hot set by that many 8-neighbour steps; keep = ~hot.
    at defaults to the lowest threshold: fire falls as the threshold rises, so what is persistent at any candidate is persistent
    there, and the region does not depend on the cell the sweep then picks.  ValueError for an empty heat, and for a region
    larger than max_share of the grid: a rate that blinds that much of the camera is a mistake, not a calibration."""
    num, den = (int(rate[0]), int(rate[1])) if isinstance(rate, (tuple, list)) else _fraction(float(rate))
    if not 1 <= num <= den:
        raise ValueError(f"rate must be a fraction in (0, 1], got {rate!r}")
    if source not in ("either", "labels", "pred"):
        raise ValueError(f"source must be either, labels or pred, got {source!r}")
    samples = int(heat["samples"])
    if samples <= 0:
        raise ValueError("the heat has no samples")
    T = heat["fire"].shape[0]
    if not -T <= int(at) < T:
        raise ValueError(f"at must index one of the {T} thresholds, got {at}")
    pred = heat["fire"][int(at)].astype(np.int64) * den >= num * samples
    lab = heat["gt"].astype(np.int64) * den >= num * samples
    hot = pred if source == "pred" else lab if source == "labels" else pred | lab
    h, w = hot.shape
    for _ in range(int(dilate)):
        pad = np.zeros((h + 2, w + 2), bool)
        pad[1:-1, 1:-1] = hot
        hot = np.zeros((h, w), bool)
        for dy in range(3):
            for dx in range(3):
                hot |= pad[dy:dy + h, dx:dx + w]
    n_hot = int(hot.sum())
    if n_hot > max_share * h * w:
        raise ValueError(f"{n_hot} of {h * w} macroblocks reach rate {num}/{den}: more than the share {max_share} an ignore region may take")
    return (~hot).astype(np.uint8)


def rects_from_keep(keep, unit: int = 16) -> list:
    """The ignored macroblocks of a keep map as pixel rectangles (left, top, width, height): macroblock-aligned, disjoint, ordered
    by (top, left).  Each row's runs of ignored macroblocks become rectangles, and a run that recurs unchanged in consecutive
    rows is one rectangle.  keep_from_rects(h, w, rects_from_keep(keep)) == keep for every keep map."""
    ign = np.asarray(keep) == 0
    if ign.ndim != 2:
        raise ValueError(f"keep must be [h][w], got {ign.shape}")
    h, w = ign.shape
    open_, rects = {}, []                                   # (x0, x1) -> first row of the rectangle still growing
    for y in range(h + 1):
        runs = set()
        if y < h:
            edge = np.flatnonzero(np.diff(np.concatenate(([0], ign[y].astype(np.int8), [0]))))
            runs = {(int(a), int(b)) for a, b in zip(edge[::2], edge[1::2])}
        for (x0, x1), y0 in list(open_.items()):
            if (x0, x1) not in runs:
                rects.append((x0 * unit, y0 * unit, (x1 - x0) * unit, (y - y0) * unit))
                del open_[(x0, x1)]
        for r in runs:
            open_.setdefault(r, y)
    return sorted(rects, key=lambda r: (r[1], r[0]))


def heat_summary(heat: dict, rate) -> str:
    """Per threshold, the macroblocks whose predictions reach the rate; and the macroblocks whose labels do."""
    num, den = (int(rate[0]), int(rate[1])) if isinstance(rate, (tuple, list)) else _fraction(float(rate))
    need = num * int(heat["samples"])
    lab = int((heat["gt"].astype(np.int64) * den >= need).sum())
    lines = [f"macroblocks that fire in at least {num}/{den} of {heat['samples']} samples (of {heat['gt'].size})",
             "  logit     prob |   pred  labels"]
    for t, thr in enumerate(heat["logit_thresh"]):
        lines.append(f"{float(thr):8.4f} {1.0 / (1.0 + np.exp(-float(thr))):7.4f} | {int((heat['fire'][t].astype(np.int64) * den >= need).sum()):6d} {lab:7d}")
    return "\n".join(lines)


_TABLES = ("pixel", "pred", "pred_true", "gt_found", "truncated")
_SCALARS = ("samples", "gt_objects", "gt_truncated")
_GRID = ("logit_thresh", "area_thresh", "gt_area", "iou", "max_boxes", "h", "w")


def add(a: dict, b: dict) -> dict:
    """The result of both sample sets together (the counts are additive).  Raises when the two sweeps' grids differ."""
    for k in _GRID:
        if not np.array_equal(np.asarray(a[k]), np.asarray(b[k])):
            raise ValueError(f"sweeps of different grids cannot be added: {k} differs")
    out = dict(a)
    for k in _TABLES:
        out[k] = a[k] + b[k]
    for k in _SCALARS:
        out[k] = a[k] + b[k]
    return out


def _ratio(num, den) -> float:
    return float(num) / float(den) if den else 1.0


def choose(result: dict, min_recall: float = 0.95) -> dict:
    """The operating point of a sweep.  Object recall of a cell = gt_found / gt_objects (1.0 when there are no labelled objects:
    nothing can be missed), object precision = pred_true / pred (1.0 when pred == 0).  Among the cells with recall >= min_recall
    the highest precision wins; ties go to the higher threshold, then to the larger area.  If no cell reaches min_recall the
    highest recall wins with the same tie-break and "met" is False."""
    T, A = result["pred"].shape
    cells = []
    for t in range(T):
        for a in range(A):
            rec = _ratio(result["gt_found"][t, a], result["gt_objects"])
            prec = _ratio(result["pred_true"][t, a], result["pred"][t, a])
            cells.append((rec, prec, t, a))
    ok = [c for c in cells if c[0] >= min_recall]
    if ok:
        rec, prec, t, a = max(ok, key=lambda c: (c[1], c[2], c[3]))
    else:
        rec, prec, t, a = max(cells, key=lambda c: (c[0], c[2], c[3]))
    tp, fp, fn = (int(v) for v in result["pixel"][t])
    return {"met": bool(ok), "min_recall": float(min_recall), "t": t, "a": a,
            "logit_thresh": float(result["logit_thresh"][t]), "cc_threshold": int(result["area_thresh"][a]),
            "object_recall": rec, "object_precision": prec,
            "pixel_recall": _ratio(tp, tp + fn), "pixel_precision": _ratio(tp, tp + fp),
            "pred": int(result["pred"][t, a]), "pred_true": int(result["pred_true"][t, a]),
            "gt_found": int(result["gt_found"][t, a]), "gt_objects": int(result["gt_objects"]),
            "truncated": int(result["truncated"][t]), "samples": int(result["samples"]),
            "grid": {"logit_thresh": [float(v) for v in result["logit_thresh"]], "area_thresh": [int(v) for v in result["area_thresh"]],
                     "gt_area": int(result["gt_area"]), "iou": [int(v) for v in result["iou"]], "max_boxes": int(result["max_boxes"])}}


def save_post(path, choice: dict, ignore_rects=(), auto_ignore=None) -> None:
    """The sidecar of a calibrated camera: logit_thresh (and the same threshold as a probability), cc_threshold, ignore_rects
    (pixel rectangles left, top, width, height), the scores of the chosen cell and the sweep's grid, as JSON.  auto_ignore (a
    dict, when the rectangles were derived from a heat) is recorded under a key of its own, which load_post does not read."""
    doc = {"format": "covahip-post-1", "logit_thresh": float(choice["logit_thresh"]),
           "prob_thresh": 1.0 / (1.0 + float(np.exp(-np.float64(choice["logit_thresh"])))),   # what pad-mask-threshold takes
           "cc_threshold": int(choice["cc_threshold"]),
           "ignore_rects": [[int(v) for v in r] for r in ignore_rects],
           "scores": {k: choice[k] for k in ("met", "min_recall", "object_recall", "object_precision", "pixel_recall", "pixel_precision",
                                             "pred", "pred_true", "gt_found", "gt_objects", "truncated", "samples") if k in choice},
           "grid": choice.get("grid", {})}
    if auto_ignore is not None:
        doc["auto_ignore"] = auto_ignore
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def load_post(path, h_mb: int, w_mb: int):
    """-> (set_post_kwargs, cc_threshold): net.set_post(model, **set_post_kwargs) and net.set_area(model, cc_threshold) -- what
    apply_post does -- or filter(..., cc_threshold) for a net that serves one camera.  The keep map is rebuilt from the sidecar's
    rectangles with keep_from_rects (None when it has none)."""
    with open(path) as f:
        doc = json.load(f)
    if doc.get("format") != "covahip-post-1":
        raise ValueError(f"{path}: not a calibration sidecar")
    rects = [tuple(r) for r in doc.get("ignore_rects", [])]
    kw = {"logit_thresh": float(np.float32(doc["logit_thresh"])), "keep": keep_from_rects(h_mb, w_mb, rects) if rects else None}
    return kw, int(doc["cc_threshold"])


def apply_post(net, model: int, path_or_doc) -> int:
    """Serves `model` of net (a BlobNetInfer) as calibrated: set_post(mask threshold, ignore region) and set_area(cc_threshold)
    from a sidecar file, or from (set_post_kwargs, cc_threshold) as load_post returns it.  -> the cc_threshold applied."""
    kw, cc = load_post(path_or_doc, net.h, net.w) if isinstance(path_or_doc, (str, bytes)) or hasattr(path_or_doc, "__fspath__") else path_or_doc
    net.set_post(model, **kw)
    net.set_area(model, int(cc))
    return int(cc)


def serving_hint(logit_thresh: float, cc_threshold: int, ignore_rects=()) -> str:
    """The element properties that serve a calibrated camera: on a pad of a blobnetfilter model set, and as the whole element's."""
    prob = 1.0 / (1.0 + float(np.exp(-np.float64(logit_thresh))))   # the element takes the threshold as a probability
    rects = "+".join(",".join(str(v) for v in r) for r in ignore_rects)
    return (f"blobnetfilter pad-mask-threshold=\"IDX={prob:.9g}\"" + (f" pad-ignore-rects=\"IDX={rects}\"" if rects else "") +
            f" pad-cc-threshold=\"IDX={int(cc_threshold)}\"   cova / bboxcc cc-threshold={int(cc_threshold)}")


def format_table(result: dict) -> str:
    """Object recall / precision per cell and pixel recall / precision per threshold, as text."""
    ar = result["area_thresh"]
    lines = ["object recall / precision per (threshold, area); pixel recall / precision per threshold",
             "  logit     prob | " + " ".join(f"   area>={int(a):<4d}" for a in ar) + " |     pixel    trunc"]
    for t, thr in enumerate(result["logit_thresh"]):
        tp, fp, fn = (int(v) for v in result["pixel"][t])
        row = " ".join(f"{_ratio(result['gt_found'][t, a], result['gt_objects']):.3f}/{_ratio(result['pred_true'][t, a], result['pred'][t, a]):.3f}"
                       for a in range(len(ar)))
        lines.append(f"{float(thr):8.4f} {1.0 / (1.0 + np.exp(-float(thr))):7.4f} | {row} | {_ratio(tp, tp + fn):.3f}/{_ratio(tp, tp + fp):.3f} {int(result['truncated'][t]):6d}")
    lines.append(f"samples {result['samples']}, labelled objects {result['gt_objects']}, samples with truncated labels {result['gt_truncated']}")
    return "\n".join(lines)


def calibrate_records(ctx, weights_flat, stacks, labels, h_mb, w_mb, thresholds=None, areas=DEFAULT_AREAS, *, prob_thresholds=None,
                      keep=None, batch=256, heat_only=False, **kw) -> dict:
    """Sweep of a held-out set through the deployed forward: stacks u8 [n][4 h][w][4] and labels u8 [n][h][w] go to the device
    in batches, BlobNetInfer writes the logits there, covahip_post_sweep reads them there.  With heat_only the same loop feeds
    covahip_post_heat_add instead (no keep map, no areas) and the heat is returned."""
    n = stacks.shape[0]
    batch = max(1, min(batch, n))
    net = BlobNetInfer(ctx, weights_flat, h_mb, w_mb, max_batch=batch)
    hw = h_mb * w_mb
    d_stack, d_gt, d_logits = ctx.malloc(batch * 16 * hw), ctx.malloc(batch * hw), ctx.malloc(batch * hw * 4)
    total = None
    try:
        if heat_only:
            th = heat_begin(ctx, h_mb, w_mb, thresholds, prob_thresholds=prob_thresholds)
        for s0 in range(0, n, batch):
            b = min(batch, n - s0)
            ctx.h2d(d_stack, stacks[s0:s0 + b])
            ctx.h2d(d_gt, labels[s0:s0 + b])
            net.infer_device(d_stack, b, d_logits, None)
            if heat_only:
                heat_add_device(ctx, d_logits, d_gt, b)
                continue
            r = sweep_device(ctx, d_logits, d_gt, b, h_mb, w_mb, thresholds, areas, prob_thresholds=prob_thresholds, keep=keep, **kw)
            total = r if total is None else add(total, r)
        if heat_only:
            total = heat_end(ctx, h_mb, w_mb, th)
    finally:
        ctx.sync()
        for d in (d_stack, d_gt, d_logits):
            ctx.free(d)
    return total


def _rect(text):
    parts = [int(v) for v in text.split(",")]
    if len(parts) != 4:
        raise argparse.ArgumentTypeError("a rectangle is LEFT,TOP,WIDTH,HEIGHT in pixels")
    return tuple(parts)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cova_amd.calibrate", description=__doc__.split("\n")[0])
    ap.add_argument("records", nargs="+", metavar="RECORDS", help="held-out TFRecord files written by tfrecordsink gt=LABELS")
    ap.add_argument("--weights", required=True, help="the camera's weight file (CVHW)")
    ap.add_argument("--h-mb", type=int, default=45)
    ap.add_argument("--w-mb", type=int, default=80)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--ignore-rects", nargs="*", type=_rect, default=[], metavar="L,T,W,H",
                    help="pixel rectangles of the camera's ignore region (set_post's keep map, blobnetfilter's pad-ignore-rects)")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--thresholds", nargs="+", type=float, metavar="LOGIT", help="mask thresholds as logits, ascending")
    g.add_argument("--probs", nargs="+", type=float, metavar="P", help="mask thresholds as probabilities, ascending "
                   "(default: 0.05, 0.10, ... 0.95, which has 0.5, the reference's threshold)")
    ap.add_argument("--areas", nargs="+", type=int, default=list(DEFAULT_AREAS), metavar="MB",
                    help="cc-threshold candidates in macroblocks, ascending (default: 1 2 4 8 16 30)")
    ap.add_argument("--gt-area", type=int, default=1, help="a label component of at least this many macroblocks is an object")
    ap.add_argument("--min-recall", type=float, default=0.95, help="object recall the chosen cell must reach")
    ap.add_argument("--iou", type=float, default=0.1, help="IoU at which a box and a labelled object hit each other")
    ap.add_argument("--max-boxes", type=int, default=256)
    ap.add_argument("--batch", type=int, default=256, help="samples per forward")
    ap.add_argument("--auto-ignore", type=float, metavar="RATE", help="derive the ignore region from per-macroblock heat: ignore "
                    "the macroblocks that fire in at least this share of the samples (added to --ignore-rects)")
    ap.add_argument("--auto-ignore-source", choices=("either", "labels", "pred"), default="either",
                    help="what has to reach the rate: the labels, the predictions at the lowest threshold, or either")
    ap.add_argument("--auto-ignore-dilate", type=int, default=0, metavar="N", help="grow the derived region by N macroblocks")
    ap.add_argument("--heat-out", metavar="FILE.npz", help="write the heat (fire, both, gt, samples, logit_thresh); needs --auto-ignore")
    ap.add_argument("-o", "--output", help="sidecar to write (JSON: logit_thresh, cc_threshold, ignore_rects, scores)")
    a = ap.parse_args(argv)
    if a.auto_ignore is None and (a.heat_out or a.auto_ignore_dilate or a.auto_ignore_source != "either"):
        ap.error("--auto-ignore-source, --auto-ignore-dilate and --heat-out need --auto-ignore RATE")
    if a.auto_ignore is not None and not 0.0 < a.auto_ignore <= 1.0:
        ap.error("--auto-ignore takes a rate in (0, 1]")
    if a.auto_ignore_dilate < 0:
        ap.error("--auto-ignore-dilate must not be negative")
    return a


def main(argv=None) -> int:
    from . import train
    from . import weights as W
    from .elements import Context
    a = parse_args(argv)
    frames, gt = train.read_tfrecords(a.records, a.h_mb, a.w_mb)
    stacks, labels = train.slide(frames, gt)
    if stacks.shape[0] == 0:
        print("no complete sample in the records", file=sys.stderr)
        return 2
    with open(a.weights, "rb") as f:
        flat = W.from_bytes(f.read())
    keep = keep_from_rects(a.h_mb, a.w_mb, a.ignore_rects) if a.ignore_rects else None
    probs = a.probs if a.probs else (None if a.thresholds else DEFAULT_PROBS)
    ctx = Context(a.device)
    auto, rects_out = None, list(a.ignore_rects)
    try:
        if a.auto_ignore is not None:
            # pass 1: the heat of the whole grid (the user's rectangles hide nothing from it), then the region it gives
            ht = calibrate_records(ctx, flat, stacks, labels, a.h_mb, a.w_mb, a.thresholds, prob_thresholds=probs, batch=a.batch,
                                   heat_only=True)
            print(heat_summary(ht, a.auto_ignore))
            derived = ignore_from_heat(ht, a.auto_ignore, source=a.auto_ignore_source, dilate=a.auto_ignore_dilate)
            keep = derived if keep is None else derived & keep
            rects_out = rects_from_keep(keep)
            num, den = _fraction(a.auto_ignore)
            auto = {"rate": [num, den], "source": a.auto_ignore_source, "dilate": a.auto_ignore_dilate,
                    "logit_thresh": float(ht["logit_thresh"][0]), "samples": ht["samples"],
                    "macroblocks_ignored": int((derived == 0).sum()), "user_rects": [[int(v) for v in r] for r in a.ignore_rects]}
            print(f"auto-ignore: {auto['macroblocks_ignored']} macroblocks reach {num}/{den} ({a.auto_ignore_source}, dilate "
                  f"{a.auto_ignore_dilate}); ignore region now {int((keep == 0).sum())} macroblocks in {len(rects_out)} rectangles")
            if a.heat_out:
                np.savez_compressed(a.heat_out, **ht)
                print(f"wrote {a.heat_out}")
            if not rects_out:
                keep = None
        res = calibrate_records(ctx, flat, stacks, labels, a.h_mb, a.w_mb, a.thresholds, a.areas, prob_thresholds=probs, keep=keep,
                                batch=a.batch, gt_area=a.gt_area, iou=a.iou, max_boxes=a.max_boxes)
    finally:
        ctx.close()
    ch = choose(res, a.min_recall)
    print(format_table(res))
    print(f"choice: logit_thresh {ch['logit_thresh']:.6g} cc_threshold {ch['cc_threshold']}  object recall {ch['object_recall']:.4f} "
          f"precision {ch['object_precision']:.4f}  pixel recall {ch['pixel_recall']:.4f} precision {ch['pixel_precision']:.4f}  "
          f"pred {ch['pred']} truncated {ch['truncated']}" + ("" if ch["met"] else f"  (no cell reaches recall {a.min_recall})"))
    rects = ";".join(",".join(str(v) for v in r) for r in rects_out)
    print(f"set_post(model, logit_thresh={ch['logit_thresh']!r}" + (f", keep=keep_from_rects({a.h_mb}, {a.w_mb}, {list(rects_out)!r})" if rects else "") + ")")
    print(f"set_area(model, {ch['cc_threshold']})")
    print(serving_hint(ch["logit_thresh"], ch["cc_threshold"], rects_out))
    if a.output:
        save_post(a.output, ch, rects_out, auto)
        print(f"wrote {a.output}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
