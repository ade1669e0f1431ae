"""Serving monitor: how the deployed models behave today, from what every filter step already has on the device.

covahip_monitor_* (include/covahip.h, "Serving monitor") count, per model of a set, how often each macroblock of the served mask
fires, how many boxes a frame emits and how large they are -- integer counts, exact, with no decode and no labels.  Attached to a
BlobNetInfer (monitor_begin / monitor_read / monitor_end there) the counting rides behind the filter batches on their own lanes;
begin / add / read / end here are the stand-alone form on a Context, fed with masks, counts and boxes from anywhere.

A snapshot (the dict read returns) answers an operator's questions:

    report(snapshot, model, baseline)        frames, foreground share, boxes per frame, truncation, the area histogram -- and,
                                             against a calibration sidecar, whether the box rate has drifted from what
                                             calibration recorded (scores.pred / scores.samples)
    persistent_rects(snapshot, model, rate)  macroblocks that fire in at least `rate` of the frames -- a new overlay, a parked
                                             lorry -- as the pixel rectangles ignore_rects / pad-ignore-rects take; what the
                                             camera already ignores cannot fire, so only NEW regions come out

    python -m cova_amd.monitor --weights CAM0.cvhw CAM1.cvhw --post P0.json P1.json --h-mb 45 --w-mb 80 RECORDS0 RECORDS1

serves one record argument per camera (several files joined with commas; labels in the records are ignored) in mixed batches,
round robin over the cameras, through the calibrated set and prints one report per camera.

The input monitor (include/covahip.h, "Input monitor") looks at what goes IN: set_inputs / add_inputs / read_inputs count, per
model, a 512-bin histogram of the packed records, how often each macroblock moves, still frames, all-intra frames and the
frames' moving-macroblock counts.  input_report(snapshot, model, baseline) turns them into marginals, a GoP estimate and, against
a baseline (save_inputs / load_inputs; python -m cova_amd.train --record-report --save-inputs writes the training side's), the
total variation distance of the record distribution.  --inputs, --save-inputs, --input-baseline and --input-drift are the command
line's form.  The tool measures; what distance a healthy camera shows from day to day nobody has measured.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys

import numpy as np

from . import _lib as L
from . import calibrate as cal

AREA_BINS = L.MONITOR_AREA_BINS
_FIELDS = ("frames", "fire", "boxes", "frames_with_boxes", "truncated", "area_hist")
INPUT_BINS, MOVE_BINS = L.INPUT_BINS, L.INPUT_MOVE_BINS
_IN_FIELDS = ("in_frames", "hist", "moving", "still_frames", "intra_frames", "move_hist")
_FORMS = {"stacked": L.INPUT_STACKED, "frames": L.INPUT_FRAMES, "packed": L.INPUT_PACKED}
INPUTS_FORMAT = "covahip-inputs-1"


# ------------------------------------------------------------------------------------------------------------------ the C-ABI
def begin(ctx, h: int, w: int, n_models: int = 1, max_boxes: int = 256, *, attach: bool = False, every: int = 1) -> None:
    """covahip_monitor_begin on ctx: zeroed counters for n_models models of grid [h][w]; an open monitor starts over.  Stand-alone
    (attach False) it is fed by add() with boxes arrays of row length max_boxes; attached it counts every `every`-th filter batch of
    the model loaded on ctx (BlobNetInfer.monitor_begin)."""
    cfg = L.MonitorCfg(int(h), int(w), int(n_models), int(max_boxes), int(bool(attach)), int(every))
    L.check(L.lib().covahip_monitor_begin(ctx.handle, C.byref(cfg)), "covahip_monitor_begin", ctx.handle)
    ctx._monitor_shape = (int(h), int(w), int(n_models))


def add_device(ctx, d_mask, d_counts, d_boxes, n: int, model_ids=None, mem_kind=L.MEM_DEVICE) -> None:
    """covahip_monitor_add: n samples, mask u8 [n][h][w], counts i32 [n] and boxes [n][max_boxes] as device pointers; model_ids
    u8 [n] on the host (None: model 0).  Synchronous."""
    ids = None if model_ids is None else np.ascontiguousarray(model_ids, dtype=np.uint8).reshape(-1)
    if ids is not None and ids.shape != (n,):
        raise ValueError(f"model_ids must be [{n}], got {ids.shape}")
    L.check(L.lib().covahip_monitor_add(ctx.handle, d_mask, d_counts, d_boxes, None if ids is None else ids.ctypes.data, int(n), mem_kind),
            "covahip_monitor_add", ctx.handle)


def add(ctx, mask, counts, boxes, model_ids=None) -> None:
    """add_device on host arrays: mask u8 [n][h][w], counts i32 [n], boxes [n][max_boxes] (BOX_DTYPE; None with max_boxes 0)."""
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    if mask.ndim != 3 or counts.shape != (mask.shape[0],):
        raise ValueError(f"mask [n][h][w] and counts [n] expected, got {mask.shape} and {counts.shape}")
    if boxes is not None:
        boxes = np.ascontiguousarray(boxes, dtype=L.BOX_DTYPE)
        if boxes.ndim != 2 or boxes.shape[0] != mask.shape[0]:
            raise ValueError(f"boxes [n][max_boxes] expected, got {boxes.shape}")
    add_device(ctx, mask.ctypes.data, counts.ctypes.data, None if boxes is None else boxes.ctypes.data, mask.shape[0], model_ids, L.MEM_HOST)


def read(ctx, reset: bool = False) -> dict:
    """covahip_monitor_read: waits for everything ctx has in flight, then -> frames, boxes, frames_with_boxes, truncated i64
    [n_models], fire i64 [n_models][h][w], area_hist i64 [n_models][16], batches_seen, batches_counted (ints).  With reset the
    tables and both batch counters are zeroed afterwards; the monitor stays open."""
    shape = getattr(ctx, "_monitor_shape", None)
    if shape is None:
        raise L.CovahipError(1, "covahip_monitor_read", "no monitor was opened on this context")
    h, w, m = shape
    out = {"frames": np.zeros(m, np.int64), "fire": np.zeros((m, h, w), np.int64), "boxes": np.zeros(m, np.int64),
           "frames_with_boxes": np.zeros(m, np.int64), "truncated": np.zeros(m, np.int64), "area_hist": np.zeros((m, AREA_BINS), np.int64)}
    seen, counted = C.c_int64(), C.c_int64()
    L.check(L.lib().covahip_monitor_read(ctx.handle, int(bool(reset)), *(out[k].ctypes.data for k in _FIELDS), C.byref(seen), C.byref(counted)),
            "covahip_monitor_read", ctx.handle)
    out["batches_seen"], out["batches_counted"] = int(seen.value), int(counted.value)
    return out


def end(ctx) -> None:
    """covahip_monitor_end: closes the monitor of ctx."""
    L.check(L.lib().covahip_monitor_end(ctx.handle), "covahip_monitor_end", ctx.handle)
    ctx._monitor_shape = None


def set_slice(ctx, samples: int = 0) -> None:
    """Developer switch (include/covahip_dev.h): samples per slice of the monitor kernel, 0 = automatic."""
    L.check(L.lib().covahip_dev_monitor_slice(ctx.handle, int(samples)), "covahip_dev_monitor_slice")


def set_inputs(ctx, on: bool = True) -> None:
    """covahip_monitor_set_inputs: switches the input statistics of the open monitor of ctx on (zeroed tables) or off."""
    L.check(L.lib().covahip_monitor_set_inputs(ctx.handle, int(bool(on))), "covahip_monitor_set_inputs", ctx.handle)


def get_inputs(ctx) -> bool:
    on = C.c_int()
    L.check(L.lib().covahip_monitor_get_inputs(ctx.handle, C.byref(on)), "covahip_monitor_get_inputs", ctx.handle)
    return bool(on.value)


def add_inputs_device(ctx, d_src, form: str, n_frames: int, stack_index, batch: int, model_ids=None, mem_kind=L.MEM_DEVICE) -> None:
    """covahip_monitor_add_inputs on a pointer: form "stacked" (u8 [batch][4h][w][4]), "frames" (u8 [n_frames][h][w][4]) or
    "packed" (u16 [n_frames][h][w]); stack_index i32 [batch][4] on the host or None (one stream in order); model_ids u8 [batch] on
    the host (None: model 0).  Stack b counts its newest slice.  Synchronous."""
    ids = None if model_ids is None else np.ascontiguousarray(model_ids, dtype=np.uint8).reshape(-1)
    if ids is not None and ids.shape != (batch,):
        raise ValueError(f"model_ids must be [{batch}], got {ids.shape}")
    idx = None if stack_index is None else np.ascontiguousarray(stack_index, dtype=np.int32).reshape(-1, 4)
    if idx is not None and idx.shape[0] != batch:
        raise ValueError(f"stack_index must be [{batch}][4], got {idx.shape}")
    L.check(L.lib().covahip_monitor_add_inputs(ctx.handle, d_src, _FORMS[form], int(n_frames), None if idx is None else idx.ctypes.data,
                                               int(batch), None if ids is None else ids.ctypes.data, mem_kind),
            "covahip_monitor_add_inputs", ctx.handle)


def add_inputs(ctx, src, form: str, stack_index=None, model_ids=None) -> None:
    """add_inputs_device on a host array of the form's shape and type."""
    src = np.ascontiguousarray(src, dtype=np.uint16 if form == "packed" else np.uint8)
    n = src.shape[0]
    batch = n if form == "stacked" else n - 3 if stack_index is None else np.asarray(stack_index).reshape(-1, 4).shape[0]
    add_inputs_device(ctx, src.ctypes.data, form, 0 if form == "stacked" else n, stack_index, batch, model_ids, L.MEM_HOST)


def read_inputs(ctx, reset: bool = False) -> dict:
    """covahip_monitor_read_inputs: waits for everything ctx has in flight, then -> in_frames, still_frames, intra_frames i64
    [n_models], hist i64 [n_models][512], moving i64 [n_models][h][w], move_hist i64 [n_models][16].  With reset the input tables
    (only) are zeroed afterwards."""
    shape = getattr(ctx, "_monitor_shape", None)
    if shape is None:
        raise L.CovahipError(1, "covahip_monitor_read_inputs", "no monitor was opened on this context")
    h, w, m = shape
    out = {"in_frames": np.zeros(m, np.int64), "hist": np.zeros((m, INPUT_BINS), np.int64), "moving": np.zeros((m, h, w), np.int64),
           "still_frames": np.zeros(m, np.int64), "intra_frames": np.zeros(m, np.int64), "move_hist": np.zeros((m, MOVE_BINS), np.int64)}
    L.check(L.lib().covahip_monitor_read_inputs(ctx.handle, int(bool(reset)), *(out[k].ctypes.data for k in _IN_FIELDS)),
            "covahip_monitor_read_inputs", ctx.handle)
    return out


def set_input_flush(ctx, samples: int = 0) -> None:
    """Developer switch (include/covahip_dev.h): samples between two flushes of the input kernel's counters, 0 = the default."""
    L.check(L.lib().covahip_dev_input_flush(ctx.handle, int(samples)), "covahip_dev_input_flush")


# ------------------------------------------------------------------------------------------------------------------ reading a snapshot
def as_heat(snapshot: dict, model: int, logit_thresh: float = 0.0) -> dict:
    """Model `model` of a snapshot in the shape calibrate.ignore_from_heat(source="pred") takes: fire [1][h][w] (the served mask
    has ONE threshold, logit_thresh says which), both and gt zero (there are no labels), samples = frames[model]."""
    fire = np.asarray(snapshot["fire"][model], np.int64)[None]
    return {"fire": fire, "both": np.zeros_like(fire), "gt": np.zeros(fire.shape[1:], np.int64), "samples": int(snapshot["frames"][model]),
            "logit_thresh": np.asarray([logit_thresh], np.float32)}


def persistent_rects(snapshot: dict, model: int, rate, dilate: int = 0, max_share: float = 0.25) -> list:
    """The macroblocks of `model` that fire in at least `rate` of its frames, as pixel rectangles (left, top, width, height):
    calibrate.ignore_from_heat and rects_from_keep on as_heat.  Macroblocks the model already ignores cannot fire, so these are NEW
    regions, to be added to the sidecar's ignore_rects.  ValueError without frames, or when they cover more than max_share."""
    keep = cal.ignore_from_heat(as_heat(snapshot, model), rate, source="pred", dilate=dilate, max_share=max_share)
    return cal.rects_from_keep(keep)


def report(snapshot: dict, model: int, baseline=None, factor: float = 2.0) -> dict:
    """What model `model` did over the snapshot: frames, foreground_share (fire.sum() / (frames * h * w)), boxes_per_frame,
    frames_with_boxes_share, truncated, area_hist (list of 16).  With baseline (a calibration sidecar document, calibrate.save_post)
    also baseline_boxes_per_frame = scores.pred / scores.samples, ratio = boxes_per_frame / baseline (None when the baseline is 0)
    and drift = ratio > factor or ratio < 1 / factor.  factor is a policy knob, not a measured quantity.  A zero baseline with no
    boxes now is no drift; a zero baseline with boxes now is.  Without frames every rate is 0.0 and drift is False."""
    if not factor > 1.0:
        raise ValueError(f"factor must exceed 1, got {factor!r}")
    frames = int(snapshot["frames"][model])
    fire = np.asarray(snapshot["fire"][model])
    boxes = int(snapshot["boxes"][model])
    out = {"model": int(model), "frames": frames,
           "foreground_share": float(fire.sum()) / (frames * fire.size) if frames else 0.0,
           "boxes": boxes, "boxes_per_frame": boxes / frames if frames else 0.0,
           "frames_with_boxes_share": int(snapshot["frames_with_boxes"][model]) / frames if frames else 0.0,
           "truncated": int(snapshot["truncated"][model]), "area_hist": [int(v) for v in snapshot["area_hist"][model]]}
    if baseline is not None:
        sc = baseline.get("scores", {})
        if "pred" not in sc or not sc.get("samples"):
            raise ValueError("the baseline has no scores.pred / scores.samples")
        base = float(sc["pred"]) / float(sc["samples"])
        now = out["boxes_per_frame"]
        out["baseline_boxes_per_frame"] = base
        out["factor"] = float(factor)
        if not frames:
            out["ratio"], out["drift"] = None, False
        elif base == 0.0:
            out["ratio"], out["drift"] = None, now > 0.0
        else:
            out["ratio"] = now / base
            out["drift"] = out["ratio"] > factor or out["ratio"] < 1.0 / factor
    return out


def format_report(rep: dict, name=None) -> str:
    """A report as text: one line of rates, one of the area histogram (bin k: areas in [2^k, 2^(k+1)), the last one open)."""
    head = f"camera {rep['model']}" + (f" ({name})" if name else "")
    line = (f"{head}: frames {rep['frames']}  foreground {100.0 * rep['foreground_share']:.3f} %  boxes/frame {rep['boxes_per_frame']:.4f}  "
            f"frames with boxes {100.0 * rep['frames_with_boxes_share']:.2f} %  truncated {rep['truncated']}")
    if "baseline_boxes_per_frame" in rep:
        ratio = "n/a" if rep["ratio"] is None else f"{rep['ratio']:.3f}"
        line += (f"  baseline boxes/frame {rep['baseline_boxes_per_frame']:.4f}  ratio {ratio}  "
                 + (f"DRIFT (outside 1/{rep['factor']:g} .. {rep['factor']:g})" if rep["drift"] else "no drift"))
    hist = " ".join(f"2^{k}:{v}" for k, v in enumerate(rep["area_hist"]) if v)
    return line + f"\n  box areas (macroblocks) {hist if hist else '-'}"


# ------------------------------------------------------------------------------------------------------------------ input statistics
def input_counts(snapshot: dict, model: int) -> dict:
    """Model `model` of a read_inputs snapshot as one set of counts (what save_inputs writes and input_report takes as a baseline)."""
    return {k: np.asarray(snapshot[k][model], np.int64) for k in _IN_FIELDS}


def _marginals(hist):
    """-> (per class [8], per max(|mv_x|, |mv_y|) [8], moving count, total) of a 512-bin record histogram."""
    hist = np.asarray(hist, np.int64).reshape(INPUT_BINS)
    r = np.arange(INPUT_BINS)
    cls = np.bincount(r & 7, weights=hist, minlength=8).astype(np.int64)
    mv = np.bincount(np.maximum((r >> 3) & 7, (r >> 6) & 7), weights=hist, minlength=8).astype(np.int64)
    return cls, mv, int(hist[(r & 0x1F8) != 0].sum()), int(hist.sum())


def tv(p_counts, q_counts):
    """Total variation distance 1/2 sum |p - q| of two count vectors, each normalised by its own sum; None when either is empty."""
    p, q = np.asarray(p_counts, np.float64).ravel(), np.asarray(q_counts, np.float64).ravel()
    if p.sum() <= 0 or q.sum() <= 0:
        return None
    return float(0.5 * np.abs(p / p.sum() - q / q.sum()).sum())


def _gop(counts):
    return int(counts["in_frames"]) / int(counts["intra_frames"]) if int(counts["intra_frames"]) else None


def input_report(snapshot: dict, model: int, baseline=None) -> dict:
    """What records model `model` was sent over a read_inputs snapshot (or, with the arrays of one model, what input_counts /
    load_inputs / TrainData.record_stats give: pass model=None): frames, the record marginals per class and per
    max(|mv_x|, |mv_y|) as shares, moving_share, still_share, intra_share, gop_estimate = in_frames / intra_frames (None without
    an all-intra frame), move_hist.  With baseline (one model's counts) also tv = 1/2 sum |p_bin - q_bin| over the 512 normalised
    bins, tv_class and tv_mv over the marginals, and baseline_gop_estimate.  A distance is None while either side is empty.  No
    threshold of tv is known to mean anything: the report measures."""
    c = input_counts(snapshot, model) if model is not None else {k: np.asarray(snapshot[k], np.int64) for k in _IN_FIELDS}
    cls, mv, moving, total = _marginals(c["hist"])
    frames = int(c["in_frames"])
    out = {"model": None if model is None else int(model), "frames": frames, "macroblocks": total,
           "class_share": [float(v) / total if total else 0.0 for v in cls], "mv_share": [float(v) / total if total else 0.0 for v in mv],
           "moving_share": moving / total if total else 0.0,
           "still_share": int(c["still_frames"]) / frames if frames else 0.0,
           "intra_share": int(c["intra_frames"]) / frames if frames else 0.0,
           "gop_estimate": _gop(c), "move_hist": [int(v) for v in np.asarray(c["move_hist"]).ravel()]}
    if baseline is not None:
        bcls, bmv, _, _ = _marginals(baseline["hist"])
        out["tv"] = tv(c["hist"], baseline["hist"])
        out["tv_class"] = tv(cls, bcls)
        out["tv_mv"] = tv(mv, bmv)
        out["baseline_gop_estimate"] = _gop(baseline)
    return out


def save_inputs(path, snapshot: dict, model) -> None:
    """One model's input counts (model None: the snapshot holds one model's arrays) as plain JSON: integer lists and the grid."""
    c = input_counts(snapshot, model) if model is not None else {k: np.asarray(snapshot[k], np.int64) for k in _IN_FIELDS}
    h, w = c["moving"].shape
    doc = {"format": INPUTS_FORMAT, "h_mb": int(h), "w_mb": int(w)}
    for k in _IN_FIELDS:
        doc[k] = int(c[k]) if c[k].ndim == 0 else c[k].ravel().tolist()
    with open(path, "w") as f:
        json.dump(doc, f)


def load_inputs(path) -> dict:
    """save_inputs' file -> one model's counts (int64 arrays; moving [h_mb][w_mb]) plus h_mb, w_mb."""
    with open(path) as f:
        doc = json.load(f)
    if doc.get("format") != INPUTS_FORMAT:
        raise ValueError(f"{path}: not a {INPUTS_FORMAT} file")
    h, w = int(doc["h_mb"]), int(doc["w_mb"])
    out = {"h_mb": h, "w_mb": w, "in_frames": np.int64(doc["in_frames"]), "still_frames": np.int64(doc["still_frames"]),
           "intra_frames": np.int64(doc["intra_frames"]), "hist": np.asarray(doc["hist"], np.int64),
           "moving": np.asarray(doc["moving"], np.int64).reshape(h, w), "move_hist": np.asarray(doc["move_hist"], np.int64)}
    if out["hist"].shape != (INPUT_BINS,) or out["move_hist"].shape != (MOVE_BINS,):
        raise ValueError(f"{path}: hist [{INPUT_BINS}] and move_hist [{MOVE_BINS}] expected")
    return out


def format_input_report(rep: dict, name=None, drift=None) -> str:
    """An input report as text: one line of rates, the class and vector marginals, and with a baseline the distances; drift: the
    command line's --input-drift X (None: none given)."""
    head = ("recording" if rep["model"] is None else f"camera {rep['model']}") + (f" ({name})" if name else "")
    gop = "n/a" if rep["gop_estimate"] is None else f"{rep['gop_estimate']:.2f}"
    lines = [f"{head} inputs: frames {rep['frames']}  moving {100.0 * rep['moving_share']:.3f} %  still frames {100.0 * rep['still_share']:.2f} %  "
             f"GoP estimate {gop}",
             "  class share " + " ".join(f"{k}:{100.0 * v:.2f}" for k, v in enumerate(rep["class_share"]) if v),
             "  max |mv| share " + " ".join(f"{k}:{100.0 * v:.2f}" for k, v in enumerate(rep["mv_share"]) if v)]
    if "tv" in rep:
        f3 = lambda v: "n/a" if v is None else f"{v:.4f}"
        bg = "n/a" if rep["baseline_gop_estimate"] is None else f"{rep['baseline_gop_estimate']:.2f}"
        line = f"  against the baseline: tv {f3(rep['tv'])}  tv class {f3(rep['tv_class'])}  tv max |mv| {f3(rep['tv_mv'])}  baseline GoP estimate {bg}"
        if drift is not None:
            line += f"  INPUT DRIFT (tv above {drift:g})" if rep["tv"] is not None and rep["tv"] > drift else f"  no input drift (tv at most {drift:g})"
        lines.append(line)
    return "\n".join(lines)


def ignore_hint(model: int, rects) -> str:
    """New ignore rectangles of one camera as the element property that takes them, in calibrate.serving_hint's format."""
    return f"blobnetfilter pad-ignore-rects=\"{int(model)}={'+'.join(','.join(str(v) for v in r) for r in rects)}\""


# ------------------------------------------------------------------------------------------------------------------ command line
def mixed_batches(frames_per_camera, batch: int):
    """The command line's batches: camera k's sample j is its frames 4 j .. 4 j + 3 (train.slide's grouping; a trailing incomplete
    group is dropped), the samples go round robin over the cameras (a camera that has run out is skipped) and every `batch` of them
    are one filter_frames call.  Yields (frames u8 [4 b][h][w][4], stack_index i32 [b][4], model_ids u8 [b])."""
    n = [f.shape[0] // 4 for f in frames_per_camera]
    order = [(k, j) for j in range(max(n, default=0)) for k in range(len(n)) if j < n[k]]
    for s0 in range(0, len(order), batch):
        part = order[s0:s0 + batch]
        frames = np.concatenate([frames_per_camera[k][4 * j:4 * j + 4] for k, j in part])
        index = np.asarray([[4 * i + 3, 4 * i + 2, 4 * i + 1, 4 * i] for i in range(len(part))], np.int32)
        yield frames, index, np.asarray([k for k, _ in part], np.uint8)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cova_amd.monitor", description=__doc__.split("\n")[0])
    ap.add_argument("records", nargs="+", metavar="RECORDS", help="TFRecord files written by tfrecordsink, one argument per camera, "
                    "several files of one camera joined with commas")
    ap.add_argument("--weights", nargs="+", required=True, metavar="CVHW", help="one weight file per camera")
    ap.add_argument("--post", nargs="+", metavar="JSON", help="one calibration sidecar per camera (calibrate -o): served with its "
                    "threshold, ignore region and cc-threshold, and the baseline of its report")
    ap.add_argument("--h-mb", type=int, default=45)
    ap.add_argument("--w-mb", type=int, default=80)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--batch", type=int, default=256, help="samples per filter call")
    ap.add_argument("--lanes", type=int, default=1, help="batches in flight")
    ap.add_argument("--every", type=int, default=1, help="count every N-th batch")
    ap.add_argument("--cc-threshold", type=int, default=30, help="area threshold of cameras without a sidecar")
    ap.add_argument("--factor", type=float, default=2.0, help="a box rate outside baseline / FACTOR .. baseline * FACTOR is drift")
    ap.add_argument("--persistent", type=float, metavar="RATE", help="print the macroblocks that fire in at least this share of a "
                    "camera's frames as new ignore rectangles")
    ap.add_argument("--out", metavar="FILE.npz", help="write the snapshot")
    ap.add_argument("--inputs", action="store_true", help="count the records every camera sends too and print its input report")
    ap.add_argument("--save-inputs", nargs="+", metavar="JSON", help="write every camera's input counts, one file per camera (implies --inputs)")
    ap.add_argument("--input-baseline", nargs="+", metavar="JSON", help="one input-count file per camera (--save-inputs here, or "
                    "python -m cova_amd.train --record-report --save-inputs): the report gives the distance to it (implies --inputs)")
    ap.add_argument("--input-drift", type=float, metavar="X", help="flag a camera whose total variation distance to its baseline "
                    "exceeds X.  There is no default: nobody has measured the day-to-day distance of a healthy camera; the report "
                    "prints the value")
    a = ap.parse_args(argv)
    for name, v in (("--save-inputs", a.save_inputs), ("--input-baseline", a.input_baseline)):
        if v and len(v) != len(a.records):
            ap.error(f"{name} takes one file per camera")
    if a.input_drift is not None and not a.input_baseline:
        ap.error("--input-drift needs --input-baseline")
    if a.input_drift is not None and not 0.0 <= a.input_drift <= 1.0:
        ap.error("--input-drift takes a distance in [0, 1]")
    a.inputs = bool(a.inputs or a.save_inputs or a.input_baseline)
    if len(a.weights) != len(a.records) or (a.post and len(a.post) != len(a.records)):
        ap.error("--weights, --post and RECORDS take one argument per camera")
    if a.persistent is not None and not 0.0 < a.persistent <= 1.0:
        ap.error("--persistent takes a rate in (0, 1]")
    if a.batch < 1 or a.every < 1 or not a.factor > 1.0:
        ap.error("--batch and --every must be at least 1, --factor above 1")
    return a


def main(argv=None) -> int:
    from . import train
    from . import weights as W
    from .elements import BlobNetInfer, Context
    a = parse_args(argv)
    frames = [train.read_tfrecords(r.split(","), a.h_mb, a.w_mb)[0] for r in a.records]
    if not any(f.shape[0] >= 4 for f in frames):
        print("no complete sample in the records", file=sys.stderr)
        return 2
    flats = []
    for path in a.weights:
        with open(path, "rb") as f:
            flats.append(W.from_bytes(f.read()))
    docs = None
    if a.post:
        docs = []
        for path in a.post:
            with open(path) as f:
                docs.append(json.load(f))
    ctx = Context(a.device)
    try:
        ctx.set_lanes(a.lanes)
        net = BlobNetInfer(ctx, flats, a.h_mb, a.w_mb, max_batch=a.batch)
        for k, path in enumerate(a.post or []):
            cal.apply_post(net, k, path)
        net.monitor_begin(every=a.every)
        if a.inputs:
            net.monitor_set_inputs(True)
        for fr, index, ids in mixed_batches(frames, a.batch):
            net.filter_frames(fr, index, a.cc_threshold, 256, model_ids=ids)
        snap = net.monitor_read()
        in_snap = net.monitor_read_inputs() if a.inputs else None
        net.monitor_end()
    finally:
        ctx.close()
    print(f"batches seen {snap['batches_seen']}, counted {snap['batches_counted']}")
    for k in range(len(frames)):
        print(format_report(report(snap, k, docs[k] if docs else None, a.factor), a.records[k]))
        if a.persistent is not None and snap["frames"][k]:
            try:
                rects = persistent_rects(snap, k, a.persistent)
            except ValueError as e:
                print(f"  persistent: {e}")
                continue
            print("  persistent: " + (ignore_hint(k, rects) if rects else f"no macroblock fires in {a.persistent:g} of the frames"))
    if in_snap is not None:
        for k in range(len(frames)):
            base = load_inputs(a.input_baseline[k]) if a.input_baseline else None
            if base is not None and (base["h_mb"], base["w_mb"]) != (a.h_mb, a.w_mb):
                print(f"{a.input_baseline[k]}: grid {base['h_mb']}x{base['w_mb']}, the cameras are served at {a.h_mb}x{a.w_mb}", file=sys.stderr)
                return 2
            print(format_input_report(input_report(in_snap, k, base), a.records[k], a.input_drift))
            if a.save_inputs:
                save_inputs(a.save_inputs[k], in_snap, k)
                print(f"  wrote {a.save_inputs[k]}")
    if a.out:
        np.savez_compressed(a.out, **snap)
        print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
