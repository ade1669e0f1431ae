"""Calibration without a GPU: covahip_post_sweep refuses every argument fault before it touches the GPU, choose / add / the
sidecar of cova_amd/calibrate.py on hand-written tables, and the numpy restatement the GPU tests compare against
(tests/sweep_ref.py) on a hand-drawn 6 x 8 case whose counts are written out here."""
import ctypes as C

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import calibrate as cal
from cova_amd.elements import keep_from_rects
from tests.sweep_ref import sweep_ref

INVALID, UNSUPPORTED = 1, 5


# ------------------------------------------------------------------------------------------------------------------ C entry
class _Call:
    """One covahip_post_sweep call with valid arguments; a test breaks one of them."""

    def __init__(self, h=16, w=16, n=2):
        self.th = np.array([-1.0, 0.0, 1.0], np.float32)
        self.ar = np.array([1, 2, 4], np.int32)
        self.keep = np.ones((h, w), np.uint8)
        self.cfg = L.SweepCfg(h, w, 3, self.th.ctypes.data, 3, self.ar.ctypes.data, 1, 1, 10, 256, self.keep.ctypes.data, 0)
        self.n, self.mem = n, L.MEM_HOST
        self.logits = np.zeros((max(n, 1), h, w), np.float32)
        self.gt = np.zeros((max(n, 1), h, w), np.uint8)
        self.pixel = np.full((3, 3), -7, np.int64)
        self.cells = np.full((3, 3, 3), -7, np.int64)
        self.trunc = np.full(3, -7, np.int64)
        self.res = L.SweepResult(-7, -7, -7)
        self.ctx = C.c_void_p(8)              # never dereferenced: every check fails first (and n == 0 returns before the GPU)
        self.args = {"cfg": C.byref(self.cfg), "logits": self.logits.ctypes.data, "gt": self.gt.ctypes.data,
                     "pixel": self.pixel.ctypes.data, "cells": self.cells.ctypes.data, "trunc": self.trunc.ctypes.data,
                     "res": C.byref(self.res)}

    def run(self):
        a = self.args
        return L.lib().covahip_post_sweep(self.ctx, a["cfg"], a["logits"], a["gt"], self.n, self.mem, a["pixel"], a["cells"],
                                          a["trunc"], a["res"])


def test_null_pointers():
    c = _Call()
    c.ctx = None
    assert c.run() == INVALID
    for name in ("cfg", "logits", "gt", "pixel", "cells", "trunc", "res"):
        c = _Call()
        c.args[name] = None
        assert c.run() == INVALID, name
    for field in ("logit_thresh", "area_thresh"):
        c = _Call()
        setattr(c.cfg, field, None)
        assert c.run() == INVALID, field


@pytest.mark.parametrize("field,value", [
    ("n_thresh", 0), ("n_thresh", 65), ("n_thresh", -1), ("n_area", 0), ("n_area", 17), ("gt_area_thresh", 0),
    ("iou_num", 0), ("iou_num", 11), ("iou_den", 0), ("max_boxes", 0), ("max_boxes", 1025), ("chunk", -1), ("h", 0), ("w", 0), ("h", -3)])
def test_counts_out_of_range(field, value):
    c = _Call()
    setattr(c.cfg, field, value)
    assert c.run() == INVALID


@pytest.mark.parametrize("th", [[0.0, float("nan"), 1.0], [0.0, float("inf"), 2.0], [float("-inf"), 0.0, 1.0],
                                [0.0, 0.0, 1.0], [0.0, 1.0, 0.5], [1.0, 0.0, -1.0]])
def test_threshold_list(th):
    c = _Call()
    c.th[:] = th
    assert c.run() == INVALID


@pytest.mark.parametrize("ar", [[0, 1, 2], [1, 1, 2], [1, 4, 2], [-1, 2, 3]])
def test_area_list(ar):
    c = _Call()
    c.ar[:] = ar
    assert c.run() == INVALID


def test_n_mem_kind_and_width():
    c = _Call()
    c.n = -1
    assert c.run() == INVALID
    for mem in (2, -1):
        c = _Call()
        c.mem = mem
        assert c.run() == INVALID
    c = _Call(h=16, w=257)                    # covahip_bboxcc's limit, reported as that entry reports it
    assert c.run() == UNSUPPORTED
    c = _Call(h=16, w=257)
    c.cfg.n_thresh = 0                        # an argument fault is an argument fault on any grid
    assert c.run() == INVALID


def test_no_samples_is_ok_with_zeros():
    c = _Call(n=0)
    c.args["logits"] = c.args["gt"] = None    # nothing to read
    assert c.run() == 0
    assert not c.pixel.any() and not c.cells.any() and not c.trunc.any()
    assert (c.res.samples, c.res.gt_objects, c.res.gt_truncated) == (0, 0, 0)


def test_struct_layouts():
    assert C.sizeof(L.SweepCell) == 24 and C.sizeof(L.SweepResult) == 24
    assert L.SweepCfg.logit_thresh.offset == 16 and L.SweepCfg.keep.offset == 56 and C.sizeof(L.SweepCfg) == 72


# ------------------------------------------------------------------------------------------------------------------ choose / add
def _table(gt_found, pred_true, pred, gt_objects, thresholds=None, areas=None):
    gt_found, pred_true, pred = (np.asarray(x, np.int64) for x in (gt_found, pred_true, pred))
    T, A = pred.shape
    return {"pixel": np.tile(np.array([[8, 2, 2]], np.int64), (T, 1)), "pred": pred, "pred_true": pred_true, "gt_found": gt_found,
            "truncated": np.arange(T, dtype=np.int64), "samples": 5, "gt_objects": gt_objects, "gt_truncated": 0,
            "logit_thresh": np.asarray(thresholds if thresholds is not None else np.arange(T) - 1.0, np.float32),
            "area_thresh": np.asarray(areas if areas is not None else [1, 2, 4][:A], np.int32), "gt_area": 1, "iou": (1, 10),
            "max_boxes": 256, "h": 16, "w": 16}


def test_choose_highest_precision_among_cells_that_meet_the_recall():
    #          recall 1.0 / 0.96 / 0.90            precision 0.5 / 0.8 / 1.0
    r = _table([[100, 96, 90]], [[50, 40, 30]], [[100, 50, 30]], 100)
    ch = cal.choose(r, 0.95)
    assert ch["met"] and (ch["t"], ch["a"]) == (0, 1) and ch["cc_threshold"] == 2 and ch["logit_thresh"] == -1.0
    assert ch["object_recall"] == 0.96 and ch["object_precision"] == 0.8
    assert ch["pixel_recall"] == 0.8 and ch["pixel_precision"] == 0.8 and ch["truncated"] == 0
    assert cal.choose(r, 0.9)["a"] == 2 and cal.choose(r, 0.97)["a"] == 0


def test_choose_tie_breaks():
    # the same precision everywhere: the higher threshold wins, then the larger area
    r = _table([[10, 10], [10, 10], [10, 9]], [[5, 5], [5, 5], [5, 5]], [[10, 10], [10, 10], [10, 10]], 10)
    ch = cal.choose(r, 1.0)                   # (2, 1) misses the recall; the threshold ranks before the area
    assert ch["met"] and (ch["t"], ch["a"]) == (2, 0) and ch["truncated"] == 2
    ch = cal.choose(r, 0.9)                   # now (2, 1) qualifies as well
    assert (ch["t"], ch["a"]) == (2, 1)
    r["gt_found"][2] = 0                      # threshold 2 out of the running
    assert (cal.choose(r, 1.0)["t"], cal.choose(r, 1.0)["a"]) == (1, 1)


def test_choose_no_cell_meets_the_target():
    r = _table([[6, 5], [6, 4]], [[1, 1], [3, 2]], [[4, 2], [3, 2]], 10)
    ch = cal.choose(r, 0.95)
    assert ch["met"] is False and (ch["t"], ch["a"]) == (1, 0) and ch["object_recall"] == 0.6   # highest recall, higher threshold
    assert ch["object_precision"] == 1.0


def test_choose_empty_predictions_and_no_objects():
    r = _table([[3, 0]], [[2, 0]], [[4, 0]], 4)
    ch = cal.choose(r, 0.0)                    # pred == 0: precision 1.0, so the empty cell wins at min_recall 0
    assert ch["met"] and (ch["t"], ch["a"]) == (0, 1) and ch["object_precision"] == 1.0 and ch["object_recall"] == 0.0
    r = _table([[0, 0]], [[0, 0]], [[4, 0]], 0)
    ch = cal.choose(r, 0.95)                   # no labelled objects: nothing can be missed, recall is 1.0 everywhere
    assert ch["met"] and ch["object_recall"] == 1.0 and (ch["t"], ch["a"]) == (0, 1)
    assert cal.choose(r, 0.95)["gt_objects"] == 0


def test_add_sums_and_rejects_other_grids():
    a = _table([[1, 2]], [[3, 4]], [[5, 6]], 7)
    s = cal.add(a, a)
    assert s["pred"].tolist() == [[10, 12]] and s["gt_objects"] == 14 and s["samples"] == 10 and s["pixel"].tolist() == [[16, 4, 4]]
    assert a["pred"].tolist() == [[5, 6]]      # the operands are left alone
    for other in (_table([[1, 2]], [[3, 4]], [[5, 6]], 7, thresholds=[0.5]), _table([[1, 2]], [[3, 4]], [[5, 6]], 7, areas=[1, 3]),
                  _table([[1]], [[3]], [[5]], 7), dict(a, iou=(1, 2)), dict(a, gt_area=2), dict(a, max_boxes=8), dict(a, w=24)):
        with pytest.raises(ValueError):
            cal.add(a, other)


def test_thresholds_as_probabilities():
    th = cal.logit_thresholds(prob_thresholds=[0.2, 0.5, 0.8])
    assert th.dtype == np.float32 and th[1] == 0.0 and th[2] == np.float32(np.log(4.0)) and th[0] == -th[2]
    assert cal.logit_thresholds([-1, 0.25]).tolist() == [-1.0, 0.25]
    for bad in ({"thresholds": [0, 0]}, {"thresholds": [1, 0]}, {"prob_thresholds": [0.5, 1.0]}, {}, {"thresholds": [0], "prob_thresholds": [0.5]}):
        with pytest.raises(ValueError):
            cal.logit_thresholds(**bad)
    probs = cal.logit_thresholds(prob_thresholds=cal.DEFAULT_PROBS)
    assert probs.size == 19 and 0.0 in probs.tolist()


def test_sidecar_round_trip(tmp_path):
    r = _table([[100, 96, 90]], [[50, 40, 30]], [[100, 50, 30]], 100, thresholds=[np.log(4.0)])
    ch = cal.choose(r, 0.95)
    rects = [(0, 0, 200, 40), (1200, 600, 80, 120)]
    path = tmp_path / "post.json"
    cal.save_post(path, ch, rects)
    kw, cc = cal.load_post(path, 45, 80)
    assert cc == 2 and kw["logit_thresh"] == float(np.float32(np.log(4.0)))
    want = keep_from_rects(45, 80, rects)
    assert not want.all() and np.array_equal(kw["keep"], want)
    cal.save_post(path, ch)
    kw, cc = cal.load_post(path, 45, 80)
    assert kw["keep"] is None and cc == 2


# ------------------------------------------------------------------------------------------------------------------ sweep_ref
def _hand_case():
    lg = np.full((1, 6, 8), -1.0, np.float32)
    lg[0, 0:2, 0:3] = 2.0        # X: box (0, 0, 3, 2), 6 macroblocks, above both thresholds
    lg[0, 3, 7] = 0.5            # Y: one macroblock, above 0 only
    lg[0, 5, 0:2] = 1.0          # Z: two macroblocks, EQUAL to the threshold 1: not above it
    lg[0, 2, 4] = np.nan         # background
    gt = np.zeros((1, 6, 8), np.uint8)
    gt[0, 0:2, 0:2] = 1          # A: box (0, 0, 2, 2)
    gt[0, 3:5, 5:8] = 200        # B: box (5, 3, 3, 2)
    return lg, gt


def test_sweep_ref_hand_case():
    lg, gt = _hand_case()
    r = sweep_ref(lg, gt, [0.0, 1.0], [1, 2, 6])
    # X hits A (4 / 6), Y hits B (1 / 6 >= 1 / 10), Z hits nothing
    assert r["pixel"].tolist() == [[5, 4, 5], [4, 2, 6]]
    assert r["pred"].tolist() == [[3, 2, 1], [1, 1, 1]]
    assert r["pred_true"].tolist() == [[2, 1, 1], [1, 1, 1]]
    assert r["gt_found"].tolist() == [[2, 1, 1], [1, 1, 1]]
    assert r["truncated"].tolist() == [0, 0] and (r["samples"], r["gt_objects"], r["gt_truncated"]) == (1, 2, 0)
    # a stricter hit rule: 1 / 6 < 1 / 2 <= 4 / 6
    r = sweep_ref(lg, gt, [0.0, 1.0], [1, 2, 6], iou=(1, 2))
    assert r["pred_true"].tolist() == [[1, 1, 1], [1, 1, 1]] and r["gt_found"].tolist() == [[1, 1, 1], [1, 1, 1]]
    # two boxes per frame: label order is X, Y, Z, so Z does not take part at threshold 0
    r = sweep_ref(lg, gt, [0.0, 1.0], [1, 2, 6], max_boxes=2)
    assert r["truncated"].tolist() == [1, 0] and r["gt_truncated"] == 0
    assert r["pred"].tolist() == [[2, 1, 1], [1, 1, 1]] and r["pred_true"].tolist() == [[2, 1, 1], [1, 1, 1]]
    assert r["gt_found"].tolist() == [[2, 1, 1], [1, 1, 1]]
    r = sweep_ref(lg, gt, [0.0], [1], max_boxes=1)
    assert (r["gt_objects"], r["gt_truncated"]) == (1, 1) and r["gt_found"].tolist() == [[1]]
    # column 7 ignored: Y is gone from the masks, B shrinks to (5, 3, 2, 2) and is no longer found
    keep = np.ones((6, 8), np.uint8)
    keep[:, 7] = 0
    r = sweep_ref(lg, gt, [0.0, 1.0], [1, 2, 6], keep=keep)
    assert r["pixel"].tolist() == [[4, 4, 4], [4, 2, 4]]
    assert r["pred"].tolist() == [[2, 2, 1], [1, 1, 1]] and r["pred_true"].tolist() == [[1, 1, 1], [1, 1, 1]]
    assert r["gt_found"].tolist() == [[1, 1, 1], [1, 1, 1]] and r["gt_objects"] == 2
    # a label object below gt_area is no object
    r = sweep_ref(lg, gt, [0.0], [1], gt_area=5)
    assert r["gt_objects"] == 1 and r["pred_true"].tolist() == [[1]] and r["gt_found"].tolist() == [[1]]
