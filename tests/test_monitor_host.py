"""The serving monitor without a GPU: the numpy restatement on hand-made cases, the snapshot readers of cova_amd.monitor, and the
host-checked errors that need no device."""
import ctypes as C

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import calibrate as cal
from cova_amd import monitor as mon
from tests.monitor_ref import BINS, area_bin, empty, monitor_ref, same


def _boxes(rows, max_boxes):
    out = np.zeros((len(rows), max_boxes), L.BOX_DTYPE)
    for b, areas in enumerate(rows):
        for i, a in enumerate(areas):
            out[b, i] = (0, 0, 1, 1, a)
    return out


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_a_255_valued_byte_counts_once():
    mask = np.zeros((3, 2, 3), np.uint8)
    mask[0, 0, 0], mask[1, 0, 0], mask[2, 0, 0] = 255, 1, 2
    mask[1, 1, 2] = 255
    r = monitor_ref(mask, [0, 0, 0], None, None, 0, 1)
    assert r["fire"][0].tolist() == [[3, 0, 0], [0, 0, 1]]
    assert r["frames"].tolist() == [3] and r["boxes"].tolist() == [0] and r["frames_with_boxes"].tolist() == [0]
    assert not r["area_hist"].any() and not r["truncated"].any()


def test_area_bins():
    assert [area_bin(a) for a in (1, 2, 3, 4, 7, 8, 2 ** 15 - 1, 2 ** 15, 2 ** 15 + 1, 2 ** 20, 2 ** 31 - 1)] == [0, 1, 1, 2, 2, 3, 14, 15, 15, 15, 15]
    mask = np.zeros((1, 1, 1), np.uint8)
    r = monitor_ref(mask, [6], _boxes([[1, 2, 3, 2 ** 15, 2 ** 24, 5]], 8), None, 8, 1)
    want = np.zeros(BINS, np.int64)
    want[0], want[1], want[15], want[2] = 1, 2, 2, 1
    assert np.array_equal(r["area_hist"][0], want)
    assert r["boxes"].tolist() == [6] and r["frames_with_boxes"].tolist() == [1] and r["truncated"].tolist() == [0]


def test_a_truncated_frame_reads_max_boxes_boxes():
    # counts says 7, the row holds 3: the fourth entry onwards is not there to read (here: a poison area that would land in bin 15)
    boxes = _boxes([[4, 4, 4, 2 ** 20], [1]], 4)
    r = monitor_ref(np.ones((2, 1, 2), np.uint8), [7, 1], boxes, [1, 1], 3, 2)
    assert r["area_hist"][1].tolist() == [1, 0, 3] + [0] * 13 and not r["area_hist"][0].any()
    assert r["boxes"].tolist() == [0, 8] and r["truncated"].tolist() == [0, 1] and r["frames_with_boxes"].tolist() == [0, 2]
    assert r["frames"].tolist() == [0, 2] and r["fire"][1].tolist() == [[2, 2]] and not r["fire"][0].any()
    # additive: into
    again = monitor_ref(np.ones((2, 1, 2), np.uint8), [7, 1], boxes, [1, 1], 3, 2, into=r)
    assert again["boxes"].tolist() == [0, 16] and again["fire"][1].tolist() == [[4, 4]]


# ------------------------------------------------------------------------------------------------------------------ snapshot readers
def _snapshot(h=6, w=10, frames=(40, 20)):
    s = empty(len(frames), h, w)
    s["frames"][:] = frames
    s["batches_seen"] = s["batches_counted"] = 3
    return s


def test_persistent_rects_find_a_planted_block():
    rng = np.random.default_rng(5)
    s = _snapshot()
    s["fire"][1] = rng.integers(0, 8, (6, 10))              # under half of 20 frames everywhere
    s["fire"][1][2:4, 5:9] = 20                             # the planted block fires in every frame
    s["fire"][0] = rng.integers(0, 15, (6, 10))             # camera 0: nothing reaches half of 40
    ht = mon.as_heat(s, 1, logit_thresh=0.25)
    assert ht["fire"].shape == (1, 6, 10) and ht["samples"] == 20 and not ht["both"].any() and not ht["gt"].any()
    assert ht["gt"].shape == (6, 10) and ht["logit_thresh"].tolist() == [0.25]
    keep = cal.ignore_from_heat(ht, 0.5, source="pred")
    want = np.ones((6, 10), np.uint8)
    want[2:4, 5:9] = 0
    assert np.array_equal(keep, want)
    assert cal.rects_from_keep(keep) == [(80, 32, 64, 32)]
    assert mon.persistent_rects(s, 1, 0.5) == [(80, 32, 64, 32)]
    assert mon.persistent_rects(s, 1, 1.0) == [(80, 32, 64, 32)]
    assert mon.persistent_rects(s, 0, 0.5) == []            # a rate nothing reaches
    assert mon.persistent_rects(s, 1, 0.5, dilate=1, max_share=0.5) == [(64, 16, 96, 64)]
    with pytest.raises(ValueError):
        mon.persistent_rects(s, 1, 0.5, dilate=1)           # 24 of 60 macroblocks: more than a quarter of the camera
    assert mon.ignore_hint(1, [(80, 32, 64, 32), (0, 0, 16, 16)]) == 'blobnetfilter pad-ignore-rects="1=80,32,64,32+0,0,16,16"'
    with pytest.raises(ValueError):
        mon.persistent_rects(_snapshot(frames=(0, 0)), 0, 0.5)          # no frames


def test_report_with_and_without_a_baseline():
    s = _snapshot()
    s["fire"][0][0, :3] = 40
    s["boxes"][:] = (100, 0)
    s["frames_with_boxes"][:] = (30, 0)
    s["truncated"][:] = (2, 0)
    s["area_hist"][0][:3] = (50, 30, 20)
    r = mon.report(s, 0)
    assert r == {"model": 0, "frames": 40, "foreground_share": 120 / (40 * 60), "boxes": 100, "boxes_per_frame": 2.5,
                 "frames_with_boxes_share": 0.75, "truncated": 2, "area_hist": [50, 30, 20] + [0] * 13}
    text = mon.format_report(r, "cam0.tfrecord")
    assert "camera 0 (cam0.tfrecord)" in text and "boxes/frame 2.5000" in text and "2^0:50 2^1:30 2^2:20" in text and "drift" not in text.lower()

    def base(pred, samples=100):
        return {"format": "covahip-post-1", "scores": {"pred": pred, "samples": samples}}
    same_rate = mon.report(s, 0, base(250))
    assert same_rate["baseline_boxes_per_frame"] == 2.5 and same_rate["ratio"] == 1.0 and same_rate["drift"] is False
    assert "no drift" in mon.format_report(same_rate)
    assert mon.report(s, 0, base(125))["drift"] is False                   # ratio 2.0 is not above the factor
    up = mon.report(s, 0, base(25))
    assert up["ratio"] == 10.0 and up["drift"] is True and "DRIFT" in mon.format_report(up)
    assert mon.report(s, 0, base(1000))["drift"] is True                  # ratio 0.25 < 1 / 2
    assert mon.report(s, 0, base(1000), factor=4.0)["drift"] is False     # ... and not below 1 / 4
    # zero baseline: boxes now is drift, none now is not
    zb = mon.report(s, 0, base(0))
    assert zb["ratio"] is None and zb["drift"] is True
    zz = mon.report(s, 1, base(0))
    assert zz["boxes_per_frame"] == 0.0 and zz["ratio"] is None and zz["drift"] is False and "ratio n/a" in mon.format_report(zz)
    assert mon.report(s, 1, base(50))["drift"] is True                    # a camera that went silent
    # no frames: nothing to judge
    e = mon.report(_snapshot(frames=(0, 0)), 0, base(50))
    assert e["frames"] == 0 and e["foreground_share"] == 0.0 and e["drift"] is False
    with pytest.raises(ValueError):
        mon.report(s, 0, {"format": "covahip-post-1"})
    with pytest.raises(ValueError):
        mon.report(s, 0, factor=1.0)


def test_mixed_batches_go_round_robin():
    cams = [np.full((4 * n + extra, 2, 2, 4), k, np.uint8) for k, (n, extra) in enumerate(((3, 0), (1, 2), (2, 3)))]
    for k, c in enumerate(cams):
        c[:, 0, 0, 1] = np.arange(c.shape[0])                     # the frame's number within its camera
    got = list(mon.mixed_batches(cams, 4))
    assert [ids.tolist() for _, _, ids in got] == [[0, 1, 2, 0], [2, 0]]
    for frames, index, ids in got:
        assert frames.shape[0] == 4 * len(ids) and index.tolist() == [[4 * i + 3, 4 * i + 2, 4 * i + 1, 4 * i] for i in range(len(ids))]
        assert (frames[index[:, 0], 0, 0, 0] == ids).all()
    # camera 0's samples in order: frames 0-3, 4-7, 8-11 (newest first in a stack)
    newest = [int(f[i[0], 0, 0, 1]) for f, idx, ids in got for i, k in zip(idx, ids) if k == 0]
    assert newest == [3, 7, 11]
    assert list(mon.mixed_batches([np.zeros((3, 2, 2, 4), np.uint8)], 4)) == []


# ------------------------------------------------------------------------------------------------------------------ the library, no device
def test_null_arguments_need_no_gpu():
    lib = L.lib()
    cfg = L.MonitorCfg(4, 4, 1, 0, 0, 1)
    assert lib.covahip_monitor_begin(None, C.byref(cfg)) == 1
    assert lib.covahip_monitor_begin(None, None) == 1
    assert lib.covahip_monitor_add(None, None, None, None, None, 0, L.MEM_HOST) == 1
    assert lib.covahip_monitor_read(None, 0, None, None, None, None, None, None, None, None) == 1
    assert lib.covahip_monitor_end(None) == 1
    assert lib.covahip_dev_monitor_slice(None, 0) == 1
    assert C.sizeof(L.MonitorCfg) == 24 and L.MONITOR_AREA_BINS == BINS


def test_same_reports_a_difference():
    a, b = empty(2, 2, 2), empty(2, 2, 2)
    same(a, b)
    b["fire"][1, 0, 1] = 1
    with pytest.raises(AssertionError):
        same(a, b)
