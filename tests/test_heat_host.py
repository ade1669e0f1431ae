"""The host half of "Ignore region from heat" (cova_amd/calibrate.py): rects_from_keep, ignore_from_heat, the sidecar and the
command line's new flags.  No GPU."""
import json

import numpy as np
import pytest

from cova_amd import calibrate as cal
from cova_amd.elements import keep_from_rects

SIZES = [(5, 7), (68, 120)]


def _check_rects(keep, unit=16):
    h, w = keep.shape
    rects = cal.rects_from_keep(keep, unit)
    assert np.array_equal(keep_from_rects(h, w, rects, unit), (keep != 0).astype(np.uint8))
    assert rects == sorted(rects, key=lambda r: (r[1], r[0]))
    cover = np.zeros((h, w), np.int32)
    for left, top, width, height in rects:
        assert all(isinstance(v, int) for v in (left, top, width, height))
        assert left % unit == 0 and top % unit == 0 and width % unit == 0 and height % unit == 0 and width > 0 and height > 0
        assert 0 <= left and left + width <= w * unit and 0 <= top and top + height <= h * unit
        cover[top // unit:(top + height) // unit, left // unit:(left + width) // unit] += 1
    assert cover.max(initial=0) <= 1                                      # disjoint
    assert np.array_equal(cover == 1, keep == 0)
    return rects


@pytest.mark.parametrize("h,w", SIZES)
def test_rects_round_trip_random(h, w):
    rng = np.random.default_rng(100 * h + w)
    for i in range(200):
        density = (0.02, 0.2, 0.5, 0.9)[i % 4]
        keep = (rng.random((h, w)) >= density).astype(np.uint8)
        if i % 3 == 0:                                                    # blocks, so that runs recur in consecutive rows
            for _ in range(4):
                y, x = rng.integers(0, h), rng.integers(0, w)
                keep[y:y + rng.integers(1, 6), x:x + rng.integers(1, 9)] = 0
        if i % 7 == 0:
            keep *= 255                                                   # any non-zero value keeps
        _check_rects(keep)


@pytest.mark.parametrize("h,w", SIZES)
def test_rects_special_maps(h, w):
    ones = np.ones((h, w), np.uint8)
    assert cal.rects_from_keep(ones) == []
    assert _check_rects(np.zeros((h, w), np.uint8)) == [(0, 0, 16 * w, 16 * h)]
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        k = ones.copy()
        k[y, x] = 0
        assert _check_rects(k) == [(16 * x, 16 * y, 16, 16)]
    corners = ones.copy()
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = 0
    assert len(_check_rects(corners)) == 4
    yy, xx = np.mgrid[0:h, 0:w]
    checker = ((yy + xx) % 2).astype(np.uint8)
    assert len(_check_rects(checker)) == int((checker == 0).sum())        # nothing merges
    assert len(_check_rects(1 - checker)) == int((checker == 1).sum())
    # rows that repeat merge vertically, and only those
    k = ones.copy()
    k[1:4, 2:5] = 0
    k[4, 2:4] = 0
    assert _check_rects(k) == [(32, 16, 48, 48), (32, 64, 32, 16)]
    assert _check_rects(k, unit=8) == [(16, 8, 24, 24), (16, 32, 16, 8)]


def _heat(h=4, w=6, T=3, samples=10):
    return {"fire": np.zeros((T, h, w), np.int64), "both": np.zeros((T, h, w), np.int64), "gt": np.zeros((h, w), np.int64),
            "samples": samples, "logit_thresh": np.arange(T, dtype=np.float32)}


def test_ignore_boundary_is_an_exact_fraction():
    ht = _heat(samples=10)
    ht["fire"][0, 0, 0] = 3                                               # exactly 0.3 * 10: hot (0.3 * 10 in floating point is not 3)
    ht["fire"][0, 0, 1] = 2                                               # one less: not
    keep = cal.ignore_from_heat(ht, 0.3)
    assert keep.dtype == np.uint8 and keep.shape == (4, 6)
    assert keep[0, 0] == 0 and keep[0, 1] == 1 and int((keep == 0).sum()) == 1
    ht = _heat(samples=7)
    ht["gt"][1, 1], ht["gt"][1, 2] = 7, 6
    assert int((cal.ignore_from_heat(ht, 1.0) == 0).sum()) == 1
    ht = _heat(samples=3)
    ht["fire"][0, 2, 2], ht["fire"][0, 2, 3] = 1, 2
    keep = cal.ignore_from_heat(ht, (2, 3))
    assert keep[2, 2] == 1 and keep[2, 3] == 0
    for bad in (0.0, -0.5, 1.5, (3, 2)):
        with pytest.raises(ValueError):
            cal.ignore_from_heat(ht, bad)


def test_ignore_sources_at_and_dilate():
    ht = _heat(h=6, w=8, samples=10)
    ht["fire"][0, 1, 1] = 9
    ht["fire"][1, 1, 1] = 2
    ht["fire"][:, 4, 6] = [9, 8, 7]
    ht["gt"][3, 3] = 10

    def hot(**kw):
        return [(int(y), int(x)) for y, x in np.argwhere(cal.ignore_from_heat(ht, 0.5, **kw) == 0)]

    assert hot() == [(1, 1), (3, 3), (4, 6)]
    assert hot(source="either") == hot()
    assert hot(source="pred") == [(1, 1), (4, 6)]
    assert hot(source="labels") == [(3, 3)]
    assert hot(at=1) == [(3, 3), (4, 6)] and hot(at=2, source="pred") == [(4, 6)] and hot(at=-1, source="pred") == [(4, 6)]
    with pytest.raises(ValueError):
        cal.ignore_from_heat(ht, 0.5, at=3)
    with pytest.raises(ValueError):
        cal.ignore_from_heat(ht, 0.5, source="both")
    # dilate: 8-neighbour steps, clipped at the border
    one = hot(source="labels", dilate=1, max_share=1.0)
    assert one == [(y, x) for y in (2, 3, 4) for x in (2, 3, 4)]
    two = hot(source="labels", dilate=2, max_share=1.0)
    assert two == [(y, x) for y in range(1, 6) for x in range(1, 6)]
    edge = _heat(h=6, w=8, samples=10)
    edge["gt"][0, 7] = 10
    assert sorted((int(y), int(x)) for y, x in np.argwhere(cal.ignore_from_heat(edge, 0.5, dilate=1) == 0)) == [(0, 6), (0, 7), (1, 6), (1, 7)]


def test_ignore_refuses_empty_and_blinding():
    ht = _heat(samples=0)
    with pytest.raises(ValueError):
        cal.ignore_from_heat(ht, 0.5)
    ht = _heat(h=4, w=6, samples=10)                                      # 24 macroblocks: a quarter is 6
    ht["gt"][0, :6] = 10
    assert int((cal.ignore_from_heat(ht, 0.5) == 0).sum()) == 6           # exactly the share: allowed
    ht["gt"][1, 0] = 10
    with pytest.raises(ValueError):
        cal.ignore_from_heat(ht, 0.5)
    assert int((cal.ignore_from_heat(ht, 0.5, max_share=0.5) == 0).sum()) == 7
    with pytest.raises(ValueError):                                       # the share is taken after the dilation
        cal.ignore_from_heat(ht, 0.5, max_share=0.5, dilate=1)


def test_add_heat():
    a, b = _heat(samples=4), _heat(samples=6)
    a["fire"][0, 0, 0], b["fire"][0, 0, 0], b["gt"][1, 1], a["both"][2, 3, 5] = 1, 2, 3, 4
    s = cal.add_heat(a, b)
    assert s["samples"] == 10 and s["fire"][0, 0, 0] == 3 and s["gt"][1, 1] == 3 and s["both"][2, 3, 5] == 4
    assert a["fire"][0, 0, 0] == 1                                        # the operands are left alone
    with pytest.raises(ValueError):
        cal.add_heat(a, _heat(T=2))
    c = _heat(samples=1)
    c["logit_thresh"] = c["logit_thresh"] + 1
    with pytest.raises(ValueError):
        cal.add_heat(a, c)


CHOICE = {"logit_thresh": 0.25, "cc_threshold": 4, "met": True, "min_recall": 0.95, "object_recall": 1.0, "object_precision": 0.5,
          "pixel_recall": 0.9, "pixel_precision": 0.8, "pred": 10, "pred_true": 5, "gt_found": 7, "gt_objects": 7, "truncated": 0,
          "samples": 40, "grid": {"logit_thresh": [0.0, 0.25], "area_thresh": [1, 4], "gt_area": 1, "iou": [1, 10], "max_boxes": 256}}


def test_sidecar_round_trip(tmp_path):
    h, w = 45, 80
    rng = np.random.default_rng(9)
    keep = (rng.random((h, w)) >= 0.1).astype(np.uint8)
    keep[2:5, 66:78] = 0
    auto = {"rate": [1, 2], "source": "either", "dilate": 0, "logit_thresh": -2.944, "samples": 40, "macroblocks_ignored": 36,
            "user_rects": [[0, 0, 320, 48]]}
    path = tmp_path / "post.json"
    cal.save_post(path, CHOICE, cal.rects_from_keep(keep), auto)
    kw, cc = cal.load_post(path, h, w)
    assert np.array_equal(kw["keep"], keep) and cc == 4 and kw["logit_thresh"] == 0.25
    doc = json.loads(path.read_text())
    assert doc["auto_ignore"] == auto and doc["format"] == "covahip-post-1"
    # without auto_ignore the sidecar has no such key, is what it was before, and still loads
    plain = tmp_path / "plain.json"
    cal.save_post(plain, CHOICE, [(0, 0, 320, 48)])
    doc = json.loads(plain.read_text())
    assert list(doc) == ["format", "logit_thresh", "prob_thresh", "cc_threshold", "ignore_rects", "scores", "grid"]
    kw, cc = cal.load_post(plain, h, w)
    assert np.array_equal(kw["keep"], keep_from_rects(h, w, [(0, 0, 320, 48)])) and cc == 4
    none = tmp_path / "none.json"
    cal.save_post(none, CHOICE, cal.rects_from_keep(np.ones((h, w), np.uint8)), auto)
    assert cal.load_post(none, h, w)[0]["keep"] is None


def test_argument_parsing(capsys):
    base = ["rec.tfrecord", "--weights", "cam.cvhw"]
    a = cal.parse_args(base)
    assert a.auto_ignore is None and a.auto_ignore_source == "either" and a.auto_ignore_dilate == 0 and a.heat_out is None
    a = cal.parse_args(base + ["--auto-ignore", "0.5"])
    assert a.auto_ignore == 0.5 and a.auto_ignore_source == "either" and a.auto_ignore_dilate == 0
    a = cal.parse_args(base + ["--auto-ignore", "0.8", "--auto-ignore-source", "labels", "--auto-ignore-dilate", "2", "--heat-out", "h.npz",
                               "--ignore-rects", "0,0,32,32"])
    assert (a.auto_ignore, a.auto_ignore_source, a.auto_ignore_dilate, a.heat_out) == (0.8, "labels", 2, "h.npz")
    assert a.ignore_rects == [(0, 0, 32, 32)]
    assert cal.parse_args(base + ["--auto-ignore", "1", "--auto-ignore-source", "pred"]).auto_ignore_source == "pred"
    for bad in (["--auto-ignore-source", "labels"], ["--auto-ignore-dilate", "1"], ["--heat-out", "h.npz"],
                ["--auto-ignore", "0"], ["--auto-ignore", "1.5"], ["--auto-ignore", "0.5", "--auto-ignore-source", "both"],
                ["--auto-ignore", "0.5", "--auto-ignore-dilate", "-1"], ["--auto-ignore"]):
        with pytest.raises(SystemExit):
            cal.parse_args(base + bad)
    capsys.readouterr()


def test_heat_summary_counts():
    ht = _heat(samples=10)
    ht["fire"][:, 0, 0] = [9, 5, 4]
    ht["fire"][:, 0, 1] = [5, 4, 0]
    ht["gt"][2, 2] = 5
    lines = cal.heat_summary(ht, 0.5).splitlines()
    assert len(lines) == 2 + 3
    assert [ln.split("|")[1].split() for ln in lines[2:]] == [["2", "1"], ["1", "1"], ["0", "1"]]
