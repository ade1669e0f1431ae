"""The MoG labeller at 2560x1440 and 3840x2160 (the macroblock grid's banded kernels, cova_amd/csrc/mog_post.hip) without a GPU:
the size lists and label shapes, the argument checks that come before any GPU call, the command line, the oracle's shapes,
the band plan, the planted masks the GPU tests use, and the ISA of the kernels."""
import ctypes as C

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import mog
from tests import mog_band_ref as B
from tests import mog_grid_ref as G
from tests import mog_isa

NEW = {(2560, 1440): ((1280, 720), (90, 160)), (3840, 2160): ((1920, 1080), (135, 240))}


def test_grid_sizes_and_dims():
    assert mog.SIZES == ((640, 360), (1280, 720), (1920, 1080))
    assert mog.GRID_SIZES == {"reference": mog.SIZES, "macroblock": mog.SIZES + ((2560, 1440), (3840, 2160))}
    for (w, h), (work, lab) in NEW.items():
        assert mog.work_dims(w, h, "macroblock") == work
        assert mog.label_dims(w, h, "macroblock") == lab
        with pytest.raises(ValueError):
            mog.label_dims(w, h)
        with pytest.raises(ValueError):
            mog.work_dims(w, h, "reference")
        with pytest.raises(ValueError):
            mog.MogLabeler(None, w, h)                 # refused before the ctx is touched
    assert mog.label_dims(1920, 1080, "macroblock") == (68, 120) and mog.label_dims(1920, 1080) == (45, 80)
    with pytest.raises(ValueError):
        mog.label_dims(800, 600, "macroblock")


def test_create_refuses_the_new_sizes_on_the_reference_grid_before_the_ctx():
    lib = L.lib()
    cfg = L.MogCfg()
    lib.covahip_mog_default_cfg(C.byref(cfg))
    fake_ctx = C.c_void_p(8)                           # never dereferenced: the size check comes first
    for w, h in NEW:
        cfg.src_w, cfg.src_h = w, h
        h_out = C.c_void_p(1)
        assert lib.covahip_mog_create_grid(fake_ctx, C.byref(cfg), 0, C.byref(h_out)) == 5 and not h_out.value
        h_out = C.c_void_p(1)
        assert lib.covahip_mog_create(fake_ctx, C.byref(cfg), C.byref(h_out)) == 5 and not h_out.value
    cfg.src_w, cfg.src_h = 800, 600
    for grid in (0, 1):
        h_out = C.c_void_p(1)
        assert lib.covahip_mog_create_grid(fake_ctx, C.byref(cfg), grid, C.byref(h_out)) == 5 and not h_out.value
    cfg.src_w, cfg.src_h = 2160, 3840                  # transposed
    assert lib.covahip_mog_create_grid(fake_ctx, C.byref(cfg), 1, C.byref(h_out)) == 5
    assert lib.covahip_dev_mog_set_post_form(None, 1, 0) == 1
    assert lib.covahip_dev_mog_post_masks(None, None, 1, None) == 1


def test_cli_size_and_grid(capsys):
    a = mog._args(["--size", "3840x2160", "--grid", "macroblock", "a.bgr"])
    assert a.size == (3840, 2160) and a.grid == "macroblock"
    assert mog._args(["--size", "2560x1440", "--grid", "macroblock", "a.bgr"]).size == (2560, 1440)
    assert mog.parse_size("3840x2160") == (3840, 2160)
    for argv in (["--size", "3840x2160", "a.bgr"], ["--size", "2560x1440", "--grid", "reference", "a.bgr"]):
        with pytest.raises(SystemExit) as e:
            mog.main(argv)
        assert e.value.code == 2
        assert "--grid macroblock" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        mog.main(["--size", "800x600", "--grid", "macroblock", "a.bgr"])
    assert e.value.code == 2


def test_oracle_label_shapes_of_the_new_sizes():
    for (w, h), (work, lab_shape) in NEW.items():
        raw, fill, lab, _ = G.label_video_grid(np.zeros((1, h, w, 3), np.uint8))
        assert raw.shape == fill.shape == (1, work[1], work[0])
        assert lab.shape == (1,) + lab_shape
        assert lab.all()                               # frame 1 is all foreground


@pytest.mark.parametrize("work", [(960, 540), (1280, 720), (1920, 1080)])
def test_band_plan(work):
    w, h = work
    rows, bands, lds = B.band_plan(w, h)
    assert rows >= 16 and rows * bands >= h and rows * (bands - 1) < h
    assert lds <= 160 * 1024 - 64
    assert lds >= 2 * min(rows + 16, h) * (w // 64) * 8          # both staged planes
    assert B.seams(h, rows) == [rows * b for b in range(1, bands)]
    # one row more per band would not fit, or there would be fewer bands
    if bands > 1:
        fewer = -(-h // (bands - 1))
        assert 2 * (fewer + 16) * (w // 64) * 8 > 160 * 1024 - 64
    lib = L.lib()
    assert lib.covahip_dev_mog_band_plan(w, h, None, None, None) == 0
    assert lib.covahip_dev_mog_band_plan(w + 1, h, None, None, None) == 1
    assert lib.covahip_dev_mog_band_plan(0, h, None, None, None) == 1


def test_band_plans_are_the_expected_ones():
    assert B.band_plan(960, 540)[:2] == (540, 1)
    assert B.band_plan(1280, 720)[:2] == (360, 2)
    assert B.band_plan(1920, 1080)[:2] == (270, 4)


def test_planted_masks_do_what_they_are_for():
    h, w = 360, 640                                    # the builders are shape-generic; small for the oracle's sake
    seam = [120, 240]
    # a 1-pixel corridor is shut by the closing (its cavity becomes a hole), a 4-pixel one survives
    for k, hole in ((1, True), (4, False)):
        m = B.seam_corridors(h, w, k, seam)
        x0 = 64 * (w // 128) - 12
        f, _ = B.post(m)
        for s in seam:
            assert not m[s, x0 - 15] and bool(f[s, x0 - 15]) == hole, (k, s)
    # gap 3 closes, gap 4 stays; bar 5 goes, bar 6 stays: at every offset around the seam
    s = 100
    m = B.seam_morphology(200, 1920, [s])              # 28 features of 64 columns each
    f, _ = B.post(m)
    for j, o in enumerate(range(-3, 4)):
        c = 1 + 4 * j
        p = s + o
        assert f[p, 64 * c] == 1 and f[p, 64 * (c + 1)] == 0 and f[p, 64 * (c + 2)] == 0 and f[p, 64 * (c + 3)] == 1, o
        assert m[p, 64 * c - 1] == 0 and m[p, 64 * (c + 2) - 1] == 1
    # the serpentine: nothing filled when open, exactly the last lane when its opening is walled up
    opened = B.serpentine(h, w)
    f, _ = B.post(opened)
    ys, xs = B.last_lane(h, w)
    # (walls of 8 pixels and openings of 8 and 24 pass close and open unchanged but for the even kernels' shift by 2 pixels)
    inner = f[ys, xs][4:-4, 4:-4]
    assert not inner.any() and f.sum() == opened.sum()
    closed = B.serpentine(h, w, closed_last=True)
    f, _ = B.post(closed)
    assert f[ys, xs][4:-4, 4:-4].all()
    assert f.sum() == closed.sum() + (ys.stop - ys.start) * (xs.stop - xs.start)
    assert B.corner_blob(h, w)[-1, -1] and B.blocks(h, w, 0.3, 1).shape == (h, w)


def test_band_kernels_isa_no_f32_fma_no_scratch():
    """With the flags of test_mog_host's ISA test: none of the three banded post kernels (mog_post.hip) uses scratch (the
    1920-wide one holds 60 64-bit words per lane in the row fill).  The update kernels of these sizes are two of the four
    instances test_mog_grid_host's ISA test counts and checks; they are named here so that they cannot leave unnoticed."""
    mog_isa.assert_post_family(r"k_mog_band_post", 3)
    mog_isa.assert_update_family(r"k_mog_grid_updateILi(1280|1920)E", 2)
