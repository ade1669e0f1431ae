"""The MoG labeller's macroblock grid without a GPU: the oracle composition (tests/mog_grid_ref.py) against tests/mog_ref.py, the
label shapes, the planted masks the GPU tests use, the argument checks that come before any GPU call, the command line, and
the ISA of the macroblock grid's kernels."""
import ctypes as C

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import mog
from tests import mog_grid_ref as G
from tests import mog_isa
from tests import mog_ref as R
from tests.test_gpu_mog import synth_video


def test_half_resize_is_the_rounded_2x2_mean():
    rng = np.random.default_rng(3)
    f = rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
    r = G.half_bgr(f)
    assert r.shape == (540, 960, 3)
    for (y, x) in ((0, 0), (539, 959), (123, 456)):
        blk = f[2 * y:2 * y + 2, 2 * x:2 * x + 2].astype(int)
        assert (r[y, x] == (blk.sum(axis=(0, 1)) + 2) // 4).all()
    f720 = rng.integers(0, 256, (720, 1280, 3), dtype=np.uint8)
    assert (G.half_bgr(f720) == R.resize_bgr(f720)).all()
    with pytest.raises(ValueError):
        G.half_bgr(np.zeros((5, 4, 3), np.uint8))


def test_oracle_at_1280x720_is_the_reference_oracle():
    vid = synth_video(6, 1280, 720, seed=8)
    raw, fill, lab, mdl = G.label_video_grid(vid)
    raw_r, fill_r, lab_r, mdl_r = R.label_video(vid)
    assert lab.shape == (6, 45, 80)
    assert (raw == raw_r).all() and (fill == fill_r).all() and (lab == lab_r).all()
    assert (mdl.W.view(np.uint32) == mdl_r.W.view(np.uint32)).all() and mdl.n == mdl_r.n


def test_label_shapes_of_the_new_sizes():
    for (w, h), shape in (((1920, 1080), (68, 120)), ((640, 360), (23, 40))):
        vid = np.zeros((1, h, w, 3), np.uint8)
        raw, fill, lab, _ = G.label_video_grid(vid)
        assert raw.shape == fill.shape == (1, h // 2, w // 2)
        assert lab.shape == (1,) + shape
        assert lab.all()                               # frame 1 is all foreground


def test_label_dims():
    assert mog.label_dims(1920, 1080, "macroblock") == (68, 120)
    assert mog.label_dims(1280, 720, "macroblock") == (45, 80)
    assert mog.label_dims(640, 360, "macroblock") == (23, 40)
    for w, h in mog.SIZES:
        assert mog.label_dims(w, h, "reference") == (45, 80) == mog.label_dims(w, h)
    assert mog.work_dims(1920, 1080, "macroblock") == (960, 540) and mog.work_dims(1920, 1080) == (640, 360)
    with pytest.raises(ValueError):
        mog.label_dims(800, 600, "macroblock")
    with pytest.raises(ValueError):
        mog.label_dims(1920, 1080, "mb")
    with pytest.raises(ValueError):
        mog.MogLabeler(None, 1920, 1080, grid="mb")    # refused before the ctx is touched


def test_corner_blob_reaches_the_labels_past_the_plane():
    """At 960x540 a blob in rows 520-539, columns 900-959 sets label row 67 (working row 536, the partial last block row), label
    column 119 (the last word column) and labels whose index is beyond the 8,100 words of a plane."""
    m = G.planted_cases(540, 960)["corner_blob"]
    filled, lab = R.post(np.where(m, 255, 0).astype(np.uint8))
    assert lab.shape == (68, 120)
    assert lab[67, 119] == 1 and lab[67].sum() > 1 and lab[:, 119].sum() > 1
    assert np.flatnonzero(lab.reshape(-1)).max() >= 8100
    assert filled[536, 952] == 1 and not filled[:500].any()


def test_planted_masks_come_out_of_the_oracle_as_planted():
    cases = G.planted_cases(180, 320)
    names = sorted(cases)
    vid = G.plant([cases[n] for n in names], 2)
    assert vid.shape == (2, len(names), 360, 640, 3)
    for s, n in enumerate(names):
        raw, _, lab, _ = G.label_video_grid(vid[:, s])
        assert (raw[1] == np.where(cases[n], 255, 0)).all(), n
        assert lab.shape == (2, 23, 40)
    # the corridor cases differ in what the fill does: 4 pixels survive the closing, 1 pixel does not
    f4, _ = R.post(np.where(cases["corridor4"], 255, 0).astype(np.uint8))
    f1, _ = R.post(np.where(cases["corridor1"], 255, 0).astype(np.uint8))
    assert not f4[130, 100] and f1[130, 100]


def test_create_grid_and_dims_argument_checks_need_no_gpu():
    lib = L.lib()
    cfg = L.MogCfg()
    lib.covahip_mog_default_cfg(C.byref(cfg))
    h = C.c_void_p(1)
    fake_ctx = C.c_void_p(8)                           # never dereferenced: these checks come first
    assert lib.covahip_mog_create_grid(None, C.byref(cfg), 1, C.byref(h)) == 1 and not h.value
    assert lib.covahip_mog_create_grid(fake_ctx, None, 1, C.byref(h)) == 1
    assert lib.covahip_mog_create_grid(fake_ctx, C.byref(cfg), 1, None) == 1
    assert lib.covahip_mog_create_grid(fake_ctx, C.byref(cfg), 2, C.byref(h)) == 1
    assert lib.covahip_mog_create_grid(fake_ctx, C.byref(cfg), -1, C.byref(h)) == 1
    cfg.src_w, cfg.src_h = 800, 600
    assert lib.covahip_mog_create_grid(fake_ctx, C.byref(cfg), 1, C.byref(h)) == 5 and not h.value
    v = C.c_int32(7)
    assert lib.covahip_mog_dims(None, C.byref(v), None, None, None) == 1 and v.value == 7


def test_cli_grid_parsing(capsys):
    a = mog._args(["--size", "1920x1080", "--grid", "macroblock", "a.bgr"])
    assert a.grid == "macroblock" and a.size == (1920, 1080)
    assert mog._args(["--size", "1920x1080", "a.bgr"]).grid == "reference"
    for argv in (["--size", "1920x1080", "--grid", "mb", "a.bgr"], ["--size", "1920x1080", "--grid", "a.bgr"]):
        with pytest.raises(SystemExit) as e:
            mog.main(argv)
        assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        mog.main(["--help"])
    assert e.value.code == 0
    assert "--grid" in capsys.readouterr().out


def test_grid_kernels_isa_no_f32_fma_no_scratch():
    """With the flags of test_mog_host's ISA test: the macroblock grid's update kernels (mog_update.hip: one template at the four
    working sizes off 640x360, those of 1440p and 4K sources among them) have no f32 fused multiply-add, and neither they nor its
    resident post kernels (mog_post.hip) use scratch (the 960x540 post kernel holds 45 64-bit words per lane in the row fill)."""
    mog_isa.assert_update_family(r"k_mog_grid_update", 4)
    mog_isa.assert_post_family(r"k_mog_grid_postILi(960|320)E", 2)
