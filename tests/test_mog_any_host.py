"""The MoG labeller at any even source size (covahip_mog_create_any, cova_amd.mog any_size=True; the general kernels) without a
GPU: the refusals that come before the ctx is touched, the Python layer's and the command line's, the label shapes, the oracle's
shapes at sizes whose working image is no multiple of 8 or 64, and the ISA of the kernels."""
import ctypes as C

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import mog
from tests import mog_grid_ref as G
from tests import mog_isa


def _cfg(w, h):
    cfg = L.MogCfg()
    L.lib().covahip_mog_default_cfg(C.byref(cfg))
    cfg.src_w, cfg.src_h = w, h
    return cfg


@pytest.mark.parametrize("size", [(801, 600), (800, 601), (254, 256), (256, 254), (4098, 256), (256, 4098)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_create_any_refuses_the_size_before_the_ctx(size):
    lib = L.lib()
    fake_ctx = C.c_void_p(8)                           # never dereferenced: the size check comes first
    cfg = _cfg(*size)
    h_out = C.c_void_p(1)
    assert lib.covahip_mog_create_any(fake_ctx, C.byref(cfg), C.byref(h_out)) == 5 and not h_out.value


def test_create_any_argument_errors_before_the_ctx():
    lib = L.lib()
    fake_ctx = C.c_void_p(8)
    cfg = _cfg(800, 600)
    h_out = C.c_void_p(1)
    assert lib.covahip_mog_create_any(fake_ctx, None, C.byref(h_out)) == 1 and not h_out.value
    assert lib.covahip_mog_create_any(fake_ctx, C.byref(cfg), None) == 1
    h_out = C.c_void_p(1)
    assert lib.covahip_mog_create_any(None, C.byref(cfg), C.byref(h_out)) == 1 and not h_out.value
    for field, bad in (("n_streams", 0), ("n_streams", 1025), ("history", 0), ("var_threshold", 0.0), ("var_threshold", float("nan"))):
        cfg = _cfg(800, 600)
        setattr(cfg, field, bad)
        h_out = C.c_void_p(1)
        assert lib.covahip_mog_create_any(fake_ctx, C.byref(cfg), C.byref(h_out)) == 1 and not h_out.value, (field, bad)
    # bad streams on a bad size: the argument error, as covahip_mog_create_grid orders them
    cfg = _cfg(801, 600)
    cfg.n_streams = 0
    assert lib.covahip_mog_create_any(fake_ctx, C.byref(cfg), C.byref(h_out)) == 1


def test_dims_any():
    assert mog.label_dims_any(800, 600) == (38, 50)
    assert mog.label_dims_any(1920, 1080) == (68, 120) == mog.label_dims(1920, 1080, "macroblock")
    assert mog.label_dims_any(1280, 960) == (60, 80) and mog.work_dims_any(1280, 960) == (640, 480)
    assert mog.label_dims_any(382, 258) == (17, 24) and mog.work_dims_any(382, 258) == (191, 129)
    assert mog.label_dims_any(256, 256) == (16, 16) and mog.label_dims_any(4096, 4096) == (256, 256)
    for w, h in ((801, 600), (800, 601), (254, 256), (256, 254), (4098, 256), (256, 4098)):
        with pytest.raises(ValueError):
            mog.work_dims_any(w, h)
        with pytest.raises(ValueError):
            mog.label_dims_any(w, h)
    # the table's lists did not grow
    assert mog.GRID_SIZES == {"reference": mog.SIZES, "macroblock": mog.SIZES + ((2560, 1440), (3840, 2160))}
    with pytest.raises(ValueError):
        mog.label_dims(800, 600, "macroblock")


def test_labeler_refuses_before_the_ctx():
    with pytest.raises(ValueError):
        mog.MogLabeler(None, 800, 600, grid="reference", any_size=True)
    with pytest.raises(ValueError):
        mog.MogLabeler(None, 800, 600, any_size=True)              # the default grid is the reference grid
    with pytest.raises(ValueError):
        mog.MogLabeler(None, 1280, 720, grid="reference", force_general=True)
    for w, h in ((801, 600), (800, 601), (254, 256), (4098, 256), (256, 4098)):
        with pytest.raises(ValueError):
            mog.MogLabeler(None, w, h, grid="macroblock", any_size=True)


def test_cli_any_size(capsys):
    a = mog._args(["--any-size", "382x258", "a.bgr"])
    assert a.size == (382, 258) and a.grid == "macroblock" and a.any_size == (382, 258)
    a = mog._args(["--any-size", "1280x960", "--grid", "macroblock", "--format", "nv12", "a.nv12"])
    assert a.size == (1280, 960) and a.grid == "macroblock"
    assert mog._args(["--any-size", "704x576", "--format", "y4m", "a.y4m"]).size == (704, 576)
    a = mog._args(["--size", "1280x720", "a.bgr"])                 # without it nothing moved
    assert a.size == (1280, 720) and a.grid == "reference" and a.any_size is None
    for argv in (["--any-size", "800x600", "--size", "1280x720", "a.bgr"],
                 ["--any-size", "800x600", "--grid", "reference", "a.bgr"],
                 ["--any-size", "801x600", "a.bgr"],
                 ["--any-size", "254x256", "a.bgr"],
                 ["--any-size", "4098x256", "a.bgr"],
                 ["--size", "800x600", "a.bgr"],
                 ["--size", "800x600", "--grid", "macroblock", "a.bgr"]):
        with pytest.raises(SystemExit) as e:
            mog.main(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()


def test_cli_y4m_header_must_state_the_any_size(tmp_path, capsys):
    p = tmp_path / "v.y4m"
    p.write_bytes(b"YUV4MPEG2 W384 H258 F25:1 C420\n")
    with pytest.raises(SystemExit) as e:
        mog.main(["--any-size", "382x258", "--format", "y4m", str(p)])
    assert e.value.code == 2
    assert "384x258" in capsys.readouterr().err


@pytest.mark.parametrize("size", [(382, 258), (264, 272), (660, 380)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_shapes_at_sizes_of_no_table(size):
    w, h = size
    raw, fill, lab, _ = G.label_video_grid(np.zeros((1, h, w, 3), np.uint8))
    assert raw.shape == fill.shape == (1,) + mog.work_dims_any(w, h)[::-1]
    assert lab.shape == (1,) + mog.label_dims_any(w, h) == (1, -(-h // 16), -(-w // 16))
    assert lab.all()                                   # frame 1 is all foreground


def test_any_kernels_isa_no_f32_fma_no_scratch():
    """With the flags of test_mog_host's ISA test: the three general update kernels (mog_update.hip) have no f32 fused
    multiply-add, and neither they nor the general post kernel (mog_post.hip) use scratch."""
    mog_isa.assert_update_family(r"k_mog_any_\w*update", 3)
    mog_isa.assert_post_family(r"k_mog_any_post", 1)
