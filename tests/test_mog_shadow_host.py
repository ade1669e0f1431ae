"""MOG2 shadow detection, the host side: the numpy restatement (tests/mog_shadow_ref.py) on known answers, the proof that the
branch clip reaches the branches of the shadow test, OpenCV parity where cv2 is installed, and the `shadows` values, the
--shadows parser and the NULL checks of the library.  No GPU.

The trace events of mog_shadow_ref.shadow_mask (per tested pixel, and per mode it visits):

  den_zero                  the mode's mean is (0, 0, 0): not a shadow, the loop ends
  num_gt_den                brighter than the mode; num_lt_tau_den: darker than tau allows
  num_eq_den, num_eq_tau_den   on the closed ends of the range tau * den <= num <= den
  dist_pass_mode{0..4}      a shadow, found at that mode; dist_fail: in the range, the colour too far
  tw_exit_mode{0..4}        the weights up to that mode exceed TB = 0.9: not a shadow
  modes_exhausted           every mode visited and none decided
  shadow_on_new_mode        a shadow of the mode step 4 made of this very pixel

modes_exhausted is the one event no clip can reach, and the test says why and asserts the argument on every frame instead of
counting it: see test_branch_coverage.
"""
import collections
import functools

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import mog
from tests import mog_clips as K
from tests import mog_ref as R
from tests import mog_shadow_ref as SR

H, W = 48, 64                                            # the clips of this file: 3,072 pixels, each its own experiment


def _px(c):
    return np.asarray(c, np.uint8).reshape(1, 1, 3)


def _after_constant(color, n=12, history=9000):
    """A one-pixel model that has seen n frames of one colour: one mode, its mean the colour itself, alphaT = 1 / (2n + 2) next."""
    m = R.Mog2(npix=1, history=history)
    for _ in range(n):
        m.apply(_px(color))
    assert m.nmodes[0] == 1 and (m.M[0, :, 0] == np.asarray(color, R.F32)).all()
    return m


# ------------------------------------------------------------------------------------------------ known answers
def test_exact_edges_of_the_brightness_range():
    tr = collections.Counter()
    assert SR.apply3(_after_constant(K.BASE), _px(SR.TAU_EDGE), 0.5, trace=tr)[0, 0] == 127     # num = 22000 = tau * den exactly
    assert tr["num_eq_tau_den"] == 1 and tr["dist_pass_mode0"] == 1
    tr = collections.Counter()
    assert SR.apply3(_after_constant(K.BASE), _px(SR.TAU_BELOW), 0.5, trace=tr)[0, 0] == 255    # 21900: out of the range
    assert tr["num_lt_tau_den"] == 1 and tr["tw_exit_mode0"] == 1
    # the numbers themselves, in f32
    d, m = np.asarray(SR.TAU_EDGE, R.F32), np.asarray(K.BASE, R.F32)
    assert (d * m).sum(dtype=R.F32) == 22000 and (m * m).sum(dtype=R.F32) == 44000
    # a pixel that is background is never tested: the colour itself stays 0, though num == den would make it a shadow
    assert SR.apply3(_after_constant(K.BASE), _px(K.BASE), 0.5)[0, 0] == 0
    assert SR.shadow_mask(_after_constant(K.BASE), _px(K.BASE), 0.5).all()


def test_planted_shadow_and_tau():
    sh = (60, 72, 84)                                        # 0.6 x (100, 120, 140)
    assert SR.apply3(_after_constant(K.BASE), _px(sh), 0.5)[0, 0] == 127
    assert SR.apply3(_after_constant(K.BASE), _px(sh), 0.6)[0, 0] == 255      # a = f32(26400 / 44000) < f32(0.6) * 1: 26400 < 0.6f * 44000
    assert SR.apply3(_after_constant(K.BASE), _px(sh), 0.59)[0, 0] == 127
    assert SR.apply3(_after_constant(K.BASE), _px(sh), 1.0)[0, 0] == 255
    # a colour cast is no shadow: the same brightness ratio with the channels pulled apart fails the distance test
    tr = collections.Counter()
    assert SR.apply3(_after_constant(K.BASE), _px((90, 72, 54)), 0.5, trace=tr)[0, 0] == 255
    assert tr["dist_fail"] == 1
    # brighter than the background is no shadow either
    assert SR.apply3(_after_constant(K.BASE), _px((140, 168, 196)), 0.5)[0, 0] == 255


def test_frame_one_is_all_shadow_but_black():
    rng = np.random.default_rng(5)
    fr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    fr[3, 4:9] = 0
    fr[7, 7] = (0, 0, 1)
    black = (fr == 0).all(-1)
    assert black.sum() >= 5
    tr = collections.Counter()
    m = R.Mog2(npix=H * W)
    raw = SR.apply3(m, fr, 0.5, trace=tr)
    assert (raw[black] == 255).all() and (raw[~black] == 127).all()
    assert tr["den_zero"] == black.sum() and tr["num_eq_den"] == (~black).sum() == tr["dist_pass_mode0"]
    # without the test frame 1 is all foreground; with shadows dropped it is background but for the black pixels
    assert (R.Mog2(npix=H * W).apply(fr) == 255).all()
    assert (SR.fg_of(raw, "drop") == np.where(black, 255, 0)).all() and (SR.fg_of(raw, "keep") == 255).all()
    # and tau does not matter there (a = 1)
    assert (SR.apply3(R.Mog2(npix=H * W), fr, 1.0) == raw).all() and (SR.apply3(R.Mog2(npix=H * W), fr, 1e-3) == raw).all()


def test_the_test_only_reads_the_model_and_keep_is_off():
    clip = SR.shadow_clip(10, 7, H, W)
    a, b = R.Mog2(npix=H * W, history=4, var_threshold=4.0), R.Mog2(npix=H * W, history=4, var_threshold=4.0)
    for fr in clip:
        raw3, raw = SR.apply3(a, fr, 0.5), b.apply(fr)
        assert ((raw3 > 0) == (raw > 0)).all() and set(np.unique(raw3)) <= {0, 127, 255}
        assert (SR.fg_of(raw3, "keep") == raw).all()
    for k in ("W", "V", "M", "nmodes"):
        assert (getattr(a, k).view(np.uint8) == getattr(b, k).view(np.uint8)).all(), k
    off = SR.label_video_shadows(clip, None, history=4, var_threshold=4.0, work=lambda f: f, post=R.post)
    keep = SR.label_video_shadows(clip, "keep", history=4, var_threshold=4.0, work=lambda f: f, post=R.post)
    drop = SR.label_video_shadows(clip, "drop", history=4, var_threshold=4.0, work=lambda f: f, post=R.post)
    assert (off[1] == keep[1]).all() and (off[2] == keep[2]).all() and (keep[0] == drop[0]).all()
    assert (drop[1] != keep[1]).any()


# ------------------------------------------------------------------------------------------------ branch coverage
@functools.lru_cache(maxsize=None)
def _traced(history, tb, frames, seed):
    """(trace of the frames after the first, the weight argument held on every frame) of one configuration at H x W."""
    clip = SR.shadow_clip(frames, seed, H, W)
    m = R.Mog2(npix=H * W, history=history, var_threshold=tb)
    tr = collections.Counter()
    held = True
    for i, fr in enumerate(clip):
        raw = SR.apply3(m, fr, SR.CLIP_TAU, trace=tr if i else None)       # frame 1 would reach num_eq_den and den_zero by itself
        # the argument of test_branch_coverage, on every pixel the test ran on
        data = fr.reshape(-1, 3).T.astype(R.F32)
        live = np.arange(R.NMIX)[:, None] < m.nmodes
        new = (live & (m.M == data).all(1) & (m.V == R.VAR_INIT)).any(0)
        wsum = np.zeros(H * W, R.F32)
        for k in range(R.NMIX):
            wsum = np.where(live[k], wsum + m.W[k], wsum)
        held &= bool((new | (wsum > R.TB))[raw.reshape(-1) != 0].all())
    return tr, held


def test_branch_coverage():
    """Every event on the clips of tests/mog_clips.CONFIGS (with the scripted pixels of shadow_clip) and on the GPU tests' clip.

    num_eq_den away from frame 1 and tw_exit_mode4 ARE reached (a pixel that fits nothing gets a mode of its own colour, and
    with a short history that mode sorts in front of modes whose weights sum to less than TB).

    modes_exhausted is not reachable, by this argument, which `held` asserts on every tested pixel of every frame: a tested
    pixel is no background.  If it fitted a mode, step 3 has just normalised the weights of the modes 0 .. nmodes - 1 to the sum
    1 (tw cannot be ~0 there: the fitted mode alone weighs alphaT * 0.95 or more), so the running sum passes TB = 0.9 at the
    last mode at the latest: tw_exit.  If it fitted none, step 4 gave it a mode whose mean is the pixel and whose variance is
    varInit; at that mode num == den, a = 1 and dist2a = 0 < Tb * 15, a shadow, unless the pixel is black and den == 0 ends the
    loop.  Either way the loop ends inside the modes.  The restatement and the kernels still carry the fall-through `not a
    shadow`, as OpenCV does; the count is asserted to be 0."""
    total = collections.Counter()
    for cfg in K.CONFIGS + (SR.GPU_CLIP,):
        tr, held = _traced(*cfg)
        assert held, cfg
        assert tr["modes_exhausted"] == 0, cfg
        total.update(tr)
    for ev in SR.EVENTS:
        if ev != "modes_exhausted":
            assert total[ev] >= 1, (ev, dict(total))
    # the scripted pixels do what they are for
    assert total["den_zero"] >= 1 and total["num_eq_tau_den"] >= 1
    # the clip of the GPU tests alone reaches all of these in its 12 frames
    gpu, _ = _traced(*SR.GPU_CLIP)
    for ev in ("den_zero", "num_gt_den", "num_lt_tau_den", "num_eq_den", "num_eq_tau_den", "dist_fail", "shadow_on_new_mode",
               "dist_pass_mode0", "dist_pass_mode1", "dist_pass_mode2", "tw_exit_mode0", "tw_exit_mode1", "tw_exit_mode2",
               "tw_exit_mode3"):
        assert gpu[ev] >= 1, (ev, dict(gpu))


def test_planted_scene_on_the_oracle():
    """What the GPU test of the planted scene relies on, at a quarter of its size: the patch is shadow, the block is not."""
    clip, boxes = SR.planted_scene(frames=3, h=184, w=320)
    off = SR.label_video_shadows(clip, None, work=lambda f: f)
    drop = SR.label_video_shadows(clip, "drop", work=lambda f: f)
    for i, (blk, pat) in enumerate(boxes):
        t = SR.SCENE_WARM + i
        assert (drop[0][t][pat[0]:pat[1], pat[2]:pat[3]] == 127).all() and (drop[0][t][blk[0]:blk[1], blk[2]:blk[3]] == 255).all()
        assert (off[0][t][pat[0]:pat[1], pat[2]:pat[3]] == 255).all()
        inner = lambda b: (slice((b[0] + 15) // 8, (b[1] - 8) // 8), slice((b[2] + 15) // 8, (b[3] - 8) // 8))   # noqa: E731
        assert off[2][t][inner(blk)].all() and off[2][t][inner(pat)].all() and off[2][t][inner(pat)].size >= 6
        assert drop[2][t][inner(blk)].all() and not drop[2][t][inner(pat)].any()
    assert not drop[2][:SR.SCENE_WARM][1:].any()


# ------------------------------------------------------------------------------------------------ OpenCV parity (where cv2 exists)
def test_restatement_matches_opencv_where_available():
    cv = pytest.importorskip("cv2")
    clip, _ = SR.planted_scene(frames=6)
    noisy = np.clip(clip.astype(np.int16) + np.random.default_rng(3).normal(0, 2, clip.shape), 0, 255).astype(np.uint8)
    for vid, hist, tb, tau in ((noisy, 9000, 32.0, 0.5), (SR.shadow_clip(24, 1), 16, 32.0, 0.5), (SR.shadow_clip(12, 3), 4, 4.0, 0.7)):
        sub = cv.createBackgroundSubtractorMOG2(history=hist, varThreshold=tb, detectShadows=True)
        sub.setShadowThreshold(tau)
        m = R.Mog2(history=hist, var_threshold=tb)
        for i, f in enumerate(vid):
            assert (sub.apply(f) == SR.apply3(m, f, tau)).all(), (hist, i)


# ------------------------------------------------------------------------------------------------ arguments
def test_shadow_mode_values():
    assert mog.shadow_mode(None) == ("off", 0.5) and mog.shadow_mode("off") == ("off", 0.5)
    assert mog.shadow_mode("drop") == ("drop", 0.5) and mog.shadow_mode(("keep", 1)) == ("keep", 1.0)
    assert mog.shadow_mode(("drop", np.float32(0.25))) == ("drop", 0.25)
    for bad in ("shadow", 3, ("drop",), ("off", 0.5), ("drop", 0), ("drop", -0.5), ("drop", 1.5), ("keep", float("nan")),
                ("keep", float("inf")), ("drop", "0.5"), ("drop", True), ("cover", 0.5), (1, 0.5)):
        with pytest.raises(ValueError):
            mog.shadow_mode(bad)
    # MogLabeler refuses them before it touches the ctx
    for bad in ("shadow", ("drop", 0), ("keep", 2)):
        with pytest.raises(ValueError):
            mog.MogLabeler(None, 640, 360, shadows=bad)


def test_shadows_parser_and_command_line():
    import argparse
    assert mog.parse_shadows("off") is None
    assert mog.parse_shadows("drop") == ("drop", 0.5) and mog.parse_shadows("keep:0.4") == ("keep", 0.4)
    assert mog.parse_shadows("drop:1") == ("drop", 1.0) and mog.parse_shadows("drop:5e-1") == ("drop", 0.5)
    for bad in ("", "on", "off:0.5", "drop:", "drop:0", "drop:1.01", "keep:nan", "keep:inf", "keep:-1", "drop:0.5:1", "Drop"):
        with pytest.raises(argparse.ArgumentTypeError):
            mog.parse_shadows(bad)
    a = mog._args(["--size", "1280x720", "--shadows", "drop:0.5", "a.bgr"])
    assert a.shadows == ("drop", 0.5) and not a.shadow_report
    a = mog._args(["--size", "1280x720", "--shadows", "keep", "--shadow-report", "a.bgr"])
    assert a.shadows == ("keep", 0.5) and a.shadow_report
    assert mog._args(["--size", "1280x720", "a.bgr"]).shadows is None
    for argv in (["--shadow-report"], ["--shadows", "off", "--shadow-report"], ["--shadows", "drop:2"], ["--shadows", "dim"]):
        with pytest.raises(SystemExit) as e:
            mog._args(["--size", "1280x720", "a.bgr"] + argv)
        assert e.value.code == 2


def test_null_labeller_is_refused():
    lib = L.lib()
    assert lib.covahip_mog_set_shadows(None, 1, 0.5) == 1 and lib.covahip_mog_get_shadows(None, None, None) == 1
    assert lib.covahip_mog_shadow_counts(None, None, None, 0, None) == 1
