"""numpy float32 restatement of MOG2's shadow test (include/covahip.h, "MoG labels", step 2a: detectShadowGMM of OpenCV 4.x), on
top of tests/mog_ref.py.  Vectorised over pixels, looped over the five modes; every product and sum is an np.float32 operation of
its own, in the order the header states, and the division goes through float64 (correctly rounded to f32, as the kernels' div_rn).

  shadow_mask          a pure function of a mog_ref.Mog2 AFTER its apply() of `frame`, and of that frame: which pixels pass the test
  apply3               Mog2.apply, then the test where the mask is 255: OpenCV's 0 / 127 / 255
  fg_of                step 3 in a shadow mode: mask == 255 (drop) or mask > 0 (keep, off)
  label_video_shadows  frames -> raw 0 / 127 / 255, filled, labels and the model, through any `work` resize and `post`
  shadow_clip          a palette walk of tests/mog_clips.py with three scripted pixels: a black mode, and the two sides of num == tau * den
  planted_scene        a block that moves over a textured background and drags a patch of 0.6 x background behind it

With a `trace` (a collections.Counter, as Mog2(trace=True) keeps one) shadow_mask counts per-pixel events over the pixels it
tests; tests/test_mog_shadow_host.py lists them and proves that its clip reaches them.
"""
from __future__ import annotations

import numpy as np

from tests import mog_clips as K
from tests import mog_ref as R

F32 = np.float32
EVENTS = (("den_zero", "num_gt_den", "num_lt_tau_den", "num_eq_den", "num_eq_tau_den", "dist_fail", "modes_exhausted",
           "shadow_on_new_mode") + tuple(f"dist_pass_mode{k}" for k in range(R.NMIX)) + tuple(f"tw_exit_mode{k}" for k in range(R.NMIX)))


def shadow_mask(model: R.Mog2, frame: np.ndarray, tau: float, where: np.ndarray | None = None, trace=None) -> np.ndarray:
    """bool [P]: the pixels of `frame` (u8 [..][3], P pixels; the frame `model` has just been given) that are a shadow of one of
    the model's modes.  `where` (bool [P]) restricts the test, and the trace, to those pixels: OpenCV runs it where the pixel
    is no background.  The model is only read.

    trace events, per tested pixel and mode visited: den_zero; num_gt_den, num_lt_tau_den (the two ways out of the brightness
    range); num_eq_den, num_eq_tau_den (on its closed ends); dist_pass_mode{k} (a shadow, found at mode k), dist_fail (in the
    range, too far in colour); tw_exit_mode{k} (the weights up to mode k exceed TB); modes_exhausted (all nmodes modes visited,
    none decided); shadow_on_new_mode (a shadow of the mode step 4 made of this very pixel: mean == data, variance varInit)."""
    data = frame.reshape(-1, 3).T.astype(F32)                    # [3][P]
    P = data.shape[1]
    tau = F32(tau)
    zero = F32(0)
    done = np.zeros(P, bool) if where is None else ~where.reshape(-1)
    tested = ~done
    shadow = np.zeros(P, bool)
    tw = np.zeros(P, F32)

    def count(name, sel):
        c = int(np.count_nonzero(sel))
        if trace is not None and c:
            trace[name] += c

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for mode in range(R.NMIX):
            act = (mode < model.nmodes) & ~done
            if not act.any():
                continue
            m = model.M[mode]
            num = ((zero + data[0] * m[0]) + data[1] * m[1]) + data[2] * m[2]
            den = ((zero + m[0] * m[0]) + m[1] * m[1]) + m[2] * m[2]
            dz = act & (den == 0)
            count("den_zero", dz)
            done |= dz
            act &= ~dz
            inr = act & (num <= den) & (num >= tau * den)
            count("num_gt_den", act & ~(num <= den))
            count("num_lt_tau_den", act & (num <= den) & ~(num >= tau * den))
            count("num_eq_den", act & (num == den))
            count("num_eq_tau_den", inr & (num == tau * den))
            a = (num.astype(np.float64) / den.astype(np.float64)).astype(F32)
            d0, d1, d2 = a * m[0] - data[0], a * m[1] - data[1], a * m[2] - data[2]
            dist2a = ((zero + d0 * d0) + d1 * d1) + d2 * d2
            hit = inr & (dist2a < ((model.Tb * model.V[mode]) * a) * a)
            count(f"dist_pass_mode{mode}", hit)
            count("dist_fail", inr & ~hit)
            count("shadow_on_new_mode", hit & (m == data).all(axis=0) & (model.V[mode] == R.VAR_INIT))
            shadow |= hit
            done |= hit
            act &= ~hit
            tw = np.where(act, tw + model.W[mode], tw)
            ex = act & (tw > R.TB)
            count(f"tw_exit_mode{mode}", ex)
            done |= ex
    count("modes_exhausted", tested & ~done)
    return shadow


def apply3(model: R.Mog2, frame: np.ndarray, tau: float, trace=None) -> np.ndarray:
    """model.apply(frame), then the shadow test on the updated model where the mask is 255: u8 of the frame's shape without the
    channels, 0 background / 127 shadow / 255 foreground (createBackgroundSubtractorMOG2(.., detectShadows=True).apply)."""
    mask = model.apply(frame)
    sh = shadow_mask(model, frame, tau, where=mask.reshape(-1) == 255, trace=trace)
    return np.where(sh.reshape(mask.shape), np.uint8(127), mask)


def fg_of(mask3: np.ndarray, mode) -> np.ndarray:
    """Step 3 of a shadow mode on a 0 / 127 / 255 mask, as the 0 / 255 mask mog_ref.post and its kin take."""
    fg = mask3 == 255 if mode == "drop" else mask3 > 0
    return np.where(fg, np.uint8(255), np.uint8(0))


def label_video_shadows(frames: np.ndarray, mode, tau: float = 0.5, history: int = 9000, var_threshold: float = 32.0,
                        model: R.Mog2 | None = None, work=R.resize_bgr, post=R.post, trace=None):
    """frames u8 [F][h][w][3] -> (raw [F][wh][ww] of 0 / 127 / 255 -- 0 / 255 with mode None --, filled, labels, the model).
    mode: None (no test), "drop" or "keep"; `work` makes the working image of a source frame (mog_ref.resize_bgr,
    mog_grid_ref.half_bgr, ..) and `post` the filled mask and the labels of a 0 / 255 mask (mog_ref.post, mog_band_ref.post)."""
    mdl = model
    raws, fills, labels = [], [], []
    for fr in frames:
        wk = work(fr)
        if mdl is None:
            mdl = R.Mog2(npix=wk.shape[0] * wk.shape[1], history=history, var_threshold=var_threshold)
        raw = mdl.apply(wk) if mode is None else apply3(mdl, wk, tau, trace=trace)
        fl, lab = post(fg_of(raw, mode))
        raws.append(raw)
        fills.append(fl)
        labels.append(lab)
    return np.stack(raws), np.stack(fills), np.stack(labels), mdl


# ------------------------------------------------------------------------------------------------ the branch clip
PX_DEN_ZERO, PX_TAU_EDGE, PX_TAU_BELOW = 4, 5, 6       # x in row 0 (0 .. 3 are the scripted pixels of tests/mog_clips.py)
TAU_EDGE, TAU_BELOW = (50, 60, 70), (49, 60, 70)       # over K.BASE = (100, 120, 140): num = 22000 = 0.5 * den, and 21900
CLIP_TAU = 0.5
GPU_CLIP = (4, 4.0, 12, 3)                             # (history, var_threshold, frames, seed): history 4 fills five modes in 12 frames


def shadow_clip(frames: int, seed: int, h: int = 360, w: int = 640, at: int = 8):
    """K.palette_walk(frames, seed, h, w) with three pixels of row 0 overwritten (frames > at >= 1):
    x = PX_DEN_ZERO   black in frame 0, (200, 200, 200) after: in frame 1 its first mode has the mean (0, 0, 0), so den == 0
    x = PX_TAU_EDGE   K.BASE up to frame at - 1 (a constant history keeps the mean exact), TAU_EDGE from frame `at`: at tau = 0.5
                      num == tau * den exactly, in the range and a shadow
    x = PX_TAU_BELOW  the same with TAU_BELOW: num < tau * den, out of the range"""
    clip = K.palette_walk(frames, seed, h, w)
    clip[0, 0, PX_DEN_ZERO] = 0
    clip[1:, 0, PX_DEN_ZERO] = 200
    for x, c in ((PX_TAU_EDGE, TAU_EDGE), (PX_TAU_BELOW, TAU_BELOW)):
        clip[:at, 0, x] = K.BASE
        clip[at:, 0, x] = c
    return clip


# ------------------------------------------------------------------------------------------------ planted scene
SCENE_BLOCK = (96, 64, 40, 56)         # (y, first x, height, width) of the moving block, working pixels
SCENE_STEP = 32                        # its x advance per frame: a pixel shows the block or the patch twice at most, before MOG2 learns it
SCENE_WARM = 12                        # frames of background alone before it enters


def planted_scene(frames: int = 4, h: int = 360, w: int = 640, seed: int = 11):
    """(clip u8 [SCENE_WARM + frames][h][w][3], boxes): a static textured background (every channel 80 .. 199, so no mode is
    black), then for `frames` frames a block of a far colour that moves right by SCENE_STEP a frame and drags, directly below
    it, a patch of the same size that shows round(0.6 x background): a cast shadow.  boxes[i] = (block, patch) rectangles
    (y0, y1, x0, x1) of frame SCENE_WARM + i."""
    rng = np.random.default_rng(seed)
    bgd = rng.integers(80, 200, (h, w, 3)).astype(np.uint8)
    clip = np.repeat(bgd[None], SCENE_WARM + frames, axis=0)
    y, x0, bh, bw = SCENE_BLOCK
    boxes = []
    for i in range(frames):
        x = x0 + i * SCENE_STEP
        fr = clip[SCENE_WARM + i]
        fr[y:y + bh, x:x + bw] = (250, 20, 250)
        fr[y + bh:y + 2 * bh, x:x + bw] = np.rint(bgd[y + bh:y + 2 * bh, x:x + bw].astype(np.float32) * np.float32(0.6)).astype(np.uint8)
        boxes.append(((y, y + bh, x, x + bw), (y + bh, y + 2 * bh, x, x + bw)))
    return clip, boxes
