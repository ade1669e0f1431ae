"""Oracle of the MoG labeller's macroblock grid (include/covahip.h, "MoG labels": COVAHIP_MOG_GRID_MACROBLOCK), composed from
tests/mog_ref.py, whose Mog2 and post are shape-generic: the working image is half the source in both axes by the 2x2 rounded
mean, and there is one label per 8x8 block of it (its top-left pixel).

  half_bgr          u8 [2h][2w][3] -> u8 [h][w][3], (a + b + c + d + 2) >> 2 per channel
  label_video_grid  the labeller on a clip: raw masks, filled masks, labels, the model
  planted_cases     hand-made masks at a working size that stress the post kernel (tests/test_gpu_mog_grid.py plants them)
  plant             two source frames per mask whose raw MOG2 mask of frame 2 is that mask
"""
from __future__ import annotations

import numpy as np

from tests import mog_ref as R


def half_bgr(frame: np.ndarray) -> np.ndarray:
    h, w, _ = frame.shape
    if h % 2 or w % 2:
        raise ValueError(f"odd source size {w}x{h}")
    f = frame.astype(np.uint32)
    s = f[0::2, 0::2] + f[0::2, 1::2] + f[1::2, 0::2] + f[1::2, 1::2]
    return ((s + 2) >> 2).astype(np.uint8)


def label_video_grid(frames: np.ndarray, history: int = 9000, var_threshold: float = 32.0, model: R.Mog2 | None = None):
    """frames u8 [F][h][w][3] -> (raw [F][h/2][w/2], filled [F][h/2][w/2], labels [F][ceil(h/16)][ceil(w/16)], the model)."""
    _, h, w, _ = frames.shape
    wh, ww = h // 2, w // 2
    mdl = model if model is not None else R.Mog2(npix=ww * wh, history=history, var_threshold=var_threshold)
    raws, fills, labels = [], [], []
    for fr in frames:
        raw = mdl.apply(half_bgr(fr))
        fl, lab = R.post(raw)
        raws.append(raw)
        fills.append(fl)
        labels.append(lab)
    return np.stack(raws), np.stack(fills), np.stack(labels), mdl


# ------------------------------------------------------------------------------------------------ planted masks
def _spiral(h, w, wall=8, gap=8):
    a = np.zeros((h, w), bool)
    top, left, bottom, right = 20, 20, h - 21, w - 21
    step = wall + gap
    while bottom - top > 2 * step and right - left > 2 * step:
        a[top:top + wall, left:right + 1] = True
        a[top:bottom + 1, right - wall + 1:right + 1] = True
        a[bottom - wall + 1:bottom + 1, left + step:right + 1] = True
        a[top + step:bottom + 1, left + step:left + step + wall] = True
        top, left, bottom, right = top + step, left + step, bottom - step, right - step
    return a


def _corridor(h, w, k):
    """A foreground slab with a cavity that a background corridor k pixels high joins to the outside.  The corridor crosses
    every word boundary from the middle of the row to its last word (words 7/8 and 13/14 at 960 wide).  Closing 4x4 shuts a
    corridor lower than 4 pixels, which turns the cavity into a hole."""
    a = np.zeros((h, w), bool)
    x0 = 64 * (w // 128) - 12
    a[100:160, x0 - 40:w - 10] = True
    a[110:150, x0 - 30:x0] = False
    a[130:130 + k, x0:w - 10] = False
    return a


def _diag(h, w):
    """Holes sealed only diagonally: a diamond outline of 1-pixel steps, and one of 8x8 blocks that touch at their corners."""
    a = np.zeros((h, w), bool)
    cy, cx, r = 100, 200, 30
    for t in range(r):
        for py, px in ((cy - r + t, cx + t), (cy + t, cx + r - t), (cy + r - t, cx - t), (cy - t, cx - r + t)):
            a[py, px] = True
    cy, cx, r = 90, 60, 4
    for t in range(r):
        for by, bx in ((-r + t, t), (t, r - t), (r - t, -t), (-t, -r + t)):
            a[cy + 8 * by:cy + 8 * by + 8, cx + 8 * bx:cx + 8 * bx + 8] = True
    return a


def planted_cases(h: int, w: int) -> dict:
    """name -> bool [h][w]; h >= 180, w >= 320."""
    sealed = _spiral(h, w)
    sealed[8:16, 8:w - 8] = sealed[h - 16:h - 8, 8:w - 8] = True
    sealed[8:h - 8, 8:16] = sealed[8:h - 8, w - 16:w - 8] = True
    corner = np.zeros((h, w), bool)
    corner[h - 20:, w - 60:] = True                # the last rows and the last word column only
    return {"spiral": _spiral(h, w), "sealed_spiral": sealed, "corner_blob": corner, "corridor1": _corridor(h, w, 1),
            "corridor4": _corridor(h, w, 4), "diag_hole": _diag(h, w)}


def plant(masks, scale: int, seed: int = 5) -> np.ndarray:
    """masks: S bool [h][w] -> u8 [2][S][scale h][scale w][3]: frame 1 is a background in 0..99, frame 2 is 255 - background
    where the mask is set.  scale 2 repeats every pixel 2x2, so the 2x2 rounded mean gives the working image back exactly."""
    h, w = masks[0].shape
    bg = np.random.default_rng(seed).integers(0, 100, (h, w, 3), dtype=np.uint8)
    up = np.ones((scale, scale, 1), np.uint8)
    vid = np.empty((2, len(masks), scale * h, scale * w, 3), np.uint8)
    for s, m in enumerate(masks):
        vid[0, s] = np.kron(bg, up)
        vid[1, s] = np.kron(np.where(m[..., None], 255 - bg, bg), up)
    return vid
