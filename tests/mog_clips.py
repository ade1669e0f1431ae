"""Clips that drive every branch of the MOG2 update (tests/mog_ref.py, cova_amd/csrc/mog.hip).  Pure numpy: the host test
(tests/test_mog_branches_host.py) proves on the traced oracle that these clips reach the branches, the GPU test
(tests/test_gpu_mog_branches.py) holds the kernel to the oracle on them.

  palette_walk      every pixel is its own experiment: it jumps among up to seven colours of its own (one pair close enough to
                    share a mode), with its own dwell probability and noise level, so pixels fill all five modes, replace the
                    last one, prune in the middle and reorder by up to four places
  scripted_pixels   the first four pixels of row 0 carry hand-written sequences that land exactly on the two strict
                    comparisons: dist2 == Tb * var (threshold 32) and dist2 == 9 * var
  CONFIGS           (history, var_threshold, frames, seed) of the five clips
"""
import numpy as np

from tests import mog_ref as R

# (history, var_threshold, frames, seed)
CONFIGS = ((16, 32.0, 64, 1), (9000, 32.0, 64, 2), (4, 4.0, 40, 3), (1, 32.0, 12, 4), (2, 100.0, 20, 5))

BASE = (100, 120, 140)             # colour c of the scripted pixels
BG_EDGE = (20, 8, 4)               # 400 + 64 + 16 = 480 = 32 * 15: not below Tb * VAR_INIT at threshold 32
BG_NEAR = (20, 8, 3)               # 473: below
FIT_EDGE = (6, 0, 0)               # 36 = 9 * VAR_MIN: not below 9 * var once the variance sits on its lower clamp
FIT_NEAR = (4, 4, 1)               # 33: below
PX_BG_EDGE, PX_BG_NEAR, PX_FIT_EDGE, PX_FIT_NEAR = 0, 1, 2, 3      # x in row 0


def palette_walk(n, seed, h=360, w=640, K=7):
    rng = np.random.default_rng(seed); P = h * w
    pal = rng.integers(0, 256, (K, P, 3)).astype(np.float32)
    near = rng.random(P) < 0.3
    off = rng.integers(-14, 15, (P, 3)).astype(np.float32)
    pal[1] = np.where(near[:, None], np.clip(pal[0] + off, 0, 255), pal[1])
    stay = rng.choice([0.0, 0.5, 0.8, 0.95], P)
    sigma = rng.choice([0.0, 1.0, 3.0, 9.0], P).astype(np.float32)
    kmax = rng.integers(1, K + 1, P)
    idx = np.zeros(P, np.int64); ar = np.arange(P)
    out = np.empty((n, h, w, 3), np.uint8)
    for t in range(n):
        move = rng.random(P) >= stay
        idx = np.where(move, rng.integers(0, K, P) % kmax, idx)
        f = pal[idx, ar] + rng.normal(0, 1, (P, 3)).astype(np.float32) * sigma[:, None]
        out[t] = np.clip(np.rint(f), 0, 255).astype(np.uint8).reshape(h, w, 3)
    return out


def frames_to_var_min(history, limit):
    """How many frames of one constant colour a pixel needs before its only mode's variance is exactly VAR_MIN (the mean
    stays the colour itself: every update moves it by k * 0).  None if `limit` frames do not get there."""
    m = R.Mog2(npix=1, history=history)
    px = np.asarray(BASE, np.uint8).reshape(1, 1, 3)
    for t in range(limit):
        m.apply(px)
        if m.nmodes[0] == 1 and m.V[0, 0] == R.VAR_MIN and (m.M[0, :, 0] == np.asarray(BASE, R.F32)).all():
            return t + 1
    return None


def scripted_pixels(clip, history):
    """Overwrites pixels 0..3 of row 0 in place and returns the frame index at which the fit-edge colours first show.

    x = 0, 1   frame 0 is c, every later frame c + BG_EDGE (x = 0) or c + BG_NEAR (x = 1): at frame 1 the only mode has the
               initial variance 15, so at threshold 32 pixel 0 sits exactly on dist2 == Tb * var and is foreground, pixel 1
               is background
    x = 2, 3   c until the mode's variance has been clamped to exactly 4.0, then c + FIT_EDGE (x = 2) or c + FIT_NEAR (x = 3):
               pixel 2 sits exactly on dist2 == 9 * var, does not fit and gets a second mode; pixel 3 fits
    """
    n = clip.shape[0]
    c = np.asarray(BASE, np.int32)
    hold = frames_to_var_min(history, n - 1)
    if hold is None:
        raise ValueError(f"a clip of {n} frames is too short to reach VAR_MIN with history {history}")
    for x, d in ((PX_BG_EDGE, BG_EDGE), (PX_BG_NEAR, BG_NEAR)):
        clip[0, 0, x] = c
        clip[1:, 0, x] = c + np.asarray(d)
    for x, d in ((PX_FIT_EDGE, FIT_EDGE), (PX_FIT_NEAR, FIT_NEAR)):
        clip[:hold, 0, x] = c
        clip[hold:, 0, x] = c + np.asarray(d)
    return hold


def branch_clip(history, frames, seed):
    """The palette walk of one configuration with the scripted pixels written in: (clip u8 [frames][360][640][3], the frame
    at which the fit-edge colours first show)."""
    clip = palette_walk(frames, seed)
    hold = scripted_pixels(clip, history)
    return clip, hold
