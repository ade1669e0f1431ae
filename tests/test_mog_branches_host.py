"""The clips of tests/mog_clips.py reach every branch of the MOG2 update, shown on the traced numpy oracle (tests/mog_ref.py,
Mog2(trace=True)) without a GPU.  tests/test_gpu_mog_branches.py holds the kernel to the oracle on the same clips; the floors
here are what keeps that comparison from being vacuous.  They are conditions on the inputs (about a quarter of the counts the
generator gives), not on the code under test.

Events, counted per pixel and frame:
  fit_mode{0..4}            the first fitting mode; fit_swaps{1..4}: how far it bubbled up; fit_sort_tie: w == W[i - 1] on the way
  prune_mode{0..4}          a mode's weight fell below -prune; prune_not_last: while later modes were still live
  new_at_nm{0..5}           nothing fitted, by the mode count then (new_at_nm5 replaces the last mode)
  new_swaps{1..4}           how far the new mode was sorted up; new_sort_tie: alphaT == W[i - 1] on the way
  vmin, vmax                a variance clamp took effect on the fitting mode
  bg_at_mode{0..4}          the background test passed at that mode; bg_blocked_by_TB: close enough, but tw >= 0.9
  bgclose_not_fit           dist2 < Tb var but not < 9 var, and fit_not_bgclose the reverse (var_threshold below 9)
  bg_edge, fit_edge         dist2 == Tb var, dist2 == 9 var exactly
  tw_zero                   |tw| <= FLT_EPSILON: the inv = 0 branch
"""
import collections
import functools

import numpy as np
import pytest

from tests import mog_clips as K
from tests import mog_ref as R

P = R.WORK_W * R.WORK_H
F32 = np.float32


@functools.lru_cache(maxsize=None)
def _traced(ci):
    """(trace, foreground share per frame, all finite) of configuration ci (0-based), computed once."""
    history, tb, frames, seed = K.CONFIGS[ci]
    clip, _ = K.branch_clip(history, frames, seed)
    m = R.Mog2(history=history, var_threshold=tb, trace=True)
    share = [float((m.apply(f) > 0).mean()) for f in clip]
    finite = all(bool(np.isfinite(a).all()) for a in (m.W, m.V, m.M))
    return m.trace, share, finite


# floors per configuration (1-based in the issue, 0-based here): event -> least count
FLOORS = (
    dict(new_at_nm5=200_000, fit_mode4=15_000, fit_swaps4=90, prune_not_last=1_500, bg_blocked_by_TB=15_000,
         bgclose_not_fit=50_000),
    dict(new_at_nm5=200_000, fit_mode4=15_000, prune_not_last=100, bg_blocked_by_TB=15_000, bgclose_not_fit=50_000),
    dict(new_at_nm5=200_000, fit_mode4=15_000, fit_swaps4=10_000, new_swaps4=30_000, prune_not_last=10_000,
         fit_not_bgclose=170_000),
    dict(prune_mode0=250_000, bgclose_not_fit=50_000),
    dict(new_swaps4=30_000, prune_not_last=50_000, bgclose_not_fit=50_000),
)


@pytest.mark.parametrize("ci", range(len(K.CONFIGS)))
def test_clip_reaches_its_branches(ci):
    trace, share, finite = _traced(ci)
    print(K.CONFIGS[ci], dict(sorted(trace.items())), "foreground share", min(share[1:]), max(share[1:]))
    for ev, least in dict(FLOORS[ci], vmin=50_000, vmax=50_000).items():
        assert trace[ev] >= least, (ev, trace[ev], least)
    if ci == 3:
        # history 1: alpha1 = 0, every unfitted mode is pruned and tw is 0 long after frame 1 (where it is 0 for every clip)
        assert trace["tw_zero"] > P
    assert share[0] == 1.0
    assert all(0.03 <= s <= 0.6 for s in share[1:]), (min(share[1:]), max(share[1:]))
    assert finite


def test_every_event_is_reached_by_some_clip():
    """new_sort_tie is reachable and is asserted: with history 2, alphaT = alpha1 = 0.5 from frame 1 on, and a pixel whose
    single mode (weight w * (1 / w) == 1, times alpha1) does not fit gets a new mode with alphaT == W[0] exactly."""
    total = collections.Counter()
    for ci in range(len(K.CONFIGS)):
        total.update(_traced(ci)[0])
    for ev in ("bg_edge", "fit_edge", "fit_sort_tie", "new_sort_tie", "tw_zero", "bg_blocked_by_TB", "bgclose_not_fit",
               "fit_not_bgclose", "prune_not_last", "vmin", "vmax"):
        assert total[ev] >= 1, ev
    for k in range(5):
        assert total[f"fit_mode{k}"] >= 1 and total[f"prune_mode{k}"] >= 1 and total[f"bg_at_mode{k}"] >= 1, k
    for k in range(1, 5):
        assert total[f"fit_swaps{k}"] >= 1 and total[f"new_swaps{k}"] >= 1, k
    for k in range(6):
        assert total[f"new_at_nm{k}"] >= 1, k


@pytest.mark.parametrize("history", [c[0] for c in K.CONFIGS])
def test_scripted_pixels_land_on_the_strict_comparisons(history):
    n = 40
    clip = np.zeros((n, 1, 4, 3), np.uint8)
    hold = K.scripted_pixels(clip, history)
    assert 2 <= hold < n
    m = R.Mog2(npix=4, history=history, var_threshold=32.0, trace=True)
    c = np.asarray(K.BASE, F32)
    for t in range(hold + 1):
        if t == hold:
            # the fit-edge pixels' only mode: mean c, variance exactly on the lower clamp
            for x in (K.PX_FIT_EDGE, K.PX_FIT_NEAR):
                assert m.nmodes[x] == 1 and m.V[0, x] == R.VAR_MIN and (m.M[0, :, x] == c).all()
            before = m.trace["fit_edge"]
        mask = m.apply(clip[t])[0]
        if t == 0:
            assert (mask == 255).all() and m.trace["bg_edge"] == 0
        if t == 1:
            # dist2 = 480 = 32 * 15 exactly: not background; 473: background
            assert mask[K.PX_BG_EDGE] == 255 and mask[K.PX_BG_NEAR] == 0
            assert m.trace["bg_edge"] == 1
    # dist2 = 36 = 9 * 4 exactly: no fit, a second mode; 33 fits
    assert m.trace["fit_edge"] == before + 1
    # (with history 1, alpha1 = 0 prunes the mode that did not fit, and the new one is the only one again)
    assert m.nmodes[K.PX_FIT_EDGE] == (1 if history == 1 else 2) and m.nmodes[K.PX_FIT_NEAR] == 1
    new = int(np.argmax(m.V[:2, K.PX_FIT_EDGE] == R.VAR_INIT))       # (sorted to the front where alphaT >= the old weight)
    assert m.V[new, K.PX_FIT_EDGE] == R.VAR_INIT and (m.M[new, :, K.PX_FIT_EDGE] == c + np.asarray(K.FIT_EDGE, F32)).all()
    assert m.V[0, K.PX_FIT_NEAR] != R.VAR_INIT and (m.M[0, :, K.PX_FIT_NEAR] != c).any()


@pytest.mark.parametrize("history,tb,seed", [(c[0], c[1], c[3]) for c in K.CONFIGS])
def test_tracing_changes_no_bit(history, tb, seed):
    clip = K.palette_walk(24, seed, h=36, w=64)
    a = R.Mog2(npix=36 * 64, history=history, var_threshold=tb)
    b = R.Mog2(npix=36 * 64, history=history, var_threshold=tb, trace=True)
    assert a.trace is None
    for f in clip:
        assert (a.apply(f) == b.apply(f)).all()
    assert b.trace and sum(b.trace[f"new_at_nm{k}"] for k in range(6)) + sum(b.trace[f"fit_mode{k}"] for k in range(5)) == 24 * 36 * 64
    for k in ("W", "V", "M"):
        assert (getattr(a, k).view(np.uint32) == getattr(b, k).view(np.uint32)).all(), k
    assert (a.nmodes == b.nmodes).all() and a.n == b.n == 24


@pytest.mark.parametrize("history,n,most_modes", [(16, 48, 4), (9000, 200, 5)])
def test_what_the_older_clips_reach(history, n, most_modes):
    """Why the clips above exist.  The two 640x360 clips of tests/test_gpu_mog.py::test_bit_exact_against_oracle (a smooth
    background with sigma 2.5 noise and four ellipses) never replace the fifth mode, never sort by four places and leave no
    pixel with five modes."""
    from tests.test_gpu_mog import synth_video
    vid = synth_video(n, 640, 360, seed=640 + history)
    m = R.Mog2(history=history, trace=True)
    most = 0
    for f in vid:
        m.apply(f)
        most = max(most, int(m.nmodes.max()))
    print(history, n, dict(sorted(m.trace.items())))
    assert most == most_modes
    assert (m.nmodes == 5).sum() == 0
    assert m.trace["new_at_nm5"] == 0
    assert m.trace["fit_swaps4"] == 0 and m.trace["new_swaps4"] == 0
    assert m.trace["fit_edge"] == 0 and m.trace["fit_not_bgclose"] == 0
