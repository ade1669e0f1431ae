"""Every branch of the GPU MOG2 update (k_mog_update, cova_amd/csrc/mog.hip) against the numpy oracle, bit for bit, on the
clips of tests/mog_clips.py: all five modes live, the fifth replaced, fits at mode 4 that bubble four places, prunes in the
middle, var_threshold below and above 9, history 1 and 2, and pixels that sit exactly on the two strict comparisons.
tests/test_mog_branches_host.py shows on the traced oracle that the clips reach these branches.  The staged host path
(several update launches per call, f0 > 0) and a ragged n_valid on device pointers are checked here too."""
import ctypes as C
import functools

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import mog
from tests import mog_clips as K
from tests import mog_ref as R

pytestmark = pytest.mark.gpu

P = R.WORK_W * R.WORK_H
STATE_KEYS = ("W", "V", "M", "nmodes")


@functools.lru_cache(maxsize=None)
def _case(ci):
    """(clip, the oracle's raw masks, the oracle's model after the clip) of configuration ci, computed once."""
    history, tb, frames, seed = K.CONFIGS[ci]
    clip, _ = K.branch_clip(history, frames, seed)
    mdl = R.Mog2(history=history, var_threshold=tb)
    raws = np.stack([mdl.apply(f) for f in clip])
    for a in (clip, raws, mdl.W, mdl.V, mdl.M, mdl.nmodes):
        a.setflags(write=False)
    return clip, raws, mdl


def _state_equal(got, mdl):
    assert got["n"] == mdl.n
    assert (got["nmodes"].reshape(P) == mdl.nmodes).all(), "nmodes"
    for k in ("W", "V"):
        assert (got[k].reshape(5, P).view(np.uint32) == getattr(mdl, k).view(np.uint32)).all(), k
    assert (got["M"].reshape(5, 3, P).view(np.uint32) == mdl.M.view(np.uint32)).all(), "M"


def _same_state(a, b, what):
    for k in STATE_KEYS:
        assert (a[k].view(np.uint8) == b[k].view(np.uint8)).all(), (what, k)
    assert a["n"] == b["n"], what


def _in_chunks(ctx, clip, chunk, **kw):
    """One stream labelled `chunk` frames per call: (labels, raw masks, filled masks, final state)."""
    m = mog.MogLabeler(ctx, 640, 360, **kw)
    lab, raw, fil = [], [], []
    for i in range(0, clip.shape[0], chunk):
        lab.append(m.apply(clip[i:i + chunk, None])[:, 0])
        r, f = m.debug_masks()
        raw.append(r[:, 0])
        fil.append(f[:, 0])
    st = m.state(0)
    m.close()
    return np.concatenate(lab), np.concatenate(raw), np.concatenate(fil), st


@pytest.mark.parametrize("ci", range(len(K.CONFIGS)))
def test_branches_bit_exact_against_oracle(ctx, ci):
    history, tb, n, _ = K.CONFIGS[ci]
    clip, raw_r, mdl = _case(ci)
    kw = dict(history=history, var_threshold=tb)
    lab, raw, fil, st = _in_chunks(ctx, clip, n, **kw)
    for i in range(n):
        assert (raw[i] == raw_r[i]).all(), f"raw mask, frame {i}"
    _state_equal(st, mdl)
    for i in (0, n // 2, n - 1):
        f_r, l_r = R.post(raw_r[i])
        assert (fil[i] == f_r).all(), f"filled mask, frame {i}"
        assert (lab[i] == l_r).all(), f"labels, frame {i}"
    # the modes reloaded from memory every frame, or every fifth, instead of staying in registers over the whole clip
    for chunk in (1, 5):
        lab_c, raw_c, fil_c, st_c = _in_chunks(ctx, clip, chunk, **kw)
        assert (raw_c == raw).all() and (fil_c == fil).all() and (lab_c == lab).all(), chunk
        _same_state(st_c, st, chunk)


def test_two_streams_forward_and_reversed(ctx):
    history, tb, n, _ = K.CONFIGS[0]
    clip, raw_r, mdl = _case(0)
    kw = dict(history=history, var_threshold=tb)
    vids = (clip, np.ascontiguousarray(clip[::-1]))
    alone = [_in_chunks(ctx, v, n, **kw) for v in vids]
    m = mog.MogLabeler(ctx, 640, 360, streams=2, **kw)
    lab = m.apply(np.stack(vids, 1))
    raw, fil = m.debug_masks()
    for s in range(2):
        assert (lab[:, s] == alone[s][0]).all() and (raw[:, s] == alone[s][1]).all() and (fil[:, s] == alone[s][2]).all(), s
        _same_state(m.state(s), alone[s][3], s)
    assert (raw[:, 0] == raw_r).all()
    _state_equal(m.state(0), mdl)
    m.close()


# ------------------------------------------------------------------------------------------------ staged host calls
ST_S, ST_F, ST_HISTORY, ST_TB = 3, 11, 4, 4.0          # history 4 fills all five modes within the 11 frames
ST_STEP = ST_S * 640 * 360 * 3                         # bytes of one frame-step: one frame of every stream
RAGGED = ([11, 5, 0], [4, 8, 9])                       # a stream ends on a launch boundary, inside a launch, before one


@functools.lru_cache(maxsize=None)
def _staged_case():
    """(frames [11][3][360][640][3], per stream: raw masks of its frames and {frames seen: model snapshot})."""
    vids = [K.palette_walk(ST_F, 50 + s) for s in range(ST_S)]
    want = [sorted({nv[s] for nv in RAGGED} | {ST_F}) for s in range(ST_S)]
    per = []
    for s in range(ST_S):
        mdl = R.Mog2(history=ST_HISTORY, var_threshold=ST_TB)
        snaps, raws = {}, []
        for t in range(ST_F + 1):
            if t in want[s]:
                snap = R.Mog2(history=ST_HISTORY, var_threshold=ST_TB)
                snap.W, snap.V, snap.M, snap.nmodes, snap.n = mdl.W.copy(), mdl.V.copy(), mdl.M.copy(), mdl.nmodes.copy(), mdl.n
                snaps[t] = snap
            if t < ST_F:
                raws.append(mdl.apply(vids[s][t]))
        per.append((np.stack(raws), snaps))
    return np.ascontiguousarray(np.stack(vids, 1)), per


@functools.lru_cache(maxsize=None)
def _staged_post(s, t):
    return R.post(_staged_case()[1][s][0][t])


def _staged_run(ctx, frames, nv, budget, device=False):
    """One call of 11 frames: (labels, raw, filled, states, update launches)."""
    m = mog.MogLabeler(ctx, 640, 360, streams=ST_S, history=ST_HISTORY, var_threshold=ST_TB)
    if budget is not None:
        m.set_stage_budget(budget)
    labels = np.full((ST_F, ST_S, 45, 80), 77, np.uint8)
    ctx.profile(True)
    try:
        if device:
            d_f, d_l = ctx.malloc(frames.nbytes), ctx.malloc(labels.nbytes)
            try:
                ctx.h2d(d_f, frames)
                ctx.h2d(d_l, labels)
                m.apply_device(d_f, ST_F, d_l, n_valid=nv)
                ctx.d2h(labels, d_l)
            finally:
                ctx.free(d_f)
                ctx.free(d_l)
        else:
            m.apply(frames, n_valid=nv, labels=labels)
        launches = ctx.profile_read()["mog_update"][1]
    finally:
        ctx.profile(False)
    raw, fil = m.debug_masks()
    states = [m.state(s) for s in range(ST_S)]
    m.close()
    return labels, raw, fil, states, launches


def _same_run(a, b, nv, what):
    assert (a[0] == b[0]).all(), (what, "labels")
    for s in range(ST_S):
        k = nv[s]
        assert (a[1][:k, s] == b[1][:k, s]).all() and (a[2][:k, s] == b[2][:k, s]).all(), (what, s, "masks")
        _same_state(a[3][s], b[3][s], (what, s))


@pytest.mark.parametrize("nv", RAGGED, ids=["11-5-0", "4-8-9"])
def test_staged_host_call_matches_one_launch_and_oracle(ctx, nv):
    frames, per = _staged_case()
    whole = _staged_run(ctx, frames, nv, None)
    staged = _staged_run(ctx, frames, nv, 4 * ST_STEP)            # launches of 4, 4 and 3 frames
    assert whole[4] == 1 and staged[4] == 3
    _same_run(staged, whole, nv, "budget of 4 frame-steps")
    for s in range(ST_S):
        k = nv[s]
        raws, snaps = per[s]
        for t in range(k):
            assert (staged[1][t, s] == raws[t]).all(), (s, t)
        for t in sorted({0, k // 2, k - 1} & set(range(k))):
            f_r, l_r = _staged_post(s, t)
            assert (staged[2][t, s] == f_r).all() and (staged[0][t, s] == l_r).all(), (s, t)
        assert (staged[0][k:, s] == 77).all(), s                 # labels past n_valid keep the caller's bytes
        _state_equal(staged[3][s], snaps[k])


def test_budget_below_one_frame_step_is_one_frame_per_launch(ctx):
    frames, _ = _staged_case()
    nv = RAGGED[1]
    whole = _staged_run(ctx, frames, nv, 0)                       # 0 = the default budget
    single = _staged_run(ctx, frames, nv, ST_STEP - 1)
    tiny = _staged_run(ctx, frames, nv, 1)
    assert whole[4] == 1 and single[4] == ST_F and tiny[4] == ST_F
    _same_run(single, whole, nv, "budget of one frame-step less a byte")
    _same_run(tiny, whole, nv, "budget of one byte")
    assert L.lib().covahip_dev_mog_set_stage_budget(None, C.c_size_t(0)) == 1


@pytest.mark.parametrize("nv", RAGGED, ids=["11-5-0", "4-8-9"])
def test_device_pointers_with_ragged_n_valid_match_host(ctx, nv):
    frames, per = _staged_case()
    host = _staged_run(ctx, frames, nv, None)
    dev = _staged_run(ctx, frames, nv, None, device=True)
    assert dev[4] == 1
    _same_run(dev, host, nv, "device pointers")
    for s in range(ST_S):
        assert (dev[0][nv[s]:, s] == 77).all(), s
        _state_equal(dev[3][s], per[s][1][nv[s]])
