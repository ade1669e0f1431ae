"""MoG labels with MOG2's shadow detection (covahip_mog_set_shadows: COVAHIP_MOG_SHADOWS_OFF / _DROP / _KEEP) against the numpy
restatement tests/mog_shadow_ref.py, bit for bit: there is no tolerance anywhere in this file.

  1. one case per update kernel, in DROP and in KEEP, on the branch clip of tests/mog_shadow_ref.py (tests/test_mog_shadow_host.py
     proves which branches of the shadow test it reaches) or its first frames resized: the raw mask 0 / 127 / 255, the filled
     mask, the labels, shadow_counts and the model
       k_mog_update          640x360 on the reference grid, 640x360 working
       k_mog_grid_update     640x360 on the macroblock grid, 320x180 working
       the same, banded      2560x1440, 1280x720 working: 3 frames, one per call (the scope mog_band_update, beside the banded post)
       k_mog_yuv_update      NV12 at 640x360, a padded surface
       k_mog_any_update      266x258, 133x129 working: 59 dead lanes in every row's last word, which must be in no count
       k_mog_any_yuv_update  I420 at 266x258
  2. frame 1: 127 wherever the pixel is not (0, 0, 0); DROP's first labels are all 0
  3. KEEP against OFF: the same filled masks and labels, and KEEP's foreground + shadow counts are OFF's foreground counts
  4. OFF -> DROP -> KEEP -> OFF between calls on three ragged streams: every call follows its mode, the model is that of a
     labeller that stayed OFF
  5. the planted scene: a moving block that drags a patch of 0.6 x background; DROP labels the block and not the patch
  6. errors and settings; the command line
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import mog
from tests import mog_grid_ref as G
from tests import mog_ref as R
from tests import mog_shadow_ref as SR
from tests import mog_yuv_ref as Y

pytestmark = pytest.mark.gpu

HIST, TB, NF, SEED = SR.GPU_CLIP
TAU = SR.CLIP_TAU
KW = dict(history=HIST, var_threshold=TB)
ANY_W, ANY_H = 266, 258


@functools.lru_cache(maxsize=None)
def _clip():
    c = SR.shadow_clip(NF, SEED)
    c.setflags(write=False)
    return c


def _up2(a):
    return a.repeat(2, -3).repeat(2, -2)


@functools.lru_cache(maxsize=None)
def _source(kind):
    """(what the labeller is given, the working frames [F][wh][ww][3] the restatement sees) of a kernel's case."""
    clip = _clip()
    if kind == "ref640":
        return clip, clip
    if kind == "grid320":
        return clip, np.stack([G.half_bgr(f) for f in clip])
    if kind == "band1280":                                   # the first frames at four times the size: the 2x2 mean gives them at twice
        src = _up2(_up2(clip[:3]))
        return src, _up2(clip[:3])
    if kind == "any":
        src = np.ascontiguousarray(clip[:, :ANY_H, :ANY_W])
        return src, np.stack([G.half_bgr(f) for f in src])
    w, h = (640, 360) if kind == "yuv640" else (ANY_W, ANY_H)
    src = clip[:8, None, :h, :w]
    y, u, v = Y.bgr_to_yuv420(src, "limited")
    bgr = Y.yuv_to_bgr(y, u, v, "limited")[:, 0]
    return (y, u, v), (bgr if kind == "yuv640" else np.stack([G.half_bgr(f) for f in bgr]))


@functools.lru_cache(maxsize=None)
def _raw(kind):
    """(raw 0 / 127 / 255 [F][wh][ww], the model) of the restatement on a case's working frames, once."""
    work = _source(kind)[1]
    mdl = R.Mog2(npix=work.shape[1] * work.shape[2], **KW)
    raw = np.stack([SR.apply3(mdl, f, TAU) for f in work])
    raw.setflags(write=False)
    return raw, mdl


@functools.lru_cache(maxsize=None)
def _post(kind, mode):
    """(filled, labels) of the restatement in a shadow mode (None: without the test, where fg = raw > 0 as in KEEP)."""
    posts = [R.post(SR.fg_of(r, mode)) for r in _raw(kind)[0]]
    return np.stack([p[0] for p in posts]), np.stack([p[1] for p in posts])


def _model_equal(st, mdl, what=""):
    P = mdl.P
    assert st["n"] == mdl.n, what
    assert (st["nmodes"].reshape(P) == mdl.nmodes).all(), (what, "nmodes")
    for k in ("W", "V"):
        assert (st[k].reshape(5, P).view(np.uint32) == getattr(mdl, k).view(np.uint32)).all(), (what, k)
    assert (st["M"].reshape(5, 3, P).view(np.uint32) == mdl.M.view(np.uint32)).all(), (what, "M")


def _counts_of(raw):
    return (raw == 127).sum((-2, -1)).astype(np.uint32), (raw == 255).sum((-2, -1)).astype(np.uint32)


def _labeller(ctx, kind, **kw):
    if kind in ("ref640", "yuv640"):
        return mog.MogLabeler(ctx, 640, 360, **KW, **kw)
    if kind == "grid320":
        return mog.MogLabeler(ctx, 640, 360, grid="macroblock", **KW, **kw)
    if kind == "band1280":
        return mog.MogLabeler(ctx, 2560, 1440, grid="macroblock", **KW, **kw)
    return mog.MogLabeler(ctx, ANY_W, ANY_H, grid="macroblock", any_size=True, **KW, **kw)


def _run(m, kind, per_call):
    """The case's frames through labeller m, per_call frames a call: (labels, raw, filled, shadow counts, foreground counts)."""
    src = _source(kind)[0]
    out = [[] for _ in range(5)]
    n = src[0].shape[0] if isinstance(src, tuple) else src.shape[0]
    for i in range(0, n, per_call):
        if isinstance(src, tuple):
            y, u, v = (a[i:i + per_call] for a in src)
            lay = Y.padded(640, 360, "nv12") if kind == "yuv640" else Y.tight(ANY_W, ANY_H, "i420")
            lab = m.apply_yuv(Y.pack(y, u, v, lay), lay.ctypes(), y.shape[0])
        else:
            lab = m.apply(src[i:i + per_call, None])
        raw, fil = m.debug_masks()
        sh, fg = m.shadow_counts()
        for o, a in zip(out, (lab, raw, fil, sh, fg)):
            o.append(a[:, 0])
    return tuple(np.concatenate(o) for o in out)


@pytest.mark.parametrize("kind,work,per_call", [("ref640", (640, 360), NF), ("grid320", (320, 180), NF), ("band1280", (1280, 720), 1),
                                                 ("yuv640", (640, 360), 8), ("any", (133, 129), NF), ("any_yuv", (133, 129), 8)])
def test_each_update_kernel_against_the_restatement(ctx, kind, work, per_call):
    raw_r, mdl = _raw(kind)
    assert raw_r.shape[1:] == work[::-1]
    assert (raw_r == 127).any() and (raw_r == 255).any() and (raw_r[1:] == 0).any()
    for mode in ("drop", "keep"):
        fil_r, lab_r = _post(kind, mode)
        m = _labeller(ctx, kind, shadows=(mode, TAU))
        assert (m.work_w, m.work_h) == work and m.shadows == (mode, TAU)
        lab, raw, fil, sh, fg = _run(m, kind, per_call)
        assert set(np.unique(raw)) <= {0, 127, 255}
        for i in range(raw_r.shape[0]):
            assert (raw[i] == raw_r[i]).all(), (kind, mode, "raw mask, frame", i, int((raw[i] != raw_r[i]).sum()))
            assert (fil[i] == fil_r[i]).all(), (kind, mode, "filled mask, frame", i)
            assert (lab[i] == lab_r[i]).all(), (kind, mode, "labels, frame", i)
        sh_r, fg_r = _counts_of(raw_r)
        assert sh.dtype == np.uint32 and (sh == sh_r).all() and (fg == fg_r).all(), (kind, mode, sh.tolist(), sh_r.tolist())
        _model_equal(m.state(0), mdl, (kind, mode))
        m.close()
    assert (_post(kind, "drop")[0] != _post(kind, "keep")[0]).any()       # the two modes differ on this clip


# ------------------------------------------------------------------------------------------------ 2. frame 1
def test_frame_one(ctx):
    fr = _clip()[:1]
    black = (fr[0] == 0).all(-1)
    assert black[0, SR.PX_DEN_ZERO] and black.sum() >= 1
    m = mog.MogLabeler(ctx, 640, 360, shadows="drop", **KW)
    m.apply(fr[:, None])
    raw = m.debug_masks()[0][0, 0]
    assert (raw[black] == 255).all() and (raw[~black] == 127).all()
    sh, fg = m.shadow_counts()
    assert sh.tolist() == [[int((~black).sum())]] and fg.tolist() == [[int(black.sum())]]
    m.close()
    scene, _ = SR.planted_scene(frames=1)
    assert not (scene[0] == 0).all(-1).any()
    for shadows, want in (("drop", 0), ("keep", 1), (None, 1)):
        m = mog.MogLabeler(ctx, 640, 360, shadows=shadows)
        lab = m.apply(scene[:1, None])
        assert (lab == want).all(), shadows
        raw = m.debug_masks()[0]
        assert (raw == (255 if shadows is None else 127)).all(), shadows
        m.close()


# ------------------------------------------------------------------------------------------------ 3. KEEP against OFF
def test_keep_is_off_but_for_the_raw_mask_and_the_counts(ctx):
    outs = {}
    for shadows in (None, ("keep", TAU)):
        m = _labeller(ctx, "ref640", shadows=shadows)
        assert m.shadows == shadows
        outs[shadows is None] = _run(m, "ref640", 5) + (m.state(0),)
        m.close()
    off, keep = outs[True], outs[False]
    assert (off[0] == keep[0]).all() and (off[2] == keep[2]).all()
    assert ((off[1] > 0) == (keep[1] > 0)).all() and set(np.unique(off[1])) == {0, 255} and (keep[1] == 127).any()
    assert not off[3].any() and (off[4] == keep[3] + keep[4]).all() and keep[3].any()
    assert (off[4] == (off[1] == 255).sum((1, 2))).all()
    _model_equal(off[5], _raw("ref640")[1], "off")
    _model_equal(keep[5], _raw("ref640")[1], "keep")
    fil_r, lab_r = _post("ref640", None)
    assert (off[2] == fil_r).all() and (off[0] == lab_r).all()


# ------------------------------------------------------------------------------------------------ 4. mode switching
SW_CALLS = ((None, (3, 2, 0)), ("drop", (3, 3, 1)), ("keep", (2, 3, 3)), (None, (3, 1, 3)))


def test_mode_switching_on_ragged_streams(ctx):
    clip = _clip()
    vids = (clip, np.ascontiguousarray(clip[::-1]), np.roll(clip, 5, axis=0))
    frames = np.ascontiguousarray(np.stack(vids, 1))                       # [12][3][360][640][3]
    mdls = [R.Mog2(npix=320 * 180, **KW) for _ in vids]
    a = mog.MogLabeler(ctx, 640, 360, streams=3, grid="macroblock", **KW)  # switches
    b = mog.MogLabeler(ctx, 640, 360, streams=3, grid="macroblock", **KW)  # stays OFF
    for c, (mode, nv) in enumerate(SW_CALLS):
        a.set_shadows(None if mode is None else (mode, TAU))
        assert a.shadows == (None if mode is None else (mode, TAU))
        chunk = frames[3 * c:3 * c + 3]
        lab = a.apply(chunk, n_valid=nv, labels=np.full((3, 3, 23, 40), 9, np.uint8))
        b.apply(chunk, n_valid=nv)
        raw, fil = a.debug_masks()
        sh, fg = a.shadow_counts()
        for s in range(3):
            for f in range(3):
                if f >= nv[s]:
                    assert (lab[f, s] == 9).all() and sh[f, s] == 0 and fg[f, s] == 0, (c, s, f)
                    continue
                wk = G.half_bgr(chunk[f, s])
                r = mdls[s].apply(wk) if mode is None else SR.apply3(mdls[s], wk, TAU)
                fl, lb = R.post(SR.fg_of(r, mode))
                assert (raw[f, s] == r).all() and (fil[f, s] == fl).all() and (lab[f, s] == lb).all(), (c, mode, s, f)
                assert sh[f, s] == (r == 127).sum() and fg[f, s] == (r == 255).sum(), (c, mode, s, f)
    for s in range(3):
        sa, sb = a.state(s), b.state(s)
        for k in ("W", "V", "M", "nmodes"):
            assert (sa[k].view(np.uint8) == sb[k].view(np.uint8)).all(), (s, k)
        _model_equal(sa, mdls[s], s)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 5. the planted scene
def test_planted_scene_drop_keeps_the_shadow_out_of_the_labels(ctx):
    clip, boxes = SR.planted_scene(frames=3)
    labs = {}
    for shadows in (None, "drop"):
        m = mog.MogLabeler(ctx, 640, 360, shadows=shadows)
        labs[shadows] = m.apply(clip[:, None])[:, 0]
        raw = m.debug_masks()[0][:, 0]
        for i, (blk, pat) in enumerate(boxes):
            t = SR.SCENE_WARM + i
            assert (raw[t][pat[0]:pat[1], pat[2]:pat[3]] == (255 if shadows is None else 127)).all(), (shadows, i)
            assert (raw[t][blk[0]:blk[1], blk[2]:blk[3]] == 255).all(), (shadows, i)
        m.close()

    def inner(b):                                            # the macroblocks whose corner pixel lies well inside rectangle b
        return slice((b[0] + 15) // 8, (b[1] - 8) // 8), slice((b[2] + 15) // 8, (b[3] - 8) // 8)

    for i, (blk, pat) in enumerate(boxes):
        t = SR.SCENE_WARM + i
        assert labs[None][t][inner(pat)].size >= 6
        assert labs[None][t][inner(blk)].all() and labs[None][t][inner(pat)].all(), i
        assert labs["drop"][t][inner(blk)].all() and not labs["drop"][t][inner(pat)].any(), i
    assert labs["drop"][SR.SCENE_WARM:].sum() < labs[None][SR.SCENE_WARM:].sum()


# ------------------------------------------------------------------------------------------------ 6. errors, settings, command line
def test_set_shadows_errors_and_settings(ctx):
    lib = L.lib()
    m = mog.MogLabeler(ctx, 640, 360, grid="macroblock", **KW)

    def get():
        mode, tau = C.c_int(-7), C.c_float(-7)
        assert lib.covahip_mog_get_shadows(m.handle, C.byref(mode), C.byref(tau)) == 0
        return mode.value, tau.value

    assert get() == (0, 0.5) and m.shadows is None
    assert lib.covahip_mog_set_shadows(m.handle, 1, 0.25) == 0 and get() == (1, 0.25)
    for mode, tau in ((1, 0.0), (2, float("nan")), (1, 1.5), (1, -0.5), (2, float("inf")), (3, 0.5), (-1, 0.5)):
        assert lib.covahip_mog_set_shadows(m.handle, mode, tau) == 1, (mode, tau)      # COVAHIP_ERR_INVALID_ARG, nothing changed
        assert get() == (1, 0.25), (mode, tau)
    assert lib.covahip_mog_set_shadows(m.handle, 2, 1.0) == 0 and get() == (2, 1.0)    # exactly 1 is admitted
    assert lib.covahip_mog_set_shadows(m.handle, 0, float("nan")) == 0 and get() == (0, 1.0)   # tau is read when mode != OFF
    assert lib.covahip_mog_get_shadows(m.handle, None, None) == 0
    assert lib.covahip_mog_set_shadows(None, 1, 0.5) == 1 and lib.covahip_mog_get_shadows(None, None, None) == 1
    with pytest.raises(ValueError):
        m.set_shadows(("drop", 0))
    # counts: nothing before the first call; then cap is checked against frames x streams
    nf = C.c_int(-1)
    assert lib.covahip_mog_shadow_counts(m.handle, None, None, 0, C.byref(nf)) == 0 and nf.value == 0
    m.set_shadows(("drop", TAU))
    clip = _clip()
    m.apply(clip[:4, None])
    buf = np.full(4, 77, np.uint32)
    assert lib.covahip_mog_shadow_counts(m.handle, buf.ctypes.data, None, 3, C.byref(nf)) == 7 and nf.value == 4   # COVAHIP_ERR_OVERFLOW
    assert (buf == 77).all()
    assert lib.covahip_mog_shadow_counts(m.handle, None, buf.ctypes.data, 3, None) == 7
    assert lib.covahip_mog_shadow_counts(m.handle, buf.ctypes.data, None, 4, None) == 0
    assert (buf == _counts_of(_raw("grid320")[0][:4])[0]).all()
    assert lib.covahip_mog_shadow_counts(m.handle, None, buf.ctypes.data, 4, None) == 0
    assert (buf == _counts_of(_raw("grid320")[0][:4])[1]).all()
    # reset keeps the setting
    m.reset(0)
    assert m.shadows == ("drop", TAU) and m.state(0)["n"] == 0
    lab = m.apply(clip[:2, None])[:, 0]
    assert (lab == _post("grid320", "drop")[1][:2]).all() and (m.debug_masks()[0][:, 0] == _raw("grid320")[0][:2]).all()
    # post_masks takes masks of its own: non-zero is foreground, and no shadow plane goes with them
    raw = _raw("grid320")[0][:2, None]
    assert (m.post_masks(raw)[:, 0] == _post("grid320", "keep")[1][:2]).all()
    assert set(np.unique(m.debug_masks()[0])) <= {0, 255} and not m.shadow_counts()[0].any()
    m.close()


def test_cli_writes_what_the_api_gives(ctx, tmp_path, capsys):
    clip = _clip()
    p = tmp_path / "v.bgr"
    p.write_bytes(clip.tobytes())
    argv = ["--size", "640x360", "--grid", "macroblock", "--history", str(HIST), "--var-threshold", str(TB), "--chunk", "5"]
    for text, mode in (("drop:0.5", "drop"), ("keep:0.5", "keep")):
        out = tmp_path / f"{mode}.dump"
        assert mog.main(argv + ["--shadows", text, "--shadow-report", f"{p}:{out}"]) == 0
        got = np.fromfile(out, np.uint8).reshape(NF, 23, 40)
        assert (got == _post("grid320", mode)[1]).all(), text
        m = _labeller(ctx, "grid320", shadows=(mode, TAU))
        assert (got == m.apply(clip[:, None])[:, 0]).all(), text
        sh, fg = m.shadow_counts()
        m.close()
        line = [ln for ln in capsys.readouterr().out.splitlines() if "shadow" in ln]
        assert len(line) == 1, line
        vals = re.search(r"shadow ([0-9.]+) foreground ([0-9.]+) of 57600 pixels per frame, 12 frames", line[0])
        assert vals, line
        sh_r, fg_r = _counts_of(_raw("grid320")[0])
        assert (sh[:, 0] == sh_r).all() and (fg[:, 0] == fg_r).all()
        assert float(vals.group(1)) == round(sh_r.sum() / (NF * 57600), 6) and float(vals.group(2)) == round(fg_r.sum() / (NF * 57600), 6)
    assert mog.main(argv + [f"{p}:{tmp_path / 'off.dump'}"]) == 0           # the default stays without the test
    assert (np.fromfile(tmp_path / "off.dump", np.uint8).reshape(NF, 23, 40) == _post("grid320", None)[1]).all()
