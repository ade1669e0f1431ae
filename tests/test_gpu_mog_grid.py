"""MoG labels on the source's macroblock grid (cova_amd.mog, grid="macroblock" / covahip_mog_create_grid) against the numpy oracle
(tests/mog_grid_ref.py over tests/mog_ref.py), bit for bit: raw mask, filled mask, labels and the model, at 1920x1080 (960x540
working frames, 68x120 labels) and 640x360 (320x180, 23x40); 1280x720 against the reference-grid labeller."""
import ctypes as C
import functools

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import mog
from tests import mog_grid_ref as G
from tests import mog_ref as R
from tests.test_gpu_mog import synth_video

pytestmark = pytest.mark.gpu

MODEL = ("W", "V", "M", "nmodes")


def _state_equal(got, mdl):
    P = mdl.P
    assert got["n"] == mdl.n
    assert (got["nmodes"].reshape(P) == mdl.nmodes).all(), "nmodes"
    for k in ("W", "V"):
        assert (got[k].reshape(5, P).view(np.uint32) == getattr(mdl, k).view(np.uint32)).all(), k
    assert (got["M"].reshape(5, 3, P).view(np.uint32) == mdl.M.view(np.uint32)).all(), "M"


def _same_model(a, b, what=""):
    for k in MODEL:
        assert (a[k].view(np.uint8) == b[k].view(np.uint8)).all(), (what, k)
    assert a["n"] == b["n"], what


@pytest.mark.parametrize("size,history,n", [((1920, 1080), 9000, 10), ((640, 360), 16, 48)])
def test_bit_exact_against_oracle(ctx, size, history, n):
    w, h = size
    vid = synth_video(n, w, h, seed=w + history)
    raw_r, fill_r, lab_r, mdl = G.label_video_grid(vid, history=history)
    m = mog.MogLabeler(ctx, w, h, streams=1, history=history, grid="macroblock")
    assert (m.work_w, m.work_h, m.label_h, m.label_w) == (w // 2, h // 2) + mog.label_dims(w, h, "macroblock")
    labels = m.apply(vid[:, None])
    raw, filled = m.debug_masks()
    assert labels.shape == (n, 1) + lab_r.shape[1:] and raw.shape == (n, 1, h // 2, w // 2)
    for i in range(n):
        assert (raw[i, 0] == raw_r[i]).all(), f"raw mask, frame {i}"
        assert (filled[i, 0] == fill_r[i]).all(), f"filled mask, frame {i}"
    assert (labels[:, 0] == lab_r).all()
    assert lab_r[1:].any() and (raw_r[1:] == 0).any() and (raw_r[1:] == 255).any()       # the clip exercises both classes
    _state_equal(m.state(0), mdl)
    m.close()


def test_1280x720_equals_the_reference_grid(ctx):
    vid = synth_video(8, 1280, 720, seed=31)[:, None]
    ref = mog.MogLabeler(ctx, 1280, 720)
    mb = mog.MogLabeler(ctx, 1280, 720, grid="macroblock")
    assert (mb.work_w, mb.work_h, mb.label_h, mb.label_w) == (640, 360, 45, 80)
    lab_r, lab_m = ref.apply(vid), mb.apply(vid)
    assert lab_r.any() and (lab_m == lab_r).all()
    for a, b in zip(ref.debug_masks(), mb.debug_masks()):
        assert (a == b).all()
    _same_model(mb.state(0), ref.state(0))
    ref.close()
    mb.close()


@pytest.mark.parametrize("work", [(960, 540), (320, 180)], ids=["960x540", "320x180"])
def test_post_planted_masks_against_oracle(ctx, work):
    """Hand-made masks reach the post kernel exactly: frame 1 = background, frame 2 differs only where the mask is set, and
    every source pixel is repeated 2x2 so that the half-resolution image is the planted one."""
    ww, wh = work
    cases = G.planted_cases(wh, ww)
    names = sorted(cases)
    vid = G.plant([cases[n] for n in names], 2)
    m = mog.MogLabeler(ctx, 2 * ww, 2 * wh, streams=len(names), grid="macroblock")
    labels = m.apply(vid)
    raw, filled = m.debug_masks()
    for s, nm in enumerate(names):
        assert (raw[1, s] == np.where(cases[nm], 255, 0)).all(), nm
        f_r, l_r = R.post(raw[1, s])
        assert (filled[1, s] == f_r).all(), nm
        assert (labels[1, s] == l_r).all(), nm
    s = names.index("corner_blob")
    assert labels[1, s, -1, -1] == 1 and labels[1, s, -1].sum() > 1 and labels[1, s, :, -1].sum() > 1
    m.close()


# ------------------------------------------------------------------------------------------------ streams, chunks, reset
SW, SH, SN = 640, 360, 40                         # the 320x180 grid


@functools.lru_cache(maxsize=None)
def _clip(seed):
    v = synth_video(SN, SW, SH, seed=seed)
    v.setflags(write=False)
    return v


def _alone(ctx, vid, w=SW, h=SH):
    m = mog.MogLabeler(ctx, w, h, grid="macroblock")
    lab = m.apply(vid[:, None])[:, 0]
    st = m.state(0)
    m.close()
    return lab, st


def test_chunk_invariance(ctx):
    vid = _clip(21)
    outs = []
    for chunk in (1, 7, 64):
        m = mog.MogLabeler(ctx, SW, SH, grid="macroblock")
        parts = [m.apply(vid[i:i + chunk, None]) for i in range(0, SN, chunk)]
        outs.append((np.concatenate(parts), m.state(0)))
        m.close()
    assert outs[0][0].shape == (SN, 1, 23, 40) and outs[0][0][1:].any()
    for lab, st in outs[1:]:
        assert (lab == outs[0][0]).all()
        _same_model(st, outs[0][1])
        assert st["n"] == SN


def test_streams_are_independent_ragged_and_reset(ctx):
    vids = [_clip(100 + s) for s in range(5)]
    alone = [_alone(ctx, v) for v in vids]
    m = mog.MogLabeler(ctx, SW, SH, streams=5, grid="macroblock")
    lab = m.apply(np.stack(vids, 1))
    for s in range(5):
        assert (lab[:, s] == alone[s][0]).all(), s
        _same_model(m.state(s), alone[s][1], s)
    m.close()
    # ragged ends: frames past n_valid are ignored and their labels untouched
    nv = np.array([SN, 12, 0, SN - 1, 1], np.int32)
    m = mog.MogLabeler(ctx, SW, SH, streams=5, grid="macroblock")
    pre = np.full((SN, 5, 23, 40), 77, np.uint8)
    lab = m.apply(np.stack(vids, 1), n_valid=nv, labels=pre)
    for s in range(5):
        k = int(nv[s])
        assert (lab[:k, s] == alone[s][0][:k]).all(), s
        assert (lab[k:, s] == 77).all(), s
        assert m.state(s)["n"] == k
    _same_model(m.state(0), alone[0][1])
    # reset + a new video in slot 2 equals a fresh labeller on that video
    m.reset(2)
    assert m.state(2)["n"] == 0 and not m.state(2)["nmodes"].any()
    new = _clip(999)
    batch = np.zeros((SN, 5, SH, SW, 3), np.uint8)
    batch[:, 2] = new
    lab2 = m.apply(batch, n_valid=np.array([0, 0, SN, 0, 0], np.int32))
    ref_lab, ref_st = _alone(ctx, new)
    assert (lab2[:, 2] == ref_lab).all()
    _same_model(m.state(2), ref_st)
    m.close()


# ------------------------------------------------------------------------------------------------ 1080p call paths
@functools.lru_cache(maxsize=None)
def _clip_1080(n, S, seed):
    v = np.stack([synth_video(n, 1920, 1080, seed=seed + s) for s in range(S)], 1)
    v.setflags(write=False)
    return v


def test_device_pointers_match_host(ctx):
    n, S = 4, 2
    vid = _clip_1080(n, S, 40)
    host = mog.MogLabeler(ctx, 1920, 1080, streams=S, grid="macroblock")
    lab_h = host.apply(vid)
    st_h = [host.state(s) for s in range(S)]
    host.close()
    assert lab_h.shape == (n, S, 68, 120) and lab_h.any()
    dev = mog.MogLabeler(ctx, 1920, 1080, streams=S, grid="macroblock")
    d_f = ctx.malloc(vid.nbytes)
    d_l = ctx.malloc(lab_h.nbytes)
    try:
        ctx.h2d(d_f, vid)
        dev.apply_device(d_f, n, d_l)
        lab_d = np.empty_like(lab_h)
        ctx.d2h(lab_d, d_l)
    finally:
        ctx.free(d_f)
        ctx.free(d_l)
    assert (lab_d == lab_h).all()
    for s in range(S):
        _same_model(dev.state(s), st_h[s], s)
    dev.close()


def test_several_update_launches_equal_one(ctx):
    n, S = 5, 2
    vid = _clip_1080(n, S, 60)
    outs = []
    for budget in (0, 2 * S * 1920 * 1080 * 3):        # the default (one launch), then two frame-steps per launch
        m = mog.MogLabeler(ctx, 1920, 1080, streams=S, grid="macroblock")
        m.set_stage_budget(budget)
        lab = m.apply(vid)
        outs.append((lab, m.debug_masks(), [m.state(s) for s in range(S)]))
        m.close()
    (lab0, masks0, st0), (lab1, masks1, st1) = outs
    assert lab0.any() and (lab1 == lab0).all()
    assert (masks1[0] == masks0[0]).all() and (masks1[1] == masks0[1]).all()
    for s in range(S):
        _same_model(st1[s], st0[s], s)


def test_argument_errors(ctx):
    lib = L.lib()
    cfg = L.MogCfg()
    lib.covahip_mog_default_cfg(C.byref(cfg))
    h = C.c_void_p()
    cfg.src_w, cfg.src_h = 800, 600
    assert lib.covahip_mog_create_grid(ctx.handle, C.byref(cfg), 1, C.byref(h)) == 5 and not h.value
    cfg.src_w, cfg.src_h = 1920, 1080
    assert lib.covahip_mog_create_grid(ctx.handle, C.byref(cfg), 2, C.byref(h)) == 1 and not h.value
    with pytest.raises(L.CovahipError) as e:
        mog.MogLabeler(ctx, 800, 600, grid="macroblock")
    assert e.value.status == 5
    ref = mog.MogLabeler(ctx, 1920, 1080)
    d = [C.c_int32() for _ in range(4)]
    assert lib.covahip_mog_dims(ref.handle, *(C.byref(v) for v in d)) == 0
    assert [v.value for v in d] == [640, 360, 80, 45]
    assert lib.covahip_mog_dims(ref.handle, None, None, None, None) == 0
    assert (ref.work_w, ref.work_h, ref.label_h, ref.label_w) == (640, 360, 45, 80)
    ref.close()
    m = mog.MogLabeler(ctx, 640, 360, streams=2, grid="macroblock")
    assert lib.covahip_mog_dims(m.handle, C.byref(d[0]), None, C.byref(d[2]), None) == 0 and (d[0].value, d[2].value) == (320, 40)
    fr = np.zeros((3, 2, 360, 640, 3), np.uint8)
    with pytest.raises(ValueError):
        m.apply(fr, labels=np.zeros((3, 2, 40, 23), np.uint8))
    with pytest.raises(ValueError):
        m.apply(fr, labels=np.zeros((3, 2, 45, 80), np.uint8))      # the reference shape on a macroblock labeller
    with pytest.raises(ValueError):
        m.apply(np.zeros((3, 2, 180, 320, 3), np.uint8))
    assert m.state(0)["n"] == 0 and m.state(1)["n"] == 0            # nothing was applied by the refused calls
    assert m.apply(fr).shape == (3, 2, 23, 40)
    m.close()


def test_cli_and_training_end_to_end_at_1080p(ctx, tmp_path):
    from cova_amd import elements, train

    lens = (5, 3)
    vids = [synth_video(k, 1920, 1080, seed=70 + i) for i, k in enumerate(lens)]
    args = ["--size", "1920x1080", "--grid", "macroblock", "--streams", "2", "--chunk", "2"]
    for i, v in enumerate(vids):
        p = tmp_path / f"v{i}.bgr"
        p.write_bytes(v.tobytes())
        args.append(str(p))
    assert mog.main(args) == 0
    for i, v in enumerate(vids):
        data = np.fromfile(tmp_path / f"v{i}_gt.dump", np.uint8)
        assert data.size == lens[i] * 68 * 120
        ref, _ = _alone(ctx, v, 1920, 1080)
        assert (data.reshape(-1, 68, 120) == ref).all(), i
    # the labels through tfrecordsink's record form, the TFRecord reader, slide and one training step at the 1080p geometry
    gt = np.fromfile(tmp_path / "v0_gt.dump", np.uint8).reshape(-1, 68, 120)
    rng = np.random.default_rng(3)
    meta = rng.integers(0, 7, (gt.shape[0], 68, 120, 4), dtype=np.uint8)
    meta[..., 3] = 0
    rec = tmp_path / "v0.tfrecord"
    with open(rec, "wb") as f:
        for i in range(gt.shape[0]):
            f.write(elements.tfrecord_example(meta[i:i + 1], gt[i:i + 1]))
    frames, gt_back = train.read_tfrecords(str(rec), 68, 120)
    assert (gt_back == gt).all() and (frames == meta).all()
    stacks, labels = train.slide(frames, gt_back)
    assert stacks.shape[0] == 1 and (labels == gt[3::4][:1]).all()
    tr = train.Trainer(ctx, 68, 120, max_batch=1, seed=0)
    loss = tr.step(stacks, labels)
    assert np.isfinite(loss)
    tr.close()
