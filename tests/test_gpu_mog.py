"""MoG labels on the GPU (cova_amd.mog / covahip_mog_*) against the numpy oracle (tests/mog_ref.py), bit for bit: the raw MOG2
mask, the filled mask, the labels and the model state.  The videos are seeded synthetic clips: a textured background with
per-pixel noise and coloured ellipses that enter, stop and leave."""
import ctypes as C

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import mog
from tests import mog_ref as R

pytestmark = pytest.mark.gpu


def synth_video(n, w, h, seed):
    """u8 [n][h][w][3] BGR."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w].astype(np.float32)
    s = w / 640.0
    base = np.stack([40 + 150 * xx / w, 30 + 170 * yy / h, 90 + 60 * np.sin(xx / (23 * s)) * np.cos(yy / (17 * s))], -1)
    tex = rng.normal(0, 14, (h // 16 + 1, w // 16 + 1, 3))
    base = base + np.kron(tex, np.ones((16, 16, 1)))[:h, :w]
    objs = []
    for _ in range(4):
        t0 = int(rng.integers(0, max(1, n // 3)))
        objs.append(dict(t0=t0, stop=t0 + int(rng.integers(3, 12)), go=t0 + int(rng.integers(14, 30)),
                         y=float(rng.uniform(0.2, 0.8) * h), v=float(rng.uniform(12, 30) * s), ax=float(rng.uniform(20, 60) * s),
                         ay=float(rng.uniform(12, 40) * s), col=rng.uniform(0, 255, 3)))
    out = np.empty((n, h, w, 3), np.uint8)
    for t in range(n):
        f = base + rng.normal(0, 2.5, base.shape)
        for o in objs:
            if t < o["t0"]:
                continue
            moving = min(t, o["stop"]) - o["t0"] + max(0, t - o["go"])
            cx = -o["ax"] + o["v"] * moving
            x0, x1 = int(max(0, cx - o["ax"])), int(min(w, cx + o["ax"] + 1))
            y0, y1 = int(max(0, o["y"] - o["ay"])), int(min(h, o["y"] + o["ay"] + 1))
            if x0 >= x1 or y0 >= y1:
                continue
            inside = ((xx[y0:y1, x0:x1] - cx) / o["ax"]) ** 2 + ((yy[y0:y1, x0:x1] - o["y"]) / o["ay"]) ** 2 <= 1
            f[y0:y1, x0:x1][inside] = o["col"] + rng.normal(0, 2.0, (int(inside.sum()), 3))
        out[t] = np.clip(f, 0, 255).astype(np.uint8)
    return out


def _state_equal(got, mdl):
    P = R.WORK_W * R.WORK_H
    assert got["n"] == mdl.n
    assert (got["nmodes"].reshape(P) == mdl.nmodes).all(), "nmodes"
    for k in ("W", "V"):
        assert (got[k].reshape(5, P).view(np.uint32) == getattr(mdl, k).view(np.uint32)).all(), k
    assert (got["M"].reshape(5, 3, P).view(np.uint32) == mdl.M.view(np.uint32)).all(), "M"


@pytest.mark.parametrize("size,history,n", [((640, 360), 9000, 200), ((640, 360), 16, 48), ((1280, 720), 9000, 24),
                                            ((1920, 1080), 9000, 20)])
def test_bit_exact_against_oracle(ctx, size, history, n):
    w, h = size
    vid = synth_video(n, w, h, seed=w + history)
    raw_r, fill_r, lab_r, mdl = R.label_video(vid, history=history)
    lab_r_any = lab_r.any()
    m = mog.MogLabeler(ctx, w, h, streams=1, history=history)
    labels = m.apply(vid[:, None])
    raw, filled = m.debug_masks()
    for i in range(n):
        assert (raw[i, 0] == raw_r[i]).all(), f"raw mask, frame {i}"
        assert (filled[i, 0] == fill_r[i]).all(), f"filled mask, frame {i}"
    assert (labels[:, 0] == lab_r).all()
    assert lab_r_any and (raw_r[1:] == 0).any() and (raw_r[1:] == 255).any()       # the clip exercises both classes
    _state_equal(m.state(0), mdl)
    m.close()


def test_post_worst_cases_against_oracle(ctx):
    """Hand-made masks reach the post kernel exactly: frame 1 = background, frame 2 differs only where the mask is set."""
    from tests.test_mog_host import HAND, _spiral
    cases = dict(HAND)
    sealed = _spiral()
    sealed[8:16, 8:632] = sealed[344:352, 8:632] = True
    sealed[8:352, 8:16] = sealed[8:352, 624:632] = True
    cases["sealed_spiral"] = sealed
    names = sorted(cases)
    S = len(names)
    rng = np.random.default_rng(5)
    bg = rng.integers(0, 100, (360, 640, 3), dtype=np.uint8)
    vid = np.empty((2, S, 360, 640, 3), np.uint8)
    for s, nm in enumerate(names):
        vid[0, s] = bg
        vid[1, s] = np.where(cases[nm][..., None], 255 - bg, bg)
    m = mog.MogLabeler(ctx, 640, 360, streams=S)
    labels = m.apply(vid)
    raw, filled = m.debug_masks()
    for s, nm in enumerate(names):
        assert (raw[1, s] == np.where(cases[nm], 255, 0)).all(), nm
        f_r, l_r = R.post(raw[1, s])
        assert (filled[1, s] == f_r).all(), nm
        assert (labels[1, s] == l_r).all(), nm
    m.close()


def test_chunk_invariance(ctx):
    vid = synth_video(80, 640, 360, seed=21)
    outs = []
    for chunk in (1, 7, 64):
        m = mog.MogLabeler(ctx, 640, 360)
        parts = [m.apply(vid[i:i + chunk, None]) for i in range(0, 80, chunk)]
        outs.append((np.concatenate(parts), m.state(0)))
        m.close()
    for lab, st in outs[1:]:
        assert (lab == outs[0][0]).all()
        for k in ("W", "V", "M", "nmodes"):
            assert (st[k].view(np.uint8) == outs[0][1][k].view(np.uint8)).all(), k
        assert st["n"] == 80


def _alone(ctx, vid, w=640, h=360):
    m = mog.MogLabeler(ctx, w, h)
    lab = m.apply(vid[:, None])[:, 0]
    st = m.state(0)
    m.close()
    return lab, st


def test_streams_are_independent_and_ragged(ctx):
    n = 30
    vids = [synth_video(n, 640, 360, seed=100 + s) for s in range(5)]
    alone = [_alone(ctx, v) for v in vids]
    m = mog.MogLabeler(ctx, 640, 360, streams=5)
    lab = m.apply(np.stack(vids, 1))
    for s in range(5):
        assert (lab[:, s] == alone[s][0]).all(), s
        st = m.state(s)
        for k in ("W", "V", "M", "nmodes"):
            assert (st[k].view(np.uint8) == alone[s][1][k].view(np.uint8)).all(), (s, k)
    m.close()
    # ragged ends: frames past n_valid are ignored and their labels untouched
    nv = np.array([30, 12, 0, 29, 1], np.int32)
    m = mog.MogLabeler(ctx, 640, 360, streams=5)
    pre = np.full((n, 5, 45, 80), 77, np.uint8)
    lab = m.apply(np.stack(vids, 1), n_valid=nv, labels=pre)
    for s in range(5):
        k = int(nv[s])
        assert (lab[:k, s] == alone[s][0][:k]).all(), s
        assert (lab[k:, s] == 77).all(), s
        assert m.state(s)["n"] == k
    assert (m.state(0)["W"].view(np.uint8) == alone[0][1]["W"].view(np.uint8)).all()
    # reset + a new video in slot 2 equals a fresh labeller on that video
    m.reset(2)
    assert m.state(2)["n"] == 0 and not m.state(2)["nmodes"].any()
    nv2 = np.array([0, 0, 30, 0, 0], np.int32)
    new = synth_video(n, 640, 360, seed=999)
    batch = np.zeros((n, 5, 360, 640, 3), np.uint8)
    batch[:, 2] = new
    lab2 = m.apply(batch, n_valid=nv2)
    ref_lab, ref_st = _alone(ctx, new)
    assert (lab2[:, 2] == ref_lab).all()
    for k in ("W", "V", "M", "nmodes"):
        assert (m.state(2)[k].view(np.uint8) == ref_st[k].view(np.uint8)).all(), k
    m.close()


def test_device_pointers_match_host(ctx):
    n, S = 10, 2
    vid = np.stack([synth_video(n, 1280, 720, seed=40 + s) for s in range(S)], 1)
    host = mog.MogLabeler(ctx, 1280, 720, streams=S)
    lab_h = host.apply(vid)
    host.close()
    dev = mog.MogLabeler(ctx, 1280, 720, streams=S)
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
    dev.close()


def test_argument_errors(ctx):
    lib = L.lib()
    cfg = L.MogCfg()
    lib.covahip_mog_default_cfg(C.byref(cfg))
    assert (cfg.src_w, cfg.src_h, cfg.n_streams, cfg.history, cfg.var_threshold) == (1280, 720, 1, 9000, 32.0)
    h = C.c_void_p()

    def create(**kw):
        c = L.MogCfg()
        lib.covahip_mog_default_cfg(C.byref(c))
        for k, v in kw.items():
            setattr(c, k, v)
        rc = lib.covahip_mog_create(ctx.handle, C.byref(c), C.byref(h))
        if rc == 0:
            lib.covahip_mog_destroy(h)
        return rc

    assert create(src_w=800, src_h=600) == 5 and not h.value
    assert create(src_w=1280, src_h=360) == 5
    assert create(n_streams=0) == 1 and create(n_streams=100000) == 1
    assert create(history=0) == 1
    assert create(var_threshold=0.0) == 1 and create(var_threshold=float("nan")) == 1
    assert lib.covahip_mog_create(None, C.byref(cfg), C.byref(h)) == 1
    assert lib.covahip_mog_create(ctx.handle, None, C.byref(h)) == 1
    assert lib.covahip_mog_create(ctx.handle, C.byref(cfg), None) == 1
    with pytest.raises(L.CovahipError) as e:
        mog.MogLabeler(ctx, 1024, 768)
    assert e.value.status == 5
    m = mog.MogLabeler(ctx, 640, 360, streams=2)
    fr = np.zeros((3, 2, 360, 640, 3), np.uint8)
    lab = np.zeros((3, 2, 45, 80), np.uint8)
    nv_bad = (C.c_int32 * 2)(4, 1)
    nv_neg = (C.c_int32 * 2)(-1, 1)
    assert lib.covahip_mog_apply(m.handle, fr.ctypes.data, 3, nv_bad, lab.ctypes.data, 0) == 1
    assert lib.covahip_mog_apply(m.handle, fr.ctypes.data, 3, nv_neg, lab.ctypes.data, 0) == 1
    assert lib.covahip_mog_apply(m.handle, None, 3, None, lab.ctypes.data, 0) == 1
    assert lib.covahip_mog_apply(m.handle, fr.ctypes.data, 3, None, None, 0) == 1
    assert lib.covahip_mog_apply(m.handle, fr.ctypes.data, 0, None, lab.ctypes.data, 0) == 1
    assert lib.covahip_mog_apply(m.handle, fr.ctypes.data, 3, None, lab.ctypes.data, 7) == 1
    assert lib.covahip_mog_apply(None, fr.ctypes.data, 3, None, lab.ctypes.data, 0) == 1
    assert lib.covahip_mog_reset(m.handle, 2) == 1 and lib.covahip_mog_reset(m.handle, -1) == 1 and lib.covahip_mog_reset(None, 0) == 1
    # nothing was applied by the failed calls
    assert m.state(0)["n"] == 0 and m.state(1)["n"] == 0
    with pytest.raises(ValueError):
        m.apply(np.zeros((3, 1, 360, 640, 3), np.uint8))
    m.close()


def test_cli_streams_and_training_end_to_end(ctx, tmp_path):
    from cova_amd import elements, train

    lens = (13, 9, 5)
    vids = [synth_video(k, 640, 360, seed=70 + i) for i, k in enumerate(lens)]
    args = ["--size", "640x360", "--streams", "2", "--chunk", "4"]
    for i, v in enumerate(vids):
        p = tmp_path / f"v{i}.bgr"
        p.write_bytes(v.tobytes())
        args.append(str(p))
    assert mog.main(args) == 0
    for i, v in enumerate(vids):
        got = np.fromfile(tmp_path / f"v{i}_gt.dump", np.uint8).reshape(-1, 45, 80)
        ref, _ = _alone(ctx, v)
        assert got.shape[0] == lens[i] and (got == ref).all(), i
    # the labels through tfrecordsink's record form, the TFRecord reader, slide and one training step
    gt = np.fromfile(tmp_path / "v0_gt.dump", np.uint8).reshape(-1, 45, 80)
    rng = np.random.default_rng(3)
    meta = rng.integers(0, 7, (gt.shape[0], 45, 80, 4), dtype=np.uint8)
    meta[..., 3] = 0
    rec = tmp_path / "v0.tfrecord"
    with open(rec, "wb") as f:
        for i in range(gt.shape[0]):
            f.write(elements.tfrecord_example(meta[i:i + 1], gt[i:i + 1]))
    frames, gt_back = train.read_tfrecords(str(rec), 45, 80)
    assert (gt_back == gt).all() and (frames == meta).all()
    stacks, labels = train.slide(frames, gt_back)
    assert stacks.shape[0] == 3 and (labels == gt[3::4][:3]).all()
    tr = train.Trainer(ctx, 45, 80, max_batch=3, seed=0)
    loss = tr.step(stacks, labels)
    assert np.isfinite(loss)
    tr.close()
