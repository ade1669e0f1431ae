"""MoG labels from NV12 / I420 surfaces (cova_amd.mog.apply_yuv / covahip_mog_apply_yuv), bit for bit everywhere: the conversion
against its numpy restatement (tests/mog_yuv_ref.py) through the model's first mode, the YUV entry against the BGR24 entry on the
converted frames, both against the numpy labeller, I420 against NV12, the layouts (pitch, plane offsets, strides, host and device
memory, staged launches), ragged streams with a reset, both entries on one model, and every refusal.  The clips are
tests/test_gpu_mog.synth_video pushed through the approximate forward transform; each one is checked on the CPU to show both mask
classes behind frame 1 and a non-empty label."""
import ctypes as C
import functools

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import mog
from tests import mog_grid_ref as G
from tests import mog_ref as R
from tests import mog_yuv_ref as Y
from tests.test_gpu_mog import synth_video

pytestmark = pytest.mark.gpu

MODEL = ("W", "V", "M", "nmodes")
# source size and grid of the seven working geometries (1280x720 runs the same kernels on either grid)
PAIRS = [(640, 360, "reference"), (1280, 720, "reference"), (1920, 1080, "reference"), (640, 360, "macroblock"),
         (1920, 1080, "macroblock"), (2560, 1440, "macroblock"), (3840, 2160, "macroblock")]
PAIR_IDS = [f"{w}x{h}-{g}" for w, h, g in PAIRS]


def _same_model(a, b, what=""):
    for k in MODEL:
        assert (a[k].view(np.uint8) == b[k].view(np.uint8)).all(), (what, k)
    assert a["n"] == b["n"], what


def _same_call(a, b, streams, what=""):
    """Two labellers after the same calls: masks of the last call and every word of the model."""
    for x, y in zip(a.debug_masks(), b.debug_masks()):
        assert (x == y).all(), what
    for s in range(streams):
        _same_model(a.state(s), b.state(s), (what, s))


def _oracle(bgr, grid, history=9000):
    """raw, filled, labels, model of one video on the CPU."""
    return (R.label_video if grid == "reference" else G.label_video_grid)(bgr, history=history)


@functools.lru_cache(maxsize=None)
def _clip(w, h, n, S, seed, rng="limited", history=9000, grid="reference"):
    """(y, u, v) planes [n][S][..] of S synthetic videos, their conversion bgr [n][S][h][w][3], and the CPU labeller's result
    per stream; every video has both mask classes behind frame 1 and a non-empty label there."""
    vids = np.stack([synth_video(n, w, h, seed=seed + s) for s in range(S)], 1)
    y, u, v = Y.bgr_to_yuv420(vids, rng)
    bgr = Y.yuv_to_bgr(y, u, v, rng)
    refs = []
    for s in range(S):
        raw, fill, lab, mdl = _oracle(bgr[:, s], grid, history)
        assert lab[1:].any() and (raw[1:] == 0).any() and (raw[1:] == 255).any(), (w, h, seed + s)
        refs.append((raw, fill, lab, mdl))
    for a in (y, u, v, bgr):
        a.setflags(write=False)
    return (y, u, v), bgr, refs


def _yuv_labels(ctx, w, h, grid, planes, lay, streams, history=9000, seed=0):
    m = mog.MogLabeler(ctx, w, h, streams=streams, history=history, grid=grid)
    buf = Y.pack(*planes, lay, seed=seed)
    lab = m.apply_yuv(buf, lay.ctypes(), planes[0].shape[0])
    return m, lab


# ------------------------------------------------------------------------------------------------ 1. the conversion itself
CONV = [(w, h, g, "nv12", "limited") for w, h, g in PAIRS] + \
       [(640, 360, "reference", "i420", "limited"), (640, 360, "macroblock", "i420", "limited"),
        (1920, 1080, "reference", "i420", "limited"), (640, 360, "reference", "nv12", "full"),
        (640, 360, "macroblock", "nv12", "full"), (1920, 1080, "reference", "nv12", "full"),
        (640, 360, "reference", "i420", "full"), (640, 360, "macroblock", "i420", "full"), (1920, 1080, "reference", "i420", "full")]


@pytest.mark.parametrize("w,h,grid,fmt,rng", CONV, ids=[f"{w}x{h}-{g}-{f}-{r}" for w, h, g, f, r in CONV])
def test_conversion_through_the_first_mode(ctx, w, h, grid, fmt, rng):
    """After a stream's first frame every pixel has one mode whose mean is the working pixel, so M[0] of the model is the
    working image of the converted frame.  Uniformly random planes reach both clamps of every channel and Y < 16."""
    r = np.random.default_rng(w + len(grid) + len(fmt) + len(rng))
    y = r.integers(0, 256, (1, 1, h, w), dtype=np.uint8)
    u = r.integers(0, 256, (1, 1, h // 2, w // 2), dtype=np.uint8)
    v = r.integers(0, 256, (1, 1, h // 2, w // 2), dtype=np.uint8)
    bgr = Y.yuv_to_bgr(y[0, 0], u[0, 0], v[0, 0], rng)
    assert (y < 16).any()
    for c in range(3):
        assert (bgr[..., c] == 0).any() and (bgr[..., c] == 255).any(), c
    want = Y.work_image(bgr, grid)
    m, _ = _yuv_labels(ctx, w, h, grid, (y, u, v), Y.padded(w, h, fmt, rng), 1, seed=3)
    st = m.state(0)
    m.close()
    assert st["n"] == 1 and (st["nmodes"] == 1).all()
    assert st["M"].shape[1:] == (3,) + want.shape[:2]
    assert (st["M"][0] == want.transpose(2, 0, 1).astype(np.float32)).all()
    assert (st["W"][0] == 1).all() and (st["V"][0] == 15).all() and not st["M"][1:].any()


# ------------------------------------------------------------------------------------------------ 2. YUV path == BGR path
@pytest.mark.parametrize("w,h,grid", PAIRS, ids=PAIR_IDS)
def test_yuv_entry_equals_bgr_entry_on_converted_frames(ctx, w, h, grid):
    small = mog.work_dims(w, h, grid)[0] <= 640
    n, S = (3, 2) if small else (2, 1)
    planes, bgr, _ = _clip(w, h, n, S, seed=w + len(grid), grid=grid)
    a, lab_a = _yuv_labels(ctx, w, h, grid, planes, Y.padded(w, h, "nv12", streams=S, frames=n), S, seed=7)
    b = mog.MogLabeler(ctx, w, h, streams=S, grid=grid)
    lab_b = b.apply(bgr)
    assert lab_b[1:].any() and (lab_a == lab_b).all()
    _same_call(a, b, S)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 3. the numpy labeller
@pytest.mark.parametrize("grid", ["reference", "macroblock"])
def test_against_the_numpy_labeller(ctx, grid):
    w, h, n = 640, 360, 8
    planes, bgr, refs = _clip(w, h, n, 1, seed=77, history=16, grid=grid)
    raw_r, fill_r, lab_r, mdl = refs[0]
    m, lab = _yuv_labels(ctx, w, h, grid, planes, Y.padded(w, h, "nv12"), 1, history=16, seed=2)
    raw, filled = m.debug_masks()
    for i in range(n):
        assert (raw[i, 0] == raw_r[i]).all(), f"raw mask, frame {i}"
        assert (filled[i, 0] == fill_r[i]).all(), f"filled mask, frame {i}"
    assert (lab[:, 0] == lab_r).all()
    got, P = m.state(0), mdl.P
    m.close()
    assert got["n"] == mdl.n and (got["nmodes"].reshape(P) == mdl.nmodes).all()
    for k in ("W", "V"):
        assert (got[k].reshape(5, P).view(np.uint32) == getattr(mdl, k).view(np.uint32)).all(), k
    assert (got["M"].reshape(5, 3, P).view(np.uint32) == mdl.M.view(np.uint32)).all()


# ------------------------------------------------------------------------------------------------ 4. I420 == NV12
@pytest.mark.parametrize("w,h,grid,rng", [(640, 360, "reference", "limited"), (640, 360, "reference", "full"),
                                          (1920, 1080, "macroblock", "limited")])
def test_i420_equals_nv12(ctx, w, h, grid, rng):
    n, S = (3, 2) if w == 640 else (2, 1)
    planes, _, _ = _clip(w, h, n, S, seed=w + len(grid), rng=rng, grid=grid)
    a, lab_a = _yuv_labels(ctx, w, h, grid, planes, Y.padded(w, h, "nv12", rng, streams=S, frames=n), S, seed=1)
    b, lab_b = _yuv_labels(ctx, w, h, grid, planes, Y.padded(w, h, "i420", rng, streams=S, frames=n), S, seed=2)
    assert lab_a[1:].any() and (lab_a == lab_b).all()
    _same_call(a, b, S)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 5. layouts
LW_, LH_, LN, LS = 640, 360, 3, 2


@pytest.fixture(scope="module")
def layout_base(ctx):
    """The frame-major padded NV12 call every layout is held against: labels, masks, models."""
    planes, _, _ = _clip(LW_, LH_, LN, LS, seed=640 + len("reference"))
    m, lab = _yuv_labels(ctx, LW_, LH_, "reference", planes, Y.padded(LW_, LH_, "nv12", streams=LS, frames=LN), LS)
    out = (planes, lab, m.debug_masks(), [m.state(s) for s in range(LS)])
    m.close()
    assert lab[1:].any()
    return out


def _equals_base(m, lab, base):
    _, lab0, masks0, st0 = base
    assert (lab == lab0).all()
    for x, y in zip(m.debug_masks(), masks0):
        assert (x == y).all()
    for s in range(LS):
        _same_model(m.state(s), st0[s], s)


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
@pytest.mark.parametrize("make", [Y.padded, Y.tight], ids=["padded", "tight"])
def test_stream_major_equals_frame_major(ctx, layout_base, fmt, make):
    lay = make(LW_, LH_, fmt, streams=LS, frames=LN, stream_major=True)
    assert lay.stream_stride == LN * lay.frame_stride
    m, lab = _yuv_labels(ctx, LW_, LH_, "reference", layout_base[0], lay, LS, seed=5)
    _equals_base(m, lab, layout_base)
    m.close()


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
@pytest.mark.parametrize("make", [Y.padded, Y.tight], ids=["padded", "tight"])
def test_host_buffer_ends_with_the_last_row(ctx, layout_base, fmt, make):
    """The buffer has not one byte behind the last row of the last plane of the last (frame, stream); the labeller's own helper
    gives the same tight layout and the same span."""
    lay = make(LW_, LH_, fmt, streams=LS, frames=LN)
    buf = Y.pack(*layout_base[0], lay, seed=9)
    m = mog.MogLabeler(ctx, LW_, LH_, streams=LS)
    assert buf.nbytes == m.yuv_span(lay.ctypes(), LN)
    if make is Y.tight:
        mine = mog.yuv_tight(LW_, LH_, fmt, streams=LS)
        assert bytes(mine) == bytes(lay.ctypes()) and buf.nbytes == LN * LS * LW_ * LH_ * 3 // 2
        lib_lay = L.MogYuv()
        assert L.lib().covahip_mog_yuv_tight(m.handle, lay.ctypes().format, 0, C.byref(lib_lay)) == 0
        assert bytes(lib_lay) == bytes(mine)
    lab = m.apply_yuv(buf, lay.ctypes(), LN)
    _equals_base(m, lab, layout_base)
    with pytest.raises(ValueError):
        m.apply_yuv(buf[:-2], lay.ctypes(), LN)         # one sample short: refused before the library sees it
    m.close()


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_device_pointers_equal_host(ctx, layout_base, fmt):
    lay = Y.padded(LW_, LH_, fmt, streams=LS, frames=LN)
    buf = Y.pack(*layout_base[0], lay, seed=11)
    m = mog.MogLabeler(ctx, LW_, LH_, streams=LS)
    lab = np.full_like(layout_base[1], 9)
    d_b, d_l = ctx.malloc(buf.nbytes), ctx.malloc(lab.nbytes)
    try:
        ctx.h2d(d_b, buf)
        m.apply_yuv_device(d_b, lay.ctypes(), LN, d_l)
        ctx.d2h(lab, d_l)
    finally:
        ctx.free(d_b)
        ctx.free(d_l)
    _equals_base(m, lab, layout_base)
    m.close()


@pytest.mark.parametrize("make", [Y.padded, Y.tight], ids=["padded", "tight"])
def test_several_staged_launches_equal_one(ctx, layout_base, make):
    lay = make(LW_, LH_, "nv12", streams=LS, frames=LN)
    buf = Y.pack(*layout_base[0], lay, seed=13)
    m = mog.MogLabeler(ctx, LW_, LH_, streams=LS)
    m.set_stage_budget(lay.frame_stride + 4096)         # a little over one frame of every stream: three launches
    lab = m.apply_yuv(buf, lay.ctypes(), LN)
    _equals_base(m, lab, layout_base)
    m.close()


# ------------------------------------------------------------------------------------------------ 6. ragged streams, reset
def test_ragged_n_valid_with_a_reset_in_the_middle(ctx):
    w, h, grid, n = 640, 360, "macroblock", 4
    planes, _, refs = _clip(w, h, n, 2, seed=300, grid=grid)
    new_planes, _, new_refs = _clip(w, h, n, 1, seed=400, grid=grid)

    def alone(pl, s):
        one = tuple(a[:, s:s + 1] for a in pl)
        m, lab = _yuv_labels(ctx, w, h, grid, one, Y.padded(w, h, "nv12"), 1)
        st = m.state(0)
        m.close()
        return lab[:, 0], st

    alone0, alone1, alone_new = alone(planes, 0), alone(planes, 1), alone(new_planes, 0)
    assert (alone0[0] == refs[0][2]).all() and (alone_new[0] == new_refs[0][2]).all()      # and the CPU labeller agrees
    lay = Y.padded(w, h, "nv12", streams=2, frames=n)
    m = mog.MogLabeler(ctx, w, h, streams=2, grid=grid)
    pre = np.full((n, 2) + mog.label_dims(w, h, grid), 77, np.uint8)
    # stream 0 takes all four frames, stream 1 only two; frames past n_valid are not read (they hold noise here)
    y, u, v = (a.copy() for a in planes)
    y[2:, 1] = 255 - y[2:, 1]
    lab = m.apply_yuv(Y.pack(y, u, v, lay, seed=4), lay.ctypes(), n, n_valid=[n, 2], labels=pre)
    assert (lab[:, 0] == alone0[0]).all() and (lab[:2, 1] == alone1[0][:2]).all() and (lab[2:, 1] == 77).all()
    _same_model(m.state(0), alone0[1])
    assert m.state(1)["n"] == 2
    # slot 1 is reset and takes a new video while slot 0 idles
    m.reset(1)
    assert m.state(1)["n"] == 0 and not m.state(1)["nmodes"].any()
    y2, u2, v2 = (np.concatenate([np.zeros_like(a), a], 1) for a in new_planes)
    lab2 = m.apply_yuv(Y.pack(y2, u2, v2, lay, seed=6), lay.ctypes(), n, n_valid=[0, n])
    assert (lab2[:, 1] == alone_new[0]).all() and not lab2[:, 0].any()
    _same_model(m.state(1), alone_new[1])
    _same_model(m.state(0), alone0[1])
    m.close()


# ------------------------------------------------------------------------------------------------ 7. one model, both entries
@pytest.mark.parametrize("w,h,grid", [(640, 360, "reference"), (640, 360, "macroblock")])
def test_both_entries_advance_one_model(ctx, w, h, grid):
    planes, bgr, _ = _clip(w, h, 4, 1, seed=500, grid=grid)
    whole, lab_w = _yuv_labels(ctx, w, h, grid, planes, Y.padded(w, h, "nv12"), 1)
    mixed, lab_a = _yuv_labels(ctx, w, h, grid, tuple(a[:2] for a in planes), Y.padded(w, h, "i420"), 1, seed=3)
    lab_b = mixed.apply(bgr[2:])
    assert lab_w[1:].any() and (np.concatenate([lab_a, lab_b]) == lab_w).all()
    for x, y in zip(mixed.debug_masks(), whole.debug_masks()):
        assert (x == y[2:]).all()
    _same_model(mixed.state(0), whole.state(0))
    assert mixed.state(0)["n"] == 4
    whole.close()
    mixed.close()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_every_refusal_leaves_the_model_untouched(ctx):
    w, h, S = 640, 360, 2
    planes, _, _ = _clip(LW_, LH_, LN, LS, seed=640 + len("reference"))
    lib = L.lib()
    m = mog.MogLabeler(ctx, w, h, streams=S)
    good = {f: Y.padded(w, h, f, streams=S, frames=LN) for f in ("nv12", "i420")}
    m.apply_yuv(Y.pack(*planes, good["nv12"]), good["nv12"].ctypes(), LN)
    before = [m.state(s) for s in range(S)]
    buf = np.zeros(2 * m.yuv_span(good["i420"].ctypes(), LN) + 64, np.uint8)
    buf = buf[buf.ctypes.data & 1:]                    # an even address, whatever numpy gave
    lab = np.zeros((LN, S, 45, 80), np.uint8)

    def call(fmt="nv12", base=None, n=LN, nv=None, labels=lab.ctypes.data, kind=L.MEM_HOST, lay=None, **change):
        lay = lay if lay is not None else good[fmt].ctypes()
        for k, val in change.items():
            if "[" in k:
                getattr(lay, k[:-3])[int(k[-2])] = val
            else:
                setattr(lay, k, val)
        nv = None if nv is None else np.asarray(nv, np.int32).ctypes.data
        return lib.covahip_mog_apply_yuv(m.handle, C.byref(lay), buf.ctypes.data if base is None else base, n, nv, labels, kind)

    refused = [
        dict(format=0), dict(format=3), dict(range=2), dict(range=-1),
        {"offset[0]": -2}, {"offset[1]": -2}, {"pitch[0]": -w}, dict(frame_stride=-2), dict(stream_stride=-2),
        {"pitch[0]": w - 2}, {"pitch[1]": w - 2}, {"offset[0]": 1}, {"offset[1]": good["nv12"].offset[1] + 1},
        {"pitch[0]": w + 65}, {"pitch[1]": w + 33}, dict(frame_stride=good["nv12"].frame_stride + 1),
        dict(stream_stride=good["nv12"].stream_stride + 1), dict(base=buf.ctypes.data + 1),
        dict(fmt="i420", **{"pitch[1]": w // 2 - 2}), dict(fmt="i420", **{"pitch[2]": w // 2 - 2}),
        dict(fmt="i420", **{"offset[2]": -2}), dict(fmt="i420", **{"offset[2]": good["i420"].offset[2] + 1}),
        dict(fmt="i420", **{"pitch[2]": w // 2 + 49}),
        dict(n=0), dict(n=-1), dict(nv=[LN + 1, 0]), dict(nv=[0, -1]), dict(kind=7), dict(labels=None), dict(base=0),
    ]
    for kw in refused:
        assert call(**kw) == 1, kw
    assert lib.covahip_mog_apply_yuv(m.handle, None, buf.ctypes.data, LN, None, lab.ctypes.data, L.MEM_HOST) == 1
    assert lib.covahip_mog_apply_yuv(None, C.byref(good["nv12"].ctypes()), buf.ctypes.data, LN, None, lab.ctypes.data, L.MEM_HOST) == 1
    out = L.MogYuv()
    for fmt, rng in ((0, 0), (3, 0), (1, 2), (2, -1)):
        assert lib.covahip_mog_yuv_tight(m.handle, fmt, rng, C.byref(out)) == 1
    assert lib.covahip_mog_yuv_tight(m.handle, 1, 0, None) == 1
    # NV12 ignores offset[2] and pitch[2], whatever they hold
    with pytest.raises(L.CovahipError) as e:
        bad = good["nv12"].ctypes()
        bad.pitch[0] = 1
        m.apply_yuv(buf, bad, LN)
    assert e.value.status == 1
    for s in range(S):
        _same_model(m.state(s), before[s], s)
    assert call(**{"offset[2]": -1, "pitch[2]": -1}) == 0
    assert m.state(0)["n"] == 2 * LN
    m.close()


# ------------------------------------------------------------------------------------------------ 9. the command line
def test_cli_y4m_and_raw_nv12_end_to_end(ctx, tmp_path):
    """Two YUV4MPEG2 inputs of different lengths side by side, sized by their headers, and a raw NV12 file with --size: every
    output is what the CPU labeller gives for that video alone."""
    w, h, grid, n = 640, 360, "macroblock", 4
    (y, u, v), _, refs = _clip(w, h, n, 2, seed=300, grid=grid)
    lens = (4, 3)
    args = ["--format", "y4m", "--grid", grid, "--streams", "2", "--chunk", "3"]
    for s, k in enumerate(lens):
        data = b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420mpeg2 XCOLORRANGE=LIMITED\n" % (w, h)
        for f in range(k):
            data += b"FRAME\n" + y[f, s].tobytes() + u[f, s].tobytes() + v[f, s].tobytes()
        (tmp_path / f"v{s}.y4m").write_bytes(data)
        args.append(str(tmp_path / f"v{s}.y4m"))
    assert mog.main(args) == 0
    lh, lw = mog.label_dims(w, h, grid)
    for s, k in enumerate(lens):
        got = np.fromfile(tmp_path / f"v{s}_gt.dump", np.uint8).reshape(-1, lh, lw)
        assert got.shape[0] == k and got[1:].any() and (got == refs[s][2][:k]).all(), s
    raw = tmp_path / "v.nv12"
    with open(raw, "wb") as f:
        for i in range(n):
            f.write(y[i, 1].tobytes() + np.stack([u[i, 1], v[i, 1]], -1).tobytes())
    assert mog.main(["--format", "nv12", "--size", f"{w}x{h}", "--grid", grid, f"{raw}:{tmp_path / 'nv12.dump'}"]) == 0
    assert (np.fromfile(tmp_path / "nv12.dump", np.uint8).reshape(-1, lh, lw) == refs[1][2]).all()
