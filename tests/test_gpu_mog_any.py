"""MoG labels at any even source size (cova_amd.mog any_size=True / covahip_mog_create_any: the general kernels of
cova_amd/csrc/mog_update.hip and mog_post.hip, geometry as kernel arguments) against the numpy oracle
(tests/mog_grid_ref.py over tests/mog_ref.py, tests/mog_yuv_ref.py), bit for bit: raw masks, filled masks, labels and every word of the model, at working sizes whose rows end
inside a plane word, whose sizes are odd and whose pixel count is no multiple of the update block; planted masks at the right
edge; the general kernels against the table's at sizes both take; decoder surfaces; streams and chunks; the command line and
a training step at a 17x24 grid.  Every comparison with the oracle first checks on the oracle alone that the clip has a frame
behind the first whose labels hold both values and whose filled mask differs from its raw mask."""
import functools

import numpy as np
import pytest

from cova_amd import mog
from tests import mog_band_ref as B
from tests import mog_grid_ref as G
from tests import mog_ref as R
from tests import mog_yuv_ref as Y
from tests.test_gpu_mog import synth_video
from tests.test_gpu_mog_grid import _same_model, _state_equal

pytestmark = pytest.mark.gpu

HIST = 16
# source sizes: work 191x129 (63 bits in the last word, odd sizes, 191 * 129 and 192 * 129 no multiples of 256), 129x128 (one bit),
# 132x136 (4 bits), 192x129 (whole words, a partial last block), 330x190, and a real camera's 640x480
SIZES = [(382, 258), (258, 256), (264, 272), (384, 258), (660, 380), (1280, 960)]
# (source size, frames) at the top of the admitted range: work 2048x128 (32 full words), 128x2048 (the maximal height),
# 2047x129 (63 live bits behind 31 full words, odd sizes), and the two cameras the README names: 2592x1944 (work 1296x972, three
# automatic bands) and 704x576 (work 352x288).  Short clips: the block moves from frame 1 on.  (tests/test_gpu_mog_any_range.py
# has the one run at 4096x4096.)
RANGE_SIZES = [((4096, 256), 4), ((256, 4096), 4), ((4094, 258), 4), ((2592, 1944), 3), ((704, 576), 4)]


def any_clip(n, w, h, seed, start=4):
    """synth_video with a 255 block of 80 x 100 source pixels that moves from frame `start` on."""
    vid = synth_video(n, w, h, seed).copy()
    for t in range(start, n):
        x0, y0 = (40 + 24 * (t - start)) % (w - 80), h // 2 - 50
        vid[t, y0:y0 + 100, x0:x0 + 80] = 255
    return vid


def _oracle_is_a_test(raw, fill, lab):
    """Some frame behind the first has labels of both values and a filled mask that differs from its raw mask."""
    assert any(lab[f].any() and not lab[f].all() and (fill[f] != (raw[f] > 0)).any() for f in range(1, len(lab)))


@functools.lru_cache(maxsize=None)
def _ref(w, h, n, seed, start=4):
    """A clip and the CPU labeller's (raw, filled, labels, model) of it."""
    vid = any_clip(n, w, h, seed, start)
    vid.setflags(write=False)
    ref = G.label_video_grid(vid, history=HIST)
    _oracle_is_a_test(*ref[:3])
    return vid, ref


def _labeler(ctx, w, h, streams=1, **kw):
    m = mog.MogLabeler(ctx, w, h, streams=streams, history=HIST, grid="macroblock", any_size=True, **kw)
    assert (m.work_w, m.work_h) == (w // 2, h // 2) and (m.label_h, m.label_w) == (-(-h // 16), -(-w // 16))
    return m


def _check_call(m, labels, ref, s=0, what=""):
    """labels [F][S][..] and the masks of that call against the oracle's (raw, filled, labels, ..) for stream s."""
    raw_r, fill_r, lab_r = ref[:3]
    raw, filled = m.debug_masks()
    assert raw.shape[2:] == raw_r.shape[1:] and labels.shape[2:] == lab_r.shape[1:], what
    for i in range(len(lab_r)):
        assert (raw[i, s] == raw_r[i]).all(), (what, "raw mask", i)
        assert (filled[i, s] == fill_r[i]).all(), (what, "filled mask", i, int((filled[i, s] != fill_r[i]).sum()))
        assert (labels[i, s] == lab_r[i]).all(), (what, "labels", i)


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("size,n", [(s, 6) for s in SIZES] + RANGE_SIZES,
                         ids=[f"{s[0]}x{s[1]}" for s in SIZES + [r[0] for r in RANGE_SIZES]])
def test_bit_exact_against_oracle(ctx, size, n):
    w, h = size
    vid, ref = _ref(w, h, n, w + h, 4 if n == 6 else 1)
    m = _labeler(ctx, w, h)
    assert m.general
    labels = m.apply(vid[:, None])
    assert labels.shape == (n, 1, -(-h // 16), -(-w // 16))        # the last row / column reads a started 8x8 block
    _check_call(m, labels, ref)
    _state_equal(m.state(0), ref[3])
    m.close()


# ------------------------------------------------------------------------------------------------ 2. planted masks
PW, PH = 330, 190                                  # working size of a 660x380 source: 10 bits in a row's last word


def _right_edge_case():
    """tests/mog_band_ref.right_edge at this working size: the thin strip at the right edge and the slab with the three cavities
    (open to column mw - 1, behind a wall of 4 columns, behind a wall of 5)."""
    return B.right_edge(PH, PW)


@functools.lru_cache(maxsize=None)
def _planted():
    cases = dict(G.planted_cases(PH, PW))
    cases["right_edge"] = _right_edge_case()
    names = sorted(cases)
    post = {n: R.post(np.where(cases[n], 255, 0).astype(np.uint8)) for n in names}
    f = post["right_edge"][0]
    assert not f[5, PW - 8:].any()                                 # the thin strip is gone
    assert not f[45, PW - 30] and not f[90, PW - 30] and f[135, PW - 30] == 1      # open, opened by the morphology, filled
    assert post["sealed_spiral"][0].sum() > cases["sealed_spiral"].sum()          # a fill happened
    return names, cases, post, G.plant([cases[n] for n in names], 2)


@pytest.mark.parametrize("rows", [0, 16], ids=["auto", "rows16"])
def test_planted_masks_against_oracle(ctx, rows):
    """The six planted cases of the macroblock grid and the right-edge case, through the update kernel (frame 2's raw mask is
    the planted one) at the automatic band plan (one band) and in twelve bands of 16 rows."""
    names, cases, post, vid = _planted()
    m = _labeler(ctx, 2 * PW, 2 * PH, streams=len(names))
    m.set_post_form(True, rows)
    labels = m.apply(vid)
    raw, filled = m.debug_masks()
    for s, nm in enumerate(names):
        assert (raw[1, s] == np.where(cases[nm], 255, 0)).all(), nm
        assert (filled[1, s] == post[nm][0]).all(), (nm, int((filled[1, s] != post[nm][0]).sum()))
        assert (labels[1, s] == post[nm][1]).all(), nm
    s = names.index("corner_blob")
    assert labels[1, s, -1, -1] == 1 and labels[1, s, -1].sum() > 1 and labels[1, s, :, -1].sum() > 1
    # the same planes through the developer entry, in bands that do not divide the height
    m.set_post_form(True, 37)
    lab_p = m.post_masks(raw[1:2])
    assert (lab_p[0] == labels[1]).all() and (m.debug_masks()[1][0] == filled[1]).all()
    m.close()


# ------------------------------------------------------------------------------------------------ 3. general == table
RESIDENT, BANDED = ("mog_update", "mog_post"), ("mog_band_update", "mog_band_post")    # the table's profile scopes at a size


@pytest.mark.parametrize("size,n,scopes", [((640, 360), 6, RESIDENT), ((1920, 1080), 2, RESIDENT), ((2560, 1440), 2, BANDED),
                                           ((3840, 2160), 2, BANDED)],
                         ids=["640x360", "1920x1080", "2560x1440", "3840x2160"])
def test_general_kernels_equal_the_tables(ctx, size, n, scopes):
    """The general kernels against the table's on the same frames.  2560x1440 is the smallest table size that runs the templated
    banded kernels (1280x720 working, two bands of 360 by the automatic plan): there the compile-time and the runtime model of
    the one banded driver are held against each other across a seam; 3840x2160 (1920x1080 working) does so at 30 words per row
    and the automatic four bands, where tests/test_gpu_mog_band.py holds the table's side to the oracle."""
    w, h = size
    vid = any_clip(n, w, h, seed=7)[:, None]
    table = mog.MogLabeler(ctx, w, h, history=HIST, grid="macroblock")
    same = mog.MogLabeler(ctx, w, h, history=HIST, grid="macroblock", any_size=True)       # a table size keeps the table's kernels
    gen = mog.MogLabeler(ctx, w, h, history=HIST, grid="macroblock", force_general=True)
    assert not same.general and gen.general
    ctx.profile(True)
    try:
        lab_s = same.apply(vid)
        prof_s = ctx.profile_read()
        lab_g = gen.apply(vid)
        prof_g = ctx.profile_read()
    finally:
        ctx.profile(False)
    assert {k: v[1] for k, v in prof_s.items()} == dict.fromkeys(scopes, 1)
    assert {k: v[1] for k, v in prof_g.items()} == dict.fromkeys(scopes + ("mog_any_update", "mog_any_post"), 1)
    lab_t = table.apply(vid)
    assert lab_t[1:].any() and not lab_t[1:].all()
    assert (lab_g == lab_t).all() and (lab_s == lab_t).all()
    for a, b in zip(gen.debug_masks(), table.debug_masks()):
        assert (a == b).all()
    _same_model(gen.state(0), table.state(0))
    for m in (table, same, gen):
        m.close()


# ------------------------------------------------------------------------------------------------ 4. decoder surfaces
YUV_N = 5


@functools.lru_cache(maxsize=None)
def _yuv_ref(w, h, rng):
    """(y, u, v) [n][1][..] of a clip, its conversion bgr [n][h][w][3] and the CPU labeller's result on that."""
    y, u, v = Y.bgr_to_yuv420(any_clip(YUV_N, w, h, seed=w)[:, None], rng)
    bgr = Y.yuv_to_bgr(y, u, v, rng)[:, 0]
    ref = G.label_video_grid(bgr, history=HIST)
    _oracle_is_a_test(*ref[:3])
    for a in (y, u, v, bgr):
        a.setflags(write=False)
    return (y, u, v), bgr, ref


def _pack_ff(planes, lay):
    """The planes at layout `lay` with every byte that is no sample 0xFF (a sample differs from its complement; the other
    bytes are the same seeded random bytes in both packings)."""
    a = Y.pack(*planes, lay, seed=3)
    b = Y.pack(*(255 - p for p in planes), lay, seed=3)
    return np.where(a != b, a, np.uint8(255))


@pytest.mark.parametrize("rng", ["limited", "full"])
@pytest.mark.parametrize("fmt", ["nv12", "i420"])
@pytest.mark.parametrize("size", [(382, 258), (1280, 960)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_decoder_surfaces_against_oracle(ctx, size, fmt, rng):
    """Tight frames, then the same picture in a pitched surface with coded rows behind it (1280x960 in 968 rows), whose padding
    is 0xFF: the oracle's result both times."""
    w, h = size
    planes, _, ref = _yuv_ref(w, h, rng)
    for make in (Y.tight, Y.padded):
        lay = make(w, h, fmt, rng)
        buf = Y.pack(*planes, lay) if make is Y.tight else _pack_ff(planes, lay)
        m = _labeler(ctx, w, h)
        labels = m.apply_yuv(buf, lay.ctypes(), YUV_N)
        _check_call(m, labels, ref, what=make.__name__)
        _state_equal(m.state(0), ref[3])
        m.close()
    m = _labeler(ctx, w, h)
    lay = m._lib.covahip_mog_yuv_tight                              # the library's tight layout is the Python one
    got = mog.L.MogYuv()
    assert lay(m.handle, mog.FORMATS[fmt], mog.RANGES[rng], got) == 0
    want = mog.yuv_tight(w, h, fmt, rng)
    assert bytes(got) == bytes(want)
    m.close()


def test_both_entries_advance_one_model(ctx):
    w, h = 382, 258
    planes, bgr, ref = _yuv_ref(w, h, "limited")
    lay = Y.tight(w, h, "nv12")
    buf = Y.pack(*planes, lay)
    fb = w * h * 3 // 2
    # apply on the converted frames is apply_yuv
    a = _labeler(ctx, w, h)
    lab_a = a.apply(bgr[:, None])
    _check_call(a, lab_a, ref)
    _state_equal(a.state(0), ref[3])
    # three frames through one entry, two through the other
    b = _labeler(ctx, w, h)
    lab_b = np.concatenate([b.apply_yuv(buf[:3 * fb], lay.ctypes(), 3), b.apply(bgr[3:, None])])
    assert (lab_b == lab_a).all()
    _same_model(b.state(0), a.state(0))
    c = _labeler(ctx, w, h)
    lab_c = np.concatenate([c.apply(bgr[:2, None]), c.apply_yuv(buf[2 * fb:], lay.ctypes(), 3)])
    assert (lab_c == lab_a).all()
    _same_model(c.state(0), a.state(0))
    for m in (a, b, c):
        m.close()


def test_odd_layouts_only_where_samples_are_loaded_singly(ctx):
    """A tight I420 frame of 382x258 has U and V rows of 191 bytes: odd chroma pitches and offsets are taken (the surfaces test
    runs them); the Y plane of either format and NV12's UV pairs, which are loaded as 16-bit words, stay refused."""
    from cova_amd import _lib as L

    w, h = 382, 258
    m = _labeler(ctx, w, h)
    assert mog.yuv_tight(w, h, "i420").pitch[1] == 191
    buf = np.zeros(4 * w * h, np.uint8)
    for fmt, field, i in (("nv12", "pitch", 1), ("nv12", "offset", 1), ("nv12", "pitch", 0), ("i420", "pitch", 0), ("i420", "offset", 0)):
        lay = mog.yuv_tight(w, h, fmt)
        getattr(lay, field)[i] += 1
        with pytest.raises(L.CovahipError) as e:
            m.apply_yuv(buf, lay, 1)
        assert e.value.status == 1, (fmt, field, i)
    assert m.state(0)["n"] == 0 and not m.state(0)["nmodes"].any()
    m.close()


# ------------------------------------------------------------------------------------------------ 5. streams and chunks
SW, SH, SN = 382, 258, 7


def test_three_streams_ragged_with_a_reset_in_the_middle(ctx):
    vids = [_ref(SW, SH, SN, 500 + s)[0] for s in range(3)]
    lh, lw = mog.label_dims_any(SW, SH)
    m = _labeler(ctx, SW, SH, streams=3)
    # call 1: frames 0 .. 3, of which the streams take 4, 2 and 3
    nv = np.array([4, 2, 3], np.int32)
    lab1 = m.apply(np.stack([v[:4] for v in vids], 1), n_valid=nv, labels=np.full((4, 3, lh, lw), 77, np.uint8))
    # stream 1 starts its video over; streams 0 and 2 go on where they were
    m.reset(1)
    assert m.state(1)["n"] == 0 and not m.state(1)["nmodes"].any()
    batch = np.zeros((3, 3, SH, SW, 3), np.uint8)
    batch[:, 0], batch[:, 1], batch[:2, 2] = vids[0][4:7], vids[1][:3], vids[2][3:5]
    nv2 = np.array([3, 3, 2], np.int32)
    lab2 = m.apply(batch, n_valid=nv2, labels=np.full((3, 3, lh, lw), 77, np.uint8))
    want = [G.label_video_grid(vids[0][:7], history=HIST), G.label_video_grid(vids[1][:3], history=HIST),
            G.label_video_grid(vids[2][:5], history=HIST)]
    first = G.label_video_grid(vids[1][:2], history=HIST)
    assert (lab1[:4, 0] == want[0][2][:4]).all() and (lab2[:, 0] == want[0][2][4:]).all()
    assert (lab1[:2, 1] == first[2]).all() and (lab1[2:, 1] == 77).all() and (lab2[:, 1] == want[1][2]).all()
    assert (lab1[:3, 2] == want[2][2][:3]).all() and (lab1[3:, 2] == 77).all()
    assert (lab2[:2, 2] == want[2][2][3:]).all() and (lab2[2:, 2] == 77).all()
    for s in range(3):
        _state_equal(m.state(s), want[s][3])
    m.close()


def test_chunk_invariance_and_device_pointers(ctx):
    vid, ref = _ref(SW, SH, SN, 500)
    outs = []
    for chunks in ((7,), (3, 4), (1,) * 7):
        m = _labeler(ctx, SW, SH)
        parts, i = [], 0
        for k in chunks:
            parts.append(m.apply(vid[i:i + k, None]))
            i += k
        outs.append((np.concatenate(parts), m.state(0)))
        m.close()
    assert (outs[0][0][:, 0] == ref[2]).all()
    _state_equal(outs[0][1], ref[3])
    for lab, st in outs[1:]:
        assert (lab == outs[0][0]).all()
        _same_model(st, outs[0][1])
    dev = _labeler(ctx, SW, SH)
    frames = np.ascontiguousarray(vid[:, None])
    lab_d = np.empty_like(outs[0][0])
    d_f, d_l = ctx.malloc(frames.nbytes), ctx.malloc(lab_d.nbytes)
    try:
        ctx.h2d(d_f, frames)
        dev.apply_device(d_f, SN, d_l)
        ctx.d2h(lab_d, d_l)
    finally:
        ctx.free(d_f)
        ctx.free(d_l)
    assert (lab_d == outs[0][0]).all()
    _same_model(dev.state(0), outs[0][1])
    dev.close()


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_cli_any_size_and_training_at_17x24(ctx, tmp_path):
    from cova_amd import elements, train

    w, h, n = 382, 258, 6
    vid, ref = _ref(w, h, n, w + h)
    p = tmp_path / "v.bgr"
    p.write_bytes(vid.tobytes())
    assert mog.main(["--any-size", f"{w}x{h}", "--history", str(HIST), "--chunk", "4", str(p)]) == 0
    gt = np.fromfile(tmp_path / "v_gt.dump", np.uint8)
    assert gt.size == n * 17 * 24
    gt = gt.reshape(n, 17, 24)
    assert (gt == ref[2]).all()
    # the same size through a YUV4MPEG2 stream: the oracle on the converted frames
    planes, _, yref = _yuv_ref(w, h, "limited")
    data = b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420mpeg2 XCOLORRANGE=LIMITED\n" % (w, h)
    for f in range(YUV_N):
        data += b"FRAME\n" + b"".join(pl[f, 0].tobytes() for pl in planes)
    (tmp_path / "y.y4m").write_bytes(data)
    assert mog.main(["--any-size", f"{w}x{h}", "--format", "y4m", "--history", str(HIST), str(tmp_path / "y.y4m")]) == 0
    assert (np.fromfile(tmp_path / "y_gt.dump", np.uint8).reshape(YUV_N, 17, 24) == yref[2]).all()
    # the labels through tfrecordsink's record form, the TFRecord reader, slide and two training steps at the 17x24 grid
    rng = np.random.default_rng(3)
    meta = rng.integers(0, 7, (n, 17, 24, 4), dtype=np.uint8)
    meta[..., 3] = 0
    rec = tmp_path / "v.tfrecord"
    with open(rec, "wb") as f:
        for i in range(n):
            f.write(elements.tfrecord_example(meta[i:i + 1], gt[i:i + 1]))
    frames, gt_back = train.read_tfrecords(str(rec), 17, 24)
    assert (gt_back == gt).all() and (frames == meta).all()
    stacks, labels = train.slide(frames, gt_back)
    assert stacks.shape[0] >= 1 and labels.shape[1:] == (17, 24) and labels.any() and not labels.all()
    tr = train.Trainer(ctx, 17, 24, max_batch=stacks.shape[0], seed=0)
    for _ in range(2):
        assert np.isfinite(tr.step(stacks, labels))
    tr.close()
