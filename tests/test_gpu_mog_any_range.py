"""The any-size MoG labeller (covahip_mog_create_any: k_mog_any_post, k_mog_any_update, k_mog_any_yuv_update) over the range it
admits, up to a 4096x4096 source, bit for bit against the numpy oracle: raw masks, filled masks, labels and, wherever MOG2 runs,
every word of the model.  There is no tolerance in this file.  tests/test_mog_any_range_host.py proves on the oracle alone that
the planes used here are live at every shape and that two planted bugs (dead bits read as pixels; bands that exchange nothing)
change their filled masks.  Sizes below are working sizes (w x h); the source is twice that.

  a. the post kernel on planted planes (post_masks, one frame, one stream per plane), at the automatic plan and forced ones:
       2047x641   32 words, 63 live bits in the last; 3 automatic bands of 214; 41 bands of 16; 287 rows, the LDS limit (288 is
                  refused and the labeller stays as it was).  All 512 lanes of the column sweep own a segment.
       2048x272   32 full words; 17 bands of 16, 8 of 37
       1985x137   32 words, 1 live bit in the last; 3 bands of 48
       1984x136   31 full words; 3 bands of 48
       129x2047   3 words, 1 live bit; the maximal height; 4 bands of 512, 128 bands of 16
       1296x972   a 2592x1944 camera: 21 words, 16 live bits; 3 automatic bands of 324
       352x288    a 704x576 camera: 6 words, 32 live bits; 2 bands of 144
     planes: tests/mog_band_ref.py's battery around the seams of the plan under test (corridors, seam morphology, serpentine open
     and closed, coarse spirals, corner blob, random pixels and blocks), right_edge, a full and an empty plane.  Then 2048x2048
     (8 automatic bands of 256, 256x256 = 65,536 labels) on the planes whose oracle is cheap there.
  b. labels by coverage at 2047x641 and 1985x137 (tests/test_gpu_mog_cover.py's planted rectangles and edge blobs; count, cover
     1 / 32 / 64, corner), and the shadow ballots at 1985x137 in DROP and KEEP (tests/mog_shadow_ref.py): raw 0 / 127 / 255, filled,
     labels, the model and shadow_counts, in which the 63 dead lanes of every row must not be.
  c. update plus post end to end: NV12 and I420 surfaces at 4094x1282 source (tight; pitched with coded rows and 0xFF padding;
     full range), two ragged streams from host memory at 4096x256 in one update launch per frame, and one run at 4096x4096
     (424 MB of model).  The BGR24 sizes 4096x256, 256x4096, 4094x258, 2592x1944 and 704x576 are cases of
     tests/test_gpu_mog_any.py::test_bit_exact_against_oracle, and 3840x2160 one of its general-against-table test.
  e. label_dims_any is the labels' shape at every shape here; create_any's refusals are tests/test_mog_any_host.py's.

Wall time per test on an MI355X (pytest --durations, call phase, the oracle's share included; 12.6 s for the file):
  test_full_path_4096x4096 2.25 s; test_post_at_2048x2048 1.74 s (the closed serpentine included: nothing had to be dropped);
  test_decoder_surfaces_at_4094x1282 1.44 s and 1.46 s for the first case of each range (they make the clip and its oracle),
  0.05 - 0.08 s for the others; test_post_on_planted_planes 1.29 s at 2047x641 (four launches of 14 planes), 0.88 s at 1296x972,
  0.64 s at 2048x272, 0.15 s at 129x2047 (the 128-band plan included), 0.15 s, 0.14 s and 0.05 s at the other shapes;
  test_two_ragged_streams_staged_at_4096x256 0.48 s; test_shadow_ballots_at_1985x137 0.47 s and 0.05 s;
  test_cover_labels_at_32_words 0.27 s and 0.05 s.
The cases added to tests/test_gpu_mog_any.py: 0.92 s at 2592x1944, 0.79 s for 3840x2160 general against table, 0.25 s or less each
at 4096x256, 256x4096, 4094x258 and 704x576.
"""
import functools

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import mog
from tests import mog_band_ref as B
from tests import mog_cover_ref as CR
from tests import mog_grid_ref as G
from tests import mog_ref as R
from tests import mog_shadow_ref as SR
from tests import mog_yuv_ref as Y
from tests.test_gpu_mog_any import HIST, _check_call, _labeler, _oracle_is_a_test, _pack_ff, any_clip
from tests.test_gpu_mog_cover import _check_modes, _planted
from tests.test_gpu_mog_grid import _state_equal
from tests.test_gpu_mog_shadow import KW as SHADOW_KW
from tests.test_gpu_mog_shadow import TAU, _counts_of, _model_equal

pytestmark = pytest.mark.gpu


def _post_labeler(ctx, w, h, streams):
    m = _labeler(ctx, 2 * w, 2 * h, streams=streams)
    assert m.general and (m.label_h, m.label_w) == mog.label_dims_any(2 * w, 2 * h) == (-(-h // 8), -(-w // 8))
    return m


def _check_planes(m, names, w, h, band_rows):
    """The named planes of the plan through one post launch against the oracle: raw, filled, labels."""
    rows = B.plan_rows(w, h, band_rows)
    raw_in = np.stack([B.to_u8(B.range_plane(n, w, h, rows)) for n in names])[None]
    labels = m.post_masks(raw_in)
    raw, filled = m.debug_masks()
    assert labels.shape == (1, len(names)) + mog.label_dims_any(2 * w, 2 * h)
    for s, n in enumerate(names):
        f_o, l_o = B.range_oracle(n, w, h, rows)
        what = (f"{w}x{h}", band_rows, n)
        assert (raw[0, s] == raw_in[0, s]).all(), what
        assert (filled[0, s] == f_o).all(), what + ("filled mask", int((filled[0, s] != f_o).sum()))
        assert (labels[0, s] == l_o).all(), what + ("labels",)


# ------------------------------------------------------------------------------------------------ a. the post kernel
@pytest.mark.parametrize("w,h,forced", B.RANGE_SHAPES, ids=[f"{w}x{h}" for w, h, _ in B.RANGE_SHAPES])
def test_post_on_planted_planes(ctx, w, h, forced):
    names = B.range_names(w, h)
    m = _post_labeler(ctx, w, h, len(names))
    for band_rows in (0,) + forced:
        m.set_post_form(True, band_rows)
        _check_planes(m, names, w, h, band_rows)
    if (w, h) == (2047, 641):
        assert forced[-1] == B.band_max_rows(w) == 287
        # one row more does not fit LDS: refused, and the labeller goes on in the plan it had
        assert L.lib().covahip_dev_mog_set_post_form(m.handle, 1, 288) == 1
        _check_planes(m, names, w, h, 287)
    lib = L.lib()
    assert lib.covahip_dev_mog_set_post_form(m.handle, 0, 0) == 1          # no resident form at any size
    assert lib.covahip_dev_mog_set_post_form(m.handle, 1, h + 1) == 1 and lib.covahip_dev_mog_set_post_form(m.handle, 1, 15) == 1
    m.close()


def test_post_at_2048x2048(ctx):
    w, h = B.RANGE_FULL
    assert B.auto_plan(w, h) == (256, 8) and mog.label_dims_any(2 * w, 2 * h) == (256, 256)
    m = _post_labeler(ctx, w, h, len(B.FULL_PLANES))
    _check_planes(m, B.FULL_PLANES, w, h, 0)
    m.close()


# ------------------------------------------------------------------------------------------------ b. coverage, shadows
@pytest.mark.parametrize("w,h", [(2047, 641), (1985, 137)], ids=["2047x641", "1985x137"])
def test_cover_labels_at_32_words(ctx, w, h):
    raw, filled_o = _planted(h, w, 1)
    m = _post_labeler(ctx, w, h, raw.shape[1])
    ins = CR.inside(h, w)
    assert (ins[:-1, -1] == 8 * (w % 8)).all() and (ins[-1, :-1] == 8 * (h % 8)).all()      # a started last column and row
    _check_modes(m, raw, filled_o, f"{w}x{h}")
    m.set_post_form(True, 16)                                # and in bands that cut through the blocks' rows
    m.set_labels("count")
    assert (m.post_masks(raw) == CR.labels(filled_o, "count")).all()
    m.close()


SH_W, SH_H, SH_N = 1985, 137, 6


@functools.lru_cache(maxsize=None)
def _shadow_ref():
    """(source [F][274][3970][3], raw 0 / 127 / 255 [F][137][1985], the model): the first frames of the branch clip, their first 137
    rows tiled to 1985 columns as the working image, every pixel repeated 2x2 as the source (whose 2x2 mean is that image)."""
    _, _, nf, seed = SR.GPU_CLIP
    clip = SR.shadow_clip(nf, seed)[:SH_N, :SH_H]
    work = np.ascontiguousarray(np.tile(clip, (1, 1, 4, 1))[:, :, :SH_W])
    src = np.ascontiguousarray(work.repeat(2, 1).repeat(2, 2))
    mdl = R.Mog2(npix=SH_W * SH_H, **SHADOW_KW)
    raw = np.stack([SR.apply3(mdl, f, TAU) for f in work])
    for a in (src, raw):
        a.setflags(write=False)
    return src, raw, mdl


@pytest.mark.parametrize("mode", ["drop", "keep"])
def test_shadow_ballots_at_1985x137(ctx, mode):
    src, raw_r, mdl = _shadow_ref()
    assert (raw_r == 127).any() and (raw_r == 255).any() and (raw_r[1:] == 0).any()
    assert (raw_r[1:, :, -1] == 127).any() and (raw_r[1:, :, -1] == 255).any()     # both planes have bits in the one live lane
    posts = [R.post(SR.fg_of(r, mode)) for r in raw_r]
    other = [R.post(SR.fg_of(r, "keep" if mode == "drop" else "drop"))[0] for r in raw_r[-1:]]
    assert (other[0] != posts[-1][0]).any()                  # the two modes differ on this clip
    m = mog.MogLabeler(ctx, 2 * SH_W, 2 * SH_H, grid="macroblock", any_size=True, shadows=(mode, TAU), **SHADOW_KW)
    assert m.general and (m.work_w, m.work_h) == (SH_W, SH_H)
    lab = m.apply(src[:, None])[:, 0]
    raw, fil = (a[:, 0] for a in m.debug_masks())
    sh, fg = m.shadow_counts()
    assert set(np.unique(raw)) <= {0, 127, 255}
    for i in range(SH_N):
        assert (raw[i] == raw_r[i]).all(), (mode, "raw mask, frame", i, int((raw[i] != raw_r[i]).sum()))
        assert (fil[i] == posts[i][0]).all(), (mode, "filled mask, frame", i)
        assert (lab[i] == posts[i][1]).all(), (mode, "labels, frame", i)
    sh_r, fg_r = _counts_of(raw_r)
    assert (sh[:, 0] == sh_r).all() and (fg[:, 0] == fg_r).all(), (mode, sh[:, 0].tolist(), sh_r.tolist())
    assert int(sh_r[0]) + int(fg_r[0]) == SH_W * SH_H        # frame 1 is all foreground: every pixel is counted, no dead lane is
    _model_equal(m.state(0), mdl, mode)
    m.close()


# ------------------------------------------------------------------------------------------------ c. update plus post
YW, YH, YN = 4094, 1282, 3


@functools.lru_cache(maxsize=None)
def _yuv_ref(rng):
    """(y, u, v) [n][1][..] of a clip at 4094x1282 and the CPU labeller's result on its conversion."""
    y, u, v = Y.bgr_to_yuv420(any_clip(YN, YW, YH, seed=YW, start=1)[:, None], rng)
    ref = G.label_video_grid(Y.yuv_to_bgr(y, u, v, rng)[:, 0], history=HIST)
    _oracle_is_a_test(*ref[:3])
    for a in (y, u, v):
        a.setflags(write=False)
    return (y, u, v), ref


@pytest.mark.parametrize("fmt,make,rng", [("nv12", "tight", "limited"), ("nv12", "padded", "limited"), ("i420", "tight", "limited"),
                                          ("i420", "padded", "limited"), ("nv12", "padded", "full")],
                         ids=lambda v: str(v))
def test_decoder_surfaces_at_4094x1282(ctx, fmt, make, rng):
    """Working 2047x641.  A padded surface has a pitch of 4158, 8 coded rows behind the picture and 0xFF wherever no sample is."""
    planes, ref = _yuv_ref(rng)
    lay = getattr(Y, make)(YW, YH, fmt, rng)
    buf = Y.pack(*planes, lay) if make == "tight" else _pack_ff(planes, lay)
    m = _labeler(ctx, YW, YH)
    labels = m.apply_yuv(buf, lay.ctypes(), YN)
    _check_call(m, labels, ref, what=f"{fmt} {make} {rng}")
    _state_equal(m.state(0), ref[3])
    m.close()


def test_two_ragged_streams_staged_at_4096x256(ctx):
    """Two streams from host memory, of which the second takes 3 of the 4 frames, with a stage budget of one frame of every stream
    and a little: one update launch per frame, one post launch."""
    w, h, n = 4096, 256, 4
    nv = np.array([4, 3], np.int32)
    vids = [any_clip(n, w, h, seed=900 + s, start=1) for s in range(2)]
    refs = [G.label_video_grid(vids[s][:nv[s]], history=HIST) for s in range(2)]
    for r in refs:
        _oracle_is_a_test(*r[:3])
    m = _labeler(ctx, w, h, streams=2)
    m.set_stage_budget(2 * w * h * 3 + 4096)
    lh, lw = mog.label_dims_any(w, h)
    ctx.profile(True)
    try:
        lab = m.apply(np.stack(vids, 1), n_valid=nv, labels=np.full((n, 2, lh, lw), 77, np.uint8))
        prof = ctx.profile_read()
    finally:
        ctx.profile(False)
    assert {k: v[1] for k, v in prof.items()} == {"mog_any_update": n, "mog_any_post": 1}
    raw, filled = m.debug_masks()
    for s in range(2):
        k = int(nv[s])
        raw_r, fill_r, lab_r, mdl = refs[s]
        assert (raw[:k, s] == raw_r).all() and (filled[:k, s] == fill_r).all(), s
        assert (lab[:k, s] == lab_r).all() and (lab[k:, s] == 77).all(), s
        _state_equal(m.state(s), mdl)
    m.close()


def test_full_path_4096x4096(ctx):
    """The one run at the top of both axes: 2048x2048 working, 4,194,304 pixels per array of the model (424 MB), 8 bands, 65,536
    labels per frame."""
    w = h = 4096
    n = 2
    vid = any_clip(n, w, h, seed=w + h, start=1)
    ref = G.label_video_grid(vid, history=HIST)
    _oracle_is_a_test(*ref[:3])
    m = _labeler(ctx, w, h)
    assert (m.label_h, m.label_w) == (256, 256) == mog.label_dims_any(w, h)
    labels = m.apply(vid[:, None])
    _check_call(m, labels, ref)
    _state_equal(m.state(0), ref[3])
    m.close()
