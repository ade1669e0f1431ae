"""MoG labels by block coverage (covahip_mog_set_labels: COVAHIP_MOG_LABELS_CORNER / _COVER / _COUNT) on all four post kernels,
bit for bit against tests/mog_cover_ref.py applied to the oracle's filled mask (tests/mog_ref.post, tests/mog_band_ref.post,
tests/mog_grid_ref.label_video_grid).  Every comparison of labels first asserts that debug_masks()' filled mask is the oracle's, so
a label mismatch points at the label step.

Planted raw masks go through MogLabeler.post_masks, three frames per call (one at 1280x720) and as many streams as the planes
need.  They hold rectangles 6x6, 7x9, 8x8 and 12x20 at all 64 offsets mod 8, a ring whose hole the fill closes, blobs that end in
the last started row and column (one starts three rows into its block, so that a started block is covered by about half), a full
frame and an empty frame; each runs in COUNT, in COVER at N = 1, 32 and 64, and in CORNER.

  1. reference grid, 640x360 (mog.hip, all blocks whole)
  2. resident macroblock grid, 640x360 source: 320x180 working, 23x40 labels, label row 22 four rows high (mog_grid.hip)
  3. banded form, forced: set_post_form(banded=True, band_rows=..) in several bands.  The table has the banded kernel beside the
     resident one at one size only, 1920x1080 (960x540 working, 68x120 labels, label row 67 four rows high), and refuses the
     switch at 320x180 (tests/test_gpu_mog_band.py holds it to that), so this case runs there, resident and banded on one labeller
  4. banded form, the table's own entry: 2560x1440, 1280x720 working, one frame per stream (mog_band.hip)
  5. any size, partial blocks: 266x258, 133x129 working, 17x17 labels, a last column of 5 and a last row of 1 pixel, a row pitch
     of 192 with 59 dead bits in a row's last word (mog_any.hip)
  6. any size, dead bits and no partial block: 272x256, 136x128 working
  7. any size, neither: 256x256, 128x128 working
  8. mode switching through apply and apply_yuv on a clip with a moving 6x10 rectangle
  9. errors of covahip_mog_set_labels, and the command line
"""
import ctypes as C
import functools

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import mog
from tests import mog_band_ref as B
from tests import mog_cover_ref as CR
from tests import mog_grid_ref as G
from tests import mog_ref as R
from tests import mog_yuv_ref as Y
from tests.test_gpu_mog_grid import _same_model

pytestmark = pytest.mark.gpu

MODES = ("count", ("cover", 1), ("cover", 32), ("cover", 64), "corner")
SHAPES = ((6, 6), (7, 9), (8, 8), (12, 20))              # (rows, columns) of the planted rectangles
HIST = 16


# ------------------------------------------------------------------------------------------------ planted masks
def _rect_planes(h, w):
    """Every shape at every offset (oy, ox) mod 8, one per cell of 24 rows x 24 (12x20: 32) columns whose origin is a multiple
    of 8, from (8, 8) on, so a rectangle keeps at least 5 pixels to the next and to the frame edge: close 4x4 joins nothing
    and open 6x6 keeps each whole.  (Both move it: with the anchor k/2 for erode and dilate alike, a closing and an opening by
    an even kernel each shift a free-standing rectangle by (+1, +1), so the filled rectangles are the planted ones at
    (+2, +2) -- still every offset mod 8.)  As many planes as that takes at h x w."""
    planes, cy, cx = [np.zeros((h, w), bool)], 8, 8
    for sh, sw in SHAPES:
        cw = 24 if sw + 7 + 5 <= 24 else 32
        for oy in range(8):
            for ox in range(8):
                if cx + cw > w:
                    cy, cx = cy + 24, 8
                if cy + 24 > h:
                    planes.append(np.zeros((h, w), bool))
                    cy = cx = 8
                planes[-1][cy + oy:cy + oy + sh, cx + ox:cx + ox + sw] = True
                cx += cw
    return planes


def _ring(h, w):
    a = np.zeros((h, w), bool)
    a[13:53, 19:67] = True
    a[21:45, 27:59] = False                                  # a hole of 24 x 32 behind a wall of 8
    return a


def _shifted(a):
    """a at (+2, +2): what close 4x4 and open 6x6 make of free-standing rectangles."""
    out = np.zeros_like(a)
    out[2:, 2:] = a[:-2, :-2]
    return out


def _edge_blobs(h, w):
    """(planted, filled): a blob that ends in the last row and column and whose filled form starts at row 3 (mod 8) of its first
    blocks, and one on the bottom edge that is 5 rows high when filled (on the edge only the free sides move)."""
    top = 8 * ((h - 20) // 8) + 1
    a, f = np.zeros((h, w), bool), np.zeros((h, w), bool)
    a[top:, w - 30:] = True
    f[top + 2:, w - 28:] = True
    a[h - 7:, 10:25] = True
    f[h - 5:, 12:27] = True
    return a, f


@functools.lru_cache(maxsize=None)
def _planted(h, w, frames_per_call=3):
    """(raw u8 [F][S][h][w], the oracle's filled [F][S][h][w]) of the planted planes at h x w, padded with empty frames."""
    rects = _rect_planes(h, w)
    planes = rects + [_ring(h, w), _edge_blobs(h, w)[0], np.ones((h, w), bool), np.zeros((h, w), bool)]
    F = frames_per_call
    S = -(-len(planes) // F)
    planes += [np.zeros((h, w), bool)] * (F * S - len(planes))
    raw = B.to_u8(np.stack(planes)).reshape(F, S, h, w)
    filled = np.stack([B.post(p)[0] for p in planes]).reshape(F, S, h, w)
    flat = filled.reshape(-1, h, w)
    # the planes are what they are for, on the oracle alone
    for i, p in enumerate(rects):
        assert (flat[i] == _shifted(p)).all()                # every rectangle survives whole and alone
    corner, cover1 = CR.corner(flat[:len(rects)]), CR.cover(flat[:len(rects)], 1)
    assert corner.sum() < cover1.sum() and (CR.count(flat[:len(rects)]) == 36).any()      # a 6x6 inside one block, no corner
    ring = flat[len(rects)]
    assert ring[15:55, 21:69].all() and ring.sum() == 40 * 48                             # the fill closed the hole
    blob = flat[len(rects) + 1]
    assert blob[-1, -1] == 1 and (blob == _edge_blobs(h, w)[1]).all()
    cnt, ins = CR.count(blob), CR.inside(h, w)
    assert (CR.cover(blob, 32) != CR.cover(blob, 1)).any() and (CR.cover(blob, 64) != CR.cover(blob, 32)).any()
    if h % 8 or w % 8:                                       # a started block where `inside` decides the label at N = 32
        assert ((64 * cnt >= 32 * ins) & (64 * cnt < 32 * 64)).any()
    assert flat[len(rects) + 2].all() and not flat[len(rects) + 3].any()
    raw.setflags(write=False)
    filled.setflags(write=False)
    return raw, filled


def _check_modes(m, raw, filled_o, what=""):
    """Every mode on one labeller and the same planes: the filled mask is the oracle's, then the labels are the helper's."""
    for mode in MODES:
        m.set_labels(mode)
        assert m.labels == mode
        lab = m.post_masks(raw)
        raw_d, filled = m.debug_masks()
        assert (raw_d == raw).all(), (what, mode)
        assert (filled == filled_o).all(), (what, mode, "filled mask", int((filled != filled_o).sum()))
        want = CR.labels(filled_o, mode)
        assert lab.shape == want.shape and lab.dtype == np.uint8, (what, mode)
        bad = np.argwhere(lab != want)
        assert not len(bad), (what, mode, len(bad), bad[:4].tolist(), lab[lab != want][:4].tolist(), want[lab != want][:4].tolist())
    assert (CR.labels(filled_o, "corner") == filled_o[..., ::8, ::8]).all()      # CORNER is the oracle's own subsample


def _planted_case(ctx, src_w, src_h, work, labels, frames_per_call=3, **kw):
    raw, filled_o = _planted(work[1], work[0], frames_per_call)
    m = mog.MogLabeler(ctx, src_w, src_h, streams=raw.shape[1], history=HIST, **kw)
    assert (m.work_w, m.work_h) == work and (m.label_h, m.label_w) == labels and m.labels == "corner"
    return m, raw, filled_o


# ------------------------------------------------------------------------------------------------ 1 - 7. the four kernels
def test_reference_grid(ctx):
    m, raw, filled_o = _planted_case(ctx, 640, 360, (640, 360), (45, 80))
    _check_modes(m, raw, filled_o)
    m.close()


def test_resident_macroblock_grid(ctx):
    m, raw, filled_o = _planted_case(ctx, 640, 360, (320, 180), (23, 40), grid="macroblock")
    assert (CR.inside(180, 320)[22] == 32).all()             # label row 22 is four rows high
    _check_modes(m, raw, filled_o)
    m.close()


def test_banded_form_forced(ctx):
    m, raw, filled_o = _planted_case(ctx, 1920, 1080, (960, 540), (68, 120), grid="macroblock")
    assert (CR.inside(540, 960)[67] == 32).all()
    _check_modes(m, raw, filled_o, "resident")
    for rows in (64, 37):                                    # nine bands; fifteen that do not divide the height or a block
        m.set_post_form(True, rows)
        _check_modes(m, raw, filled_o, f"banded, {rows} rows")
    m.close()


def test_banded_form_table_entry(ctx):
    m, raw, filled_o = _planted_case(ctx, 2560, 1440, (1280, 720), (90, 160), frames_per_call=1, grid="macroblock")
    assert raw.shape[0] == 1
    _check_modes(m, raw, filled_o)
    m.close()


@pytest.mark.parametrize("src,work,labels", [((266, 258), (133, 129), (17, 17)), ((272, 256), (136, 128), (16, 17)),
                                             ((256, 256), (128, 128), (16, 16))], ids=["partial_blocks", "dead_bits", "neither"])
def test_any_size(ctx, src, work, labels):
    m, raw, filled_o = _planted_case(ctx, src[0], src[1], work, labels, grid="macroblock", any_size=True)
    assert m.general
    if work == (133, 129):
        ins = CR.inside(129, 133)
        assert (ins[:-1, -1] == 40).all() and (ins[-1, :-1] == 8).all() and ins[-1, -1] == 5
    _check_modes(m, raw, filled_o)
    for rows in (16, 37):                                    # several bands
        m.set_post_form(True, rows)
        m.set_labels("count")
        assert (m.post_masks(raw) == CR.labels(filled_o, "count")).all(), rows
    m.close()


# ------------------------------------------------------------------------------------------------ 8. mode switching
@functools.lru_cache(maxsize=None)
def _moving_clip():
    """Eight frames 640x360: a fixed background in 0 .. 99 (2x2 repeated, so the working image is exact) and from frame 1 on a
    rectangle of 6 x 10 working pixels of 255 - background that moves by (3, 11) working pixels per frame; the oracle on it."""
    w, h, n = 640, 360, 8
    bg = np.random.default_rng(11).integers(0, 100, (h // 2, w // 2, 3), dtype=np.uint8).repeat(2, 0).repeat(2, 1)
    vid = np.repeat(bg[None], n, 0)
    for t in range(1, n):
        y, x = 2 * (41 + 3 * t), 2 * (50 + 11 * t)
        vid[t, y:y + 12, x:x + 20] = 255 - bg[y:y + 12, x:x + 20]
    ref = G.label_video_grid(vid, history=HIST)
    filled = ref[1]
    for t in range(1, n):
        want = np.zeros((180, 320), np.uint8)
        want[43 + 3 * t:49 + 3 * t, 52 + 11 * t:62 + 11 * t] = 1      # (close and open move it by (+2, +2): _rect_planes)
        assert (filled[t] == want).all(), t
    corner = CR.corner(filled[1:]).sum((1, 2))
    assert (corner == 0).any() and (corner > 0).any()        # the object blinks in and out of its corner labels
    assert (CR.cover(filled[1:], 1).sum((1, 2)) >= 2).all()  # and never out of its coverage labels
    vid.setflags(write=False)
    return vid, ref


def test_mode_switching_keeps_the_model(ctx):
    vid, ref = _moving_clip()
    filled_o = ref[1]
    a = mog.MogLabeler(ctx, 640, 360, history=HIST, grid="macroblock", labels=("cover", 1))
    assert a.labels == ("cover", 1)
    lab_a = a.apply(vid[:, None])
    assert (a.debug_masks()[1][:, 0] == filled_o).all()
    assert (lab_a[:, 0] == CR.cover(filled_o, 1)).all()
    assert (lab_a[:, 0] != ref[2]).any()
    # CORNER -> COUNT -> COVER between calls: each call's labels follow its mode, the model is that of the labeller above
    b = mog.MogLabeler(ctx, 640, 360, history=HIST, grid="macroblock")
    for (lo, hi), mode in (((0, 3), "corner"), ((3, 5), "count"), ((5, 8), ("cover", 1))):
        b.set_labels(mode)
        lab = b.apply(vid[lo:hi, None])
        assert (b.debug_masks()[1][:, 0] == filled_o[lo:hi]).all(), mode
        assert (lab[:, 0] == CR.labels(filled_o[lo:hi], mode)).all(), mode
        if mode == "corner":
            assert (lab[:, 0] == ref[2][lo:hi]).all()
    sa, sb = a.state(0), b.state(0)
    assert sa["n"] == 8
    _same_model(sa, sb, "switched")
    for k in ("W", "V", "M"):                                # (every bit, not every value)
        assert (sa[k].view(np.uint32) == sb[k].view(np.uint32)).all(), k
    b.reset(0)                                               # reset keeps the setting
    assert b.labels == ("cover", 1) and b.state(0)["n"] == 0
    assert (b.apply(vid[:2, None])[:, 0] == CR.cover(filled_o[:2], 1)).all()
    a.close()
    b.close()


def test_setting_reaches_apply_yuv(ctx):
    vid, _ = _moving_clip()
    n = 4
    y, u, v = Y.bgr_to_yuv420(vid[:n, None], "limited")
    bgr = Y.yuv_to_bgr(y, u, v, "limited")[:, 0]
    ref = G.label_video_grid(bgr, history=HIST)
    assert (CR.cover(ref[1][1:], 1) != ref[2][1:]).any()              # (a corner labeller would give other labels)
    lay = Y.tight(640, 360, "nv12")
    m = mog.MogLabeler(ctx, 640, 360, history=HIST, grid="macroblock", labels=("cover", 1))
    lab = m.apply_yuv(Y.pack(y, u, v, lay), lay.ctypes(), n)
    assert (m.debug_masks()[1][:, 0] == ref[1]).all()
    assert (lab[:, 0] == CR.cover(ref[1], 1)).all()
    m.close()


# ------------------------------------------------------------------------------------------------ 9. errors, command line
def test_set_labels_errors(ctx):
    lib = L.lib()
    m = mog.MogLabeler(ctx, 640, 360, grid="macroblock")

    def get():
        mode, n = C.c_int(-7), C.c_int(-7)
        assert lib.covahip_mog_get_labels(m.handle, C.byref(mode), C.byref(n)) == 0
        return mode.value, n.value

    assert get() == (0, 1)
    assert lib.covahip_mog_set_labels(m.handle, 1, 48) == 0 and get() == (1, 48)
    for mode, n in ((3, 1), (-1, 1), (1, 0), (1, 65), (1, -5)):
        assert lib.covahip_mog_set_labels(m.handle, mode, n) == 1, (mode, n)      # COVAHIP_ERR_INVALID_ARG
        assert get() == (1, 48), (mode, n)
    assert lib.covahip_mog_set_labels(m.handle, 2, 0) == 0 and get() == (2, 48)    # min_cover is read in COVER mode only
    assert lib.covahip_mog_get_labels(m.handle, None, None) == 0
    assert lib.covahip_mog_set_labels(m.handle, 0, 99) == 0 and m.labels == "corner"
    with pytest.raises(ValueError):
        m.set_labels(("cover", 65))
    assert m.labels == "corner"
    m.close()


def test_cli_writes_what_the_api_gives(ctx, tmp_path):
    vid, ref = _moving_clip()
    p = tmp_path / "v.bgr"
    p.write_bytes(vid.tobytes())
    argv = ["--size", "640x360", "--grid", "macroblock", "--history", str(HIST), "--chunk", "3"]
    m = mog.MogLabeler(ctx, 640, 360, history=HIST, grid="macroblock")
    for text, mode, out in (("cover:32", ("cover", 32), "c32.dump"), ("cover", ("cover", 1), "c1.dump"), ("count", "count", "n.dump")):
        assert mog.main(argv + ["--labels", text, f"{p}:{tmp_path / out}"]) == 0
        got = np.fromfile(tmp_path / out, np.uint8).reshape(8, 23, 40)
        m.reset(0)
        m.set_labels(mode)
        assert (got == m.apply(vid[:, None])[:, 0]).all(), text
        assert (got == CR.labels(ref[1], mode)).all(), text
    assert mog.main(argv + [f"{p}:{tmp_path / 'd.dump'}"]) == 0           # the default stays the corner pixel
    assert (np.fromfile(tmp_path / "d.dump", np.uint8).reshape(8, 23, 40) == ref[2]).all()
    m.close()
