"""MoG labels without a GPU: the oracle (tests/mog_ref.py) against scipy.ndimage and hand-worked MOG2 cases, the resize rules,
and the host side of cova_amd.mog (raw BGR24 reader, command-line checks)."""
import io

import numpy as np
import pytest
from scipy import ndimage as nd

from cova_amd import mog
from tests import mog_ref as R

F32 = np.float32
B4 = nd.generate_binary_structure(2, 1)


# ------------------------------------------------------------------------------------------------ morphology and fill
def _scipy_post(fg):
    """close 4x4 then open 6x6 with OpenCV's anchor, then fill with 4-connected background.  scipy reflects the structure for
    dilation only, so the same window x - k/2 .. x + k - 1 - k/2 is origin -1 there and origin 0 for erosion."""
    k4, k6 = np.ones((4, 4), bool), np.ones((6, 6), bool)
    cl = nd.binary_erosion(nd.binary_dilation(fg, k4, origin=-1), k4, origin=0, border_value=1)
    op = nd.binary_dilation(nd.binary_erosion(cl, k6, origin=0, border_value=1), k6, origin=-1)
    return op, nd.binary_fill_holes(op, structure=B4)


def _spiral(h=360, w=640, wall=8, gap=8):
    a = np.zeros((h, w), bool)
    top, left, bottom, right = 20, 20, h - 21, w - 21
    step = wall + gap
    while bottom - top > 2 * step and right - left > 2 * step:
        a[top:top + wall, left:right + 1] = True             # top edge
        a[top:bottom + 1, right - wall + 1:right + 1] = True  # right edge
        a[bottom - wall + 1:bottom + 1, left + step:right + 1] = True
        a[top + step:bottom + 1, left + step:left + step + wall] = True
        top, left, bottom, right = top + step, left + step, bottom - step, right - step
    return a


def _rings(h=360, w=640):
    y, x = np.mgrid[:h, :w]
    r = np.hypot(y - h / 2, x - w / 2)
    return ((r // 12) % 2 == 1) & (r < 170)


def _diag_hole():
    a = np.zeros((360, 640), bool)
    # a diamond outline: 1-pixel foreground segments that touch only diagonally seal a hole for 4-connected background
    cy, cx, r = 100, 200, 30
    for t in range(r):
        for py, px in ((cy - r + t, cx + t), (cy + t, cx + r - t), (cy + r - t, cx - t), (cy - t, cx - r + t)):
            a[py, px] = True
    return a


def _edge_touch():
    a = np.zeros((360, 640), bool)
    a[0:60, 100:110] = True
    a[0:60, 150:160] = True
    a[50:60, 100:160] = True          # a U open at the top edge: not a hole
    a[200:300, 300:400] = True
    a[230:270, 330:370] = False       # a real hole
    return a


HAND = {"spiral": _spiral(), "rings": _rings(), "diag_hole": _diag_hole(), "edge_touch": _edge_touch(),
        "empty": np.zeros((360, 640), bool), "full": np.ones((360, 640), bool)}


@pytest.mark.parametrize("name", sorted(HAND))
def test_fill_holes_hand_cases_match_scipy(name):
    a = HAND[name]
    ref = nd.binary_fill_holes(a, structure=B4)
    assert (R.fill_holes(a) == ref).all()


def test_diagonally_sealed_hole_is_filled():
    a = _diag_hole()
    f = R.fill_holes(a)
    assert f[100, 200] and not a[100, 200]
    assert not f[5, 5]


def test_spiral_corridor_is_not_a_hole():
    a = _spiral()
    f = R.fill_holes(a)
    # the spiral's corridor reaches the outside: nothing is filled
    assert (f == a).all()


@pytest.mark.parametrize("k", [4, 6])
def test_dilate_erode_match_scipy(k):
    rng = np.random.default_rng(k)
    for density in (0.05, 0.3, 0.7, 0.95):
        a = rng.random((360, 640)) < density
        kk = np.ones((k, k), bool)
        assert (R.dilate(a, k) == nd.binary_dilation(a, kk, origin=-1)).all()
        assert (R.erode(a, k) == nd.binary_erosion(a, kk, origin=0, border_value=1)).all()


def test_dilate_window_offsets():
    a = np.zeros((360, 640), bool)
    a[100, 300] = True
    d4 = R.dilate(a, 4)
    ys, xs = np.nonzero(d4)
    # out(x) = OR over x - 2 .. x + 1: a single pixel at 300 reaches x = 299 .. 302
    assert (ys.min(), ys.max(), xs.min(), xs.max()) == (99, 102, 299, 302)
    d6 = R.dilate(a, 6)
    ys, xs = np.nonzero(d6)
    assert (ys.min(), ys.max(), xs.min(), xs.max()) == (98, 103, 298, 303)


@pytest.mark.parametrize("seed", range(4))
def test_post_random_masks_match_scipy(seed):
    rng = np.random.default_rng(seed)
    # blobs of varied size so close, open and fill all act
    small = rng.random((46, 81)) < 0.35
    a = np.kron(small, np.ones((8, 8), bool))[:360, :640] ^ (rng.random((360, 640)) < 0.04)
    assert 0 < R.erode(R.dilate(a, 4), 4).sum() and 0 < R.post(np.where(a, 255, 0).astype(np.uint8))[1].sum()
    op, ref = _scipy_post(a)
    filled, labels = R.post(np.where(a, 255, 0).astype(np.uint8))
    assert (filled.astype(bool) == ref).all()
    assert (labels == ref[::8, ::8]).all() and labels.shape == (45, 80)


@pytest.mark.parametrize("name", sorted(HAND))
def test_post_hand_cases_match_scipy(name):
    a = HAND[name]
    _, ref = _scipy_post(a)
    filled, _ = R.post(np.where(a, 255, 0).astype(np.uint8))
    assert (filled.astype(bool) == ref).all()


# ------------------------------------------------------------------------------------------------ MOG2 by hand
def _model(nmodes, W, V, M, n=0, history=9000):
    m = R.Mog2(npix=1, history=history)
    m.nmodes[:] = nmodes
    m.W[:, 0] = np.array(W + [0] * (5 - len(W)), F32)
    m.V[:, 0] = np.array(V + [0] * (5 - len(V)), F32)
    for k, mu in enumerate(M):
        m.M[k, :, 0] = np.array(mu, F32)
    m.n = n
    return m


def _run(m, bgr):
    """applies one frame of one pixel; returns its mask byte"""
    return int(m.apply(np.asarray(bgr, np.uint8).reshape(1, 1, 3))[0, 0])


def test_learning_rates_in_double():
    a, p = R.learning_rates(1, 9000)
    assert a == F32(0.5) and p == F32(-0.5 * float(F32(0.05)))
    a, p = R.learning_rates(5000, 9000)
    assert a == F32(1.0 / 9000) and p == F32(-(1.0 / 9000) * float(F32(0.05)))
    assert R.learning_rates(8, 16)[0] == F32(1 / 16) and R.learning_rates(100, 16)[0] == F32(1 / 16)


def test_frame_one_is_all_foreground_then_static_turns_background():
    m = R.Mog2(npix=1)
    assert _run(m, (10, 20, 30)) == 255
    assert m.nmodes[0] == 1 and m.W[0, 0] == 1 and m.V[0, 0] == 15 and (m.M[0, :, 0] == [10, 20, 30]).all()
    assert _run(m, (10, 20, 30)) == 0
    # the fitted mode: w = alpha1 * 1 + prune + alphaT, renormalised to 1
    a, p = R.learning_rates(2, 9000)
    w = (F32(1) - a) * F32(1) + p + a
    assert m.W[0, 0] == w * (F32(1) / w)
    k = a / w
    assert m.V[0, 0] == max(F32(15) + k * (F32(0) - F32(15)), F32(4))


def test_prune_with_shrinking_bound_leaves_a_zero_weight_slot():
    # mode 1 is pruned; the bound drops to 2, so mode 2 (weight 0.4) is never visited and keeps its stale weight
    n = 4999
    m = _model(3, [0.6, 1e-7, 0.4], [15, 15, 15], [(0, 0, 0), (100, 100, 100), (200, 200, 200)], n=n)
    out = _run(m, (50, 50, 50))
    a, p = R.learning_rates(n + 1, 9000)
    a1 = F32(1) - a
    w0 = a1 * F32(0.6) + p
    tw = w0 + F32(0)
    inv = F32(1) / tw
    # nothing fits: a new mode goes into slot nmodes = 2 (the stale slot), then bubbles over the zero-weight slot 1
    assert out == 255
    assert m.nmodes[0] == 3
    assert m.W[0, 0] == (w0 * inv) * a1
    assert m.W[1, 0] == a and m.W[2, 0] == 0
    assert (m.M[1, :, 0] == 50).all() and (m.M[2, :, 0] == 100).all()       # the pruned mode's mean moved down one slot
    assert m.V[1, 0] == 15


def test_five_modes_replace_the_last():
    n = 100
    W = [0.4, 0.25, 0.15, 0.12, 0.08]
    m = _model(5, W, [15] * 5, [(i * 40, i * 40, i * 40) for i in range(5)], n=n)
    out = _run(m, (250, 5, 250))
    a, p = R.learning_rates(n + 1, 9000)
    a1 = F32(1) - a
    ws = [a1 * F32(w) + p for w in W]
    tw = F32(0)
    for w in ws:
        tw = tw + w
    inv = F32(1) / tw
    exp = [(w * inv) * a1 for w in ws[:4]]
    assert out == 255 and m.nmodes[0] == 5
    assert list(m.W[:4, 0]) == exp
    assert m.W[4, 0] == a and (m.M[4, :, 0] == [250, 5, 250]).all() and m.V[4, 0] == 15


def test_fitting_mode_bubbles_up_in_order():
    # mode 2 fits and its weight after the update exceeds mode 1's but not mode 0's: it swaps once
    n = 2
    m = _model(3, [0.5, 0.24, 0.26], [15, 15, 15], [(0, 0, 0), (100, 100, 100), (200, 200, 200)], n=n)
    out = _run(m, (201, 200, 200))
    a, p = R.learning_rates(n + 1, 9000)
    a1 = F32(1) - a
    w0, w1 = a1 * F32(0.5) + p, a1 * F32(0.24) + p
    w2 = a1 * F32(0.26) + p + a
    assert w2 >= w1 and w2 < w0
    # mode 2 is background only if the weight before it is below TB
    assert out == (0 if w0 + w1 < R.TB else 255)
    tw = (w0 + w1) + w2
    inv = F32(1) / tw
    assert list(m.W[:3, 0]) == [w0 * inv, w2 * inv, w1 * inv]
    k = a / w2
    assert m.M[1, 0, 0] == F32(200) - k * (F32(200) - F32(201))
    assert (m.M[2, :, 0] == 100).all()


# ------------------------------------------------------------------------------------------------ resize
def test_resize_rules():
    rng = np.random.default_rng(7)
    f720 = rng.integers(0, 256, (720, 1280, 3), dtype=np.uint8)
    r = R.resize_bgr(f720)
    for (y, x) in ((0, 0), (359, 639), (123, 456)):
        blk = f720[2 * y:2 * y + 2, 2 * x:2 * x + 2].astype(int)
        assert (r[y, x] == (blk.sum(axis=(0, 1)) + 2) // 4).all()
    f1080 = rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
    r = R.resize_bgr(f1080)
    assert (r[10, 20] == f1080[31, 61]).all() and r.shape == (360, 640, 3)
    f360 = rng.integers(0, 256, (360, 640, 3), dtype=np.uint8)
    assert (R.resize_bgr(f360) == f360).all()
    with pytest.raises(ValueError):
        R.resize_bgr(np.zeros((480, 640, 3), np.uint8))


# ------------------------------------------------------------------------------------------------ cova_amd.mog host side
def test_read_bgr24_chunks_and_truncation(tmp_path):
    w, h = 640, 360
    fb = w * h * 3
    data = (np.arange(5 * fb) % 251).astype(np.uint8)
    p = tmp_path / "v.bgr"
    p.write_bytes(data.tobytes())
    chunks = list(mog.read_bgr24(str(p), w, h, 2))
    assert [c.shape[0] for c in chunks] == [2, 2, 1]
    assert (np.concatenate(chunks).reshape(-1) == data).all()
    # a partial trailing frame is an error, not silently dropped
    p.write_bytes(data[:2 * fb + fb // 2].tobytes())
    it = mog.read_bgr24(str(p), w, h, 4)
    with pytest.raises(ValueError, match="truncated"):
        list(it)
    # file objects with short reads (a pipe) still give whole frames
    class Dribble(io.RawIOBase):
        def __init__(self, b):
            self.b, self.pos = b, 0

        def readinto(self, mv):
            n = min(len(mv), 7919, len(self.b) - self.pos)
            mv[:n] = self.b[self.pos:self.pos + n]
            self.pos += n
            return n

    got = list(mog.read_bgr24(Dribble(data.tobytes()[:3 * fb]), w, h, 8))
    assert len(got) == 1 and got[0].shape == (3, h, w, 3)
    assert list(mog.read_bgr24(io.BytesIO(b""), w, h, 3)) == []


def test_cli_default_output_and_parsing():
    assert mog.parse_io("a/b.bgr") == ("a/b.bgr", "a/b_gt.dump")
    assert mog.parse_io("a.bgr:x.dump") == ("a.bgr", "x.dump")
    assert mog.parse_io("-:x.dump") == ("-", "x.dump")
    assert mog.parse_size("1280x720") == (1280, 720)


@pytest.mark.parametrize("argv", [
    ["--size", "800x600", "a.bgr"],              # unsupported size
    ["--size", "1280by720", "a.bgr"],            # not WxH
    ["a.bgr"],                                   # no size
    ["--size", "1280x720"],                      # no input
    ["--size", "1280x720", "-"],                 # stdin without an output
    ["--size", "1280x720", "-:a.dump", "-:b.dump"],
    ["--size", "1280x720", "a.bgr:x.dump", "b.bgr:x.dump"],
    ["--size", "1280x720", "--streams", "0", "a.bgr"],
    ["--size", "1280x720", "--chunk", "0", "a.bgr"],
    ["--size", "1280x720", "--history", "0", "a.bgr"],
    ["--size", "1280x720", "--var-threshold", "0", "a.bgr"],
])
def test_cli_argument_errors(argv, capsys):
    with pytest.raises(SystemExit) as e:
        mog.main(argv)
    assert e.value.code == 2


# ------------------------------------------------------------------------------------------------ OpenCV parity (where cv2 exists)
def test_oracle_matches_opencv_where_available():
    cv = pytest.importorskip("cv2")
    rng = np.random.default_rng(11)
    bg = rng.integers(0, 256, (720, 1280, 3), dtype=np.uint8)
    frames = []
    for t in range(24):
        f = np.clip(bg.astype(np.int16) + rng.normal(0, 3, bg.shape), 0, 255).astype(np.uint8)
        cv.ellipse(f, (200 + 30 * t, 300), (60, 40), 0, 0, 360, (20, 200, 60), -1)
        frames.append(f)
    frames = np.stack(frames)
    raw, _, labels, _ = R.label_video(frames)
    sub = cv.createBackgroundSubtractorMOG2(history=9000, varThreshold=32, detectShadows=False)
    for i, f in enumerate(frames):
        m = sub.apply(cv.resize(f, (640, 360)))
        assert (m == raw[i]).all(), f"frame {i}"
        fg = (m > 0).astype(np.uint8)
        cl = cv.morphologyEx(fg, cv.MORPH_CLOSE, np.ones((4, 4)))
        op = cv.morphologyEx(cl, cv.MORPH_OPEN, np.ones((6, 6)))
        cnt, _ = cv.findContours(op.copy(), cv.RETR_EXTERNAL, cv.CHAIN_APPROX_SIMPLE)
        fill = cv.drawContours(op.copy(), cnt, -1, 1, cv.FILLED)
        assert (fill[::8, ::8] == labels[i]).all(), f"frame {i}"


# ------------------------------------------------------------------------------------------------ ISA of the update kernel
def test_update_kernel_isa_no_f32_fma_no_scratch():
    """The reference grid's update kernels (mog_update.hip) compile without contraction (no f32 fused multiply-add) and keep the
    five modes in registers; its post kernel (mog_post.hip, the resident template at 640x360) has no scratch either."""
    from tests import mog_isa

    mog_isa.assert_update_family(r"k_mog_update", 3)
    mog_isa.assert_post_family(r"k_mog_grid_postILi640E", 1)
