"""The planes and plans of tests/test_gpu_mog_any_range.py (the any-size MoG labeller up to 4096x4096) without a GPU: that the GPU
tests can fail.  For every (shape, plan, plane) the GPU file uses, on the oracle alone (tests/mog_ref.py through
tests/mog_band_ref.py):

  * the band plan restated in Python is the library's, and is the plan the shapes were chosen for;
  * no plane is empty (but `empty`), the sealed spiral and the closed serpentine get filled, the corner blob labels the last label
    row and column, the right-edge plane keeps its three outcomes; corridors, morphology, right edge, sealed spiral and corner
    blob are live at every shape (the coarse spiral is left out below 170 rows or columns by mog_band_ref.range_names, by name);
  * two bugs planted on the numpy side each change the filled mask inside the image:
      dead bits leak      the oracle on the plane padded with background columns up to the row pitch, cropped back: what a
                          kernel computes that reads the bits beyond the image as pixels.  Differs on right_edge at every shape
                          whose width is no multiple of 64.
      bands do not talk   the hole fill run on every band of the plan by itself, in two forms: a seam is an image edge (every
                          background pixel on a seam row is reached: a hole that crosses a seam is not filled), or a seam is a
                          wall (nothing crosses it: background that is reached only through another band is filled).  The first
                          differs on corridor1 and on the closed serpentine, the second on the open serpentine, at every
                          multi-band (shape, plan).  corridor4 is in neither list: its cavity is open in either half by the half of
                          its corridor that lies on the same side of the seam, so neither form changes it; it tests that a 4-row
                          corridor survives the closing across a seam.
"""
import numpy as np
import pytest

from tests import mog_band_ref as B
from tests import mog_ref as R

CASES = [(w, h, rows) for w, h, forced in B.RANGE_SHAPES for rows in (0,) + forced] + [B.RANGE_FULL + (0,)]
IDS = [f"{w}x{h}-{'auto' if not r else r}" for w, h, r in CASES]


def _names(w, h):
    return B.FULL_PLANES if (w, h) == B.RANGE_FULL else B.range_names(w, h)


def test_band_plans_restated():
    assert B.LDS_MAX == 163776
    assert B.band_max_rows(2047) == B.band_max_rows(2048) == 287
    assert B.band_lds_bytes(2047, 641, 287) <= B.LDS_MAX < B.band_lds_bytes(2047, 641, 288)
    want = {(2047, 641): (214, 3), (2048, 272): (272, 1), (1985, 137): (137, 1), (1984, 136): (136, 1), (129, 2047): (2047, 1),
            (1296, 972): (324, 3), (352, 288): (288, 1), (2048, 2048): (256, 8)}
    for (w, h), plan in want.items():
        assert B.auto_plan(w, h) == plan, (w, h)           # (auto_plan itself asserts that the library gives the same)
    for w, h in ((960, 540), (1280, 720), (1920, 1080)):   # the table's sizes, as tests/test_mog_band_host.py pins them
        assert B.auto_plan(w, h) == B.band_plan(w, h)[:2]
    for w, h, forced in B.RANGE_SHAPES:
        for rows in forced:
            assert 16 <= rows <= h and B.band_lds_bytes(w, h, rows) <= B.LDS_MAX, (w, h, rows)
    assert -(-2047 // 16) == 128 and -(-2047 // 512) == 4


def test_right_edge_is_the_330x190_case():
    a = np.zeros((190, 330), bool)                         # as tests/test_gpu_mog_any.py had it before it became a function
    a[:, 327:] = True
    a[20:170, 270:] = True
    a[35:55, 290:330] = False
    a[80:100, 290:326] = False
    a[125:145, 290:325] = False
    assert (B.right_edge(190, 330) == a).all()


@pytest.mark.parametrize("w,h,rows", CASES, ids=IDS)
def test_planes_do_what_they_are_for(w, h, rows):
    r = B.plan_rows(w, h, rows)
    names = _names(w, h)
    for must in ("corridor1", "corridor4", "seam_morphology", "right_edge", "sealed_spiral", "corner_blob"):
        assert must in names, must
    if "spiral" not in names and (w, h) != B.RANGE_FULL:
        assert min(w, h) < 170 and not B.coarse_spirals(h, w)[0].any()       # left out because it is empty there
    seam = B.pick_seams(h, r)
    assert all(s - 30 >= 0 and s + 30 <= h for s in seam) and (B.seams(h, r) == [] or set(seam) <= set(B.seams(h, r)))
    for nm in names:
        mask = B.range_plane(nm, w, h, r)
        f, l = B.range_oracle(nm, w, h, r)
        assert mask.shape == f.shape == (h, w) and l.shape == (-(-h // 8), -(-w // 8)), nm
        assert mask.any() or nm == "empty", nm
        if nm == "sealed_spiral":
            assert f.sum() > mask.sum()
        elif nm == "serpentine_closed":
            ys, xs = B.last_lane(h, w, B.serpentine_lanes(w))
            assert f[ys, xs][4:-4, 4:-4].all() and not mask[ys, xs][4:-4, 4:-4].any()
        elif nm == "serpentine":
            assert f.sum() == mask.sum()                   # every lane is open to the entrance
        elif nm == "corner_blob":
            assert l[-1, -1] == 1 and l[-1].sum() > 1 and l[:, -1].sum() > 1
        elif nm in ("corridor1", "corridor4"):
            x0 = 64 * (w // 128) - 12
            for s in seam:
                assert not mask[s, x0 - 15] and bool(f[s, x0 - 15]) == (nm == "corridor1"), (nm, s)
        elif nm == "seam_morphology":
            s, c = seam[0], 1                              # the first feature: a gap of 3 rows at offset -3, which the closing shuts
            assert not mask[s - 3, 64 * c] and f[s - 3, 64 * c] == 1
        elif nm == "right_edge":
            (y0, _), cav = B.right_edge_rows(h)
            assert not f[y0 // 2, w - 8:].any()            # the thin strip is gone
            assert [int(f[c + 10, w - 30]) for c in cav] == [0, 0, 1]      # open, opened by the morphology, filled
        elif nm == "full":
            assert f.all() and l.all()
        elif nm == "empty":
            assert not f.any() and not l.any()


@pytest.mark.parametrize("w,h", sorted({(w, h) for w, h, _ in CASES if w % 64}), ids=lambda v: str(v))
def test_planted_bug_dead_bits_leak(w, h):
    mask = B.range_plane("right_edge", w, h, h)
    padded = np.zeros((h, B.pitch(w)), bool)
    padded[:, :w] = mask
    leaked = B.post(padded)[0][:, :w]
    true = B.range_oracle("right_edge", w, h, h)[0]
    _, cav = B.right_edge_rows(h)
    probes = [(c + 10, w - 30) for c in cav]               # inside the three cavities: the walls stand differently off the edge
    assert (leaked != true).any() and any(leaked[p] != true[p] for p in probes)


def _morph(mask):
    return R.dilate(R.erode(R.erode(R.dilate(mask, 4), 4), 6), 6)


def _fill_per_band(op, rows, seam_is_edge):
    """fill_holes of tests/mog_ref.py on every band of `rows` rows by itself.  seam_is_edge: the band is an image of its own;
    else a foreground row stands on every seam, so the fill starts from the image's own edge pixels alone."""
    h = op.shape[0]
    out = np.empty(op.shape, np.uint8)
    for y0 in range(0, h, rows):
        y1 = min(y0 + rows, h)
        band = op[y0:y1]
        if seam_is_edge:
            out[y0:y1] = R.fill_holes(band)
            continue
        top, bot = int(y0 > 0), int(y1 < h)
        walled = np.ones((y1 - y0 + top + bot, op.shape[1]), bool)
        walled[top:top + y1 - y0] = band
        out[y0:y1] = R.fill_holes(walled)[top:top + y1 - y0]
    return out


MULTI = [(w, h, rows) for w, h, rows in CASES if B.plan_rows(w, h, rows) < h]


@pytest.mark.parametrize("w,h,rows", MULTI, ids=[i for i, c in zip(IDS, CASES) if c in MULTI])
def test_planted_bug_bands_do_not_talk(w, h, rows):
    r = B.plan_rows(w, h, rows)
    assert len(B.seams(h, r)) >= 1
    for nm, seam_is_edge in (("corridor1", True), ("serpentine_closed", True), ("serpentine", False)):
        if nm not in _names(w, h):
            assert (w, h) == B.RANGE_FULL and nm == "serpentine"           # (the 2048x2048 case has the closed one only)
            continue
        true = B.range_oracle(nm, w, h, r)[0]
        alone = _fill_per_band(_morph(B.range_plane(nm, w, h, r)), r, seam_is_edge)
        assert alone.shape == true.shape and (alone != true).any(), (nm, seam_is_edge)


def test_the_cases_cover_the_range():
    shapes = {(w, h) for w, h, _ in CASES}
    words = {(-(-w // 64), w % 64 or 64) for w, _ in shapes}
    assert {(32, 63), (32, 64), (32, 1), (31, 64), (3, 1)} <= words
    assert max(h for _, h in shapes) >= 2047 and B.RANGE_FULL in shapes
    assert (1296, 972) in shapes and (352, 288) in shapes                  # 2592x1944 and 704x576
    plans = {(w, h, rows): (B.plan_rows(w, h, rows), -(-h // B.plan_rows(w, h, rows))) for w, h, rows in CASES}
    assert plans[(2047, 641, 0)] == (214, 3) and plans[(2047, 641, 287)][0] == B.band_max_rows(2047)
    assert plans[(129, 2047, 16)][1] == 128 and plans[(2048, 2048, 0)] == (256, 8)
