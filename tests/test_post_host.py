"""Per-model post-processing, the parts that need no GPU: the C entries refuse a NULL ctx, keep_from_rects turns pixel rectangles
into a keep map, and BlobNetInfer converts a probability threshold into the float32 logit threshold the library takes."""
import ctypes as C

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd.elements import BlobNetInfer, keep_from_rects


def test_null_ctx_is_invalid_argument():
    lib = L.lib()
    post = L.BlobNetPost(0.5, None)
    assert lib.covahip_blobnet_set_post(None, 0, C.byref(post)) == 1
    assert lib.covahip_blobnet_set_post(None, 0, None) == 1
    thr, has = C.c_float(), C.c_int()
    assert lib.covahip_blobnet_get_post(None, 0, C.byref(thr), None, C.byref(has)) == 1


def test_post_struct_layout_matches_header():
    # float, padding, pointer
    assert C.sizeof(L.BlobNetPost) == 2 * C.sizeof(C.c_void_p)
    assert L.BlobNetPost.keep.offset == C.sizeof(C.c_void_p)


def test_keep_from_rects_empty_list():
    k = keep_from_rects(5, 7)
    assert k.dtype == np.uint8 and k.shape == (5, 7) and k.all()
    assert keep_from_rects(5, 7, ignore=[]).all()
    assert keep_from_rects(5, 7, ignore=[(20, 20, 0, 10)]).all()          # an empty rectangle


def test_keep_from_rects_inside_one_macroblock():
    k = keep_from_rects(5, 7, [(33, 17, 10, 10)])                        # pixels x 33..42, y 17..26: macroblock (1, 2)
    want = np.ones((5, 7), np.uint8)
    want[1, 2] = 0
    assert np.array_equal(k, want)
    # touching the macroblock's last pixel is still inside; one pixel more reaches the next one
    assert np.array_equal(keep_from_rects(5, 7, [(32, 16, 16, 16)]), want)
    assert keep_from_rects(5, 7, [(32, 16, 17, 16)])[1, 3] == 0


def test_keep_from_rects_straddles_four_macroblocks():
    k = keep_from_rects(5, 7, [(47, 31, 2, 2)])                          # pixels x 47..48, y 31..32
    want = np.ones((5, 7), np.uint8)
    want[1:3, 2:4] = 0
    assert np.array_equal(k, want)


def test_keep_from_rects_clipped_to_the_grid():
    k = keep_from_rects(5, 7, [(100, 70, 500, 500)])                     # hangs over the right and bottom edge
    want = np.ones((5, 7), np.uint8)
    want[4:, 6:] = 0
    assert np.array_equal(k, want)
    assert keep_from_rects(5, 7, [(7 * 16, 0, 50, 50), (0, 5 * 16, 50, 50)]).all()   # wholly outside
    k = keep_from_rects(5, 7, [(-40, -40, 50, 50)])                      # over the left and top edge: pixels up to 9
    want = np.ones((5, 7), np.uint8)
    want[0, 0] = 0
    assert np.array_equal(k, want)


def test_keep_from_rects_unit_8():
    k = keep_from_rects(6, 6, [(9, 17, 8, 2)], unit=8)                   # pixels x 9..16, y 17..18
    want = np.ones((6, 6), np.uint8)
    want[2, 1:3] = 0
    assert np.array_equal(k, want)
    # several rectangles add up
    k = keep_from_rects(6, 6, [(0, 0, 8, 8), (40, 40, 8, 8)], unit=8)
    assert k.sum() == 34 and k[0, 0] == 0 and k[5, 5] == 0


def test_prob_thresh_conversion():
    f = BlobNetInfer.post_logit_thresh
    assert f() == 0.0
    assert f(prob_thresh=0.5) == 0.0 and np.signbit(f(prob_thresh=0.5)) == False  # noqa: E712
    assert f(prob_thresh=0.8) == float(np.float32(np.log(4.0)))
    assert f(prob_thresh=0.2) == float(np.float32(-np.log(4.0)))
    assert f(logit_thresh=-1.5) == -1.5
    assert f(logit_thresh=0.1) == float(np.float32(0.1))                 # rounded to float32
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            f(prob_thresh=bad)


def test_both_thresholds_rejected():
    with pytest.raises(ValueError):
        BlobNetInfer.post_logit_thresh(prob_thresh=0.5, logit_thresh=0.0)
    with pytest.raises(ValueError):
        BlobNetInfer.set_post(object(), 0, prob_thresh=0.7, logit_thresh=1.0)     # rejected before anything is touched
