"""The last decoder block inside the decoder launch (dec012_mfma ending in bboxcc's parity planes, cc_planes behind it) against the
two launches it replaces (dec012_mfma -> dact[2] -> dec3cc_rows_mfma), the chain as it was before the form existed.

Block 2 scatters its output into the row tail's tile in LDS instead of HBM, the folded last block runs there on eight waves with the
text of the row tail (tail_row_tile), and what crosses to the second launch is the frame's parity planes.  No operand and no order
of a sum changes, so counts, boxes INCLUDING their order, mask and logits are compared with np.array_equal: no tolerance.  Every
case asserts through covahip_dev_blobnet_tail_in_dec012 that the form it forced is the one that ran (and that the reference did not
take it): a case that fell back would prove nothing.

Grids: 16x16 smallest; 17x24 odd H (crop offsets, the zero grid row behind the image); 16x24 one-tile rows; 35x64 odd H at half
scale (one full tile and one position of a second); 67x120 and 68x120 the workload's (two tiles per row, the second partial).
17x20 and 35x60, odd H with a W that is no multiple of 8, are outside the row tiles' geometry (the run-based bboxcc, ccwave::wv_plan,
takes whole 8-pixel pieces): there the form must NOT engage even when forced, and their case asserts that and unchanged results.  Batch 3 everywhere; at 16x24 also 2 x CUs + 3, where
a workgroup takes several frames and the tile t3 and the planes are reused under the next frame's requests (the loop-head barrier).
"""
import numpy as np
import pytest

from cova_amd import synth, weights as W
from cova_amd.elements import BlobNetInfer

pytestmark = pytest.mark.gpu

GRIDS = [(16, 16), (17, 24), (16, 24), (35, 64), (67, 120), (68, 120)]


def _mixed_gamma_weights(seed):
    """Every second BN gamma of every encoder level negative: the other gamma-sign class of kernels."""
    wts = W.unflatten(W.random_init(seed))
    for i in range(4):
        wts[f"enc{i}.bn.gamma"][::2] *= -1.0
    return W.flatten(wts)


WEIGHTS = {"seed": lambda: W.random_init(1234), "mixed": lambda: _mixed_gamma_weights(57), "blob": lambda: W.blob_like(7)}


def _run(net, entry, inputs, cc, max_boxes, want_mask, want_logits):
    """-> (boxes, counts, mask or None, logits or None)"""
    if entry == "frames":
        return net.filter_frames(inputs[0], inputs[1], cc, max_boxes=max_boxes, want_mask=want_mask, want_logits=want_logits)
    return net.filter_full(inputs, cc, max_boxes=max_boxes, want_mask=want_mask, want_logits=want_logits)


def _same(got, ref, b, max_boxes, what):
    np.testing.assert_array_equal(got[1], ref[1], err_msg=what + " counts")
    for a, c, name in zip(got[2:], ref[2:], ("mask", "logits")):
        assert (a is None) == (c is None)
        if a is not None:
            assert np.array_equal(a, c), f"{what}: {name} differ at {np.argwhere(a != c)[:5].tolist()}"
    for i in range(b):
        n = min(int(got[1][i]), max_boxes)   # (entries behind a frame's count are unspecified)
        assert np.array_equal(got[0][i, :n], ref[0][i, :n]), f"{what}: boxes of frame {i} differ"


def _compare(ctx, h, w, b, wname, entry, calls):
    """calls: (cc threshold, max_boxes, want_mask, want_logits) each run in both forms on one model and one input."""
    what = f"{h}x{w} b={b} {wname} {entry}"
    net = BlobNetInfer(ctx, WEIGHTS[wname](), h, w, max_batch=b)
    streams = 3 if b > 2 else 1
    inputs = synth.carrier_batch(b, h, w, seed=43, streams=streams) if entry == "frames" else synth.stacked_batch(b, h, w, seed=43, streams=streams)
    net.set_impl("tail_in_dec012")
    try:
        got = []
        for c in calls:
            got.append(_run(net, entry, inputs, *c))
            assert net.tail_in_dec012(), what + ": the forced form did not run"
            assert net.tail_form() == BlobNetInfer.TAIL_ROWS
        net.set_impl("tail_separate")
        for c, g in zip(calls, got):
            ref = _run(net, entry, inputs, *c)
            # (the parent's chain: the row tail, at 16x16 -- whose planes do not fit that launch's LDS plan -- the band tiles)
            assert not net.tail_in_dec012() and net.tail_form() == (BlobNetInfer.TAIL_BANDS + 3 if (h, w) == (16, 16) else BlobNetInfer.TAIL_ROWS), what
            _same(g, ref, b, c[1], f"{what} {c}")
    finally:
        net.set_impl("mfma")
    return got


# with and without the logits and mask outputs; max_boxes small enough to truncate; a cc threshold > 1
CALLS = [(1, 2048, True, True), (1, 8, False, False), (3, 2048, True, False)]


@pytest.mark.parametrize("wname", ["seed", "mixed"])
@pytest.mark.parametrize("hw", GRIDS, ids=[f"{h}x{w}" for h, w in GRIDS])
def test_bit_identical_to_the_two_launches(ctx, hw, wname):
    h, w = hw
    got = _compare(ctx, h, w, 3, wname, "frames", CALLS)
    boxes, counts, mask, logits = got[0]
    assert np.array_equal(mask, (logits > 0).astype(np.uint8))
    assert counts.sum() > 0 and 0 < mask.mean() < 1                      # (an empty or a full mask would compare nothing)
    if h >= 67:
        assert (got[1][1] > 8).any()                                     # the small max_boxes did truncate
        assert got[2][1].sum() < counts.sum()                     # the area threshold did drop components


@pytest.mark.parametrize("h,w", [(17, 20), (35, 60)])
def test_a_grid_outside_the_row_tiles_keeps_the_two_launches(ctx, weights_flat, h, w):
    """W % 8 != 0: neither the row tail nor this form takes the grid; forcing the form changes nothing."""
    b = 3
    net = BlobNetInfer(ctx, weights_flat, h, w, max_batch=b)
    frames, index = synth.carrier_batch(b, h, w, seed=43, streams=3)
    out = {}
    for impl in ("tail_in_dec012", "tail_separate"):
        net.set_impl(impl)
        try:
            out[impl] = net.filter_frames(frames, index, 1, max_boxes=2048, want_mask=True, want_logits=True)
            assert not net.tail_in_dec012() and net.tail_form() != BlobNetInfer.TAIL_ROWS
        finally:
            net.set_impl("mfma")
    _same(out["tail_in_dec012"], out["tail_separate"], b, 2048, f"{h}x{w}")


def test_stack_entry(ctx):
    _compare(ctx, 35, 64, 3, "seed", "stack", CALLS)


@pytest.mark.parametrize("hw", [(35, 64), (68, 120)], ids=["35x64", "68x120"])
def test_blob_like_weights(ctx, hw):
    got = _compare(ctx, hw[0], hw[1], 3, "blob", "frames", CALLS[:2])
    assert got[0][1].sum() > 0


def test_a_workgroup_takes_several_frames(ctx):
    """2 x CUs + 3 frames on min(batch, CUs) workgroups: t3 and the planes of a frame are overwritten by the next frame's tile
    requests, border zeros and scatter -- behind the barrier at the head of the frame loop."""
    b = 2 * ctx.info()["num_cu"] + 3
    got = _compare(ctx, 16, 24, b, "seed", "frames", [(1, 256, True, True), (2, 4, False, False)])
    assert (got[0][1] > 0).sum() > b // 2


def test_automatic_gate(ctx, weights_flat):
    """The default chain takes the form when the batch fills the chip (three quarters of a frame per CU, enc23_mfma's rule) and the
    call does not ask for the logits; never for a mixed batch of a model set or with per-model post-processing, forced or not."""
    h, w = 16, 24
    cu = ctx.info()["num_cu"]
    big, small = max(192, (3 * cu + 3) // 4), 3                           # (192 on the 256 CUs of an MI355X)
    net = BlobNetInfer(ctx, weights_flat, h, w, max_batch=big)
    fb, ib = synth.carrier_batch(big, h, w, seed=5, streams=4)
    fs, is_ = synth.carrier_batch(small, h, w, seed=5, streams=1)
    auto = net.filter_frames(fb, ib, 1, max_boxes=64, want_mask=True)
    assert net.tail_in_dec012()
    net.filter_frames(fb, ib, 1, max_boxes=64, want_mask=True, want_logits=True)
    assert not net.tail_in_dec012()                                      # (the logits keep the two launches and dact[2])
    net.filter_frames(fs, is_, 1, max_boxes=64, want_mask=True)
    assert not net.tail_in_dec012()
    net.set_impl("tail_separate")
    try:
        ref = net.filter_frames(fb, ib, 1, max_boxes=64, want_mask=True)
        assert not net.tail_in_dec012()
    finally:
        net.set_impl("mfma")
    _same(auto, ref, len(ib), 64, "automatic at a full batch")
    # per-model post-processing: the POST kernels are the two launches'
    net.set_post(0, logit_thresh=0.25)
    try:
        for impl in ("mfma", "tail_in_dec012"):
            net.set_impl(impl)
            net.filter_frames(fb, ib, 1, max_boxes=64)
            assert not net.tail_in_dec012() and net.tail_form() == BlobNetInfer.TAIL_ROWS
    finally:
        net.set_impl("mfma")
        net.reset_post(0)
    net.filter_frames(fb, ib, 1, max_boxes=64)
    assert net.tail_in_dec012()


def test_a_mixed_batch_of_a_model_set_never_takes_it(ctx, weights_flat):
    h, w, b = 16, 24, 192
    net = BlobNetInfer(ctx, [weights_flat, W.random_init(99)], h, w, max_batch=b)
    frames, index = synth.carrier_batch(b, h, w, seed=6, streams=4)
    ids = (np.arange(b) % 2).astype(np.uint8)
    for impl in ("mfma", "tail_in_dec012"):
        net.set_impl(impl)
        try:
            net.filter_frames(frames, index, 1, max_boxes=64, model_ids=ids)
            assert not net.tail_in_dec012() and net.tail_form() == BlobNetInfer.TAIL_ROWS
            net.filter_frames(frames, index, 1, max_boxes=64, model_ids=np.ones(b, np.uint8))   # a batch of ONE model of the set
            assert net.tail_in_dec012()
        finally:
            net.set_impl("mfma")
