"""The forward kernels take their weight fragments as global loads that stay in flight across barriers and are waited for
fragment by fragment ("Weight loads are global loads").  A wait that is one load short shows as a product
with a stale operand, in the frame's first tile only -- so the chain that holds those kernels (enc1_mfma, enc23_mfma,
dec012_mfma, dec3cc_rows_mfma) is compared bit for bit, on logits, mask, counts and boxes, against the forms that load their
weights once in front of everything: decoder blocks 0..2 as three launches ("dec_separate"), encoder levels 2 + 3 as two
("enc23_separate"), the band-tile tail ("tail_band_tiles").

Shapes: the smallest grid the geometry admits, odd grids with pad rows and columns, rows of one and two tail tiles, the
benchmark's grid, and more frames than workgroups (the frame loop re-requests the weights while LDS is reused).  A small batch
takes levels 2 + 3 as two launches by default, so every case also runs with the one-launch form forced ("enc23_force")."""
import numpy as np
import pytest

from cova_amd import synth
from cova_amd import weights as W
from cova_amd.elements import BlobNetInfer

pytestmark = pytest.mark.gpu

REFERENCE_FORMS = ("dec_separate", "enc23_separate", "tail_band_tiles")
MAX_BOXES = 256


def _mixed_gamma(seed):
    """Every second BN gamma of every encoder level negative: the kernels' non-ALLPOS instantiations."""
    t = W.unflatten(W.random_init(seed))
    for i in range(4):
        t[f"enc{i}.bn.gamma"][::2] *= -1.0
    return W.flatten(t)


def _run(net, impl, frames, index, ids):
    net.set_impl(impl)
    try:
        return net.filter_frames(frames, index, 1, max_boxes=MAX_BOXES, want_mask=True, want_logits=True, model_ids=ids)
    finally:
        net.set_impl("mfma")


def _assert_same_bits(got, ref, what):
    boxes, counts, mask, logits = got
    boxes_r, counts_r, mask_r, logits_r = ref
    assert logits.tobytes() == logits_r.tobytes(), what
    assert mask.tobytes() == mask_r.tobytes(), what
    assert counts.tobytes() == counts_r.tobytes(), what
    for i in range(len(counts)):       # (the slots behind a frame's count hold nothing)
        n = min(int(counts[i]), MAX_BOXES)
        assert boxes[i, :n].tobytes() == boxes_r[i, :n].tobytes(), (what, i)


def _check(ctx, models, ids, h, w, b, frames, index):
    net = BlobNetInfer(ctx, models, h, w, max_batch=b)
    refs = {impl: _run(net, impl, frames, index, ids) for impl in REFERENCE_FORMS}
    for form in ("mfma", "enc23_force"):
        got = _run(net, form, frames, index, ids)
        for impl, ref in refs.items():
            _assert_same_bits(got, ref, (form, impl))
    again = _run(net, "mfma", frames, index, ids)      # the same workspace a second time: borders, ring and tiles reused
    _assert_same_bits(again, refs["dec_separate"], ("mfma, second run", "dec_separate"))
    assert refs["dec_separate"][3].size == b * h * w and np.isfinite(refs["dec_separate"][3]).all()


# (h, w, b, mixed-sign gamma); b < 0: that many frames more than two per CU
CASES = [(16, 16, 3, False), (17, 20, 3, True), (35, 60, 8, False), (67, 120, 5, True), (68, 120, 4, False), (16, 16, -3, True)]


@pytest.mark.parametrize("h,w,b,mixed", CASES, ids=[f"{h}x{w}-b{b if b > 0 else '2cu+3'}-{'mixed' if m else 'pos'}" for h, w, b, m in CASES])
def test_default_chain_matches_the_separate_forms_bitwise(ctx, weights_flat, h, w, b, mixed):
    if b < 0:
        b = 2 * ctx.info()["num_cu"] - b
    frames, index = synth.carrier_batch(b, h, w, seed=61, streams=min(b, 3))
    _check(ctx, _mixed_gamma(77) if mixed else weights_flat, None, h, w, b, frames, index)


@pytest.mark.parametrize("h,w,b", [(68, 120, 6), (16, 16, -3)], ids=["68x120-b6", "16x16-b2cu+3"])
def test_two_models_alternating_per_stack(ctx, weights_flat, h, w, b):
    """A set of two models (one of them with mixed-sign gammas), stack i served by model i & 1 (drawn at random where a
    workgroup takes more than one frame): a workgroup that takes a second item finds another model there and loads its fragments and constants again.  (A carrier frame goes through level 0
    with the model of its stack, so every stack has four frames of its own.)"""
    if b < 0:
        b = 2 * ctx.info()["num_cu"] - b
    ids = (np.arange(b) & 1).astype(np.uint8)
    if b > 2 * ctx.info()["num_cu"]:       # frames k and k + grid share a workgroup, and the grid is even: there the ids are drawn
        ids = np.random.default_rng(5).integers(0, 2, b).astype(np.uint8)
    frames = synth.carrier_frames(4 * b, h, w, seed=67)
    index = np.arange(4 * b, dtype=np.int32).reshape(b, 4)[:, ::-1].copy()
    _check(ctx, [weights_flat, _mixed_gamma(78)], ids, h, w, b, frames, index)
