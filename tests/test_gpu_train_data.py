"""Training from a device-resident data set on the GPU (include/covahip.h, "Training data"): the gather launch against numpy,
Contract D -- the data forms of step and eval are bit-identical to their pointer forms on the batches the samples describe --
for a solo trainer, a set, an evaluation, a plan with a post; the refusals; offsets past 32 bits; the epoch loop (fit_data is
fit on slide's windows, and resumes exactly under augmentation) and the command line."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import train as T, weights as W
from cova_amd.elements import BlobNetInfer, tfrecord_example

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, OVERFLOW = 1, 7


def _frames(seed, f, h, w):
    """frames u8 [f][h][w][4] and gt u8 [f][h][w]: half of the record bytes in 0..8 (around the clip at 6), half anywhere in
    0..255, byte 3 random; labels 0 / 1 with one in a hundred anywhere in 0..255 (the byte is stored as given)."""
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 9, (f, h, w, 4), dtype=np.uint8)
    frames = np.where(rng.random((f, h, w, 4)) < 0.5, low, rng.integers(0, 256, (f, h, w, 4), dtype=np.uint8)).astype(np.uint8)
    gt = rng.integers(0, 2, (f, h, w), dtype=np.uint8)
    gt = np.where(rng.random((f, h, w)) < 0.01, rng.integers(0, 256, (f, h, w), dtype=np.uint8), gt).astype(np.uint8)
    return frames, gt


def _batch(frames, gt, samples, packed):
    """The batch `samples` describe, in numpy.  packed: what the data set returns (bytes 0..2 clipped at 6, byte 3 zero);
    otherwise built from the frames as they were appended, for the pointer forms."""
    n, (_, h, w, _) = len(samples), frames.shape
    stack = np.empty((n, 4, h, w, 4), np.uint8)
    lab = np.empty((n, h, w), np.uint8)
    for b, s in enumerate(samples):
        sx = slice(None, None, -1) if s["flags"] & 1 else slice(None)
        sy = slice(None, None, -1) if s["flags"] & 2 else slice(None)
        for t in range(4):
            stack[b, t] = frames[s["frame"][t]][sy, sx]
        lab[b] = gt[s["label"]][sy, sx]
    if packed:
        stack = np.minimum(stack, 6)
        stack[..., 3] = 0
    return stack.reshape(n, 4 * h, w, 4), lab


def _samples(rows):
    out = np.zeros(len(rows), T.SAMPLE)
    for i, (frame, label, flags) in enumerate(rows):
        out[i] = (frame, label, flags)
    return out


def _mixed(n_frames, count, seed):
    """`count` samples that mix overlapping windows, strides 1 and 2, time reversal and the four mirror settings."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(count):
        s = 1 + (i % 3 == 1)
        k = int(rng.integers(3 * s, n_frames))
        fr = [k, k - s, k - 2 * s, k - 3 * s]
        if (i // 2) % 2:
            fr = fr[::-1]
        rows.append((fr, fr[0], i % 4))
    return _samples(rows)


def _state(tr):
    """Everything Contract D names of a solo trainer or a set, as bytes."""
    s = getattr(tr, "_set", tr)
    return [(s.grads(k).tobytes(), s.metrics(k), s.weights_bytes(k)) for k in range(s.n_models)] + [s.state_bytes(), list(s.step_counts)]


def _data(ctx, frames, gt, capacity=None):
    d = T.TrainData(ctx, frames.shape[1], frames.shape[2], capacity or frames.shape[0])
    assert d.append(frames, gt) == (0, frames.shape[0])
    return d


def _f32_bits(v):
    return np.asarray(v, np.float32).view(np.uint32).tolist()


# ------------------------------------------------------------------------------------------------ 1. gather against numpy
@pytest.mark.parametrize("h,w", [(16, 16), (17, 33), (24, 50), (45, 80)])      # 45x80: 15 workgroups per sample, the last partial
def test_gather_against_numpy(ctx, h, w):
    frames, gt = _frames(1, 15, h, w)
    assert frames.min() == 0 and frames.max() == 255
    d = T.TrainData(ctx, h, w, 15)
    d_fr, d_gt = ctx.malloc(6 * h * w * 4), ctx.malloc(6 * h * w)
    try:
        assert d.append(frames[:5], gt[:5]) == (0, 5)                      # host, device, host
        ctx.h2d(d_fr, frames[5:11])
        ctx.h2d(d_gt, gt[5:11])
        assert d.append_device(d_fr, d_gt, 6) == (5, 11)
        assert d.append(frames[11:], gt[11:]) == (11, 15) and d.frames == 15
        nine = _samples([([3, 2, 1, 0], 3, 0), ([14, 13, 12, 11], 14, 1), ([7, 5, 3, 1], 7, 2), ([4, 6, 8, 10], 4, 3),
                         ([9, 8, 7, 6], 2, 1),                            # label != frame[0]
                         ([5, 5, 5, 5], 5, 3),                            # one frame in all four slots
                         ([0, 0, 14, 14], 14, 2), ([12, 4, 10, 6], 0, 0), ([14, 0, 14, 0], 13, 3)])
        for samples in (nine, nine[3:4]):                                  # n = 9 and n = 1
            n = len(samples)
            want_stack, want_gt = _batch(frames, gt, samples, packed=True)
            stack, lab = d.gather(samples)                                 # host output
            assert stack.shape == (n, 4 * h, w, 4) and (stack == want_stack).all()
            assert (lab == want_gt).all()
            o_stack, o_gt = ctx.malloc(stack.nbytes), ctx.malloc(lab.nbytes)   # device output
            try:
                d.gather_device(samples, o_stack, o_gt)
                stack2, lab2 = np.full_like(stack, 0xAA), np.full_like(lab, 0xAA)
                ctx.d2h(stack2, o_stack)
                ctx.d2h(lab2, o_gt)
            finally:
                ctx.free(o_stack)
                ctx.free(o_gt)
            assert (stack2 == want_stack).all() and (lab2 == want_gt).all()
    finally:
        ctx.free(d_fr)
        ctx.free(d_gt)
        d.close()


# ------------------------------------------------------------------------------------------------ 1b. the host's choices
def _every_frame_mirrored(n_frames):
    """Every frame in slot 0 and as the label, under each of the four mirror settings; the other slots walk on."""
    return _samples([([f, (f + 1) % n_frames, (f + 2) % n_frames, (f + 3) % n_frames], f, m) for f in range(n_frames) for m in range(4)])


@pytest.mark.parametrize("shift", [1, 2, 3])
@pytest.mark.parametrize("h,w", [(16, 16), (17, 33)])
def test_append_device_from_an_unaligned_source(ctx, h, w, shift):
    """A device source off a 4-byte boundary is packed byte by byte instead of a record at a time."""
    f = 6
    frames, gt = _frames(20 + shift, f, h, w)
    assert frames[..., :3].min() == 0 and frames[..., :3].max() == 255 and len(np.unique(frames[..., 3])) > 200
    d = T.TrainData(ctx, h, w, f)
    d_fr, d_gt = ctx.malloc(frames.nbytes + 4), ctx.malloc(gt.nbytes + 4)
    try:
        assert d_fr % 4 == 0
        ctx.h2d(d_fr + shift, frames)
        ctx.h2d(d_gt + shift, gt)
        assert d.append_device(d_fr + shift, d_gt + shift, f) == (0, f)
        samples = _every_frame_mirrored(f)
        want_stack, want_gt = _batch(frames, gt, samples, packed=True)
        stack, lab = d.gather(samples)
        assert (stack == want_stack).all() and (lab == want_gt).all()
    finally:
        ctx.free(d_fr)
        ctx.free(d_gt)
        d.close()


def test_append_device_past_one_round_of_the_pack_grid(ctx):
    """One device append of 2^18 + 3 frames of 16x16: the pack kernel's grid stops at 2^18 workgroups of 256 macroblocks, so the
    macroblocks from index 2^26 on -- the last three frames -- are packed in the second round of its loop."""
    h = w = 16
    block_n = 1024                                                         # 1 MiB of frames
    total = (1 << 18) + 3
    assert total * h * w > (1 << 18) * 256 and (1 << 26) == (1 << 18) * h * w
    rng = np.random.default_rng(12)
    block = rng.integers(0, 256, (block_n, h, w, 4), dtype=np.uint8)
    block[::2, ..., :3] = rng.integers(0, 9, (block_n // 2, h, w, 3), dtype=np.uint8)    # every other frame around the clip at 6
    block_gt = rng.integers(0, 256, (block_n, h, w), dtype=np.uint8)
    d = T.TrainData(ctx, h, w, total)
    d_fr, d_gt = ctx.malloc(total * h * w * 4), ctx.malloc(total * h * w)
    try:
        for at in range(0, total, block_n):
            m = min(block_n, total - at)
            ctx.h2d(d_fr + at * h * w * 4, block[:m])
            ctx.h2d(d_gt + at * h * w, block_gt[:m])
        assert d.append_device(d_fr, d_gt, total) == (0, total) and d.frames == total
        edge = 1 << 18                                                     # the frame whose first macroblock is index 2^26
        samples = _samples([([0, 1, 2, 3], 0, 0), ([4, 5, 6, 7], 4, 3),
                            ([total - 1, total - 2, total - 3, total - 4], total - 1, 1),
                            ([edge - 1, edge, edge + 1, edge + 2], edge, 2), ([edge, edge - 1, edge - 2, edge - 3], edge - 1, 0),
                            ([edge - 1, edge - 1, edge, edge], total - 2, 3)])
        stack, lab = d.gather(samples)
        for b, smp in enumerate(samples):
            sx = slice(None, None, -1) if smp["flags"] & 1 else slice(None)
            sy = slice(None, None, -1) if smp["flags"] & 2 else slice(None)
            for t in range(4):
                want = np.minimum(block[int(smp["frame"][t]) % block_n][sy, sx], 6)
                want[..., 3] = 0
                assert (stack[b, t * h:(t + 1) * h] == want).all(), (b, t)
            assert (lab[b] == block_gt[int(smp["label"]) % block_n][sy, sx]).all(), b
    finally:
        ctx.free(d_fr)
        ctx.free(d_gt)
        d.close()


def test_host_append_and_gather_in_staging_rounds(ctx):
    """The developer's staging budget: a host append whose rounds end in the middle of a frame, the last one ragged, and a
    host-bound gather of 23 samples through a staging that holds 5.  Both equal numpy, as with the default budget."""
    h, w, f = 17, 33, 7
    frames, gt = _frames(13, f, h, w)
    hw = h * w
    d = T.TrainData(ctx, h, w, 2 * f)
    try:
        d.set_stage(2 * 1000)                                              # 1000 macroblocks a round: 3927 = 3 * 1000 + 927
        assert 1000 % hw != 0 and (f * hw) % 1000 not in (0, hw)
        assert d.append(frames, gt) == (0, f)
        d.set_stage(0)
        assert d.append(frames[::-1], gt[::-1]) == (f, 2 * f)              # the default budget: one round
        both, both_gt = np.concatenate([frames, frames[::-1]]), np.concatenate([gt, gt[::-1]])
        samples = np.concatenate([_every_frame_mirrored(2 * f)[::3], _mixed(2 * f, 4, 5)])
        assert len(samples) == 23
        want_stack, want_gt = _batch(both, both_gt, samples, packed=True)
        per = 17 * hw                                                      # a sample's staging: four slices of four bytes and a label byte
        for budget in (5 * per + per // 2, per - 1, 0):                    # 5 + 5 + 5 + 5 + 3 samples; one at a time; the default
            d.set_stage(budget)
            stack, lab = d.gather(samples)
            assert (stack == want_stack).all() and (lab == want_gt).all(), budget
    finally:
        d.close()


def test_device_gather_past_one_grid(ctx):
    """65535 + 9 samples to device memory: a launch's grid holds 65535, so the gather runs twice, the second time from the
    table's and the outputs' offsets.  285 MB of output, checked where the launches meet, at both ends and on every 4099th."""
    h = w = 16
    hw = h * w
    frames, gt = _frames(14, 15, h, w)
    n = 65535 + 9
    samples = np.tile(_mixed(15, 997, 15), n // 997 + 1)[:n]               # 997: a prime period, so the meeting point is mid-pattern
    assert {int(f) for f in samples["flags"]} == {0, 1, 2, 3}
    d = _data(ctx, frames, gt)
    o_stack, o_gt = ctx.malloc(n * 16 * hw), ctx.malloc(n * hw)
    try:
        d.gather_device(samples, o_stack, o_gt)
        runs = [(0, 4), (65535 - 8, 65535 + 8), (n - 4, n)] + [(i, i + 1) for i in range(4099, n, 4099)]
        for a, b in runs:
            want_stack, want_gt = _batch(frames, gt, samples[a:b], packed=True)
            stack, lab = np.full_like(want_stack, 0xAA), np.full_like(want_gt, 0xAA)
            ctx.d2h(stack, o_stack + a * 16 * hw)
            ctx.d2h(lab, o_gt + a * hw)
            assert (stack == want_stack).all() and (lab == want_gt).all(), (a, b)
    finally:
        ctx.free(o_stack)
        ctx.free(o_gt)
        d.close()


# ------------------------------------------------------------------------------------------------ 2. Contract D, step
@pytest.mark.parametrize("h,w,batch", [(17, 33, 4), (16, 16, 3)])
def test_contract_d_step(ctx, h, w, batch):
    frames, gt = _frames(2, 20, h, w)
    flat = T.init_weights(5)
    d = _data(ctx, frames, gt)
    a = T.Trainer(ctx, h, w, max_batch=4, weights_flat=flat, seed=3)      # default dropout
    b = T.Trainer(ctx, h, w, max_batch=4, weights_flat=flat, seed=3)
    try:
        samples = _mixed(20, 3 * batch, 7)
        assert {int(f) for f in samples["flags"]} == {0, 1, 2, 3}
        for i in range(3):
            s = samples[i * batch:(i + 1) * batch]
            la = a.step_data(d, s)
            lb = b.step(*_batch(frames, gt, s, packed=False))
            print(f"{h}x{w} step {i}: loss {la!r} / {lb!r}")
            assert _f32_bits(la) == _f32_bits(lb) and np.isfinite(la)
            assert _state(a) == _state(b)
        assert a.step_count == 3
    finally:
        a.close()
        b.close()
        d.close()


# ------------------------------------------------------------------------------------------------ 3. Contract D, set
def test_contract_d_set(ctx):
    h, w = 17, 33
    frames, gt = _frames(3, 24, h, w)
    flats = [T.init_weights(10 + k) for k in range(3)]
    d = _data(ctx, frames, gt)                                            # one data set for the three models
    a = T.TrainerSet(ctx, h, w, weights=flats, seeds=[4, 5, 6], max_batch=4)
    b = T.TrainerSet(ctx, h, w, weights=flats, seeds=[4, 5, 6], max_batch=4)
    try:
        at = 0
        for batches in ([2, 0, 3], [1, 4, 0]):
            per = []
            for n in batches:
                per.append(_mixed(24, 9, 20 + at)[at % 5:at % 5 + n] if n else None)
                at += 1
            before = _state(a)
            la = a.step_data(d, per)
            pairs = [(None, None) if s is None else _batch(frames, gt, s, packed=False) for s in per]
            lb = b.step([p[0] for p in pairs], [p[1] for p in pairs])
            assert _f32_bits(la) == _f32_bits(lb)
            after = _state(a)
            assert after == _state(b)
            for k, n in enumerate(batches):                                # the model sitting out is untouched
                assert (after[k] == before[k]) == (n == 0), (k, n)
                assert la[k] == 0.0 if n == 0 else la[k] > 0.0
        assert a.step_counts == [2, 1, 1]
    finally:
        a.close()
        b.close()
        d.close()


# ------------------------------------------------------------------------------------------------ 4. Contract D, eval
def _eval_raw(tr, data, samples, stack, gt):
    """covahip_train_eval_data (data given) or covahip_train_eval through the binding: (counts and loss, sample_loss, logits)."""
    n = len(samples)
    sl = np.full(n, np.nan, np.float32)
    lg = np.full((n, tr.h, tr.w), np.nan, np.float32)
    res = L.TrainEvalResult()
    if data is not None:
        L.check(tr._lib.covahip_train_eval_data(tr.handle, data.handle, samples.ctypes.data, n, sl.ctypes.data, lg.ctypes.data,
                                                C.byref(res), L.MEM_HOST), "covahip_train_eval_data", tr.ctx.handle)
    else:
        L.check(tr._lib.covahip_train_eval(tr.handle, stack.ctypes.data, gt.ctypes.data, n, sl.ctypes.data, lg.ctypes.data,
                                           C.byref(res), L.MEM_HOST), "covahip_train_eval", tr.ctx.handle)
    return (res.loss, res.tp, res.fp, res.fn, res.samples), sl.tobytes(), lg.tobytes()


def test_contract_d_eval(ctx):
    h, w = 17, 33
    frames, gt = _frames(4, 20, h, w)
    flat = T.init_weights(8)
    d = _data(ctx, frames, gt)
    samples = _mixed(20, 7, 9)                                             # n = 7 with max_batch 4: a chunk of 4 and one of 3
    stack, lab = _batch(frames, gt, samples, packed=False)
    a = T.Trainer(ctx, h, w, max_batch=4, weights_flat=flat, seed=1)
    b = T.Trainer(ctx, h, w, max_batch=4, weights_flat=flat, seed=1)
    sa = T.TrainerSet(ctx, h, w, weights=[flat, T.init_weights(9), T.init_weights(10)], max_batch=4)
    try:
        first = samples[:4]
        a.step_data(d, first)                                              # moving statistics that are not the initial ones
        b.step(*_batch(frames, gt, first, packed=False))
        got = _eval_raw(a, d, samples, None, None)
        want = _eval_raw(b, None, samples, stack, lab)
        assert got[0][4] == 7 and got == want
        ev = a.evaluate_data(d, samples, want_sample_loss=True, want_logits=True)
        assert ev["samples"] == 7 and ev["sample_loss"].tobytes() == want[1] and ev["logits"].tobytes() == want[2]
        # a table is scored as its windows are: forward, unmirrored, canonical order
        table = T.windows([(2, 9)], "overlap")
        plain = T.plain_samples(table)
        assert plain["frame"].tolist() == [[k, k - 1, k - 2, k - 3] for k in range(5, 9)] and not plain["flags"].any()
        assert a.evaluate_data(d, table) == b.evaluate(_batch(frames, gt, plain, packed=False))
        # a set, counts [3, 0, 4]
        evs = sa.evaluate_data(d, [samples[:3], None, samples[3:]], want_sample_loss=True, want_logits=True)
        ref = sa.evaluate([(stack[:3], lab[:3]), None, (stack[3:], lab[3:])], want_sample_loss=True, want_logits=True)
        assert [e["samples"] for e in evs] == [3, 0, 4]
        for e, r in zip(evs, ref):
            assert {k: v for k, v in e.items() if k not in ("sample_loss", "logits")} == {k: v for k, v in r.items()
                                                                                           if k not in ("sample_loss", "logits")}
            assert e["sample_loss"].tobytes() == r["sample_loss"].tobytes() and e["logits"].tobytes() == r["logits"].tobytes()
        # Contract B: the step after the evaluation is the step without it (b's evaluation was the pointer form's)
        c = T.Trainer(ctx, h, w, max_batch=4, weights_flat=flat, seed=1)
        try:
            c.step_data(d, first)
            nxt = samples[3:7]
            la, lc = a.step_data(d, nxt), c.step_data(d, nxt)
            assert _f32_bits(la) == _f32_bits(lc) and _state(a) == _state(c)
        finally:
            c.close()
    finally:
        a.close()
        b.close()
        sa.close()
        d.close()


# ------------------------------------------------------------------------------------------------ 5. plan and post carry over
def test_plan_and_post_carry_over(ctx):
    h, w = 17, 33
    frames, gt = _frames(5, 16, h, w)
    flat = T.init_weights(2)
    keep = np.ones((h, w), np.uint8)
    keep[:4, 5:20] = 0
    keep[11, :] = 0
    d = _data(ctx, frames, gt)
    trs = [T.Trainer(ctx, h, w, max_batch=4, weights_flat=flat, seed=2, freeze="encoder", bn_inference="all") for _ in range(2)]
    try:
        for tr in trs:
            tr.set_post(prob_thresh=0.6, keep=keep)
        samples = _mixed(16, 8, 11)
        for i in range(2):
            s = samples[4 * i:4 * i + 4]
            la = trs[0].step_data(d, s)
            lb = trs[1].step(*_batch(frames, gt, s, packed=False))
            assert _f32_bits(la) == _f32_bits(lb) and _state(trs[0]) == _state(trs[1])
        assert trs[0].plan["freeze"] == ("enc0", "enc1", "enc2", "enc3") and trs[0].get_post() is not None
    finally:
        for tr in trs:
            tr.close()
        d.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_change_nothing(ctx):
    h, w = 17, 33
    frames, gt = _frames(6, 10, h, w)
    small_fr, small_gt = _frames(6, 10, 16, 16)
    d = _data(ctx, frames, gt, capacity=12)
    other = _data(ctx, small_fr, small_gt)
    tr = T.Trainer(ctx, h, w, max_batch=4, weights_flat=T.init_weights(1), seed=0)
    lib = tr._lib
    try:
        good = _mixed(10, 5, 1)
        tr.step_data(d, good[:4])
        before = _state(tr)
        loss = C.c_float(-1.0)
        res = L.TrainEvalResult()

        def step(data, s, batch):
            return lib.covahip_train_step_data(tr.handle, data.handle, s.ctypes.data, batch, 1e-3, C.byref(loss))

        def ev(data, s, n):
            return lib.covahip_train_eval_data(tr.handle, data.handle, s.ctypes.data, n, None, None, C.byref(res), L.MEM_HOST)

        def bad(field, value, t=None):
            s = good[:4].copy()
            if t is None:
                s[field][2] = value
            else:
                s[field][2, t] = value
            return s

        cases = [bad("frame", -1, 3), bad("frame", 10, 0), bad("label", -1), bad("label", 10), bad("flags", 4), bad("flags", 1 << 31)]
        for s in cases:
            assert step(d, s, 4) == INVALID_ARG and ev(d, s, 4) == INVALID_ARG
            bt, lr, ls = np.array([4], np.int32), np.array([1e-3], np.float32), np.zeros(1, np.float32)
            assert lib.covahip_train_step_set_data(tr.handle, d.handle, s.ctypes.data, bt.ctypes.data, lr.ctypes.data, ls.ctypes.data) == INVALID_ARG
            st, lb = np.zeros((4, 4 * h, w, 4), np.uint8), np.zeros((4, h, w), np.uint8)
            assert lib.covahip_train_data_gather(d.handle, s.ctypes.data, 4, st.ctypes.data, lb.ctypes.data, L.MEM_HOST) == INVALID_ARG
        d_out = ctx.malloc(4 * 17 * h * w + 4)                                                        # a device stack off a 4-byte boundary
        try:
            assert lib.covahip_train_data_gather(d.handle, good.ctypes.data, 4, d_out + 2, d_out + 4 + 4 * 16 * h * w, L.MEM_DEVICE) == INVALID_ARG
            assert lib.covahip_train_data_gather(d.handle, good.ctypes.data, 4, d_out + 4, d_out + 4 + 4 * 16 * h * w, L.MEM_DEVICE) == 0
        finally:
            ctx.free(d_out)
        assert step(other, good[:4], 4) == INVALID_ARG and ev(other, good[:4], 4) == INVALID_ARG      # a 16x16 set, a 17x33 trainer
        assert step(d, good, 5) == INVALID_ARG                                                        # max_batch + 1
        assert ev(d, good, 5) == 0 and res.samples == 5                                               # eval takes any n
        assert step(d, good, 0) == INVALID_ARG
        assert lib.covahip_train_step_data(tr.handle, d.handle, None, 4, 1e-3, C.byref(loss)) == INVALID_ARG
        assert lib.covahip_train_step_data(tr.handle, None, good.ctypes.data, 4, 1e-3, C.byref(loss)) == INVALID_ARG
        assert lib.covahip_train_eval_data(tr.handle, d.handle, None, 4, None, None, C.byref(res), L.MEM_HOST) == INVALID_ARG
        with pytest.raises(ValueError):
            tr.step_data(other, good[:4])
        with pytest.raises(L.CovahipError):
            tr.step_data(d, good)
        assert loss.value == -1.0 and _state(tr) == before and tr.step_count == 1
        # an append past the capacity: 10 of 12 frames are taken
        first = C.c_int64(-1)
        assert lib.covahip_train_data_append(d.handle, frames.ctypes.data, gt.ctypes.data, 3, L.MEM_HOST, C.byref(first)) == OVERFLOW
        assert lib.covahip_train_data_append(d.handle, None, gt.ctypes.data, 1, L.MEM_HOST, C.byref(first)) == INVALID_ARG
        assert lib.covahip_train_data_append(d.handle, frames.ctypes.data, gt.ctypes.data, 0, L.MEM_HOST, C.byref(first)) == INVALID_ARG
        assert first.value == -1 and d.frames == 10
        with pytest.raises(L.CovahipError) as e:
            d.append(frames[:3], gt[:3])
        assert e.value.status == OVERFLOW and d.frames == 10
        assert d.append(frames[:2], gt[:2]) == (10, 12)
        h_out = C.c_void_p()
        for args in ((15, 16, 4), (16, 1025, 4), (16, 16, 0), (16, 16, 1 << 31)):
            assert lib.covahip_train_data_create(ctx.handle, *args, C.byref(h_out)) == INVALID_ARG and not h_out.value
        # and the trainer still trains, as one that saw none of this
        twin = T.Trainer(ctx, h, w, max_batch=4, weights_flat=T.init_weights(1), seed=0)
        try:
            twin.step_data(d, good[:4])
            assert _f32_bits(tr.step_data(d, good[1:5])) == _f32_bits(twin.step_data(d, good[1:5])) and _state(tr) == _state(twin)
        finally:
            twin.close()
    finally:
        tr.close()
        d.close()
        other.close()


# ------------------------------------------------------------------------------------------------ 7. offsets past 32 bits
def test_offsets_past_32_bits(ctx):
    h = w = 16
    block_n, rounds = 1 << 16, 130
    total = rounds * block_n + 3                                           # 8.5 M frames: 4.4 GB of records, 2.2 GB of labels
    assert total * h * w * 2 > 1 << 32 and total * h * w > 1 << 31
    rng = np.random.default_rng(7)
    block = rng.integers(0, 9, (block_n, h, w, 4), dtype=np.uint8)
    block_gt = rng.integers(0, 256, (block_n, h, w), dtype=np.uint8)
    tail, tail_gt = _frames(8, 3, h, w)
    d = T.TrainData(ctx, h, w, total)
    d_fr, d_gt = ctx.malloc(block.nbytes), ctx.malloc(block_gt.nbytes)
    try:
        ctx.h2d(d_fr, block)
        ctx.h2d(d_gt, block_gt)
        for i in range(rounds):
            assert d.append_device(d_fr, d_gt, block_n) == (i * block_n, (i + 1) * block_n)
        assert d.append(tail, tail_gt) == (total - 3, total) and d.frames == total
        past = (1 << 32) // (h * w * 2) + 5                                # a frame whose records start just past 4 GiB
        samples = _samples([([total - 1, total - 2, total - 3, total - 4], total - 1, 3), ([3, 2, 1, 0], 3, 0),
                            ([past, past - 1, total - 2, 0], past, 1)])
        stack, lab = d.gather(samples)

        def frame(i):
            return (tail[i - (total - 3)], tail_gt[i - (total - 3)]) if i >= total - 3 else (block[i % block_n], block_gt[i % block_n])

        for b, s in enumerate(samples):
            sx = slice(None, None, -1) if s["flags"] & 1 else slice(None)
            sy = slice(None, None, -1) if s["flags"] & 2 else slice(None)
            for t in range(4):
                want = np.minimum(frame(int(s["frame"][t]))[0][sy, sx], 6)
                want[..., 3] = 0
                assert (stack[b, t * h:(t + 1) * h] == want).all(), (b, t)
            assert (lab[b] == frame(int(s["label"]))[1][sy, sx]).all(), b
    finally:
        ctx.free(d_fr)
        ctx.free(d_gt)
        d.close()


# ------------------------------------------------------------------------------------------------ 8. the old epoch loop
def test_fit_data_on_skip_windows_is_fit_on_slide(ctx):
    h = w = 16
    frames, gt = _frames(9, 26, h, w)
    flat = T.init_weights(3)
    d = _data(ctx, frames, gt)
    a = T.Trainer(ctx, h, w, max_batch=4, weights_flat=flat, seed=6)
    b = T.Trainer(ctx, h, w, max_batch=4, weights_flat=flat, seed=6)
    try:
        ha = a.fit((T.slide(frames, gt)), epochs=2, batch=4)               # 6 stacks: a batch of 4 and a partial one of 2
        lines = []
        hb = b.fit_data(d, T.windows([(0, 26)], "skip"), epochs=2, batch=4, log=lines.append)
        assert ha == hb and a.weights_bytes() == b.weights_bytes() and a.state_bytes() == b.state_bytes()
        assert a.step_count == b.step_count == 4
        assert len(lines) == 2 and all(ln.endswith(" windows 6") for ln in lines)
    finally:
        a.close()
        b.close()
        d.close()


# ------------------------------------------------------------------------------------------------ 9. exact resume
def test_exact_resume_with_augmentation(ctx, tmp_path):
    h = w = 16
    frames, gt = _frames(10, 30, h, w)
    flat = T.init_weights(4)
    d = _data(ctx, frames, gt)
    segs = [(0, 17), (17, 30)]
    train, val = T.split_frames_tail(segs, 0.2)
    kw = dict(strides=(1, 2), shuffle=True, flip="xy", reverse=True, data_seed=77, val_table=T.windows(val, "overlap", (1, 2)))
    table = T.windows(train, "overlap", (1, 2))
    assert train == [(0, 17), (17, 24)] and len(table) == 14 + 4
    whole = T.Trainer(ctx, h, w, max_batch=4, weights_flat=flat, seed=1)
    first = T.Trainer(ctx, h, w, max_batch=4, weights_flat=flat, seed=1)
    rest = T.Trainer(ctx, h, w, max_batch=4, weights_flat=T.init_weights(99), seed=5)     # the state comes from the checkpoint
    try:
        hist = whole.fit_data(d, table, epochs=3, batch=4, **kw)
        ck = tmp_path / "run.cvhs"
        h0 = first.fit_data(d, table, epochs=1, batch=4, checkpoint=ck, **kw)
        start = rest.load_state(ck)
        assert start == 1
        h12 = rest.fit_data(d, table, epochs=3, batch=4, start_epoch=start, **kw)
        assert h0 + h12 == hist and "val_iou" in hist[0]
        assert rest.weights_bytes() == whole.weights_bytes() and rest.state_bytes() == whole.state_bytes()
        assert whole.step_count == 3 * 5
        # the epochs did differ: without the augmentation the same run ends elsewhere
        plain = T.Trainer(ctx, h, w, max_batch=4, weights_flat=flat, seed=1)
        try:
            plain.fit_data(d, table, epochs=3, batch=4, strides=(1, 2), data_seed=77, val_table=kw["val_table"])
            assert plain.weights_bytes() != whole.weights_bytes()
        finally:
            plain.close()
    finally:
        whole.close()
        first.close()
        rest.close()
        d.close()


# ------------------------------------------------------------------------------------------------ 10. command line
def test_command_line(ctx, tmp_path):
    h = w = 16
    fa, fb = 14, 9
    frames, gt = _frames(11, fa + fb, h, w)
    gt &= 1
    paths = [tmp_path / "a.tfrecord", tmp_path / "b.tfrecord"]
    for path, sl in zip(paths, (slice(0, fa), slice(fa, fa + fb))):
        with open(path, "wb") as f:
            for i in range(sl.start, sl.stop):
                f.write(tfrecord_example(frames[i:i + 1], gt[i:i + 1]))

    def run(*args):
        r = subprocess.run([sys.executable, "-m", "cova_amd.train", *args, "--h-mb", str(h), "--w-mb", str(w)], cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r

    n_windows = (fa - 3) + (fb - 3)
    outs = [tmp_path / "one.cvhw", tmp_path / "two.cvhw"]
    for out in outs:
        r = run(str(paths[0]), str(paths[1]), "-o", str(out), "--windows", "overlap", "--flip", "x", "--shuffle", "--epochs", "2")
        assert f"{fa + fb} frames -> {n_windows} windows of {h}x{w}" in r.stderr, r.stderr
        assert r.stderr.count(f" windows {n_windows}\n") == 2, r.stderr    # the two epoch lines
    assert outs[0].read_bytes() == outs[1].read_bytes()
    net = BlobNetInfer(ctx, W.from_bytes(outs[0].read_bytes()), h, w, max_batch=4)
    _, mask = net.infer(T.slide(frames, gt)[0][:4], want_logits=False)
    assert mask.shape == (4, h, w)
    r = run("--eval-only", str(outs[0]), str(paths[0]), str(paths[1]), "--windows", "overlap")
    ev = json.loads(r.stdout.strip().splitlines()[-1])
    assert ev["samples"] == n_windows and ev["weights"] == str(outs[0]) and 0.0 <= ev["iou"] <= 1.0
