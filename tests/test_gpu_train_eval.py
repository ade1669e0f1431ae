"""Held-out evaluation and exact resume of BlobNet training on the GPU (covahip_train_eval*, covahip_train_*_state): the
inference-mode forward against torch in f64, and the three contracts of include/covahip.h, "Evaluation and resume" -- A: a
sample's result depends on the sample and the model only; B: evaluation is invisible to training; C: a saved state continues
bit for bit in any trainer of the same shape -- then the epoch loop and the command line on top of them."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cova_amd import _lib as L
from cova_amd import train as T, weights as W
from cova_amd.elements import BlobNetInfer, Context, tfrecord_example
from tests import torch_blobnet as TB
from tests import torch_blobnet_train as TT
from tests.golden_util import GOLDEN, blobnet_tolerance
from tests.test_gpu_train import METRIC_BAND, _streams

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOOTH = 100.0
# max |logit - f64 reference| measured on the MI355X over CASES: 5.9e-6 (at 45x80; DESIGN.md, "Evaluation and resume"); torch in
# float32 on a CPU differs from f64 by 4.2e-6 on the same inputs.  The assertion allows ten times the measured value.
LOGIT_BOUND = 5.9e-5
CASES = [(45, 80, 5), (17, 33, 7), (68, 120, 3), (16, 16, 4), (24, 50, 4)]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _weights(seed):
    """init_weights(seed) with every BN gamma / moving variance redrawn from U(0.5, 1.5) and every beta / moving mean from
    N(0, 0.1): with the default moving statistics 0 / 1 a wrong BN path would go unnoticed."""
    flat = T.init_weights(seed).astype(np.float32).copy()
    rng = np.random.default_rng(1000 + seed)
    off = 0
    for name, shape in W.tensor_specs().items():
        n = int(np.prod(shape))
        if name.endswith((".bn.gamma", ".bn.var")):
            flat[off:off + n] = rng.uniform(0.5, 1.5, n)
        elif name.endswith((".bn.beta", ".bn.mean")):
            flat[off:off + n] = rng.normal(0.0, 0.1, n)
        off += n
    assert off == W.N_PARAMS
    return flat


def _reference(flat, stack, gt, h, w):
    """(logits, per-sample loss) in f64: tests/torch_blobnet.py's forward and the header's loss formula."""
    logit = TB.forward(flat, stack, h, w, dtype=torch.float64)
    assert logit.dtype == np.float64
    p = 1.0 / (1.0 + np.exp(-logit))
    y = gt.astype(np.float64)
    inter = (y * p).sum(axis=(1, 2))
    s = (y + p).sum(axis=(1, 2))
    return logit, (1.0 - (inter + SMOOTH) / (s - inter + SMOOTH)) * SMOOTH


def _assert_counts(ev_counts, logit_ref, gt):
    """The rule of tests/test_gpu_train.py::_assert_metrics, with FN checked the same way."""
    tp, fp, fn = ev_counts
    lab = gt.astype(bool)
    pos = logit_ref > 0
    near = np.abs(logit_ref) < METRIC_BAND
    print(f"  pixels in the band: {int(near.sum())} (cap {max(2, 0.005 * near.size):.0f})")
    assert near.sum() <= max(2, 0.005 * near.size), int(near.sum())
    assert tp + fn == int(lab.sum()), (ev_counts, int(lab.sum()))
    assert abs(tp - int((pos & lab).sum())) <= int((near & lab).sum()), (ev_counts, int((pos & lab).sum()))
    assert abs(fp - int((pos & ~lab).sum())) <= int((near & ~lab).sum()), (ev_counts, int((pos & ~lab).sum()))


def _eval_raw(tr, stack, gt):
    """covahip_train_eval through the binding, keeping the integer counts: (result struct, sample_loss, logits)."""
    n = stack.shape[0]
    sl = np.full(n, np.nan, np.float32)
    lg = np.full((n, tr.h, tr.w), np.nan, np.float32)
    res = L.TrainEvalResult()
    stack, gt = np.ascontiguousarray(stack), np.ascontiguousarray(gt)
    L.check(tr._lib.covahip_train_eval(tr.handle, stack.ctypes.data, gt.ctypes.data, n, sl.ctypes.data, lg.ctypes.data,
                                       C.byref(res), L.MEM_HOST), "covahip_train_eval", tr.ctx.handle)
    return res, sl, lg


def _res_tuple(res):
    return (res.loss, res.tp, res.fp, res.fn, res.samples)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_against_f64(what, res, sl, lg, flat, stack, gt, h, w):
    logit_ref, loss_ref = _reference(flat, stack, gt, h, w)
    rel = np.abs(sl.astype(np.float64) - loss_ref) / np.abs(loss_ref)
    mean_rel = abs(res.loss - loss_ref.mean()) / abs(loss_ref.mean())
    dl = float(np.abs(lg.astype(np.float64) - logit_ref).max())
    print(f"{what}: per-sample loss rel {rel.max():.2e}, mean loss rel {mean_rel:.2e}, max |dlogit| {dl:.3e}")
    assert res.samples == stack.shape[0]
    assert (rel <= TT.BOUNDS["loss"]).all(), rel
    assert mean_rel <= TT.BOUNDS["loss"], mean_rel
    _assert_counts((res.tp, res.fp, res.fn), logit_ref, gt)
    assert dl <= LOGIT_BOUND, dl
    return dl


# ------------------------------------------------------------------------------------------------ 1. against f64
def test_evaluation_matches_torch_f64(ctx):
    flat = _weights(3)
    worst = 0.0
    for h, w, b in CASES:
        stack, gt = TT.sample_batch(h, w, b, 5)
        tr = T.Trainer(ctx, h, w, max_batch=3, weights_flat=flat, seed=0)
        try:
            res, sl, lg = _eval_raw(tr, stack, gt)       # chunks of 3 and a partial last chunk
            ev = tr.evaluate((stack, gt))
        finally:
            tr.close()
        worst = max(worst, _check_against_f64(f"{h}x{w} b={b}", res, sl, lg, flat, stack, gt, h, w))
        tp, fp, fn = res.tp, res.fp, res.fn
        assert ev == {"loss": res.loss, "precision": tp / max(1, tp + fp), "recall": tp / max(1, tp + fn),
                      "iou": tp / max(1, tp + fp + fn), "samples": b}
    print(f"max |logit - f64| over the five cases: {worst:.3e}")


# ------------------------------------------------------------------------------------------------ 2. Contract A
@pytest.mark.parametrize("h,w,n", CASES[:2])
def test_contract_a_a_sample_depends_on_itself_and_the_model_only(ctx, h, w, n):
    flat = _weights(3)
    stack, gt = TT.sample_batch(h, w, n, 5)

    def solo(mb, st, g):
        tr = T.Trainer(ctx, h, w, max_batch=mb, weights_flat=flat, seed=0)
        try:
            return tr, _eval_raw(tr, st, g)
        except Exception:
            tr.close()
            raise

    tr, (res0, sl0, lg0) = solo(3, stack, gt)
    assert np.isfinite(sl0).all() and np.isfinite(lg0).all()
    # the loss is the double sum of the per-sample values in sample order
    acc = 0.0
    for v in sl0:
        acc += float(v)
    assert res0.loss == acc / n
    # from device memory, same trainer
    nb = [stack.nbytes, gt.nbytes, 4 * n, 4 * n * h * w]
    ptrs = [ctx.malloc(b) for b in nb]
    try:
        ctx.h2d(ptrs[0], stack)
        ctx.h2d(ptrs[1], gt)
        res = L.TrainEvalResult()
        L.check(tr._lib.covahip_train_eval(tr.handle, ptrs[0], ptrs[1], n, ptrs[2], ptrs[3], C.byref(res), L.MEM_DEVICE),
                "covahip_train_eval", ctx.handle)
        sl, lg = np.empty(n, np.float32), np.empty((n, h, w), np.float32)
        ctx.d2h(sl, ptrs[2])
        ctx.d2h(lg, ptrs[3])
    finally:
        for p in ptrs:
            ctx.free(p)
        tr.close()
    assert _res_tuple(res) == _res_tuple(res0) and (_bits(sl) == _bits(sl0)).all() and (_bits(lg) == _bits(lg0)).all()
    # other chunkings
    for mb in (1, n):
        tr, (res, sl, lg) = solo(mb, stack, gt)
        tr.close()
        assert _res_tuple(res) == _res_tuple(res0), (mb, _res_tuple(res), _res_tuple(res0))
        assert (_bits(sl) == _bits(sl0)).all() and (_bits(lg) == _bits(lg0)).all(), mb
    # reversed order: every sample keeps its bits; the mean is then summed in the new order
    tr, (res, sl, lg) = solo(3, stack[::-1], gt[::-1])
    tr.close()
    assert (res.tp, res.fp, res.fn, res.samples) == (res0.tp, res0.fp, res0.fn, n)
    assert (_bits(sl) == _bits(sl0[::-1])).all() and (_bits(lg) == _bits(lg0[::-1])).all()
    acc = 0.0
    for v in sl0[::-1]:
        acc += float(v)
    assert res.loss == acc / n
    # as model 1 of a three-model set whose neighbours hold other weights and other sample counts, one of them none
    others = TT.sample_batch(h, w, 4, 6)
    ts = T.TrainerSet(ctx, h, w, weights=[_weights(4), flat, _weights(5)], max_batch=3)
    try:
        evs = ts.evaluate([others, (stack, gt), None], want_sample_loss=True, want_logits=True)
        evs2 = ts.evaluate([None, (stack, gt), (others[0][:2], others[1][:2])], want_sample_loss=True, want_logits=True)
    finally:
        ts.close()
    for e in (evs, evs2):
        assert e[1]["loss"] == res0.loss and e[1]["samples"] == n
        assert (_bits(e[1]["sample_loss"]) == _bits(sl0)).all() and (_bits(e[1]["logits"]) == _bits(lg0)).all()
        tp, fp, fn = res0.tp, res0.fp, res0.fn
        assert (e[1]["precision"], e[1]["recall"], e[1]["iou"]) == (tp / max(1, tp + fp), tp / max(1, tp + fn), tp / max(1, tp + fp + fn))
    assert [evs[2][k] for k in ("loss", "precision", "recall", "iou", "samples")] == [0.0, 0.0, 0.0, 0.0, 0]
    assert evs[2]["logits"].shape == (0, h, w) and evs[2]["sample_loss"].shape == (0,)
    assert evs[0]["samples"] == 4 and evs2[2]["samples"] == 2
    assert (_bits(evs2[2]["logits"]) != 0).any()


# ------------------------------------------------------------------------------------------------ 3. Contract B
def _solo_snap(tr):
    return _bits(tr.grads()).copy(), tr.metrics(), _bits(tr.weights()).copy()


def _same(a, b):
    return all((x == y).all() if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def test_contract_b_evaluation_is_invisible_to_training_solo(ctx):
    h, w, mb = 24, 50, 3
    flat = T.init_weights(12)
    steps = [TT.sample_batch(h, w, b, 70 + k) for k, b in enumerate((3, 2, 3))]
    held = TT.sample_batch(h, w, 5, 79)
    a = T.Trainer(ctx, h, w, max_batch=mb, weights_flat=flat, seed=8, dropout=0.2)
    b = T.Trainer(ctx, h, w, max_batch=mb, weights_flat=flat, seed=8, dropout=0.2)
    try:
        ev0 = b.evaluate(held)                         # before any step: the weights the trainer was created with
        assert ev0["samples"] == 5 and (_bits(b.grads()) == 0).all() and b.metrics() == (0, 0, 0)
        for k, (s, g) in enumerate(steps):
            la, lb = a.step(s, g), b.step(s, g)
            sa, sb = _solo_snap(a), _solo_snap(b)
            assert la == lb and _same(sa, sb), f"step {k}"
            for _ in range((1, 2, 0)[k]):              # one evaluation after s0, two after s1
                ev = b.evaluate(held)
                assert _same(_solo_snap(b), sb) and b.step_count == a.step_count
                assert ev["loss"] != ev0["loss"]       # (the weights moved: the evaluation sees them)
    finally:
        a.close()
        b.close()


def test_contract_b_evaluation_is_invisible_to_training_set(ctx):
    h, w, mb, K = 17, 33, 3, 3
    flats = [T.init_weights(20 + k) for k in range(K)]
    sizes = [(3, 2, 1), (2, 0, 3), (1, 3, 2)]         # model 1 sits s1 out
    steps = [[TT.sample_batch(h, w, b, 100 + 10 * i + k) if b else None for k, b in enumerate(bs)] for i, bs in enumerate(sizes)]
    held = [TT.sample_batch(h, w, n, 150 + k) for k, n in enumerate((4, 2, 5))]

    def snap(ts):
        return [(_bits(ts.grads(k)).copy(), ts.metrics(k), _bits(ts.weights(k)).copy()) for k in range(K)]

    a = T.TrainerSet(ctx, h, w, weights=flats, seeds=[5, 6, 7], max_batch=mb, dropout=0.2)
    b = T.TrainerSet(ctx, h, w, weights=flats, seeds=[5, 6, 7], max_batch=mb, dropout=0.2)
    try:
        for i, st in enumerate(steps):
            xs, ys = [None if r is None else r[0] for r in st], [None if r is None else r[1] for r in st]
            la, lb = a.step(xs, ys, [1e-3, 2e-3, 5e-4]), b.step(xs, ys, [1e-3, 2e-3, 5e-4])
            sa, sb = snap(a), snap(b)
            assert la == lb and all(_same(x, y) for x, y in zip(sa, sb)), f"step {i}"
            for _ in range((1, 2, 0)[i]):
                b.evaluate(held)
                assert all(_same(x, y) for x, y in zip(snap(b), sb)) and b.step_counts == a.step_counts
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 4. moving statistics
def test_moving_statistics_are_what_is_read(ctx):
    h, w, mb = 17, 33, 4
    flat = _weights(6)
    held = TT.sample_batch(h, w, 5, 41)
    tr = T.Trainer(ctx, h, w, max_batch=mb, weights_flat=flat, seed=1, dropout=0.2)
    try:
        res0, sl0, lg0 = _eval_raw(tr, *held)
        for k in range(3):
            tr.step(*TT.sample_batch(h, w, mb, 42 + k), lr=0.0)
        now = tr.weights()
        mk = T.trainable_mask()
        assert (_bits(now[mk]) == _bits(flat[mk])).all() and (now[~mk] != flat[~mk]).mean() > 0.9
        res, sl, lg = _eval_raw(tr, *held)
    finally:
        tr.close()
    assert res.loss != res0.loss and (_bits(lg) != _bits(lg0)).mean() > 0.9
    _check_against_f64("after 3 steps at lr = 0", res, sl, lg, now, *held, h, w)


# ------------------------------------------------------------------------------------------------ 5. serving agrees
@pytest.mark.parametrize("h,w,n", [(45, 80, 5), (68, 120, 3)])
def test_serving_agrees_with_the_evaluation(ctx, h, w, n):
    flat = _weights(3)
    stack, gt = TT.sample_batch(h, w, n, 5)
    tr = T.Trainer(ctx, h, w, max_batch=3, weights_flat=flat, seed=0)
    try:
        _, _, lg = _eval_raw(tr, stack, gt)
        exported = tr.weights()
    finally:
        tr.close()
    net = BlobNetInfer(ctx, exported, h, w, max_batch=n)
    logits, _ = net.infer(stack)
    atol, rtol = blobnet_tolerance(lg)
    err = np.abs(logits - lg)
    print(f"{h}x{w}: max |fp16 serving - evaluation| {err.max():.3e}, atol {atol:.3e}")
    assert (err <= atol + rtol * np.abs(lg)).all(), float((err - atol - rtol * np.abs(lg)).max())


# ------------------------------------------------------------------------------------------------ 6. Contract C
def test_contract_c_exact_resume_solo(ctx):
    h, w, mb = 17, 33, 4
    steps = [TT.sample_batch(h, w, b, 200 + k) for k, b in enumerate((4, 3, 4, 2, 4, 4, 3))]
    a = T.Trainer(ctx, h, w, max_batch=mb, weights_flat=T.init_weights(30), seed=77, dropout=0.2)
    b = T.Trainer(ctx, h, w, max_batch=mb, weights_flat=T.init_weights(99), seed=123456789, dropout=0.2)
    try:
        for s, g in steps[:3]:
            a.step(s, g, 2e-3)
        blob = a.state_bytes(epoch=41)
        hdr = T.read_state_header(blob)
        assert (hdr["n_models"], hdr["n_params"], hdr["h_mb"], hdr["w_mb"], hdr["user_tag"]) == (1, W.N_PARAMS, h, w, 41)
        assert hdr["steps"] == [3] and hdr["seeds"] == [77] and hdr["dropout"] == np.float32(0.2)
        b.step(*steps[5], 1e-3)                        # b has a past of its own
        assert b.load_state_bytes(blob) == 41 and b.step_count == 3
        assert (_bits(b.grads()) == 0).all() and b.metrics() == (0, 0, 0)
        assert (_bits(b.weights()) == _bits(a.weights())).all()
        for k, (s, g) in enumerate(steps[3:6]):
            la, lb = a.step(s, g, 1e-3), b.step(s, g, 1e-3)
            assert la == lb and _same(_solo_snap(a), _solo_snap(b)), f"step {3 + k}"
        assert a.state_bytes(5) == b.state_bytes(5)
        # refused blobs leave the trainer untouched
        bad = bytearray(blob)
        bad[64 + 16 + 4 * 1000] ^= 1
        for data, status in ((bytes(bad), 8), (blob[:-100], 8), (blob[:30], 8), (blob + blob[-4:], 8)):
            with pytest.raises(L.CovahipError) as e:
                b.load_state_bytes(data)
            assert e.value.status == status
        la, lb = a.step(*steps[6], 1e-3), b.step(*steps[6], 1e-3)
        assert la == lb and _same(_solo_snap(a), _solo_snap(b)) and b.step_count == 7
    finally:
        a.close()
        b.close()


def test_contract_c_exact_resume_set(ctx):
    h, w, mb, K = 45, 80, 4, 3
    lrs = [1e-3, 5e-4, 2e-3]
    sizes = [(4, 1, 3), (4, 0, 3), (4, 1, 3), (4, 1, 3), (4, 1, 0), (4, 1, 3), (2, 1, 3)]      # model 1, later model 2, sit a step out
    steps = [[TT.sample_batch(h, w, n, 300 + 10 * i + k) if n else None for k, n in enumerate(bs)] for i, bs in enumerate(sizes)]

    def step(ts, st):
        return ts.step([None if r is None else r[0] for r in st], [None if r is None else r[1] for r in st], lrs)

    def snap(ts):
        return [(_bits(ts.grads(k)).copy(), ts.metrics(k), _bits(ts.weights(k)).copy()) for k in range(K)]

    a = T.TrainerSet(ctx, h, w, weights=[T.init_weights(40 + k) for k in range(K)], seeds=[9, 8, 7], max_batch=mb, dropout=0.2)
    b = T.TrainerSet(ctx, h, w, weights=[T.init_weights(99)] * K, seeds=[1, 2, 3], max_batch=mb, dropout=0.2)
    solo = T.Trainer(ctx, h, w, max_batch=mb, weights_flat=T.init_weights(99), seed=0)
    try:
        for st in steps[:3]:
            step(a, st)
        blob = a.state_bytes(epoch=2)
        hdr = T.read_state_header(blob)
        assert hdr["steps"] == [3, 2, 3] and hdr["seeds"] == [9, 8, 7] and hdr["n_models"] == K
        assert b.load_state_bytes(blob) == 2 and b.step_counts == [3, 2, 3]
        for i, st in enumerate(steps[3:6]):
            la, lb = step(a, st), step(b, st)
            assert la == lb and all(_same(x, y) for x, y in zip(snap(a), snap(b))), f"step {3 + i}"
        assert a.state_bytes(9) == b.state_bytes(9)
        bad = bytearray(blob)
        bad[len(blob) // 2] ^= 0x80
        for data, status in ((bytes(bad), 8), (blob[:len(blob) // 3], 8), (solo.state_bytes(), 1)):   # corrupted, truncated, wrong K
            with pytest.raises(L.CovahipError) as e:
                b.load_state_bytes(data)
            assert e.value.status == status
        with pytest.raises(L.CovahipError) as e:
            solo.load_state_bytes(blob)
        assert e.value.status == 1
        la, lb = step(a, steps[6]), step(b, steps[6])
        assert la == lb and all(_same(x, y) for x, y in zip(snap(a), snap(b))) and b.step_counts == [7, 6, 6]
    finally:
        a.close()
        b.close()
        solo.close()


# ------------------------------------------------------------------------------------------------ 7. the loop
def test_fit_with_validation_best_epoch_and_resume(ctx, tmp_path):
    h, w, b = 45, 80, 8
    x, y = _streams(range(100, 108), 40, h, w)
    train, val = T.split_tail(x, y, 0.125)
    assert val[0].shape[0] == 37 and (val[0] == x[-37:]).all()                 # the last stream
    flat0 = T.init_weights(1)
    ck1, ck2 = tmp_path / "full.cvhs", tmp_path / "cut.cvhs"
    lines = []
    tr = T.Trainer(ctx, h, w, max_batch=b, weights_flat=flat0, seed=1)
    try:
        hist = tr.fit(train, epochs=2, batch=b, val=val, keep="best", checkpoint=ck1, log=lines.append)
        ev = tr.evaluate(val)
        final, best = tr.weights_bytes(), tr.best_weights_bytes()
        with pytest.raises(ValueError):
            tr.fit(train, epochs=1, batch=b, keep="best")
    finally:
        tr.close()
    assert [r["epoch"] for r in hist] == [0, 1] and all(k in hist[0] for k in ("val_loss", "val_precision", "val_recall", "val_iou"))
    assert hist[1]["val_iou"] == ev["iou"] and hist[1]["val_loss"] == ev["loss"]
    assert "val_iou" in lines[0] and len(lines) == 2
    k_best = min(range(2), key=lambda i: (hist[i]["val_loss"], i))
    if k_best == 1:
        assert best == final
    else:
        assert best != final
    assert T.read_state_header(ck1.read_bytes())["user_tag"] == 2 and not os.path.exists(str(ck1) + ".tmp")
    # the same run, stopped after epoch 1 and resumed in a fresh trainer created from other weights
    tr = T.Trainer(ctx, h, w, max_batch=b, weights_flat=flat0, seed=1)
    try:
        h1 = tr.fit(train, epochs=1, batch=b, val=val, keep="best", checkpoint=ck2)
    finally:
        tr.close()
    tr = T.Trainer(ctx, h, w, max_batch=b, weights_flat=T.init_weights(50), seed=3)
    try:
        start = tr.load_state(ck2)
        assert start == 1 and tr.step_count == 33
        h2 = tr.fit(train, epochs=2, batch=b, val=val, keep="best", checkpoint=ck2, start_epoch=start)
        assert h1 + h2 == hist
        assert tr.weights_bytes() == final and tr.best_weights_bytes() == best
    finally:
        tr.close()
    assert ck1.read_bytes() == ck2.read_bytes()


def test_set_fit_with_validation_matches_solo(ctx):
    h, w, b = 17, 33, 3
    recs = [TT.sample_batch(h, w, n, 400 + k) for k, n in enumerate((7, 4))]
    vals = [TT.sample_batch(h, w, n, 410 + k) for k, n in enumerate((5, 2))]
    ts = T.TrainerSet(ctx, h, w, weights=[T.init_weights(60), T.init_weights(61)], seeds=[60, 61], max_batch=b)
    try:
        hs = ts.fit(recs, epochs=2, batch=b, val=vals, keep="best")
        bests = [ts.best_weights_bytes(k) for k in range(2)]
    finally:
        ts.close()
    for k in range(2):
        tr = T.Trainer(ctx, h, w, max_batch=b, weights_flat=T.init_weights(60 + k), seed=60 + k)
        try:
            assert tr.fit(recs[k], epochs=2, batch=b, val=vals[k], keep="best") == hs[k]
            assert tr.best_weights_bytes() == bests[k]
        finally:
            tr.close()


def test_command_line_validates_checkpoints_resumes_and_scores(ctx, tmp_path):
    z = np.load(os.path.join(GOLDEN, "demo_records_excerpt.npz"))
    frames = z["records"]
    h, w = frames.shape[1:3]
    gt = ((frames[..., 1] != 0) | (frames[..., 2] != 0)).astype(np.uint8)
    path = tmp_path / "demo.tfrecord"
    with open(path, "wb") as f:
        for i in range(0, frames.shape[0], 8):
            f.write(tfrecord_example(frames[i:i + 8], gt[i:i + 8], gop=8))

    def run(*args):
        r = subprocess.run([sys.executable, "-m", "cova_amd.train", *args, "--h-mb", str(h), "--w-mb", str(w)], cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r

    common = [str(path), "--val-frac", "0.25", "--keep", "best"]
    full, cut, ck = tmp_path / "full.cvhw", tmp_path / "cut.cvhw", tmp_path / "run.cvhs"
    r = run(*common, "-o", str(full), "--epochs", "3")
    assert "val_iou" in r.stderr and "12 samples" in r.stderr and "4 to validate" in r.stderr
    run(*common, "-o", str(cut), "--epochs", "2", "--checkpoint", str(ck))
    assert T.read_state_header(ck.read_bytes())["user_tag"] == 2
    r = run(*common, "-o", str(cut), "--epochs", "3", "--checkpoint", str(ck), "--resume", str(ck))
    assert "epoch 3/3" in r.stderr and "epoch 2/3" not in r.stderr
    assert cut.read_bytes() == full.read_bytes()
    r = run("--eval-only", str(cut), str(path))
    out = [json.loads(line) for line in r.stdout.splitlines() if line.strip()]
    assert len(out) == 1 and out[0]["samples"] == 16 and out[0]["weights"] == str(cut)
    tr = T.Trainer(ctx, h, w, max_batch=4, weights_flat=W.from_bytes(cut.read_bytes()))
    try:
        ev = tr.evaluate(T.slide(*T.read_tfrecords([str(path)], h, w)))
    finally:
        tr.close()
    assert {k: out[0][k] for k in ev} == ev
