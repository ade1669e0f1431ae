"""Fine-tuning on the GPU (covahip_train_set_plan: frozen layer groups, inference-mode BatchNorm; include/covahip.h "Fine-tuning").

Loss and gradients under five plans against torch autograd in f64 (tests/torch_blobnet_finetune.py; the bounds are
torch_blobnet_train.BOUNDS, shown meaningful under a plan by tests/test_finetune_bounds.py), what a plan freezes staying put bit
for bit, the empty plan being no plan, set = solo, exact resume and plan changes between steps, argument errors, and a base
model adapting to another synthetic camera with its encoder frozen."""
import ctypes as C

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import train as T, weights as W
from cova_amd.elements import BlobNetInfer, Context
from tests import torch_blobnet_finetune as FT
from tests import torch_blobnet_train as TT

pytestmark = pytest.mark.gpu

PLAN_B = FT.PLANS["b-encoder"]
PLAN_C = FT.PLANS["c-enc2-dec1"]
STAT = tuple(n for n in W.tensor_specs() if n.endswith((".bn.mean", ".bn.var")))


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _assert_within_bounds(case, loss, g, ref_loss, g_ref):
    errs = case.errors(loss, g, ref_loss, g_ref)
    print(f"{case.id}: " + ", ".join(f"{k} {v:.2e} ({n})" for k, (v, n) in TT.worst(errs).items()))
    bad = {f"{k} {n}": f"{v:.3g} > {FT.BOUNDS[k]:g}" for (k, n), v in errs.items() if not v <= FT.BOUNDS[k]}
    assert not bad, (case.id, bad)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return bool((_bits(a) == _bits(b)).all())


def _state(trainer):
    """[(params, adam_m, adam_v) per model] of a trainer's state blob, each {tensor name: array}."""
    data = trainer.state_bytes()
    k = T.read_state_header(data)["n_models"]
    out = []
    for m in range(k):
        off = 64 + m * (16 + 12 * W.N_PARAMS) + 16
        out.append(tuple(W.unflatten(np.frombuffer(data, "<f4", W.N_PARAMS, off + a * 4 * W.N_PARAMS)) for a in range(3)))
    return out


# ------------------------------------------------------------------------------------------------ 1. against f64 autograd
@pytest.mark.parametrize("case", FT.CASES, ids=[c.id for c in FT.CASES])
def test_gradients_match_torch_f64(ctx, case):
    flat, pre, stack, gt = case.inputs()
    tr = T.Trainer(ctx, case.h, case.w, max_batch=FT.MAX_BATCH, weights_flat=flat, seed=case.seed, dropout=case.p, **case.plan)
    try:
        frozen, inference = FT.effective(**case.plan)
        assert set(tr.plan["freeze"]) == frozen and set(tr.plan["bn_inference"]) == inference
        tr.step(*pre, lr=0.0)
        now = tr.weights()                       # lr = 0: only the moving statistics of batch-mode layers have moved
        mk = T.trainable_mask()
        assert _same(now[mk], flat[mk])
        loss = tr.step(stack, gt)
        g = tr.grads()
    finally:
        tr.close()
    ref_loss, g_ref, _ = case.reference(flat=now)
    _assert_within_bounds(case, loss, g, ref_loss, g_ref)
    gu, wu = W.unflatten(g), W.unflatten(now)
    for name in gu:                              # exact, not within a bound: zeros, and the moving values themselves
        grp = FT.group_of(name)
        if name in STAT:
            assert _same(gu[name], wu[name]) == (grp in inference), name
        elif grp in frozen:
            assert not gu[name].any(), name
    if case.plan_id == "e-bn-dec0":              # the bias in front of the inference-mode layer has a gradient of its own size
        ref = FT._unflatten64(g_ref)
        assert np.linalg.norm(ref["dec0.up.bias"]) > 1e-3 * np.linalg.norm(ref["dec0.bn.beta"])
        assert np.linalg.norm(gu["dec0.up.bias"]) > 1e-3 * np.linalg.norm(gu["dec0.bn.beta"])


def test_set_model_index_matches_torch_f64(ctx):
    """Model 2 of a set of three, each with its own weights, batch and seed, against autograd under plan (c)."""
    case = next(c for c in FT.CASES if c.id == "17x33-p0.2-c-enc2-dec1")
    h, w = case.h, case.w
    flats = [FT.finetune_weights(s) for s in (21, 22, 3)]
    seeds = [5, 6, case.seed]
    _, pre, stack, gt = case.inputs()
    others = [TT.sample_batch(h, w, b, 70 + k) for k, b in enumerate((3, 1))]
    ts = T.TrainerSet(ctx, h, w, weights=flats, seeds=seeds, max_batch=FT.MAX_BATCH, dropout=case.p, **case.plan)
    try:
        ts.step([pre[0]] * 3, [pre[1]] * 3, lrs=0.0)
        now = ts.weights(2)
        losses = ts.step([others[0][0], others[1][0], stack], [others[0][1], others[1][1], gt])
        g = ts.grads(2)
    finally:
        ts.close()
    ref_loss, g_ref, _ = case.reference(flat=now)
    _assert_within_bounds(case, losses[2], g, ref_loss, g_ref)


# ------------------------------------------------------------------------------------------------ 2. what is frozen stays put
def test_frozen_groups_stay_put(ctx):
    h, w, b = 17, 33, 3
    flat = FT.finetune_weights(4)
    frozen, inference = FT.effective(**PLAN_C)
    tr = T.Trainer(ctx, h, w, max_batch=b, weights_flat=flat, seed=2, **PLAN_C)
    try:
        (p0, m0, v0), = _state(tr)
        for k in range(3):
            tr.step(*TT.sample_batch(h, w, b, 20 + k), lr=1e-3)
        (p1, m1, v1), = _state(tr)
    finally:
        tr.close()
    for name in p0:
        grp = FT.group_of(name)
        if name in STAT:
            assert _same(p0[name], p1[name]) == (grp in inference), name       # moving statistics: kept / moved by the batch
            assert not m1[name].any() and not v1[name].any(), name
        elif grp in frozen:
            assert _same(p0[name], p1[name]) and _same(m0[name], m1[name]) and _same(v0[name], v1[name]), name
            assert not m1[name].any() and not v1[name].any(), name
        else:
            assert not _same(p0[name], p1[name]) and m1[name].any() and v1[name].any(), name


# ------------------------------------------------------------------------------------------------ 3. empty plan = no plan
def test_empty_plan_is_no_plan(ctx):
    h, w, b = 17, 33, 3
    flat = FT.finetune_weights(5)
    outs = []
    for set_empty in (False, True):
        tr = T.Trainer(ctx, h, w, max_batch=b, weights_flat=flat, seed=3)
        if set_empty:
            tr.set_plan()
        assert tr.plan == {"freeze": (), "bn_inference": ()}
        losses = [tr.step(*TT.sample_batch(h, w, b, 30 + k), lr=1e-3) for k in range(3)]
        outs.append((losses, tr.state_bytes(), tr.grads()))
        tr.close()
    assert outs[0][0] == outs[1][0]
    assert outs[0][1] == outs[1][1]
    assert _same(outs[0][2], outs[1][2])


# ------------------------------------------------------------------------------------------------ 4. set = solo under a plan
@pytest.mark.parametrize("plan", [PLAN_B, PLAN_C], ids=["b-encoder", "c-enc2-dec1"])
def test_set_equals_solo_under_a_plan(ctx, plan):
    h, w, mb = 17, 33, 4
    flats = [FT.finetune_weights(40 + k) for k in range(3)]
    seeds = [7, 8, 9]
    lrs = [1e-3, 3e-3, 5e-4]
    # two steps: batches (4, 1, 3), then model 1 sits out
    steps = [[TT.sample_batch(h, w, n, 50 + 10 * s + k) if n else None for k, n in enumerate(bs)] for s, bs in enumerate(((4, 1, 3), (2, 0, 4)))]
    ts = T.TrainerSet(ctx, h, w, weights=flats, seeds=seeds, max_batch=mb, **plan)
    set_losses = []
    for st in steps:
        set_losses.append(ts.step([None if r is None else r[0] for r in st], [None if r is None else r[1] for r in st], lrs=lrs))
    set_out = [(ts.weights(k), ts.grads(k), ts.metrics(k)) for k in range(3)]
    set_state = _state(ts)
    ts.close()
    for k in range(3):
        tr = T.Trainer(ctx, h, w, max_batch=mb, weights_flat=flats[k], seed=seeds[k], **plan)
        losses = [tr.step(*st[k], lr=lrs[k]) if st[k] is not None else 0.0 for st in steps]
        assert losses == [sl[k] for sl in set_losses], k
        assert _same(tr.weights(), set_out[k][0]) and _same(tr.grads(), set_out[k][1]) and tr.metrics() == set_out[k][2], k
        (p, m, v), = _state(tr)
        for a, b_ in zip((p, m, v), set_state[k]):
            assert all(_same(a[n], b_[n]) for n in a), k
        tr.close()


# ------------------------------------------------------------------------------------------------ 5. resume under a plan
def test_resume_under_a_plan(ctx):
    h, w, b = 17, 33, 3
    flat = FT.finetune_weights(6)
    data = [TT.sample_batch(h, w, b, 80 + k) for k in range(4)]
    held = TT.sample_batch(h, w, 5, 90)
    tr = T.Trainer(ctx, h, w, max_batch=b, weights_flat=flat, seed=4, **PLAN_C)
    ref_losses = [tr.step(*d, lr=1e-3) for d in data]
    ref = (tr.state_bytes(), tr.grads(), tr.metrics())
    tr.close()
    a = T.Trainer(ctx, h, w, max_batch=b, weights_flat=flat, seed=4, **PLAN_C)
    la = [a.step(*d, lr=1e-3) for d in data[:2]]
    a.evaluate(held)                                    # evaluation rewrites every BN stat row: the step must not notice
    blob = a.state_bytes()
    a.close()
    r = T.Trainer(ctx, h, w, max_batch=b, weights_flat=FT.finetune_weights(99), seed=1234, **PLAN_C)
    r.load_state_bytes(blob)
    assert r.plan == {"freeze": ("enc2", "dec1"), "bn_inference": ("enc2", "dec1")}      # load_state does not touch the plan
    ev = r.evaluate(held)
    lr_ = [r.step(*data[2], lr=1e-3)]
    assert r.evaluate(held)["loss"] != ev["loss"]       # (the step did train)
    lr_.append(r.step(*data[3], lr=1e-3))
    assert la + lr_ == ref_losses
    assert r.state_bytes() == ref[0] and _same(r.grads(), ref[1]) and r.metrics() == ref[2]
    r.close()


# ------------------------------------------------------------------------------------------------ 6. plan changed between steps
def test_plan_changed_between_steps(ctx):
    h, w, b = 17, 33, 3
    flat = FT.finetune_weights(7)
    data = [TT.sample_batch(h, w, b, 100 + k) for k in range(4)]
    outs = []
    for as_set in (False, True):
        if as_set:
            t = T.TrainerSet(ctx, h, w, weights=[flat], seeds=[5], max_batch=b)
            step = lambda d: t.step([d[0]], [d[1]], lrs=1e-3)[0]
            grads, weights = (lambda: t.grads(0)), (lambda: t.weights(0))
        else:
            t = T.Trainer(ctx, h, w, max_batch=b, weights_flat=flat, seed=5)
            step = lambda d: t.step(*d, lr=1e-3)
            grads, weights = t.grads, t.weights
        t.set_plan(freeze="encoder", bn_inference="all")
        losses = [step(d) for d in data[:2]]
        g_frozen, w_frozen = W.unflatten(grads()), W.unflatten(weights())
        for name in STAT:                               # every layer normalised with its moving values
            assert _same(g_frozen[name], w_frozen[name]), name
        assert not g_frozen["enc1.conv.kernel"].any()
        t.set_plan()
        assert t.plan == {"freeze": (), "bn_inference": ()}
        before = W.unflatten(weights())
        losses.append(step(data[2]))
        g_full = W.unflatten(grads())
        for name in STAT:                               # batch statistics again, in the stat rows and in the slots
            assert not _same(g_full[name], before[name]), name
        assert g_full["enc1.conv.kernel"].any() and g_full["enc0.tmix.w1"].any()
        losses.append(step(data[3]))
        outs.append((losses, t.state_bytes(), grads()))
        t.close()
    assert outs[0][0] == outs[1][0]
    assert outs[0][1] == outs[1][1]                     # a set of one and the solo trainer: the same blob
    assert _same(outs[0][2], outs[1][2])


# ------------------------------------------------------------------------------------------------ 7. argument errors
def test_plan_argument_errors(ctx):
    lib = L.lib()
    tr = T.Trainer(ctx, 16, 16, max_batch=1, freeze=("enc0",), bn_inference=("dec2",))
    try:
        want = {"freeze": ("enc0",), "bn_inference": ("enc0", "dec2")}
        assert tr.plan == want
        for fz, bn in ((0x100, 0), (0, 0x80), (0xFF, 0), (1 << 31, 0), (0, 1 << 31), (0xFF, 0x7F)):
            assert lib.covahip_train_set_plan(tr.handle, C.byref(L.TrainPlan(fz, bn))) == 1, (fz, bn)
            assert tr.plan == want, (fz, bn)
        assert lib.covahip_train_set_plan(tr.handle, None) == 1
        assert lib.covahip_train_set_plan(None, C.byref(L.TrainPlan(0, 0))) == 1
        assert lib.covahip_train_get_plan(tr.handle, None) == 1
        assert lib.covahip_train_get_plan(None, C.byref(L.TrainPlan())) == 1
        assert tr.plan == want
        with pytest.raises(ValueError):
            tr.set_plan(freeze=("encoder", "decoder"))
        with pytest.raises(ValueError):
            tr.set_plan(freeze=("enc4",))
        assert tr.plan == want
        assert lib.covahip_train_set_plan(tr.handle, C.byref(L.TrainPlan(0x7F, 0))) == 0       # all but dec3: allowed
        assert tr.plan["freeze"] == T.GROUPS[:7] and tr.plan["bn_inference"] == T.BN_LAYERS
    finally:
        tr.close()
    with pytest.raises(ValueError):
        T.Trainer(ctx, 16, 16, max_batch=1, freeze="encoder,decoder")


# ------------------------------------------------------------------------------------------------ 8. it adapts
def _camera(seed, n_frames, h, w, r_lo, r_hi, noise, n_objects=6):
    """A synthetic camera in the manner of synth.carrier_frames: ellipses with radii in [r_lo, r_hi) moving over a background
    whose motion-vector bytes are non-zero on `noise` of the macroblocks; the label is the union of the ellipses' insides.
    Every overlapping window of 4 frames as a stack, newest first."""
    rng = np.random.default_rng(seed)
    f = np.zeros((n_frames, h, w, 4), np.uint8)
    f[..., 0] = np.where(rng.random(f.shape[:3]) < 0.8, 0, rng.integers(0, 8, size=f.shape[:3], dtype=np.uint8))
    for c in (1, 2):
        f[..., c] = np.where(rng.random(f.shape[:3]) < 1.0 - noise, 0, rng.integers(1, 4, size=f.shape[:3], dtype=np.uint8))
    gt = np.zeros((n_frames, h, w), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(n_objects):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        ry, rx = rng.uniform(r_lo, r_hi), rng.uniform(r_lo, r_hi)
        vy, vx = rng.uniform(-2, 2), rng.uniform(-2, 2)
        for i in range(n_frames):
            inside = ((yy - (cy + vy * i)) / ry) ** 2 + ((xx - (cx + vx * i)) / rx) ** 2 <= 1.0
            n = int(inside.sum())
            if n:
                f[i, inside, 0] = rng.integers(1, 8, size=n, dtype=np.uint8)
                f[i, inside, 1] = rng.integers(1, 13, size=n, dtype=np.uint8)
                f[i, inside, 2] = rng.integers(1, 13, size=n, dtype=np.uint8)
                gt[i, inside] = 1
    n = n_frames - 3
    st = np.stack([f[i:i + 4][::-1].reshape(4 * h, w, 4) for i in range(n)])
    return np.ascontiguousarray(st), np.ascontiguousarray(gt[3:])


def _cameras(seeds, n_frames, h, w, **kw):
    parts = [_camera(s, n_frames, h, w, **kw) for s in seeds]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _iou(mask, gt):
    inter = (mask.astype(bool) & gt.astype(bool)).sum(axis=(1, 2))
    union = (mask.astype(bool) | gt.astype(bool)).sum(axis=(1, 2))
    return float(np.mean(np.where(union > 0, inter / np.maximum(union, 1), 1.0)))


BASE_STEPS, TUNE_STEPS = 300, 150
BASE_CAM = dict(r_lo=1, r_hi=10, noise=0.1)     # the setting of test_learns_synthetic_ellipses
NEW_CAM = dict(r_lo=4, r_hi=16, noise=0.3)      # another camera: larger objects, three times the background noise


def test_adapts_with_the_encoder_frozen(ctx):
    h, w, b = 45, 80, 8
    base_x, base_y = _cameras(range(100, 106), 40, h, w, **BASE_CAM)
    new_x, new_y = _cameras(range(200, 203), 40, h, w, **NEW_CAM)            # a few hundred windows is all the new camera gives
    held_x, held_y = _cameras((777, 778), 20, h, w, **NEW_CAM)
    tr = T.Trainer(ctx, h, w, max_batch=b, seed=1)
    rng = np.random.default_rng(0)
    for _ in range(BASE_STEPS):
        idx = rng.choice(base_x.shape[0], b, replace=False)
        tr.step(base_x[idx], base_y[idx])
    base = tr.weights()
    ev_base = tr.evaluate((held_x, held_y))
    tr.set_plan(freeze="encoder", bn_inference="all")                          # --freeze encoder --freeze-bn
    for _ in range(TUNE_STEPS):
        idx = rng.choice(new_x.shape[0], b, replace=False)
        tr.step(new_x[idx], new_y[idx])
    tuned = tr.weights()
    ev_tuned = tr.evaluate((held_x, held_y))
    tr.close()
    bu, tu = W.unflatten(base), W.unflatten(tuned)
    for name in bu:                                                            # the encoder and every moving statistic: the base's
        if name.startswith("enc") or name in STAT:
            assert _same(bu[name], tu[name]), name
    ious = []
    for flat in (base, tuned):
        net = BlobNetInfer(ctx, flat, h, w, max_batch=held_x.shape[0])
        ious.append(_iou(net.infer(held_x, want_logits=False)[1], held_y))
    print(f"new camera, held out: loss {ev_base['loss']:.4f} (base, {BASE_STEPS} steps) -> {ev_tuned['loss']:.4f} after {TUNE_STEPS} "
          f"decoder-only steps; IoU through the fp16 inference path {ious[0]:.3f} -> {ious[1]:.3f}")
    assert ev_tuned["loss"] < ev_base["loss"], (ev_base, ev_tuned)
