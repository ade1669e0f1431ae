"""BlobNet training on the GPU (covahip_train_*): loss, gradients, batch statistics and TP / FP / FN against torch autograd
in f64 over the case matrix of tests/torch_blobnet_train.py (bounds there, shown not vacuous by tests/test_train_bounds.py),
partial batches bit for bit, a batch of 320 through the capped reduction plans, steps on device memory, optimiser state,
determinism, learning on labelled synthetic streams, export into the fp16 inference path, and the record -> train -> infer loop."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from cova_amd import _lib as L, synth, train as T, weights as W
from cova_amd.elements import BlobNetInfer, Context, tfrecord_example
from tests import torch_blobnet as TB
from tests import torch_blobnet_train as TT
from tests.golden_util import GOLDEN, blobnet_tolerance

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.0)


def _tensor_errors(g, g_ref):
    gu, ru = W.unflatten(g), W.unflatten(g_ref.astype(np.float32))
    return {k: _relerr(gu[k], ru[k]) for k in gu}


def _batch(h, w, b, seed):
    stack = synth.stacked_batch(b, h, w, seed=seed, streams=b)
    gt = synth.random_masks(b, h, w, 0.3, seed=seed)
    return stack, gt


def _run_case(ctx, case):
    """The GPU's (loss, flat gradient, (TP, FP, FN), labels) on a case of TT.CASES."""
    flat, pre, stack, gt = case.inputs()
    tr = T.Trainer(ctx, case.h, case.w, max_batch=case.max_batch, weights_flat=flat, seed=case.seed, dropout=case.p)
    try:
        assert tr.cfg.seed == case.seed and tr.cfg.dropout == case.p32
        for st, g in pre:
            tr.step(st, g, lr=0.0)
        assert tr.step_count == case.steps
        if pre:     # lr = 0: the trainable weights are the initial ones, bit for bit
            mk = T.trainable_mask()
            assert (tr.weights()[mk].view(np.uint32) == flat[mk].view(np.uint32)).all()
        loss = tr.step(stack, gt)
        return loss, tr.grads(), tr.metrics(), gt
    finally:
        tr.close()


def _assert_within_bounds(what, loss, g, ref_loss, g_ref):
    errs = TT.errors(loss, g, ref_loss, g_ref)
    print(f"{what}: " + ", ".join(f"{k} {v:.2e} ({n})" for k, (v, n) in TT.worst(errs).items()))
    bad = {f"{k} {n}": f"{v:.3g} > {TT.BOUNDS[k]:g}" for (k, n), v in errs.items() if not v <= TT.BOUNDS[k]}
    assert not bad, (what, bad)


METRIC_BAND = 1e-3   # |logit| below which the f32 and the f64 side may disagree on sigmoid > 0.5


def _assert_metrics(counts, logit_ref, gt):
    """TP / FP / FN at sigmoid > 0.5 against the reference logits: a pixel may only move between classes inside the band."""
    tp, fp, fn = counts
    lab = gt.astype(bool)
    pos = logit_ref > 0
    near = np.abs(logit_ref) < METRIC_BAND
    assert near.sum() <= max(2, 0.005 * near.size), int(near.sum())
    assert tp + fn == int(lab.sum()), (counts, int(lab.sum()))
    assert abs(tp - int((pos & lab).sum())) <= int((near & lab).sum()), (counts, int((pos & lab).sum()))
    assert abs(fp - int((pos & ~lab).sum())) <= int((near & ~lab).sum()), (counts, int((pos & ~lab).sum()))


def _check_case(ctx, case):
    loss, g, counts, gt = _run_case(ctx, case)
    ref_loss, g_ref, logit = case.reference()
    _assert_within_bounds(case.id, loss, g, ref_loss, g_ref)
    _assert_metrics(counts, logit, gt)


@pytest.mark.parametrize("hw", [(45, 80), (68, 120)])
def test_gradients_match_torch_f64(ctx, hw):
    case = {(c.h, c.w): c for c in TT.CASES[:2]}[hw]
    assert (case.batch, case.max_batch, case.steps, case.p, case.seed) == (3, 3, 0, 0.2, 11)
    _check_case(ctx, case)


@pytest.mark.parametrize("case", TT.CASES[2:], ids=[c.id for c in TT.CASES[2:]])
def test_gradient_matrix_matches_torch_f64(ctx, case):
    _check_case(ctx, case)


@pytest.mark.parametrize("hw", [(17, 33), (45, 80)])
def test_partial_batch_is_exact(ctx, hw):
    """A batch of 3 on a trainer sized for 8 that has just taken a batch of 8 gives the bits of the same batch on a trainer
    sized for 3: buffers are sized for max_batch, every launch, stride and reduction split follows the batch."""
    h, w = hw
    flat = T.init_weights(6)
    s8, g8 = TT.sample_batch(h, w, 8, 30)
    s3, g3 = TT.sample_batch(h, w, 3, 31)
    outs = []
    for mb, first in ((8, (s8, g8)), (3, (s8[:3], g8[:3]))):
        tr = T.Trainer(ctx, h, w, max_batch=mb, weights_flat=flat, seed=21, dropout=0.2)
        tr.step(*first, lr=0.0)
        loss = tr.step(s3, g3, lr=0.0)
        outs.append((loss, tr.grads(), tr.metrics()))
        tr.close()
    (la, ga, ma), (lb, gb, mb_) = outs
    assert la == lb and ma == mb_, (la, lb, ma, mb_)
    diff = ga.view(np.uint32) != gb.view(np.uint32)
    assert not diff.any(), f"{int(diff.sum())} gradient slots differ"


def test_large_batch_through_capped_plans(ctx):
    """B = 320 as 80 interleaved copies of 4 samples: batch statistics and the mean per-sample loss are those of the 4, so are
    the gradients, while the reduction plans of train.hip run at their caps."""
    h, w, n, b = 45, 80, 4, 320
    hp, wp = (h + 1) // 2, (w + 1) // 2
    p0 = b * W.T * h * w                                   # encoder level 0 weight-gradient positions
    assert -(-p0 // 1024) > 4096                           # wg_slabs: 4096 slabs, chunk > WG_CHUNK
    assert -(-(b * 16 * hp * wp) // (4 * 256)) > 512       # k_tmix_bwd's blocks at TMIX_BLOCKS_MAX
    assert b > 128                                         # the loss's per-sample sums: red of 2 * B
    flat = T.init_weights(8)
    s4, g4 = TT.sample_batch(h, w, n, 50)
    s, g = np.tile(s4, (b // n, 1, 1, 1)), np.tile(g4, (b // n, 1, 1))
    assert (s[n * 37 + 2] == s4[2]).all()
    tr = T.Trainer(ctx, h, w, max_batch=b, weights_flat=flat, seed=0, dropout=0.0)
    big = tr.step(s, g, lr=0.0), tr.grads()
    small = tr.step(s4, g4, lr=0.0), tr.grads()
    tr.close()
    ref = TT.grads_flat(flat, s4, g4, h, w, seed=0, step=0, p=0.0)[:2]
    _assert_within_bounds("B=320 vs f64 of the 4", *big, *ref)
    _assert_within_bounds("B=4 vs f64", *small, *ref)
    _assert_within_bounds("B=320 vs B=4 on the GPU", *big, *small)


def test_device_memory_step_is_bit_identical(ctx):
    h, w, mb = 24, 50, 3
    flat = T.init_weights(10)
    batches = [TT.sample_batch(h, w, b, 60 + k) for k, b in enumerate((3, 2))]
    outs = []
    for dev in (False, True):
        tr = T.Trainer(ctx, h, w, max_batch=mb, weights_flat=flat, seed=4, dropout=0.2)
        res = []
        for s, g in batches:
            if dev:
                ds, dg = ctx.malloc(s.nbytes), ctx.malloc(g.nbytes)
                try:
                    ctx.h2d(ds, s)
                    ctx.h2d(dg, g)
                    loss = tr.step_device(ds, dg, s.shape[0])
                finally:
                    ctx.free(ds)
                    ctx.free(dg)
            else:
                loss = tr.step(s, g)
            res.append((loss, tr.metrics(), tr.grads().view(np.uint32)))
        outs.append((res, tr.weights().view(np.uint32)))
        tr.close()
    (rh, wh), (rd, wd) = outs
    for (lh, mh, gh), (ld, md, gd) in zip(rh, rd):
        assert lh == ld and mh == md and (gh == gd).all()
    assert (wh == wd).all()


def test_solo_abi_matches_trainer(ctx):
    """covahip_train_create / _step / _metrics / _weights / _grads driven through ctypes (the Python Trainer is a set of one and
    no longer calls them): loss, metrics, gradients and weights equal the Trainer's bit for bit after every step, the last one
    a partial batch."""
    h, w, mb, seed, lr = 16, 16, 2, 5, 1e-3
    flat = T.init_weights(12)
    lib = L.lib()
    cfg = L.TrainCfg()
    lib.covahip_train_default_cfg(C.byref(cfg))
    cfg.h_mb, cfg.w_mb, cfg.max_batch, cfg.seed = h, w, mb, seed
    blob = W.to_bytes(flat)
    hd = C.c_void_p()
    L.check(lib.covahip_train_create(ctx.handle, C.byref(cfg), blob, len(blob), C.byref(hd)), "covahip_train_create", ctx.handle)
    tr = T.Trainer(ctx, h, w, max_batch=mb, weights_flat=flat, seed=seed)
    try:
        assert (tr.cfg.dropout, tr.cfg.lr) == (cfg.dropout, cfg.lr)
        for k, b in enumerate((2, 2, 1)):
            s, g = TT.sample_batch(h, w, b, 70 + k)
            loss = C.c_float()
            L.check(lib.covahip_train_step(hd, s.ctypes.data, g.ctypes.data, b, lr, C.byref(loss), L.MEM_HOST), "covahip_train_step",
                    ctx.handle)
            assert np.float32(loss.value).view(np.uint32) == np.float32(tr.step(s, g, lr=lr)).view(np.uint32), k
            m = (C.c_int64 * 3)()
            L.check(lib.covahip_train_metrics(hd, m), "covahip_train_metrics")
            assert tuple(m) == tr.metrics(), k
            gr = np.empty(W.N_PARAMS, np.float32)
            L.check(lib.covahip_train_grads(hd, gr.ctypes.data, gr.size), "covahip_train_grads", ctx.handle)
            assert (gr.view(np.uint32) == tr.grads().view(np.uint32)).all(), k
            n = C.c_size_t()
            assert lib.covahip_train_weights(hd, None, 0, C.byref(n)) == 7 and n.value == len(blob)   # the size query
            buf = np.zeros(n.value, np.uint8)
            L.check(lib.covahip_train_weights(hd, buf.ctypes.data, n.value, C.byref(n)), "covahip_train_weights", ctx.handle)
            assert buf.tobytes() == tr.weights_bytes(), k
        assert not (tr.weights().view(np.uint32) == flat.view(np.uint32)).all()       # (the weights moved)
    finally:
        tr.close()
        lib.covahip_train_destroy(hd)


def test_optimiser_state_after_three_steps(ctx):
    h, w, b = 45, 80, 2
    flat = T.init_weights(4)
    tr = T.Trainer(ctx, h, w, max_batch=b, weights_flat=flat, seed=2, dropout=0.2)
    wts = flat.astype(np.float64).copy()
    wts_biased = wts.copy()                 # the same moving variance updated with the biased batch variance
    m = np.zeros_like(wts)
    v = np.zeros_like(wts)
    train = T.trainable_mask()
    stat_names = [n for n in W.tensor_specs() if n.endswith((".bn.mean", ".bn.var"))]
    lr = 1e-3
    for k in range(3):
        stack, gt = _batch(h, w, b, 20 + k)
        tr.step(stack, gt, lr)
        g = tr.grads().astype(np.float64)
        # Adam (Keras form) on the trained weights
        m[train] = 0.9 * m[train] + 0.1 * g[train]
        v[train] = 0.999 * v[train] + 0.001 * g[train] ** 2
        wts[train] -= T.adam_lr_t(lr, k) * m[train] / (np.sqrt(v[train]) + 1e-7)
        # moving statistics: 0.99 * moving + 0.01 * batch, the variance's batch value unbiased
        gu = W.unflatten(g)
        off = 0
        for name, shape in W.tensor_specs().items():
            n = int(np.prod(shape))
            if name in stat_names:
                batch_v = gu[name].astype(np.float64)
                if name.endswith(".var"):
                    cnt = b * (W.T if name.startswith("enc") else 1) * _level_hw(name, h, w)
                    batch_v = batch_v * cnt / (cnt - 1)
                wts[off:off + n] = 0.99 * wts[off:off + n] + 0.01 * batch_v.reshape(-1)
                wts_biased[off:off + n] = 0.99 * wts_biased[off:off + n] + 0.01 * gu[name].astype(np.float64).reshape(-1)
            off += n
    got = tr.weights()
    tr.close()
    errs = _tensor_errors(got, wts)
    # the moving statistics start at mean 0 / var 1 and move by 1 % of a batch value per step: compare what they moved by, so
    # that the n / (n - 1) of the variance update is resolved (at decoder block 0, n = 120 here: a 0.8 % change of the increment)
    init, gu, wu, ref_biased = W.unflatten(flat), W.unflatten(got), W.unflatten(wts), W.unflatten(wts_biased)
    for name in stat_names:
        errs[name] = _relerr(gu[name].astype(np.float64) - init[name], wu[name] - init[name])
        if name == "dec0.bn.var":   # the test tells the unbiased update from the biased one
            assert _relerr(ref_biased[name] - init[name], wu[name] - init[name]) > 3e-3
    bad = {k: v for k, v in errs.items() if not v <= 1e-3}
    assert not bad, bad


def _level_hw(name, h, w):
    """H*W of the tensor a BN layer normalises: encoder level i at its conv resolution, decoder block j at its output."""
    lv = [(h, w)]
    for _ in range(4):
        lv.append(((lv[-1][0] + 1) // 2, (lv[-1][1] + 1) // 2))
    if name.startswith("enc"):
        hh, ww = lv[int(name[3])]
    else:
        hh, ww = lv[3 - int(name[3])]
    return hh * ww


def test_bit_identical_runs(ctx):
    h, w, b = 45, 80, 4
    flat = T.init_weights(9)
    outs = []
    for _ in range(2):
        tr = T.Trainer(ctx, h, w, max_batch=b, weights_flat=flat, seed=5, dropout=0.2)
        losses = [tr.step(*_batch(h, w, b, 40 + k)) for k in range(10)]
        outs.append((losses, tr.weights(), tr.grads()))
        tr.close()
    assert outs[0][0] == outs[1][0]
    assert (outs[0][1].view(np.uint32) == outs[1][1].view(np.uint32)).all()
    assert (outs[0][2].view(np.uint32) == outs[1][2].view(np.uint32)).all()


def _ellipse_data(n_frames, h, w, seed, n_objects=6):
    """synth.carrier_frames restated step for step (the same frames, asserted below), also returning each frame's label: the
    union of the ellipses' insides.  The background keeps the generator's motion-vector noise (1..3 on ~10 % of the
    macroblocks per component), so the label is the geometry, not 'mv byte nonzero'."""
    rng = np.random.default_rng(seed)
    f = np.zeros((n_frames, h, w, 4), dtype=np.uint8)
    bg_type = rng.integers(0, 8, size=f.shape[:3], dtype=np.uint8)
    f[..., 0] = np.where(rng.random(f.shape[:3]) < 0.8, 0, bg_type)
    for c in (1, 2):
        mv = rng.integers(1, 4, size=f.shape[:3], dtype=np.uint8)
        f[..., c] = np.where(rng.random(f.shape[:3]) < 0.9, 0, mv)
    f[..., 3] = rng.integers(0, 256, size=f.shape[:3], dtype=np.uint8)
    gt = np.zeros((n_frames, h, w), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(n_objects):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        ry, rx = rng.uniform(1, 10), rng.uniform(1, 10)
        vy, vx = rng.uniform(-2, 2), rng.uniform(-2, 2)
        for i in range(n_frames):
            inside = ((yy - (cy + vy * i)) / ry) ** 2 + ((xx - (cx + vx * i)) / rx) ** 2 <= 1.0
            n = int(inside.sum())
            if n == 0:
                continue
            f[i, inside, 0] = rng.integers(1, 8, size=n, dtype=np.uint8)
            f[i, inside, 1] = rng.integers(1, 13, size=n, dtype=np.uint8)
            f[i, inside, 2] = rng.integers(1, 13, size=n, dtype=np.uint8)
            gt[i, inside] = 1
    assert (f == synth.carrier_frames(n_frames, h, w, seed=seed, n_objects=n_objects)).all()
    return f, gt


def _streams(seeds, n_frames, h, w):
    """Every overlapping window of several independent streams."""
    parts = [_stacks(*_ellipse_data(n_frames, h, w, s)) for s in seeds]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _stacks(frames, gt):
    """Every overlapping window (more samples than slide's non-overlapping ones)."""
    n = frames.shape[0] - 3
    st = np.stack([frames[i:i + 4][::-1].reshape(4 * frames.shape[1], frames.shape[2], 4) for i in range(n)])
    return np.ascontiguousarray(st), np.ascontiguousarray(gt[3:])


def _iou(mask, gt):
    inter = (mask.astype(bool) & gt.astype(bool)).sum(axis=(1, 2))
    union = (mask.astype(bool) | gt.astype(bool)).sum(axis=(1, 2))
    return float(np.mean(np.where(union > 0, inter / np.maximum(union, 1), 1.0)))


LEARN_STEPS = 600


def test_learns_synthetic_ellipses(ctx):
    h, w, b = 45, 80, 8
    tr_x, tr_y = _streams(range(100, 108), 40, h, w)          # 8 streams x 37 windows
    te_x, te_y = _streams((777, 778), 20, h, w)               # 2 held-out streams x 17 windows
    flat0 = T.init_weights(1)
    net = BlobNetInfer(ctx, flat0, h, w, max_batch=te_x.shape[0])
    iou0 = _iou(net.infer(te_x, want_logits=False)[1], te_y)
    tr = T.Trainer(ctx, h, w, max_batch=b, weights_flat=flat0, seed=1)
    rng = np.random.default_rng(0)
    for k in range(LEARN_STEPS):
        idx = rng.choice(tr_x.shape[0], b, replace=False)
        tr.step(tr_x[idx], tr_y[idx])
    flat = tr.weights()
    tr.close()
    net = BlobNetInfer(ctx, flat, h, w, max_batch=te_x.shape[0])
    iou = _iou(net.infer(te_x, want_logits=False)[1], te_y)
    print(f"held-out IoU: {iou0:.3f} at initialisation -> {iou:.3f} after {LEARN_STEPS} steps")
    assert iou >= 0.5 and iou >= 3 * iou0, (iou0, iou)
    # export into the fp16 inference path: within the inference tolerance of the f32 composition on the same file
    logits, _ = net.infer(te_x[:8])
    ref = TB.forward(flat, te_x[:8], h, w)
    atol, rtol = blobnet_tolerance(ref)
    err = np.abs(logits - ref)
    assert (err <= atol + rtol * np.abs(ref)).all(), float((err - atol - rtol * np.abs(ref)).max())


def test_records_to_weights_end_to_end(ctx, tmp_path):
    z = np.load(os.path.join(GOLDEN, "demo_records_excerpt.npz"))
    frames = z["records"]
    h, w = frames.shape[1:3]
    gt = ((frames[..., 1] != 0) | (frames[..., 2] != 0)).astype(np.uint8)    # derived label: "mv byte nonzero"
    path = tmp_path / "demo.tfrecord"
    with open(path, "wb") as f:
        for i in range(0, frames.shape[0], 8):                                  # gop form, 8 frames per record
            f.write(tfrecord_example(frames[i:i + 8], gt[i:i + 8], gop=8))
    fr, g = T.read_tfrecords([str(path)], h, w)
    assert (fr[..., :3] == frames[..., :3]).all() and (g == gt).all()
    stacks, labels = T.slide(fr, g)
    tr = T.Trainer(ctx, h, w, max_batch=4, seed=0)
    with pytest.raises(ValueError):
        tr.fit((stacks, labels), epochs=1, batch=8)
    hist = tr.fit((stacks, labels), epochs=5, batch=4)                          # 16 samples: 4 steps per epoch, 20 steps
    tr.close()
    losses = [r["loss"] for r in hist]
    assert losses[-1] < losses[0], losses
    out = tmp_path / "blobnet.cvhw"
    r = subprocess.run([sys.executable, "-m", "cova_amd.train", str(path), "-o", str(out), "--epochs", "2", "--h-mb", str(h),
                        "--w-mb", str(w)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    flat = W.from_bytes(out.read_bytes())
    net = BlobNetInfer(ctx, flat, h, w, max_batch=4)
    _, mask = net.infer(stacks[:4], want_logits=False)
    assert mask.shape == (4, h, w)
