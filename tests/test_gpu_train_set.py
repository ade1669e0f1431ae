"""Training sets (covahip_train_create_set / _step_set, cova_amd.train.TrainerSet): model k of a set is bit-identical to the
same model trained alone.  Solo trainers (cova_amd.train.Trainer: covahip_train_create_set with one model and the seed given,
which is the trainer covahip_train_create makes -- K = 1, the kernels' solo instantiation; tests/test_gpu_train.py holds the
two equal) are the reference throughout and every comparison is np.array_equal on the float bits, never a tolerance -- but for
one check of a non-zero model index against float64 autograd, so that the set does not rest on equality alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from cova_amd import _lib as L, train as T, weights as W
from cova_amd.elements import BlobNetInfer, Context, tfrecord_example
from tests import torch_blobnet_train as TT

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _loss_bits(x):
    return np.float32(x).view(np.uint32)


class _Solo:
    """Model k's reference: a solo Trainer fed the steps in which k had a batch."""

    def __init__(self, ctx, h, w, flat, seed, max_batch, p):
        self.tr = T.Trainer(ctx, h, w, max_batch=max_batch, weights_flat=flat, seed=seed, dropout=p)

    def step(self, x, y, lr):
        loss = self.tr.step(x, y, lr=lr)
        return loss, self.tr.grads(), self.tr.metrics(), self.tr.weights()


def _run_and_compare(ctx, h, w, flats, seeds, steps, max_batch, p, check=None, device=False):
    """steps: a list of per-step lists [(stack, gt, lr) or None per model].  Runs them on a set and on one solo trainer per
    checked model, comparing loss, gradients, metrics and weights after every step; a skipped model must keep its weights
    (moving statistics included), gradients and metrics of before."""
    k_all = len(flats)
    check = list(range(k_all)) if check is None else check
    ts = T.TrainerSet(ctx, h, w, weights=flats, seeds=seeds, max_batch=max_batch, dropout=p)
    solos = {k: _Solo(ctx, h, w, flats[k], seeds[k], max_batch, p) for k in check}
    last = {k: (ts.grads(k), ts.metrics(k), ts.weights(k)) for k in check}
    try:
        for si, st in enumerate(steps):
            xs = [None if e is None else e[0] for e in st]
            ys = [None if e is None else e[1] for e in st]
            lrs = [0.0 if e is None else e[2] for e in st]
            if device:
                xa = np.concatenate([x for x in xs if x is not None])
                ya = np.concatenate([y for y in ys if y is not None])
                dx, dy = ctx.malloc(xa.nbytes), ctx.malloc(ya.nbytes)
                try:
                    ctx.h2d(dx, xa)
                    ctx.h2d(dy, ya)
                    losses = ts.step_device(dx, dy, [0 if x is None else len(x) for x in xs], lrs)
                finally:
                    ctx.free(dx)
                    ctx.free(dy)
            else:
                losses = ts.step(xs, ys, lrs)
            for k in check:
                got = (ts.grads(k), ts.metrics(k), ts.weights(k))
                if st[k] is None:
                    assert losses[k] == 0.0
                    assert _same(got[0], last[k][0]) and got[1] == last[k][1] and _same(got[2], last[k][2]), (si, k, "skipped")
                    continue
                loss, g, m, wts = solos[k].step(*st[k])
                assert _loss_bits(losses[k]) == _loss_bits(loss), (si, k, losses[k], loss)
                assert got[1] == m, (si, k, got[1], m)
                nd = int((_bits(got[0]) != _bits(g)).sum())
                assert nd == 0, f"step {si} model {k}: {nd} gradient slots differ"
                nd = int((_bits(got[2]) != _bits(wts)).sum())
                assert nd == 0, f"step {si} model {k}: {nd} weights differ"
                last[k] = got
        assert ts.step_counts == [sum(st[k] is not None for st in steps) for k in range(k_all)]
    finally:
        ts.close()
        for s in solos.values():
            s.tr.close()


def _equal_steps(h, w, k, b, n, seed, lr=1e-3):
    return [[TT.sample_batch(h, w, b, seed + 10 * s + m) + (lr,) for m in range(k)] for s in range(n)]


def test_set_of_one_equals_solo(ctx):
    h, w = 45, 80
    _run_and_compare(ctx, h, w, [T.init_weights(3)], [7], _equal_steps(h, w, 1, 4, 3, 100), 4, 0.2)


@pytest.mark.parametrize("p", [0.2, 0.0])
@pytest.mark.parametrize("hw", [(17, 33), (45, 80)])
def test_three_models_equal_batches(ctx, hw, p):
    h, w = hw
    flats = [T.init_weights(10 + k) for k in range(3)]
    _run_and_compare(ctx, h, w, flats, [5, 900, 2**40 + 3], _equal_steps(h, w, 3, 4, 3, 200), 4, p)


@pytest.mark.parametrize("hw", [(17, 33), (45, 80)])
def test_mixed_batches_skip_and_learning_rates(ctx, hw):
    """Batches (4, 1, 3) in one step, model 1 skipped in the middle step, a learning rate per model."""
    h, w = hw
    flats = [T.init_weights(20 + k) for k in range(3)]
    sb = TT.sample_batch
    steps = [
        [sb(h, w, 4, 1) + (1e-3,), sb(h, w, 1, 2) + (3e-3,), sb(h, w, 3, 3) + (5e-4,)],
        [sb(h, w, 2, 4) + (1e-3,), None, sb(h, w, 4, 5) + (5e-4,)],
        [sb(h, w, 1, 6) + (2e-3,), sb(h, w, 4, 7) + (3e-3,), sb(h, w, 3, 8) + (0.0,)],
    ]
    _run_and_compare(ctx, h, w, flats, [1, 2, 3], steps, 4, 0.2)


@pytest.mark.parametrize("hw", [(17, 33), (45, 80)])
def test_partial_batch_after_full_in_a_set(ctx, hw):
    """As test_gpu_train.test_partial_batch_is_exact, inside a set: batches of 3 and 5 on a set sized for 8 that has just taken
    full batches give the bits of solo trainers sized for 8 -- and of a solo trainer sized for 3."""
    h, w = hw
    flats = [T.init_weights(6), T.init_weights(7)]
    s8a, g8a = TT.sample_batch(h, w, 8, 30)
    s8b, g8b = TT.sample_batch(h, w, 8, 32)
    s3, g3 = TT.sample_batch(h, w, 3, 31)
    s5, g5 = TT.sample_batch(h, w, 5, 33)
    steps = [[(s8a, g8a, 0.0), (s8b, g8b, 0.0)], [(s3, g3, 0.0), (s5, g5, 0.0)]]
    _run_and_compare(ctx, h, w, flats, [21, 22], steps, 8, 0.2)
    ts = T.TrainerSet(ctx, h, w, weights=flats, seeds=[21, 22], max_batch=8)
    small = T.Trainer(ctx, h, w, max_batch=3, weights_flat=flats[0], seed=21)
    ts.step([s8a, s8b], [g8a, g8b], 0.0)
    small.step(s8a[:3], g8a[:3], lr=0.0)
    la = ts.step([s3, s5], [g3, g5], 0.0)[0]
    lb = small.step(s3, g3, lr=0.0)
    assert _loss_bits(la) == _loss_bits(lb) and ts.metrics(0) == small.metrics()
    assert _same(ts.grads(0), small.grads())
    ts.close()
    small.close()


@pytest.mark.parametrize("k", [16, 64])
def test_many_models(ctx, k):
    """The model dimension across workgroup-count boundaries: first, middle and last model against solo trainers."""
    h = w = 16
    flats = [T.init_weights(100 + m) for m in range(k)]
    rng = np.random.default_rng(k)
    bs = rng.integers(1, 5, (3, k))
    steps = [[TT.sample_batch(h, w, int(bs[s, m]), 1000 * s + m) + (1e-3,) for m in range(k)] for s in range(3)]
    _run_and_compare(ctx, h, w, flats, list(range(50, 50 + k)), steps, 4, 0.2, check=[0, k // 2, k - 1])


def test_nonzero_model_against_autograd_f64(ctx):
    """Model 2 of a set of three, batch 3 beside batches 4 and 1, against torch autograd in float64 with the bounds of
    tests/test_gpu_train.py (TT.BOUNDS: loss 1e-6, normwise 1e-4, max-norm 8e-5)."""
    h, w, p, seed = 45, 80, 0.2, 11
    flats = [T.init_weights(40 + m) for m in range(3)]
    data = [TT.sample_batch(h, w, b, 60 + b) for b in (4, 1, 3)]
    ts = T.TrainerSet(ctx, h, w, weights=flats, seeds=[9, 10, seed], max_batch=4, dropout=p)
    losses = ts.step([d[0] for d in data], [d[1] for d in data], 1e-3)
    g = ts.grads(2)
    ts.close()
    ref_loss, g_ref, _ = TT.grads_flat(flats[2], data[2][0], data[2][1], h, w, seed=seed, step=0, p=float(np.float32(p)))
    errs = TT.errors(losses[2], g, ref_loss, g_ref)
    print(", ".join(f"{kind} {v:.2e} ({n})" for kind, (v, n) in TT.worst(errs).items()))
    bad = {f"{kind} {n}": f"{v:.3g} > {TT.BOUNDS[kind]:g}" for (kind, n), v in errs.items() if not v <= TT.BOUNDS[kind]}
    assert not bad, bad


def test_device_pointer_step_equals_host_step(ctx):
    h, w = 45, 80
    flats = [T.init_weights(70 + m) for m in range(3)]
    sb = TT.sample_batch
    steps = [[sb(h, w, 4, 1) + (1e-3,), sb(h, w, 2, 2) + (1e-3,), sb(h, w, 3, 3) + (1e-3,)],
             [None, sb(h, w, 4, 4) + (1e-3,), sb(h, w, 1, 5) + (2e-3,)]]
    _run_and_compare(ctx, h, w, flats, [4, 5, 6], steps, 4, 0.2, device=True)   # the solo side steps on host pointers


def _streams(h, w, sizes, seed):
    return [TT.sample_batch(h, w, n, seed + i) for i, n in enumerate(sizes)]


def test_fit_equals_three_solo_fits(ctx):
    h, w = 17, 33
    recs = _streams(h, w, (10, 4, 7), 300)
    ts = T.TrainerSet(ctx, h, w, n_models=3, seeds=[3, 4, 5], max_batch=4)
    hist = ts.fit(recs, epochs=2, batch=4)
    for k in range(3):
        tr = T.Trainer(ctx, h, w, max_batch=4, seed=3 + k)
        href = tr.fit(recs[k], epochs=2, batch=4)
        assert _same(ts.weights(k), tr.weights()), k
        assert ts.weights_bytes(k) == tr.weights_bytes()
        assert [r["loss"] for r in hist[k]] == [r["loss"] for r in href], k
        assert [(r["precision"], r["recall"]) for r in hist[k]] == [(r["precision"], r["recall"]) for r in href]
        tr.close()
    assert ts.step_counts == [6, 2, 4]
    ts.close()


def test_cli_set_to_model_set_end_to_end(ctx, tmp_path):
    """--set on three record streams -> three weight files -> one inference model set; a mixed-id forward gives every stack
    the logits of its file loaded alone."""
    h, w = 45, 80
    names = ["cam0", "cam1", "cam2"]
    rng = np.random.default_rng(12)
    all_frames = []
    for i, name in enumerate(names):
        n = 16 + 8 * i
        frames = np.zeros((n, h, w, 4), np.uint8)
        frames[..., :3] = rng.integers(0, 7, (n, h, w, 3))
        gt = ((frames[..., 1] > 3) | (frames[..., 2] > 4)).astype(np.uint8)
        with open(tmp_path / f"{name}.tfrecord", "wb") as f:
            for j in range(0, n, 8):
                f.write(tfrecord_example(frames[j:j + 8], gt[j:j + 8], gop=8))
        all_frames.append(frames)
    out = tmp_path / "models"
    r = subprocess.run([sys.executable, "-m", "cova_amd.train", "--set", "-o", str(out), "--epochs", "2", "--seed", "5"]
                       + [str(tmp_path / f"{n}.tfrecord") for n in names], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    files = [out / f"{n}.cvhw" for n in names]
    models = [W.from_bytes(f.read_bytes()) for f in files]
    # model 1 of the CLI's set = the solo CLI's recipe on cam1's records with --seed 6
    fr, g = T.read_tfrecords([str(tmp_path / "cam1.tfrecord")], h, w)
    tr = T.Trainer(ctx, h, w, max_batch=4, seed=6)
    tr.fit(T.slide(fr, g), epochs=2, batch=4)
    assert tr.weights_bytes() == files[1].read_bytes()
    tr.close()
    b = 9
    stack = np.concatenate([all_frames[i % 3][4 * (i // 3):4 * (i // 3) + 4][::-1].reshape(1, 4 * h, w, 4) for i in range(b)])
    ids = (np.arange(b) % 3).astype(np.uint8)
    net = BlobNetInfer(ctx, models, h, w, max_batch=b)
    assert net.num_models == 3
    logits, mask = net.infer(stack, model_ids=ids)
    for k in range(3):
        one = BlobNetInfer(ctx, models[k], h, w, max_batch=b)
        l1, m1 = one.infer(stack)
        assert np.array_equal(_bits(logits[ids == k]), _bits(l1[ids == k])) and np.array_equal(mask[ids == k], m1[ids == k]), k


def test_errors(ctx):
    lib = L.lib()
    h, w = 16, 16
    cfg = L.TrainCfg()
    lib.covahip_train_default_cfg(C.byref(cfg))
    cfg.h_mb, cfg.w_mb, cfg.max_batch = h, w, 2
    good = W.to_bytes(T.init_weights(0))

    def create(blobs, n=None, seeds=None):
        ptrs = (C.c_char_p * len(blobs))(*blobs)
        sizes = (C.c_size_t * len(blobs))(*[len(b) for b in blobs])
        tr = C.c_void_p()
        rc = lib.covahip_train_create_set(ctx.handle, C.byref(cfg), len(blobs) if n is None else n, ptrs, sizes, seeds, C.byref(tr))
        return rc, tr

    rc, tr = create([good, good[:-4], good])                       # a bad blob in the middle slot
    assert rc == 6 and not tr.value
    rc, tr = create([good, good, b"x" * 80])
    assert rc == 6 and not tr.value
    assert create([good], n=0)[0] == 1 and create([good], n=257)[0] == 1
    rc, tr = create([good, good, good])                            # seeds NULL: cfg.seed for all
    assert rc == 0 and tr.value
    n = C.c_int()
    assert lib.covahip_train_num_models(tr, C.byref(n)) == 0 and n.value == 3
    x, y = TT.sample_batch(h, w, 6, 1)
    loss = C.c_float()
    losses = (C.c_float * 3)()
    lrs = (C.c_float * 3)(1e-3, 1e-3, 1e-3)

    def step(batches, lrs_=lrs, losses_=losses, stack=x.ctypes.data, gt=y.ctypes.data, kind=L.MEM_HOST):
        bt = None if batches is None else (C.c_int32 * 3)(*batches)
        return lib.covahip_train_step_set(tr, stack, gt, bt, lrs_, losses_, kind)

    assert lib.covahip_train_step(tr, x.ctypes.data, y.ctypes.data, 1, 1e-3, C.byref(loss), L.MEM_HOST) == 1   # a set of three
    assert step([0, 0, 0]) == 1 and step([1, 3, 1]) == 1 and step([1, -1, 1]) == 1
    assert step(None) == 1 and step([1, 1, 1], lrs_=None) == 1 and step([1, 1, 1], losses_=None) == 1
    assert step([1, 1, 1], stack=None) == 1 and step([1, 1, 1], gt=None) == 1 and step([1, 1, 1], kind=7) == 1
    assert step([1, 1, 1], lrs_=(C.c_float * 3)(1e-3, float("nan"), 1e-3)) == 1
    v = (C.c_int64 * 3)()
    sz = C.c_size_t()
    g = np.empty(W.N_PARAMS, np.float32)
    for bad in (-1, 3):
        assert lib.covahip_train_metrics_m(tr, bad, v) == 1
        assert lib.covahip_train_weights_m(tr, bad, None, 0, C.byref(sz)) == 1
        assert lib.covahip_train_grads_m(tr, bad, g.ctypes.data, g.size) == 1
    before = bytes(good)
    assert step([2, 0, 2]) == 0 and losses[1] == 0.0 and losses[0] > 0 and losses[2] > 0
    buf = np.zeros(len(good), np.uint8)
    assert lib.covahip_train_weights_m(tr, 1, buf.ctypes.data, buf.size, C.byref(sz)) == 0 and buf.tobytes() == before
    assert lib.covahip_train_weights_m(tr, 2, buf.ctypes.data, buf.size, C.byref(sz)) == 0 and buf.tobytes() != before
    assert lib.covahip_train_weights(tr, buf.ctypes.data, 8, C.byref(sz)) == 7 and sz.value == len(good)      # model 0, overflow
    lib.covahip_train_destroy(tr)
