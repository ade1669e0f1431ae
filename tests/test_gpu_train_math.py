"""BlobNet training with the convolutions on the matrix cores (covahip_train_set_math, COVAHIP_TRAIN_MATH_MATRIX; include/covahip.h,
"Training arithmetic"): the trainer's own checks repeated in matrix mode, at the project's own bounds.

1. Gradients against f64 autograd (tests/torch_blobnet_train.py, its BOUNDS unchanged).  The matrix kernels keep the slab split of
   the plain ones (wg_slabs: 1,024 positions per slab), so the cases are the plain kernels' smallest that reach every branch:
     16x16 b1          1x1 bottleneck; one slab in every weight gradient; tiles of 64 positions holding several rows and, at
                       levels 2 and 3, fewer than 64 positions in all
     17x33 b2 of 5     odd at every level, stale rows of a larger batch behind the model's own; level 0 has five slabs, the last
                       two positions short, level 1 two
     24x50 b3          parity differs by level; level 0 fifteen slabs, level 1 four
     33x36 b4          two slabs in the last convT block (its 1,224 input positions), tiles that span samples
     16x523 b1         rows wider than a tile in every new kernel: level 3 rows of 66 (> 64, conv kernels), the first convT block's
                       of 33 (> 32); levels 0 - 2 and the last convT block with 33 / 9 / 3 / 3 slabs, each with a shorter last one
2. The bitwise guarantees, each at 17x33.  3. Sets against solo trainers, with a skipped model.  4. Plan, post, evaluation and
resume.  5. Switching between the modes.  6. The kernels of a step pinned through the ctx profile.  7. Learning: the recipe of
tests/test_gpu_train.py::test_learns_synthetic_ellipses at 300 steps in both modes."""
import ctypes as C

import numpy as np
import pytest

from cova_amd import _lib as L, train as T, weights as W
from cova_amd.elements import BlobNetInfer, Context
from tests import torch_blobnet_finetune as FT
from tests import torch_blobnet_post as TP
from tests import torch_blobnet_train as TT
from tests.torch_blobnet_train import BOUNDS, Case, errors, excess, worst
from tests.test_gpu_train import _assert_metrics, _iou, _streams
from tests.test_gpu_train_data import _batch, _data, _frames, _mixed
from tests.test_gpu_train_eval import _eval_raw, _reference, _weights
from tests.test_gpu_train_post import _assert_metrics_post

pytestmark = pytest.mark.gpu
EXACT, MATRIX = 0, 1
INVALID_ARG = 1
PLAIN = {"k_conv3_wgrad", "k_convT_wgrad", "k_conv3_fwd", "k_conv3_dgrad"}
MATRIX_KERNELS = {"k_conv3_wgrad_mm", "k_convT_wgrad_mm", "k_conv3_mm_fwd", "k_conv3_mm_dgrad"}
H, Wd = 17, 33

CASES = [
    Case(16, 16, 1, 1, 0.2),
    Case(17, 33, 2, 5, 0.5, steps=2),
    Case(24, 50, 3, 3, 0.0),
    Case(33, 36, 4, 4, 0.2),
    Case(16, 523, 1, 1, 0.2),
]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _trainer(ctx, h, w, math="matrix", **kw):
    tr = T.Trainer(ctx, h, w, **kw)
    tr.set_math(math)
    assert tr.math == math
    return tr


def _check(what, errs, bounds=BOUNDS):
    print(f"{what}: " + ", ".join(f"{k} {v:.2e} ({n})" for k, (v, n) in worst(errs).items()) + f"; {excess(errs):.3f} of the bounds")
    bad = {f"{k} {n}": f"{v:.3g} > {bounds[k]:g}" for (k, n), v in errs.items() if not v <= bounds[k]}
    assert not bad, (what, bad)


def _snap(tr):
    s = getattr(tr, "_set", tr)
    return [(s.grads(k).tobytes(), s.metrics(k)) for k in range(s.n_models)] + [s.state_bytes(), list(s.step_counts)]


# ------------------------------------------------------------------------------------------------ 1. against f64 autograd
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_gradients_match_torch_f64_in_matrix_mode(ctx, case):
    flat, pre, stack, gt = case.inputs()
    tr = _trainer(ctx, case.h, case.w, max_batch=case.max_batch, weights_flat=flat, seed=case.seed, dropout=case.p)
    try:
        for st, g in pre:
            tr.step(st, g, lr=0.0)
        loss = tr.step(stack, gt)
        g, counts = tr.grads(), tr.metrics()
    finally:
        tr.close()
    ref_loss, g_ref, logit = case.reference()
    _check(f"matrix {case.id}", errors(loss, g, ref_loss, g_ref))
    _assert_metrics(counts, logit, gt)


# ------------------------------------------------------------------------------------------------ 2. bitwise properties
def test_two_runs_are_bit_identical(ctx):
    flat = T.init_weights(9)
    outs = []
    for _ in range(2):
        tr = _trainer(ctx, H, Wd, max_batch=4, weights_flat=flat, seed=5, dropout=0.2)
        losses = [tr.step(*TT.sample_batch(H, Wd, 4, 40 + k)) for k in range(4)]
        outs.append((_bits(losses).tolist(), _snap(tr), tr.weights().tobytes()))
        tr.close()
    assert outs[0] == outs[1]


def test_partial_batch_after_a_full_one_is_exact(ctx):
    flat = T.init_weights(6)
    s5, g5 = TT.sample_batch(H, Wd, 5, 30)
    s2, g2 = TT.sample_batch(H, Wd, 2, 31)
    outs = []
    for mb, first in ((5, (s5, g5)), (2, (s5[:2], g5[:2]))):
        tr = _trainer(ctx, H, Wd, max_batch=mb, weights_flat=flat, seed=21, dropout=0.2)
        tr.step(*first, lr=0.0)
        loss = tr.step(s2, g2, lr=0.0)
        outs.append((_bits(loss).tolist(), tr.grads().tobytes(), tr.metrics()))
        tr.close()
    assert outs[0] == outs[1]


def test_device_pointer_steps_equal_host_pointer_steps(ctx):
    flat = T.init_weights(10)
    batches = [TT.sample_batch(H, Wd, b, 60 + k) for k, b in enumerate((3, 2))]
    outs = []
    for dev in (False, True):
        tr = _trainer(ctx, H, Wd, max_batch=3, weights_flat=flat, seed=4, dropout=0.2)
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
            res.append((_bits(loss).tolist(), _snap(tr)))
        outs.append(res)
        tr.close()
    assert outs[0] == outs[1]


def test_step_data_equals_the_pointer_form(ctx):
    frames, gt = _frames(2, 20, H, Wd)
    flat = T.init_weights(5)
    d = _data(ctx, frames, gt)
    a = _trainer(ctx, H, Wd, max_batch=4, weights_flat=flat, seed=3)
    b = _trainer(ctx, H, Wd, max_batch=4, weights_flat=flat, seed=3)
    try:
        samples = _mixed(20, 8, 7)
        for i in range(2):
            s = samples[i * 4:(i + 1) * 4]
            la = a.step_data(d, s)
            lb = b.step(*_batch(frames, gt, s, packed=False))
            assert _bits(la).tolist() == _bits(lb).tolist() and np.isfinite(la)
            assert _snap(a) == _snap(b)
    finally:
        a.close()
        b.close()
        d.close()


# ------------------------------------------------------------------------------------------------ 3. sets
def test_set_models_equal_solo_trainers_with_a_model_skipped(ctx):
    k, mb, p = 3, 4, 0.2
    flats = [T.init_weights(20 + m) for m in range(k)]
    seeds = [7, 8, 9]
    steps = [((4, 1, 3), (1e-3, 2e-3, 5e-4)), ((2, 0, 4), (1e-3, 2e-3, 5e-4))]
    ts = T.TrainerSet(ctx, H, Wd, weights=flats, seeds=seeds, max_batch=mb, dropout=p)
    ts.set_math("matrix")
    assert ts.math == "matrix"
    solos = [_trainer(ctx, H, Wd, max_batch=mb, weights_flat=flats[m], seed=seeds[m], dropout=p) for m in range(k)]
    try:
        for i, (bs, lrs) in enumerate(steps):
            data = [TT.sample_batch(H, Wd, b, 80 + 10 * i + m) if b else None for m, b in enumerate(bs)]
            before = (ts.weights_bytes(1), ts.step_counts[1])
            losses = ts.step([d[0] if d else None for d in data], [d[1] if d else None for d in data], lrs=list(lrs))
            for m, b in enumerate(bs):
                if not b:     # skipped: weights and step counter as they were
                    assert (ts.weights_bytes(m), ts.step_counts[m]) == before
                    continue
                lo = solos[m].step(*data[m], lr=lrs[m])
                assert _bits(losses[m]).tolist() == _bits(lo).tolist(), (i, m)
                assert ts.grads(m).tobytes() == solos[m].grads().tobytes(), (i, m)
                assert ts.metrics(m) == solos[m].metrics(), (i, m)
                assert ts.weights_bytes(m) == solos[m].weights_bytes(), (i, m)
        assert list(ts.step_counts) == [2, 1, 2]
    finally:
        ts.close()
        for s in solos:
            s.close()


# ------------------------------------------------------------------------------------------------ 4. plan, post, eval, resume
def test_step_under_a_plan_matches_torch_f64(ctx):
    case = next(c for c in FT.CASES if c.id == "17x33-p0.2-b-encoder")
    plan = dict(case.plan, bn_inference="all")       # the encoder frozen and every BN layer in inference mode
    flat, pre, stack, gt = case.inputs()
    tr = _trainer(ctx, case.h, case.w, max_batch=FT.MAX_BATCH, weights_flat=flat, seed=case.seed, dropout=case.p, **plan)
    try:
        tr.step(*pre, lr=0.0)
        now = tr.weights()
        loss = tr.step(stack, gt)
        g, after = tr.grads(), tr.weights()
    finally:
        tr.close()
    ref_loss, g_ref, _ = FT.grads_flat_plan(now, stack, gt, case.h, case.w, **plan, seed=case.seed, step=1, p=case.p32)
    _check("matrix plan", FT.errors(loss, g, ref_loss, g_ref, **plan), FT.BOUNDS)
    frozen, _ = FT.effective(**plan)
    wa, wb, gu = W.unflatten(flat), W.unflatten(after), W.unflatten(g)
    moved = 0
    for name in wa:
        if FT.group_of(name) in frozen or name.endswith((".bn.mean", ".bn.var")):
            assert (_bits(wa[name]) == _bits(wb[name])).all(), name      # frozen tensors and moving statistics: bit-unchanged
            if not name.endswith((".bn.mean", ".bn.var")):
                assert not gu[name].any(), name
        else:
            moved += int((_bits(wa[name]) != _bits(wb[name])).sum())
    assert moved


def test_step_with_a_post_matches_masked_torch_f64(ctx):
    geo = TP.GEOMETRIES[0]
    h, w, b, p, seed = geo
    flat, stack, gt = TP.inputs(h, w, b)
    keep = TP.keep_map(h, w)
    ref_loss, g_ref, logit_ref = TP.reference(*geo)
    tr = _trainer(ctx, h, w, max_batch=b, weights_flat=flat, seed=seed, dropout=p)
    try:
        tr.set_post(logit_thresh=0.5, keep=keep)
        loss = tr.step(stack, gt)
        g, counts = tr.grads(), tr.metrics()
    finally:
        tr.close()
    _check("matrix post", errors(loss, g, ref_loss, g_ref))
    _assert_metrics_post(counts, logit_ref, gt, keep, 0.5)


def test_evaluation_matches_torch_f64(ctx):
    flat = _weights(3)
    stack, gt = TT.sample_batch(H, Wd, 7, 5)
    tr = _trainer(ctx, H, Wd, max_batch=3, weights_flat=flat, seed=0)
    try:
        res, sl, lg = _eval_raw(tr, stack, gt)           # chunks of 3 and a partial last one
    finally:
        tr.close()
    logit_ref, loss_ref = _reference(flat, stack, gt, H, Wd)
    rel = abs(res.loss - loss_ref.mean()) / abs(loss_ref.mean())
    print(f"matrix eval: mean loss rel {rel:.2e}")
    assert res.samples == 7 and rel <= BOUNDS["loss"], rel
    _assert_metrics((res.tp, res.fp, res.fn), logit_ref, gt)


def test_resume_is_exact_and_blobs_cross_the_modes(ctx):
    flat = T.init_weights(14)
    batches = [TT.sample_batch(H, Wd, 3, 90 + k) for k in range(4)]

    def run(math, upto, state=None):
        tr = _trainer(ctx, H, Wd, math, max_batch=3, weights_flat=flat, seed=6, dropout=0.2)
        try:
            first = 0
            if state is not None:
                tr.load_state_bytes(state)
                first = tr.step_count
            losses = [_bits(tr.step(*batches[k])).tolist() for k in range(first, upto)]
            return losses, _snap(tr), tr.state_bytes()
        finally:
            tr.close()

    four = run("matrix", 4)
    two = run("matrix", 2)
    rest = run("matrix", 4, two[2])
    assert two[0] + rest[0] == four[0] and rest[1] == four[1]
    # a blob of either mode loads in the other, and continues there as a trainer of that mode that had the same two steps would
    ex_two = run("exact", 2)
    crossed = run("matrix", 4, ex_two[2])
    back = run("exact", 4, two[2])
    assert crossed[1][-1] == [4] and back[1][-1] == [4]
    assert crossed[1] != four[1] and back[1] != four[1]          # (the first two steps were the other mode's)


# ------------------------------------------------------------------------------------------------ 5. switching
def test_switching(ctx):
    flat = T.init_weights(9)
    batches = [TT.sample_batch(H, Wd, 4, 40 + k) for k in range(4)]
    lib = L.lib()

    def four(prepare):
        tr = T.Trainer(ctx, H, Wd, max_batch=4, weights_flat=flat, seed=5, dropout=0.2)
        try:
            prepare(tr)
            return [_bits(tr.step(*b)).tolist() for b in batches], _snap(tr)
        finally:
            tr.close()

    def there_and_back(tr):
        got = C.c_int(-1)
        assert lib.covahip_train_get_math(tr.handle, C.byref(got)) == 0 and got.value == EXACT
        assert lib.covahip_train_set_math(tr.handle, MATRIX) == 0
        assert lib.covahip_train_get_math(tr.handle, C.byref(got)) == 0 and got.value == MATRIX
        assert lib.covahip_train_set_math(tr.handle, 7) == INVALID_ARG
        assert lib.covahip_train_set_math(tr.handle, -1) == INVALID_ARG
        assert lib.covahip_train_get_math(tr.handle, C.byref(got)) == 0 and got.value == MATRIX
        assert lib.covahip_train_set_math(tr.handle, EXACT) == 0
        assert lib.covahip_train_get_math(tr.handle, C.byref(got)) == 0 and got.value == EXACT
        assert lib.covahip_train_set_math(None, EXACT) == INVALID_ARG and lib.covahip_train_get_math(tr.handle, None) == INVALID_ARG

    assert four(there_and_back) == four(lambda tr: None)
    with pytest.raises(ValueError):
        four(lambda tr: tr.set_math("fast"))
    # one matrix step against one exact step on the same batch: the same gradient within the bounds' scale, not the same bits
    grads = {}
    for math in T.MATH_MODES:
        tr = _trainer(ctx, H, Wd, math, max_batch=4, weights_flat=flat, seed=5, dropout=0.2)
        tr.step(*batches[0])
        grads[math] = tr.grads()
        tr.close()
    diff = _bits(grads["exact"]) != _bits(grads["matrix"])
    print(f"{int(diff.sum())} of {diff.size} gradient slots differ in a bit between the modes")
    assert diff.any()


# ------------------------------------------------------------------------------------------------ 6. the kernels of a step
def test_kernels_of_a_step_through_the_profile(ctx):
    flat = T.init_weights(2)
    stack, gt = TT.sample_batch(H, Wd, 2, 3)
    seen = {}
    for math in T.MATH_MODES:
        tr = _trainer(ctx, H, Wd, math, max_batch=2, weights_flat=flat, seed=1)
        try:
            ctx.profile(True)
            tr.step(stack, gt)
            seen[math] = ctx.profile_read()
        finally:
            ctx.profile(False)
            tr.close()
        print(math, sorted((n, c) for n, (_, c) in seen[math].items()))
    assert MATRIX_KERNELS <= set(seen["matrix"]) and not PLAIN & set(seen["matrix"])
    assert PLAIN <= set(seen["exact"]) and not MATRIX_KERNELS & set(seen["exact"])
    launches = {m: {n: c for n, (_, c) in seen[m].items()} for m in seen}
    assert launches["matrix"]["k_conv3_mm_fwd"] == launches["exact"]["k_conv3_fwd"] == 4
    assert launches["matrix"]["k_conv3_mm_dgrad"] == launches["exact"]["k_conv3_dgrad"] == 3
    assert launches["matrix"]["k_conv3_wgrad_mm"] == launches["exact"]["k_conv3_wgrad"] == 4
    assert launches["matrix"]["k_convT_wgrad_mm"] == launches["exact"]["k_convT_wgrad"] == 4
    # nothing else changes: every other kernel launches as often in either mode
    rest = {m: {n: c for n, c in launches[m].items() if n not in PLAIN | MATRIX_KERNELS} for m in launches}
    assert rest["matrix"] == rest["exact"]
    # frozen groups launch no weight-gradient work, and the backward stops where the plan says: the encoder frozen
    tr = _trainer(ctx, H, Wd, max_batch=2, weights_flat=flat, seed=1, freeze="encoder")
    try:
        ctx.profile(True)
        tr.step(stack, gt)
        names = ctx.profile_read()
    finally:
        ctx.profile(False)
        tr.close()
    assert "k_conv3_wgrad_mm" not in names and "k_conv3_mm_dgrad" not in names and names["k_convT_wgrad_mm"][1] == 4


# ------------------------------------------------------------------------------------------------ 7. learning
LEARN_STEPS = 300


def test_learns_synthetic_ellipses_as_the_exact_mode_does(ctx):
    h, w, b = 45, 80, 8
    tr_x, tr_y = _streams(range(100, 108), 40, h, w)
    te_x, te_y = _streams((777, 778), 20, h, w)
    flat0 = T.init_weights(1)
    ious = {}
    for math in T.MATH_MODES:
        tr = _trainer(ctx, h, w, math, max_batch=b, weights_flat=flat0, seed=1)
        rng = np.random.default_rng(0)
        for _ in range(LEARN_STEPS):
            idx = rng.choice(tr_x.shape[0], b, replace=False)
            tr.step(tr_x[idx], tr_y[idx])
        flat = tr.weights()
        tr.close()
        net = BlobNetInfer(ctx, flat, h, w, max_batch=te_x.shape[0])
        ious[math] = _iou(net.infer(te_x, want_logits=False)[1], te_y)
    print(f"held-out IoU after {LEARN_STEPS} steps: exact {ious['exact']:.3f}, matrix {ious['matrix']:.3f}")
    assert ious["matrix"] >= ious["exact"] - 0.02, ious
