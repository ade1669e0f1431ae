"""Training and evaluation with a post (covahip_train_set_post; include/covahip.h, "Training with a post"): the step against
the masked f64 reference of tests/torch_blobnet_post.py within tests/torch_blobnet_train.py's BOUNDS (shown to tell a post from
no post by tests/test_train_post_host.py), the evaluation's counts exactly against numpy and against covahip_post_sweep on
the evaluation's own logits, Contracts F (an all-ones keep map changes no float) and G (what is ignored does not exist), sets
against solo trainers, a post under a training plan across save / load, the errors, and the command line."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from cova_amd import _lib as L, calibrate, train as T
from cova_amd.elements import Context, keep_from_rects, tfrecord_example
from tests import torch_blobnet_post as TP
from tests import torch_blobnet_train as TT
from tests.golden_util import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRIC_BAND = 1e-3   # |logit - threshold| below which the f32 and the f64 side may disagree (tests/test_gpu_train.py's band)
GEO = pytest.mark.parametrize("geo", TP.GEOMETRIES, ids=TP.IDS)
N_EVAL, EVAL_MB = 7, 3   # seven samples in chunks of three: two full chunks and a partial last one


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return len(a) == len(b) and all((x == y).all() if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def _trainer(ctx, geo, max_batch=None, **kw):
    h, w, b, p, seed = geo
    return T.Trainer(ctx, h, w, max_batch=max_batch or b, weights_flat=TP.inputs(h, w, b)[0], seed=seed, dropout=p, **kw)


def _held_out(h, w):
    return TT.sample_batch(h, w, N_EVAL, 6)


def _snap(tr):
    """Everything a step leaves behind: gradients, metrics and the state blob (weights, moving statistics, Adam moments)."""
    return _bits(tr.grads()).copy(), tr.metrics(), tr.state_bytes()


def _eval_snap(ev):
    return (ev["loss"], ev["precision"], ev["recall"], ev["iou"], ev["samples"], _bits(ev["sample_loss"]).copy(),
            _bits(ev["logits"]).copy())


def _counts(tr, stack, gt):
    """covahip_train_eval through the binding, keeping the integer counts: ((tp, fp, fn), sample_loss, logits, mean loss)."""
    n = stack.shape[0]
    stack, gt = np.ascontiguousarray(stack), np.ascontiguousarray(gt)
    sl = np.full(n, np.nan, np.float32)
    lg = np.full((n, tr.h, tr.w), np.nan, np.float32)
    res = L.TrainEvalResult()
    L.check(tr._lib.covahip_train_eval(tr.handle, stack.ctypes.data, gt.ctypes.data, n, sl.ctypes.data, lg.ctypes.data,
                                       C.byref(res), L.MEM_HOST), "covahip_train_eval", tr.ctx.handle)
    assert res.samples == n
    return (res.tp, res.fp, res.fn), sl, lg, res.loss


def _run(tr, steps, held):
    """The losses and snapshots of `steps` and an evaluation of `held` afterwards."""
    out = []
    for s, g in steps:
        out.append((np.float32(tr.step(s, g)).view(np.uint32), *_snap(tr)))
    ev = tr.evaluate(held, want_sample_loss=True, want_logits=True)
    return out, _eval_snap(ev)


def _steps(h, w, b, n=3):
    return [TT.sample_batch(h, w, b, 40 + k) for k in range(n)]


# ------------------------------------------------------------------------------------------------ 1. the step against f64
def _assert_metrics_post(counts, logit_ref, gt, keep, thr):
    """The rule of tests/test_gpu_train.py::_assert_metrics with the band centred on the threshold and everything restricted
    to kept pixels; the cap on band pixels is asserted on the reference alone."""
    tp, fp, fn = counts
    kp = np.broadcast_to(keep != 0, gt.shape)
    lab = gt.astype(bool) & kp
    bg = ~gt.astype(bool) & kp
    pos = logit_ref > thr
    near = (np.abs(logit_ref - thr) < METRIC_BAND) & kp
    cap = max(2, 0.005 * int(kp.sum()))
    print(f"  threshold {thr}: {int(near.sum())} band pixels (cap {cap:.0f}), counts {counts}")
    assert near.sum() <= cap, int(near.sum())
    assert tp + fn == int(lab.sum()), (counts, int(lab.sum()))
    assert abs(tp - int((pos & lab).sum())) <= int((near & lab).sum()), (counts, int((pos & lab).sum()))
    assert abs(fp - int((pos & bg).sum())) <= int((near & bg).sum()), (counts, int((pos & bg).sum()))


@GEO
def test_step_with_a_post_matches_masked_torch_f64(ctx, geo):
    h, w, b, p, seed = geo
    _, stack, gt = TP.inputs(h, w, b)
    keep = TP.keep_map(h, w)
    ref_loss, g_ref, logit_ref = TP.reference(*geo)
    first = None
    for thr in (0.0, 0.5):
        tr = _trainer(ctx, geo)
        try:
            tr.set_post(logit_thresh=thr, keep=keep)
            got_thr, got_keep = tr.get_post()
            assert got_thr == thr and (got_keep == keep).all()
            loss = tr.step(stack, gt)
            g, counts = tr.grads(), tr.metrics()
        finally:
            tr.close()
        errs = TT.errors(loss, g, ref_loss, g_ref)
        print(f"{TP.IDS[TP.GEOMETRIES.index(geo)]} threshold {thr}: " + ", ".join(f"{k} {v:.2e} ({n})" for k, (v, n) in TT.worst(errs).items()))
        bad = {f"{k} {n}": f"{v:.3g} > {TT.BOUNDS[k]:g}" for (k, n), v in errs.items() if not v <= TT.BOUNDS[k]}
        assert not bad, bad
        _assert_metrics_post(counts, logit_ref, gt, keep, thr)
        if first is None:
            first = (loss, _bits(g).copy())
        else:   # the threshold moves the counts only
            assert loss == first[0] and (_bits(g) == first[1]).all()


# ------------------------------------------------------------------------------------------------ 2. the evaluation, exactly
@GEO
def test_evaluation_counts_are_exact_and_sample_loss_matches_f64(ctx, geo):
    h, w = geo[:2]
    keep = TP.keep_map(h, w)
    stack, gt = _held_out(h, w)
    tr = _trainer(ctx, geo, max_batch=EVAL_MB)
    try:
        tr.set_post(keep=keep)
        _, _, lg0, _ = _counts(tr, stack, gt)
        thresholds = [0.0, float(np.float32(np.quantile(lg0, 0.7)))]
        for thr in thresholds:
            tr.set_post(logit_thresh=thr, keep=keep)
            (tp, fp, fn), sl, lg, mean_loss = _counts(tr, stack, gt)
            assert (_bits(lg) == _bits(lg0)).all()
            kp = np.broadcast_to(keep != 0, gt.shape)
            pos, lab = (lg > np.float32(thr)) & kp, (gt != 0) & kp
            want = (int((pos & lab).sum()), int((pos & ~lab).sum()), int((~pos & lab).sum()))
            print(f"  threshold {thr}: tp, fp, fn {(tp, fp, fn)}")
            assert (tp, fp, fn) == want
            assert thr == 0.0 or min(want) > 0                         # (at the quantile every count is exercised)
            sw = calibrate.sweep(ctx, lg, gt, thresholds=[thr], areas=(1,), keep=keep)
            assert tuple(int(v) for v in sw["pixel"][0]) == want       # two GPU paths, one rule
            ref = TP.sample_loss_f64(lg, gt, keep)
            rel = np.abs(sl.astype(np.float64) - ref) / np.abs(ref)
            print(f"  per-sample loss rel {rel.max():.2e}")
            assert (rel <= TT.BOUNDS["loss"]).all(), rel
            assert abs(mean_loss - float(np.mean(sl.astype(np.float64)))) <= 1e-12 * abs(mean_loss)
            unmasked = TP.sample_loss_f64(lg, gt, np.ones_like(keep))
            assert (np.abs(unmasked - ref) / np.abs(ref) > 100 * TT.BOUNDS["loss"]).any()   # (the mask matters here)
    finally:
        tr.close()


# ------------------------------------------------------------------------------------------------ 3. Contract F
@GEO
def test_contract_f_an_all_ones_keep_map_changes_no_float(ctx, geo):
    h, w, b = geo[:3]
    steps, held = _steps(h, w, b), _held_out(h, w)
    ones = np.ones((h, w), np.uint8)
    ones[::2, 1::3] = 7                                                  # non-zero is kept, whatever the value
    runs = {}
    for name, post in (("none", None), ("ones", dict(logit_thresh=0.5, keep=ones)), ("null", dict(logit_thresh=0.5)),
                       ("ones0", dict(logit_thresh=0.0, keep=ones))):
        tr = _trainer(ctx, geo, max_batch=max(b, EVAL_MB))
        try:
            if post:
                tr.set_post(**post)
            assert (tr.get_post() is None) == (post is None)
            runs[name] = _run(tr, steps, held)
        finally:
            tr.close()
    (st0, ev0) = runs["none"]
    lg = ev0[6].view(np.float32)
    assert not ((lg > 0) & (lg <= 1e-6)).any()                           # sigmoid > 0.5 and logit > 0 agree on these logits
    for name in ("ones", "null", "ones0"):
        st, ev = runs[name]
        for k, (a, c) in enumerate(zip(st0, st)):
            assert a[0] == c[0] and (a[1] == c[1]).all() and a[3] == c[3], f"{name}: step {k}"   # loss, gradients, state blob
        assert ev[0] == ev0[0] and (ev[5] == ev0[5]).all() and (ev[6] == ev0[6]).all(), name       # loss, sample_loss, logits
    st, ev = runs["ones0"]                                               # at threshold 0 the counts are those without a post
    assert [s[2] for s in st] == [s[2] for s in st0] and ev[1:4] == ev0[1:4]
    assert runs["ones"][0][-1][2] != st0[-1][2] and _same(runs["ones"][1], runs["null"][1])   # at 0.5 they follow the threshold
    assert [s[2] for s in runs["ones"][0]] == [s[2] for s in runs["null"][0]]


# ------------------------------------------------------------------------------------------------ 4. Contract G
@GEO
def test_contract_g_what_is_ignored_does_not_exist(ctx, geo):
    h, w, b = geo[:3]
    keep = TP.keep_map(h, w)
    steps, held = _steps(h, w, b), _held_out(h, w)

    def scribble(gt):
        g = gt.copy()
        g[:, keep == 0] ^= 1
        g[0, keep == 0] = 255
        g[-1, h - 1, w - 1] = 3
        assert (g[:, keep != 0] == gt[:, keep != 0]).all() and (g != gt).any()
        return g

    outs = []
    for change in (False, True):
        tr = _trainer(ctx, geo, max_batch=max(b, EVAL_MB))
        try:
            tr.set_post(logit_thresh=0.25, keep=keep)
            outs.append(_run(tr, [(s, scribble(g) if change else g) for s, g in steps],
                             (held[0], scribble(held[1]) if change else held[1])))
        finally:
            tr.close()
    (sa, ea), (sb, eb) = outs
    for k, (a, c) in enumerate(zip(sa, sb)):
        assert _same(a, c), f"step {k}"
    assert _same(ea, eb)


# ------------------------------------------------------------------------------------------------ 5. sets
@pytest.mark.parametrize("h,w", [(17, 33), (24, 50)])
def test_set_models_equal_their_solo_trainers_and_do_not_see_each_others_posts(ctx, h, w):
    K, mb, p = 3, 3, 0.2
    flats = [T.init_weights(20 + k) for k in range(K)]
    seeds = [5, 6, 7]
    posts = [None, dict(logit_thresh=0.5, keep=TP.keep_map(h, w)),
             dict(logit_thresh=-0.25, keep=keep_from_rects(h, w, [(0, 0, 48, 32), (16 * (w - 1), 0, 16, 16 * h)]))]
    sizes = [(3, 2, 3), (3, 0, 3), (3, 2, 3)]                            # model 1 sits the second step out
    steps = [[TT.sample_batch(h, w, n, 100 + 10 * i + k) if n else None for k, n in enumerate(bs)] for i, bs in enumerate(sizes)]
    held = [TT.sample_batch(h, w, n, 150 + k) for k, n in enumerate((4, 2, 5))]
    lrs = [1e-3, 2e-3, 5e-4]

    def run_set(toggle):
        ts = T.TrainerSet(ctx, h, w, weights=flats, seeds=seeds, max_batch=mb, dropout=p)
        try:
            for k, post in enumerate(posts):
                if post:
                    ts.set_post(k, **post)
            out = [[] for _ in range(K)]
            for i, st in enumerate(steps):
                if toggle and i == 1:                                     # model 1 sits this step out: nothing of it runs
                    ts.reset_post(1)
                    assert ts.get_post(1) is None and ts.get_post(2) is not None
                if toggle and i == 2:
                    ts.set_post(1, logit_thresh=-1.0)                     # another post than before: model 1 may move
                losses = ts.step([None if r is None else r[0] for r in st], [None if r is None else r[1] for r in st], lrs)
                for k in range(K):
                    if st[k] is not None:
                        out[k].append((np.float32(losses[k]).view(np.uint32), _bits(ts.grads(k)).copy(), ts.metrics(k),
                                       _bits(ts.weights(k)).copy()))
            evs = ts.evaluate(held, want_sample_loss=True, want_logits=True)
            return out, [_eval_snap(e) for e in evs], ts.state_bytes()
        finally:
            ts.close()

    got, got_ev, _ = run_set(False)
    for k in range(K):
        tr = T.Trainer(ctx, h, w, max_batch=mb, weights_flat=flats[k], seed=seeds[k], dropout=p)
        try:
            if posts[k]:
                tr.set_post(**posts[k])
            solo = []
            for st in steps:
                if st[k] is not None:
                    loss = tr.step(*st[k], lr=lrs[k])
                    solo.append((np.float32(loss).view(np.uint32), _bits(tr.grads()).copy(), tr.metrics(), _bits(tr.weights()).copy()))
            ev = _eval_snap(tr.evaluate(held[k], want_sample_loss=True, want_logits=True))
        finally:
            tr.close()
        assert len(solo) == len(got[k])
        for i, (a, c) in enumerate(zip(solo, got[k])):
            assert _same(a, c), f"model {k}, its step {i}"
        assert _same(ev, got_ev[k]), f"model {k}: evaluation"
    moved, moved_ev, _ = run_set(True)
    for k in (0, 2):
        for i, (a, c) in enumerate(zip(got[k], moved[k])):
            assert _same(a, c), f"model {k} moved at step {i} when model 1's post changed"
        assert _same(got_ev[k], moved_ev[k])
    assert not _same(got[1][-1], moved[1][-1])                           # (model 1 did take the other post)


# ------------------------------------------------------------------------------------------------ 6. with a plan, across resume
def test_post_with_a_plan_across_save_and_load(ctx):
    geo = TP.GEOMETRIES[0]
    h, w, b = geo[:3]
    keep = TP.keep_map(h, w)
    steps = _steps(h, w, b, 4)
    post = dict(logit_thresh=0.5, keep=keep)

    def go(tr, some):
        return [(np.float32(tr.step(s, g)).view(np.uint32), *_snap(tr)) for s, g in some]

    a = _trainer(ctx, geo, freeze="encoder")
    try:
        a.set_post(**post)
        whole = go(a, steps)
    finally:
        a.close()
    c = _trainer(ctx, geo, freeze="encoder")
    try:
        c.set_post(**post)
        go(c, steps[:2])
        blob = c.state_bytes(epoch=2)
    finally:
        c.close()
    outs = {}
    for again in (True, False):
        d = T.Trainer(ctx, h, w, max_batch=b, weights_flat=T.init_weights(99), seed=1234, dropout=geo[3], freeze="encoder")
        try:
            if again:
                d.set_post(**post)
            assert d.load_state_bytes(blob) == 2
            assert (d.get_post() is not None) == again                   # a load does not touch the post
            outs[again] = go(d, steps[2:])
        finally:
            d.close()
    for k, (x, y) in enumerate(zip(whole[2:], outs[True])):
        assert _same(x, y), f"step {2 + k} after the load"
    assert outs[False][0][0] != whole[2][0]                              # the blob does not carry the post


# ------------------------------------------------------------------------------------------------ 7. errors and the command line
def test_errors_leave_the_trainer_untouched(ctx):
    geo = TP.GEOMETRIES[0]
    h, w, b = geo[:3]
    lib = L.lib()
    keep = TP.keep_map(h, w)
    zeros = np.zeros((h, w), np.uint8)
    (s, g), = _steps(h, w, b, 1)
    a, c = _trainer(ctx, geo), _trainer(ctx, geo)
    try:
        for tr in (a, c):
            tr.set_post(logit_thresh=0.5, keep=keep)

        def call(handle, model, thr, kp):
            return lib.covahip_train_set_post(handle, model, C.byref(L.BlobNetPost(thr, None if kp is None else kp.ctypes.data)))

        assert call(None, 0, 0.0, None) == 1
        assert lib.covahip_train_set_post(None, 0, None) == 1
        assert call(a.handle, -1, 0.0, None) == 1 and call(a.handle, 1, 0.0, None) == 1
        assert lib.covahip_train_set_post(a.handle, 1, None) == 1
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert call(a.handle, 0, bad, None) == 1 and call(a.handle, 0, bad, keep) == 1
        assert call(a.handle, 0, 0.0, zeros) == 1                        # nothing would be left to train on
        thr, has = C.c_float(), C.c_int()
        assert lib.covahip_train_get_post(None, 0, C.byref(thr), None, C.byref(has)) == 1
        assert lib.covahip_train_get_post(a.handle, 1, C.byref(thr), None, C.byref(has)) == 1
        assert lib.covahip_train_get_post(a.handle, 0, None, None, None) == 0
        got_thr, got_keep = a.get_post()
        assert got_thr == 0.5 and (got_keep == keep).all()
        with pytest.raises(ValueError):
            a.set_post(keep=zeros[:-1])
        with pytest.raises(ValueError):
            a.set_post(prob_thresh=0.5, logit_thresh=0.0)
        with pytest.raises(L.CovahipError):
            a.set_post(keep=zeros)
        la, lc = a.step(s, g), c.step(s, g)
        assert la == lc and _same(_snap(a), _snap(c))
        a.reset_post()
        assert a.get_post() is None
    finally:
        a.close()
        c.close()


def test_command_line_trains_and_scores_with_a_post(ctx, tmp_path):
    z = np.load(os.path.join(GOLDEN, "demo_records_excerpt.npz"))
    frames = z["records"]
    h, w = frames.shape[1:3]
    gt = ((frames[..., 1] != 0) | (frames[..., 2] != 0)).astype(np.uint8)
    path, side, out = tmp_path / "demo.tfrecord", tmp_path / "post.json", tmp_path / "post.cvhw"
    with open(path, "wb") as f:
        for i in range(0, frames.shape[0], 8):
            f.write(tfrecord_example(frames[i:i + 8], gt[i:i + 8], gop=8))
    calibrate.save_post(side, {"logit_thresh": 0.4054651, "cc_threshold": 4}, ignore_rects=TP.ignore_rects(h, w))
    kw, _ = calibrate.load_post(side, h, w)

    def run(*args):
        r = subprocess.run([sys.executable, "-m", "cova_amd.train", *args, "--h-mb", str(h), "--w-mb", str(w)], cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r

    run(str(path), "-o", str(out), "--epochs", "1", "--post", str(side))
    records = T.slide(*T.read_tfrecords([str(path)], h, w))
    tr = T.Trainer(ctx, h, w, max_batch=4, seed=0)
    try:
        tr.set_post(**kw)
        tr.fit(records, epochs=1, batch=4)
        assert tr.weights_bytes() == out.read_bytes()                   # the command line trained with the post
        ev = tr.evaluate(records)
        tr.reset_post()
        assert tr.evaluate(records) != ev
    finally:
        tr.close()
    r = run("--eval-only", str(out), str(path), "--post", str(side))
    lines = [json.loads(line) for line in r.stdout.splitlines() if line.strip()]
    assert len(lines) == 1 and lines[0]["weights"] == str(out)
    assert {k: lines[0][k] for k in ev} == ev
    assert lines[0]["post"] == {"logit_thresh": kw["logit_thresh"], "ignored": 23}
