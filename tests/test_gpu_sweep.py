"""covahip_post_sweep on the GPU against its numpy restatement (tests/sweep_ref.py, which stands on the CPU oracle's regionprops):
every table must be EQUAL -- all quantities are integer counts.  The reference of a grid is computed once per sample; the
reference of fewer samples, thresholds or areas is a sum or a selection of it, which the rules allow as long as nothing is
truncated (asserted on the reference's own numbers), so truncation cannot hide a mismatch.  Truncation has its own case."""
import json

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import calibrate as cal
from cova_amd import synth
from cova_amd import weights as W
from cova_amd.elements import BlobNetInfer, keep_from_rects, tfrecord_example
from tests.sweep_ref import smooth_field, sweep_ref

pytestmark = pytest.mark.gpu

GRIDS = [(16, 16), (9, 20), (45, 80), (67, 120)]          # 9 x 20: width no multiple of 8; 45 x 80: odd height
ODD_GRIDS = [(5, 7), (17, 33)]                            # h * w = 35, 561: no multiple of 4, one macroblock per work item
AREAS16 = [1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 30, 40, 60, 100]
N_ALL, N_FULL = 37, 5                                     # samples at three thresholds / at all 64
T3 = [10, 32, 50]                                         # the three thresholds, as indices into the 64
TABLES = ("pixel", "pred", "pred_true", "gt_found", "truncated")
SCALARS = ("samples", "gt_objects", "gt_truncated")


def _keep(h, w):
    k = np.ones((h, w), np.uint8)
    k[: h // 3, w // 2:] = 0                              # a corner region
    k[h - 2, ::3] = 0                                     # and scattered macroblocks, some inside blobs
    return k


def _per_sample(logits, gt, th, keep):
    return [sweep_ref(logits[i:i + 1], gt[i:i + 1], th, AREAS16, keep=keep) for i in range(logits.shape[0])]


def _sum(per, t_idx=None, a_idx=None):
    """The reference of these samples at a selection of thresholds / areas."""
    t_idx = list(range(per[0]["pred"].shape[0])) if t_idx is None else t_idx
    a_idx = list(range(len(AREAS16))) if a_idx is None else a_idx
    out = {k: sum(p[k] for p in per) for k in SCALARS}
    for k in TABLES:
        tot = sum(p[k] for p in per)[t_idx]
        out[k] = tot[:, a_idx] if k in ("pred", "pred_true", "gt_found") else tot
    assert out["gt_truncated"] == 0 and not out["truncated"].any()      # selections are valid, and nothing hides behind truncation
    return out


@pytest.fixture(scope="module")
def cases():
    """Per grid: seeded smooth logits and labels, 64 thresholds that ARE logit values, and the per-sample references."""
    made = {}

    def get(h, w):
        if (h, w) not in made:
            # (5 x 7's own seed: 35 macroblocks are few, and the first sample must hold a labelled object that is hit and a prediction
            # that is not, which test_samples_and_chunks asserts on the reference at n = 1)
            rng = np.random.default_rng(5008 if (h, w) == (5, 7) else 1000 * h + w)
            k = 3 if h * w <= 256 else 7
            logits = smooth_field(rng, N_ALL, h, w, k)
            gt = (smooth_field(rng, N_ALL, h, w, k) > 1.0).astype(np.uint8) * 255
            u = np.unique(logits)
            th = u[np.linspace(0.1 * u.size, 0.9 * u.size, 64).astype(int)]     # every threshold equals some logit
            assert (np.diff(th) > 0).all()
            keep = _keep(h, w)
            made[(h, w)] = {"logits": logits, "gt": gt, "th": th, "keep": keep,
                            "ref3": _per_sample(logits, gt, th[T3], None),
                            "ref64": _per_sample(logits[:N_FULL], gt[:N_FULL], th, None),
                            "ref64k": _per_sample(logits[:N_FULL], gt[:N_FULL], th, keep)}
        return made[(h, w)]
    return get


def _same(got, want):
    for k in SCALARS:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in TABLES:
        assert np.array_equal(got[k], want[k]), (k, got[k].tolist(), want[k].tolist())


def _on_device(ctx, logits, gt, fn):
    d_l, d_g = ctx.malloc(logits.nbytes), ctx.malloc(gt.nbytes)
    try:
        ctx.h2d(d_l, logits)
        ctx.h2d(d_g, gt)
        return fn(d_l, d_g)
    finally:
        ctx.free(d_l)
        ctx.free(d_g)


# ------------------------------------------------------------------------------------------------------------------ exact agreement
@pytest.mark.parametrize("chunk", [0, 4])
@pytest.mark.parametrize("n", [1, 5, N_ALL])
@pytest.mark.parametrize("h,w", GRIDS + ODD_GRIDS)
def test_samples_and_chunks(ctx, cases, h, w, n, chunk):
    c = cases(h, w)
    want = _sum(c["ref3"][:n])
    assert want["gt_objects"] > 0 and want["pred_true"].any() and (want["pred_true"] != want["pred"]).any()
    got = cal.sweep(ctx, c["logits"][:n], c["gt"][:n], c["th"][T3], AREAS16, chunk=chunk)
    _same(got, want)


@pytest.mark.parametrize("n_area", [1, 16])
@pytest.mark.parametrize("n_thresh", [1, 3, 64])
@pytest.mark.parametrize("h,w", GRIDS)
def test_thresholds_and_areas(ctx, cases, h, w, n_thresh, n_area):
    c = cases(h, w)
    t_idx = {1: [32], 3: T3, 64: list(range(64))}[n_thresh]
    a_idx = [3] if n_area == 1 else list(range(16))        # a single area threshold of 4: area_thresh[0] need not be 1
    want = _sum(c["ref64"], t_idx, a_idx)
    assert want["pred"].any()
    got = cal.sweep(ctx, c["logits"][:N_FULL], c["gt"][:N_FULL], c["th"][t_idx], [AREAS16[a] for a in a_idx])
    _same(got, want)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("with_keep", [False, True])
@pytest.mark.parametrize("h,w", GRIDS + ODD_GRIDS)
def test_keep_map_and_mem_kind(ctx, cases, h, w, with_keep, device):
    c = cases(h, w)
    keep = c["keep"] if with_keep else None
    want = _sum(c["ref64k" if with_keep else "ref64"])
    if with_keep:
        plain = _sum(c["ref64"])
        assert not np.array_equal(plain["pixel"], want["pixel"]) and not np.array_equal(plain["pred"], want["pred"])
    lg, gt = c["logits"][:N_FULL], c["gt"][:N_FULL]
    if device:
        got = _on_device(ctx, lg, gt, lambda d_l, d_g: cal.sweep_device(ctx, d_l, d_g, N_FULL, h, w, c["th"], AREAS16, keep=keep))
    else:
        got = cal.sweep(ctx, lg, gt, c["th"], AREAS16, keep=keep)
    _same(got, want)


@pytest.mark.parametrize("chunk", [0, 2])
@pytest.mark.parametrize("which", ["logits+4", "labels+1"])
@pytest.mark.parametrize("h,w", [(16, 16), (45, 80)])
def test_offset_device_pointers(ctx, cases, h, w, which, chunk):
    """h * w is a multiple of 4 here, so only the caller's pointers decide: logits that are float-aligned but not 16-byte
    aligned, or labels on an odd address, take the one-macroblock kernel and must give the aligned call's tables."""
    c = cases(h, w)
    want = _sum(c["ref64k"])
    lg, gt = c["logits"][:N_FULL], c["gt"][:N_FULL]
    off_l, off_g = (4, 0) if which == "logits+4" else (0, 1)
    d_l, d_g = ctx.malloc(lg.nbytes + 16), ctx.malloc(gt.nbytes + 16)
    try:
        assert d_l % 16 == 0 and d_g % 16 == 0             # the allocation is aligned, so the offset is what the kernel sees
        ctx.h2d(d_l + off_l, lg)
        ctx.h2d(d_g + off_g, gt)
        got = cal.sweep_device(ctx, d_l + off_l, d_g + off_g, N_FULL, h, w, c["th"], AREAS16, keep=c["keep"], chunk=chunk)
    finally:
        ctx.free(d_l)
        ctx.free(d_g)
    _same(got, want)


def test_infinities_and_nan(ctx, cases):
    h, w = 45, 80
    c = cases(h, w)
    lg = c["logits"][:N_FULL].copy()
    rng = np.random.default_rng(5)
    for val in (np.inf, -np.inf, np.nan):
        idx = rng.integers(0, lg.size, 12)
        lg.reshape(-1)[idx] = val
    lg[0, 10:12, 10:12] = np.nan                           # inside whatever is there: NaN is background at every threshold
    lg[1, 20, 20:23] = np.inf                              # foreground at every threshold
    th = c["th"][T3]
    want = sweep_ref(lg, c["gt"][:N_FULL], th, AREAS16)
    assert not want["truncated"].any() and want["gt_truncated"] == 0
    assert not np.array_equal(want["pixel"], _sum(c["ref3"][:N_FULL])["pixel"])
    _same(cal.sweep(ctx, lg, c["gt"][:N_FULL], th, AREAS16), want)
    _same(cal.sweep(ctx, lg, c["gt"][:N_FULL], th, AREAS16, chunk=2), want)


# ------------------------------------------------------------------------------------------------------------------ truncation, dense
def test_truncation(ctx):
    n, h, w = 8, 16, 16
    lg = synth.random_masks(n, h, w, 0.3, seed=7).astype(np.float32) * 2 - 1
    gt = synth.random_masks(n, h, w, 0.3, seed=8)
    th, areas = [-0.5, 0.0], [1, 2, 4]
    want = sweep_ref(lg, gt, th, areas, max_boxes=2)
    assert want["truncated"].tolist() == [n, n] and want["gt_truncated"] == n and want["gt_objects"] == 2 * n
    assert want["pred"][0, 0] == 2 * n
    _same(cal.sweep(ctx, lg, gt, th, areas, max_boxes=2), want)
    _same(cal.sweep(ctx, lg, gt, th, areas, max_boxes=2, chunk=3), want)


def test_dense_masks(ctx):
    n, h, w = 6, 16, 16
    rng = np.random.default_rng(11)
    lg = rng.standard_normal((n, h, w)).astype(np.float32)
    gt = synth.random_masks(n, h, w, 0.3, seed=12)
    th, areas = [-0.5, 0.0, 0.5, 1.0], [1, 2, 3, 5]
    want = sweep_ref(lg, gt, th, areas)
    assert want["pred"][:, 0].max() >= 12 * n and not want["truncated"].any() and want["gt_truncated"] == 0   # many components a frame
    _same(cal.sweep(ctx, lg, gt, th, areas), want)
    _same(cal.sweep(ctx, lg, gt, th, areas, iou=(1, 2)), sweep_ref(lg, gt, th, areas, iou=(1, 2)))
    _same(cal.sweep(ctx, lg, gt, th, areas, gt_area=3), sweep_ref(lg, gt, th, areas, gt_area=3))


# ------------------------------------------------------------------------------------------------------------------ additivity
def test_additivity(ctx, cases):
    h, w = 45, 80
    c = cases(h, w)
    th = c["th"][T3]

    def run(a, b):
        return cal.sweep(ctx, c["logits"][a:b], c["gt"][a:b], th, AREAS16)

    whole = run(0, N_ALL)
    _same(whole, _sum(c["ref3"]))
    _same(cal.add(run(0, 10), run(10, N_ALL)), whole)
    total = run(0, 1)
    for i in range(1, N_ALL):
        total = cal.add(total, run(i, i + 1))
    _same(total, whole)


# ------------------------------------------------------------------------------------------------------------------ serving path
@pytest.mark.parametrize("h,w", [(16, 16), (45, 80)])
def test_sweep_agrees_with_the_serving_path(ctx, h, w):
    b = 8
    stack = synth.stacked_batch(b, h, w, seed=21, streams=2)
    net = BlobNetInfer(ctx, W.blob_like(), h, w, max_batch=b)
    logits, _ = net.infer(stack)
    u = np.unique(logits)
    th = u[np.linspace(0.2 * u.size, 0.98 * u.size, 6).astype(int)]          # thresholds that are logits of this forward
    areas = [1, 2, 4, 8]
    gt = (smooth_field(np.random.default_rng(3), b, h, w, 5) > 0.5).astype(np.uint8)
    keep = _keep(h, w)
    mb = 1024                                              # more than a 45 x 80 grid can hold components: nothing is truncated
    got = cal.sweep(ctx, logits, gt, th, areas, keep=keep, max_boxes=mb)
    want = sweep_ref(logits, gt, th, areas, keep=keep, max_boxes=mb, want_boxes=True)
    assert not want["truncated"].any() and want["gt_truncated"] == 0
    _same(got, want)
    try:
        for t in (1, 4):
            for a in (0, 2):
                net.set_post(0, logit_thresh=float(th[t]), keep=keep)
                boxes, counts, _ = net.filter(stack, cc_threshold=areas[a], max_boxes=mb)
                assert int(counts.sum()) == got["pred"][t, a]
                for s in range(b):
                    P = want["boxes"][s][t][a]
                    assert counts[s] == len(P) and boxes[s, :len(P)].tobytes() == P.tobytes(), (s, t, a)
        assert got["pred"][1, 0] > 0 and got["pred"][1, 0] != got["pred"][4, 0]
    finally:
        net.reset_post(0)


@pytest.mark.parametrize("lanes", [1, 3])
def test_a_forward_is_not_disturbed(ctx, cases, lanes):
    h, w, b = 45, 80, 8
    c = cases(h, w)
    stack = synth.stacked_batch(b, h, w, seed=22, streams=2)
    old = ctx.lanes()
    ctx.set_lanes(lanes)
    try:
        net = BlobNetInfer(ctx, W.blob_like(), h, w, max_batch=b)
        net.set_post(0, logit_thresh=0.25, keep=_keep(h, w))
        before = net.filter_full(stack, 2, 256, True, True)
        assert before[1].sum() > 0
        _same(cal.sweep(ctx, c["logits"][:N_FULL], c["gt"][:N_FULL], c["th"][T3], AREAS16, keep=c["keep"], chunk=2),
              _sum([sweep_ref(c["logits"][i:i + 1], c["gt"][i:i + 1], c["th"][T3], AREAS16, keep=c["keep"]) for i in range(N_FULL)]))
        after = net.filter_full(stack, 2, 256, True, True)
        assert np.array_equal(before[1], after[1]) and before[0].tobytes() == after[0].tobytes()
        assert np.array_equal(before[2], after[2]) and np.array_equal(before[3], after[3])
        thr, kp = net.post(0)
        assert thr == 0.25 and np.array_equal(kp, _keep(h, w))
    finally:
        ctx.set_lanes(old)


# ------------------------------------------------------------------------------------------------------------------ command line
def test_command_line(ctx, tmp_path, capsys):
    h, w, n = 45, 80, 40
    frames = synth.carrier_frames(4 * n, h, w, seed=31, n_objects=5)
    frames[..., 3] = 0
    flat = W.blob_like()
    # labels: the model's own default mask, so the reference threshold finds every object and the choice cannot be an empty cell
    from cova_amd import train
    stacks, _ = train.slide(frames, np.zeros((4 * n, h, w), np.uint8))
    _, own = BlobNetInfer(ctx, flat, h, w, max_batch=n).infer(stacks, want_logits=False)
    assert own.any()
    gt = np.zeros((4 * n, h, w), np.uint8)
    gt[3::4] = own
    rec, wts, post = tmp_path / "held_out.tfrecord", tmp_path / "cam.cvhw", tmp_path / "post.json"
    with open(rec, "wb") as f:
        for i in range(0, 4 * n, 8):
            f.write(tfrecord_example(frames[i:i + 8], gt[i:i + 8], gop=8))
    wts.write_bytes(W.to_bytes(flat))
    rects = ["0,0,320,48", "1000,600,100,100"]
    assert cal.main([str(rec), "--weights", str(wts), "--h-mb", str(h), "--w-mb", str(w), "--batch", "16",
                     "--ignore-rects", *rects, "-o", str(post)]) == 0
    text = capsys.readouterr().out
    assert "choice:" in text and "pad-mask-threshold" in text and "cc-threshold=" in text and "set_post(" in text
    doc = json.loads(post.read_text())
    assert doc["scores"]["samples"] == n and doc["scores"]["truncated"] == 0 and doc["scores"]["pred"] > 0
    assert len(doc["grid"]["logit_thresh"]) == 19 and doc["grid"]["area_thresh"] == [1, 2, 4, 8, 16, 30]
    kw, cc = cal.load_post(post, h, w)
    assert np.array_equal(kw["keep"], keep_from_rects(h, w, [(0, 0, 320, 48), (1000, 600, 100, 100)]))
    stacks2, labels2 = train.slide(*train.read_tfrecords([str(rec)], h, w))
    assert np.array_equal(stacks2, stacks) and np.array_equal(labels2, own)
    net = BlobNetInfer(ctx, flat, h, w, max_batch=n)
    net.set_post(0, **kw)
    _, counts, _ = net.filter(stacks, cc_threshold=cc)
    assert int(counts.sum()) == doc["scores"]["pred"]
