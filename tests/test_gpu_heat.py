"""covahip_post_heat_* on the GPU against its numpy restatement (tests/heat_ref.py): every table must be EQUAL -- all quantities are
integer counts.  Per grid the restatement is computed once per sample count at 64 thresholds; the reference at fewer thresholds
is a selection of its planes, which the rules allow (fire[t] and both[t] depend on thresh[t] alone)."""
import ctypes as C
import json

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import calibrate as cal
from cova_amd import synth
from cova_amd import weights as W
from cova_amd.elements import BlobNetInfer, tfrecord_example
from tests.heat_ref import heat_ref
from tests.sweep_ref import smooth_field

pytestmark = pytest.mark.gpu

# 5 x 7: under a wave, no multiple of 4; 17 x 16: one macroblock row over a 256-tile; 67 x 120: no multiple of the tile
GRIDS = [(1, 1), (5, 7), (9, 20), (17, 16), (45, 80), (67, 120)]
NS = [1, 2, 37, 257]                                      # 37 and 257: uneven sample slices
N_MAX = 257
T_SEL = {1: [32], 3: [10, 32, 50], 64: list(range(64))}
# the edges of the kernel's 16 / 32 / 64-threshold instantiations: evenly spread planes of the 64, the last one included
T_SEL.update({k: np.linspace(0, 63, k).astype(int).tolist() for k in (16, 17, 32, 33)})
TABLES = ("fire", "both", "gt")
INVALID = 1


@pytest.fixture(scope="module")
def cases():
    """Per grid: seeded smooth logits and labels of 257 samples and 64 thresholds that ARE logit values (the last one the largest
    logit, where a compare that is not strict would fire); per (grid, n) the restatement over the first n samples."""
    data, refs = {}, {}

    def get(h, w, n):
        if (h, w) not in data:
            rng = np.random.default_rng(1000 * h + w)
            k = 3 if h * w <= 256 else 7
            logits = smooth_field(rng, N_MAX, h, w, k)
            gt = (smooth_field(rng, N_MAX, h, w, k) > 1.0).astype(np.uint8) * 255
            u = np.unique(logits)
            th = u[np.linspace(0.1 * u.size, u.size - 1, 64).astype(int)]
            assert (np.diff(th) > 0).all() and th[-1] == logits.max()
            data[(h, w)] = {"logits": logits, "gt": gt, "th": th}
        if (h, w, n) not in refs:
            d = data[(h, w)]
            refs[(h, w, n)] = heat_ref(d["logits"][:n], d["gt"][:n], d["th"])
        return data[(h, w)], refs[(h, w, n)]
    return get


def _select(ref, t_idx):
    return {"fire": ref["fire"][t_idx], "both": ref["both"][t_idx], "gt": ref["gt"], "samples": ref["samples"]}


def _same(got, want):
    assert got["samples"] == want["samples"], (got["samples"], want["samples"])
    for k in TABLES:
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (k, len(bad), bad[:4].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


def _on_device(ctx, logits, gt, fn):
    d_l, d_g = ctx.malloc(logits.nbytes), ctx.malloc(gt.nbytes)
    try:
        ctx.h2d(d_l, logits)
        ctx.h2d(d_g, gt)
        return fn(d_l, d_g)
    finally:
        ctx.free(d_l)
        ctx.free(d_g)


def _heat_device(ctx, logits, gt, th):
    n, h, w = logits.shape

    def run(d_l, d_g):
        t = cal.heat_begin(ctx, h, w, th)
        cal.heat_add_device(ctx, d_l, d_g, n)
        return cal.heat_end(ctx, h, w, t)
    return _on_device(ctx, logits, gt, run)


# ------------------------------------------------------------------------------------------------------------------ exact agreement
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("n_thresh", [1, 3, 64])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("h,w", GRIDS)
def test_tables_equal_the_restatement(ctx, cases, h, w, n, n_thresh, device):
    d, ref = cases(h, w, n)
    t_idx = T_SEL[n_thresh]
    want = _select(ref, t_idx)
    # all-pass cannot come from empty tables: over the grid's 64 planes some macroblock never fires and some does, and in this
    # case's own planes some macroblock has 0 < both < fire.  That needs samples that disagree within one macroblock, which one
    # or two samples cannot be relied on to do, so it is asserted from 37 samples on.
    assert (ref["fire"] == 0).any() and ref["fire"].any()
    if n >= 37:
        assert ((want["both"] > 0) & (want["both"] < want["fire"])).any()
    lg, gt, th = d["logits"][:n], d["gt"][:n], d["th"][t_idx]
    got = _heat_device(ctx, lg, gt, th) if device else cal.heat(ctx, lg, gt, th)
    _same(got, want)
    assert np.array_equal(got["logit_thresh"], th)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("n_thresh", [16, 17, 32, 33])
@pytest.mark.parametrize("h,w", [(5, 7), (17, 16)])
def test_threshold_count_edges(ctx, cases, h, w, n_thresh, device):
    """16 | 17 and 32 | 33 thresholds: either side of the choice between the kernel's 16-, 32- and 64-threshold forms."""
    n = 37
    d, ref = cases(h, w, n)
    t_idx = T_SEL[n_thresh]
    assert len(set(t_idx)) == n_thresh and t_idx[-1] == 63
    want = _select(ref, t_idx)
    assert want["fire"][0].any() and ((want["both"] > 0) & (want["both"] < want["fire"])).any()
    assert (want["fire"][-1] != want["fire"][-2]).any()                 # the last plane is not a copy of the one below it
    lg, gt, th = d["logits"][:n], d["gt"][:n], d["th"][t_idx]
    got = _heat_device(ctx, lg, gt, th) if device else cal.heat(ctx, lg, gt, th)
    _same(got, want)


def test_slices_clamped_to_their_counter_width(ctx):
    """One macroblock, num_cu * 32768 + 5 samples: one slice per CU would be longer than the 32768 samples a bin's two 16-bit
    halves are sized for, so the slice count is raised.  The first three quarters are one logit above every threshold with the
    label set: whole slices land in ONE bin, in both halves of the packed word.  The reference is three counts per threshold."""
    n = ctx.info()["num_cu"] * 32768 + 5
    rng = np.random.default_rng(41)
    lg = rng.standard_normal(n).astype(np.float32)
    gt = (rng.random(n) < 0.3).astype(np.uint8) * 255
    const = 3 * n // 4
    th = np.array([-0.5, 0.0, 0.7], np.float32)
    lg[:const], gt[:const] = 5.0, 1
    fire = np.array([int((lg > t).sum()) for t in th])
    both = np.array([int(((lg > t) & (gt != 0)).sum()) for t in th])
    assert fire[2] > const and (np.diff(fire) < 0).all() and (both < fire).all() and both[2] > const
    got = _heat_device(ctx, lg.reshape(n, 1, 1), gt.reshape(n, 1, 1), th)
    assert got["samples"] == n
    assert got["fire"].reshape(-1).tolist() == fire.tolist() and got["both"].reshape(-1).tolist() == both.tolist()
    assert got["gt"].reshape(-1).tolist() == [int((gt != 0).sum())]


@pytest.mark.parametrize("per_piece", [10, 1])
@pytest.mark.parametrize("h,w", [(5, 7), (45, 80)])
def test_host_samples_staged_in_pieces(ctx, cases, h, w, per_piece):
    """The developer's staging budget: 37 host samples go up in pieces of 10, 10, 10 and 7, and -- with a budget below one
    sample -- one at a time.  The tables are the unstaged call's."""
    n = 37
    d, ref = cases(h, w, n)
    want = _select(ref, T_SEL[3])
    lg, gt, th = d["logits"][:n], d["gt"][:n], d["th"][T_SEL[3]]
    sample = h * w * 5                                                   # four bytes of logit and a label byte per macroblock
    budget = 10 * sample + sample // 2 if per_piece == 10 else sample - 1
    assert budget // sample == (10 if per_piece == 10 else 0) and n % 10 == 7
    try:
        cal.heat_set_stage(ctx, budget)
        got = cal.heat(ctx, lg, gt, th)
    finally:
        cal.heat_set_stage(ctx, 0)
    _same(got, want)
    _same(cal.heat(ctx, lg, gt, th), want)                               # and with the default restored


def test_specials(ctx):
    h, w, n = 3, 4, 4
    lg = np.linspace(-1.5, 1.5, n * h * w, dtype=np.float32).reshape(n, h, w)
    lg[:, 0, 0] = [np.nan, np.nan, 2.0, -2.0]         # NaN is background at every threshold
    lg[:, 0, 1] = np.inf                                                  # fires at every threshold
    lg[:, 0, 2] = -np.inf
    lg[0, 1, 0], lg[1, 1, 0], lg[2, 1, 0], lg[3, 1, 0] = -0.0, 0.0, np.float32(1e-45), -np.float32(1e-45)   # around a threshold of 0.0
    lg[:, 1, 1] = [1.0, 1.0, -1.0, np.float32(1.0000001)]                 # at and just above thresholds that are listed
    gt = np.zeros((n, h, w), np.uint8)
    gt[:, 0, 0] = [0, 1, 2, 255]
    gt[:, 0, 1] = [255, 0, 2, 1]
    gt[:, 1, 0] = [1, 1, 2, 0]
    gt[:, 2, :] = [[0, 1, 2, 255]] * n
    th = np.array([-1.0, 0.0, 1.0], np.float32)
    want = heat_ref(lg, gt, th)
    assert want["fire"][:, 0, 0].tolist() == [1, 1, 1] and want["both"][:, 0, 0].tolist() == [1, 1, 1] and want["gt"][0, 0] == 3
    assert want["fire"][:, 0, 1].tolist() == [4, 4, 4] and want["both"][:, 0, 1].tolist() == [3, 3, 3]
    assert not want["fire"][:, 0, 2].any()
    assert want["fire"][:, 1, 0].tolist() == [4, 1, 0]                    # -0.0 > 0.0 is false; the denormal above it fires
    assert want["fire"][:, 1, 1].tolist() == [3, 3, 1]
    assert want["gt"][2].tolist() == [0, n, n, n]
    _same(cal.heat(ctx, lg, gt, th), want)
    _same(_heat_device(ctx, lg, gt, th), want)


# ------------------------------------------------------------------------------------------------------------------ additivity, state
def test_additivity_and_state(ctx, cases):
    h, w = 9, 20
    d, ref = cases(h, w, N_MAX)
    t_idx = T_SEL[3]
    th, lg, gt = d["th"][t_idx], d["logits"], d["gt"]
    want = _select(ref, t_idx)

    def split(*parts):
        t = cal.heat_begin(ctx, h, w, th)
        s0 = 0
        for c in parts:
            a, b = np.ascontiguousarray(lg[s0:s0 + c]), np.ascontiguousarray(gt[s0:s0 + c])
            cal.heat_add_device(ctx, a.ctypes.data, b.ctypes.data, c, L.MEM_HOST)
            s0 += c
        return cal.heat_end(ctx, h, w, t)

    _same(split(257), want)
    _same(split(1, 256), want)
    _same(split(100, 100, 57), want)
    _same(split(100, 0, 100, 0, 57), want)                               # n == 0 changes nothing
    # a null pointer is fine with n == 0
    t = cal.heat_begin(ctx, h, w, th)
    cal.heat_add_device(ctx, None, None, 0)
    empty = cal.heat_end(ctx, h, w, t)
    assert empty["samples"] == 0 and not any(empty[k].any() for k in TABLES)
    # begin after add starts from zero
    t = cal.heat_begin(ctx, h, w, th)
    cal.heat_add_device(ctx, lg[:50].ctypes.data, gt[:50].ctypes.data, 50, L.MEM_HOST)
    cal.heat_begin(ctx, h, w, th)
    cal.heat_add_device(ctx, lg[:37].ctypes.data, gt[:37].ctypes.data, 37, L.MEM_HOST)
    _same(cal.heat_end(ctx, h, w, t), _select(cases(h, w, 37)[1], t_idx))
    # a second begin ... end after an end, at another grid and another number of thresholds
    d2, ref2 = cases(5, 7, 37)
    _same(cal.heat(ctx, d2["logits"][:37], d2["gt"][:37], d2["th"]), _select(ref2, T_SEL[64]))
    _same(split(257), want)
    # add_heat
    a, b = cal.heat(ctx, lg[:100], gt[:100], th), cal.heat(ctx, lg[100:], gt[100:], th)
    _same(cal.add_heat(a, b), want)
    with pytest.raises(ValueError):
        cal.add_heat(a, cal.heat(ctx, lg[100:], gt[100:], d["th"][[10, 32, 51]]))


def test_end_takes_null_outputs(ctx, cases):
    h, w = 5, 7
    d, ref = cases(h, w, 37)
    lib = L.lib()
    lg, gt = d["logits"][:37], d["gt"][:37]
    cal.heat_begin(ctx, h, w, d["th"])
    cal.heat_add_device(ctx, lg.ctypes.data, gt.ctypes.data, 37, L.MEM_HOST)
    assert lib.covahip_post_heat_end(ctx.handle, None, None, None, None) == 0
    assert lib.covahip_post_heat_end(ctx.handle, None, None, None, None) == INVALID            # it closed the heat
    t = cal.heat_begin(ctx, h, w, d["th"])
    cal.heat_add_device(ctx, lg.ctypes.data, gt.ctypes.data, 37, L.MEM_HOST)
    both = np.zeros((64, h, w), np.int64)
    samples = C.c_int64()
    assert lib.covahip_post_heat_end(ctx.handle, None, both.ctypes.data, None, C.byref(samples)) == 0
    assert samples.value == 37 and np.array_equal(both, ref["both"])


# ------------------------------------------------------------------------------------------------------------------ the sweep's pixel counts
def test_sums_equal_the_sweep_without_keep(ctx, cases):
    h, w, n = 45, 80, 37
    d, _ = cases(h, w, n)
    lg, gt, th = d["logits"][:n], d["gt"][:n], d["th"]
    ht = cal.heat(ctx, lg, gt, th)
    sw = cal.sweep(ctx, lg, gt, th, [1])
    tp = ht["both"].sum(axis=(1, 2))
    assert tp.any()
    assert np.array_equal(np.stack([tp, ht["fire"].sum(axis=(1, 2)) - tp, ht["gt"].sum() - tp], axis=1), sw["pixel"])


# ------------------------------------------------------------------------------------------------------------------ errors
def test_errors(ctx, cases):
    lib = L.lib()
    h, w = 5, 7
    d, _ = cases(h, w, 2)
    lg, gt = d["logits"][:2], d["gt"][:2]
    good = np.array([-1.0, 0.0, 1.0], np.float32)

    def cfg(hh=h, ww=w, n=3, th=good):
        c = L.HeatCfg(hh, ww, n, th.ctypes.data if th is not None else None)
        c._th = th
        return c

    begin, add, end = lib.covahip_post_heat_begin, lib.covahip_post_heat_add, lib.covahip_post_heat_end
    # add and end without begin (whatever earlier tests left open is closed first)
    begin(ctx.handle, C.byref(cfg()))
    assert end(ctx.handle, None, None, None, None) == 0
    assert add(ctx.handle, lg.ctypes.data, gt.ctypes.data, 2, L.MEM_HOST) == INVALID
    assert end(ctx.handle, None, None, None, None) == INVALID
    # begin
    assert begin(None, C.byref(cfg())) == INVALID
    assert begin(ctx.handle, None) == INVALID
    assert begin(ctx.handle, C.byref(cfg(th=None))) == INVALID
    for bad in ([-1.0, np.nan, 1.0], [-1.0, np.inf, 2.0], [-np.inf, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.5]):
        assert begin(ctx.handle, C.byref(cfg(th=np.array(bad, np.float32)))) == INVALID, bad
    many = np.arange(65, dtype=np.float32)
    assert begin(ctx.handle, C.byref(cfg(n=0))) == INVALID
    assert begin(ctx.handle, C.byref(cfg(n=-1))) == INVALID
    assert begin(ctx.handle, C.byref(cfg(n=65, th=many))) == INVALID
    assert begin(ctx.handle, C.byref(cfg(n=64, th=many))) == 0
    assert end(ctx.handle, None, None, None, None) == 0
    for hh, ww in ((0, w), (h, 0), (-1, w), (h, -3)):
        assert begin(ctx.handle, C.byref(cfg(hh, ww))) == INVALID
    assert end(ctx.handle, None, None, None, None) == INVALID            # none of the failed begins opened a heat
    # add
    assert add(None, lg.ctypes.data, gt.ctypes.data, 2, L.MEM_HOST) == INVALID
    assert end(None, None, None, None, None) == INVALID
    assert begin(ctx.handle, C.byref(cfg())) == 0
    assert add(ctx.handle, lg.ctypes.data, gt.ctypes.data, -1, L.MEM_HOST) == INVALID
    assert add(ctx.handle, None, gt.ctypes.data, 2, L.MEM_HOST) == INVALID
    assert add(ctx.handle, lg.ctypes.data, None, 2, L.MEM_HOST) == INVALID
    assert add(ctx.handle, lg.ctypes.data, gt.ctypes.data, 2, 2) == INVALID
    assert add(ctx.handle, lg.ctypes.data, gt.ctypes.data, 2, -1) == INVALID
    assert add(ctx.handle, lg.ctypes.data, gt.ctypes.data, 2, L.MEM_HOST) == 0
    # a total above INT32_MAX samples: refused on the host, before any of the samples is looked at
    assert add(ctx.handle, lg.ctypes.data, gt.ctypes.data, 2 ** 31 - 2, L.MEM_HOST) == INVALID
    # a failed begin leaves the open heat as it was, and so did every refused add
    assert begin(ctx.handle, C.byref(cfg(n=0))) == INVALID
    got = cal.heat_end(ctx, h, w, good)
    _same(got, heat_ref(lg, gt, good))
    with pytest.raises(L.CovahipError):
        cal.heat_end(ctx, h, w, good)


@pytest.mark.parametrize("lanes", [1, 3])
def test_a_forward_is_not_disturbed(ctx, cases, lanes):
    h, w, b = 45, 80, 8
    d, ref = cases(h, w, 37)
    stack = synth.stacked_batch(b, h, w, seed=22, streams=2)
    old = ctx.lanes()
    ctx.set_lanes(lanes)
    try:
        net = BlobNetInfer(ctx, W.blob_like(), h, w, max_batch=b)
        before = net.filter_full(stack, 2, 256, True, True)
        assert before[1].sum() > 0
        t = cal.heat_begin(ctx, h, w, d["th"])
        cal.heat_add_device(ctx, d["logits"][:20].ctypes.data, d["gt"][:20].ctypes.data, 20, L.MEM_HOST)
        mid = net.filter_full(stack, 2, 256, True, True)                 # a forward inside the bracket leaves the heat alone
        cal.heat_add_device(ctx, d["logits"][20:37].ctypes.data, d["gt"][20:37].ctypes.data, 17, L.MEM_HOST)
        _same(cal.heat_end(ctx, h, w, t), ref)
        after = net.filter_full(stack, 2, 256, True, True)
        for other in (mid, after):
            assert np.array_equal(before[1], other[1]) and before[0].tobytes() == other[0].tobytes()
            assert np.array_equal(before[2], other[2]) and before[3].tobytes() == other[3].tobytes()
    finally:
        ctx.set_lanes(old)


# ------------------------------------------------------------------------------------------------------------------ command line
def test_command_line_auto_ignore(ctx, tmp_path, capsys):
    from cova_amd import train
    h, w, n = 45, 80, 40                                   # the geometry of test_gpu_sweep.py's command-line test
    frames = synth.carrier_frames(4 * n, h, w, seed=31, n_objects=5)
    frames[..., 3] = 0
    flat = W.blob_like()
    stacks, _ = train.slide(frames, np.zeros((4 * n, h, w), np.uint8))
    net = BlobNetInfer(ctx, flat, h, w, max_batch=n)
    logits, own = net.infer(stacks)
    assert own.any()
    # labels: the model's own default mask (blobs that move) plus a block that is there in every sample (the burned-in clock)
    block = np.zeros((h, w), bool)
    block[2:5, 66:78] = True
    labels = own | block.astype(np.uint8)
    gt = np.zeros((4 * n, h, w), np.uint8)
    gt[3::4] = labels
    th = cal.logit_thresholds(prob_thresholds=cal.DEFAULT_PROBS)         # the command line's default grid
    ref = heat_ref(logits, labels, th)
    # precondition: the block reaches the rate, and nothing outside it does, in the labels or in the predictions
    assert (ref["gt"][block] == n).all()
    assert (2 * ref["gt"][~block] < n).all() and (2 * ref["fire"][0][~block] < n).all()
    want_keep = cal.ignore_from_heat(ref, 0.5)
    assert np.array_equal(want_keep == 0, block)

    rec, wts, post, npz = tmp_path / "held_out.tfrecord", tmp_path / "cam.cvhw", tmp_path / "post.json", tmp_path / "heat.npz"
    with open(rec, "wb") as f:
        for i in range(0, 4 * n, 8):
            f.write(tfrecord_example(frames[i:i + 8], gt[i:i + 8], gop=8))
    wts.write_bytes(W.to_bytes(flat))
    assert cal.main([str(rec), "--weights", str(wts), "--h-mb", str(h), "--w-mb", str(w), "--batch", "16",
                     "--auto-ignore", "0.5", "--heat-out", str(npz), "-o", str(post)]) == 0
    text = capsys.readouterr().out
    assert "auto-ignore: 36 macroblocks" in text and 'pad-ignore-rects="IDX=1056,32,192,48"' in text and "choice:" in text
    kw, cc = cal.load_post(post, h, w)
    assert np.array_equal(kw["keep"], want_keep)
    assert not kw["keep"][block].any() and kw["keep"][~block].all()
    doc = json.loads(post.read_text())
    assert doc["ignore_rects"] == [[1056, 32, 192, 48]]
    assert doc["auto_ignore"] == {"rate": [1, 2], "source": "either", "dilate": 0, "logit_thresh": float(th[0]), "samples": n,
                                  "macroblocks_ignored": 36, "user_rects": []}
    saved = np.load(npz)
    for k in TABLES:
        assert np.array_equal(saved[k], ref[k]), k
    assert int(saved["samples"]) == n
    # the sidecar's scores are those of a sweep with that keep map
    res = cal.calibrate_records(ctx, flat, stacks, labels, h, w, prob_thresholds=cal.DEFAULT_PROBS, keep=want_keep, batch=16)
    ch = cal.choose(res, 0.95)
    assert doc["scores"] == {k: ch[k] for k in doc["scores"]} and doc["scores"]["samples"] == n
    assert doc["logit_thresh"] == ch["logit_thresh"] and cc == ch["cc_threshold"]
    # and differ from the scores without it: the block is a labelled object in every sample
    plain = cal.calibrate_records(ctx, flat, stacks, labels, h, w, prob_thresholds=cal.DEFAULT_PROBS, batch=16)
    assert plain["gt_objects"] > res["gt_objects"]
    # a user's rectangle is added to the derived region and recorded
    assert cal.main([str(rec), "--weights", str(wts), "--h-mb", str(h), "--w-mb", str(w), "--batch", "16",
                     "--auto-ignore", "0.5", "--ignore-rects", "0,0,320,48", "-o", str(post)]) == 0
    kw2, _ = cal.load_post(post, h, w)
    both = want_keep.copy()
    both[0:3, 0:20] = 0
    assert np.array_equal(kw2["keep"], both)
    assert json.loads(post.read_text())["auto_ignore"]["user_rects"] == [[0, 0, 320, 48]]
