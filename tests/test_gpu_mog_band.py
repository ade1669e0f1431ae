"""MoG labels at 2560x1440 and 3840x2160 (cova_amd.mog, grid="macroblock": working frames of 1280x720 and 1920x1080, whose post
kernel works in row bands; cova_amd/csrc/mog_band.hip) against the numpy oracle, bit for bit: raw masks, filled masks, labels
and, where MOG2 runs, every word of the model.  The banded post kernel is also held against the resident one at 960x540 on
identical planes (covahip_dev_mog_post_masks, covahip_dev_mog_set_post_form), for band heights that do and do not divide the
frame."""
import ctypes as C
import functools

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import mog
from tests import mog_band_ref as B
from tests import mog_grid_ref as G
from tests.test_gpu_mog import synth_video
from tests.test_gpu_mog_grid import _same_model, _state_equal

pytestmark = pytest.mark.gpu

W4K, H4K = 1920, 1080                             # working size of a 3840x2160 source


# ------------------------------------------------------------------------------------------------ planes and their oracle
@functools.lru_cache(maxsize=None)
def _planes_960():
    """name -> bool [540][960]: the six planted cases, three Bernoulli masks and a mask of random 8x8 blocks."""
    p = dict(G.planted_cases(540, 960))
    for d in (0.02, 0.2, 0.5):
        p[f"bernoulli{d}"] = B.bernoulli(540, 960, d, seed=int(d * 100))
    p["blocks0.3"] = B.blocks(540, 960, 0.3, seed=7)
    return p


@functools.lru_cache(maxsize=None)
def _plane_4k(name):
    h, w = H4K, W4K
    seam = B.seams(h, B.band_plan(w, h)[0])
    if name in ("spiral", "sealed_spiral"):
        return B.coarse_spirals(h, w)[name == "sealed_spiral"]
    if name == "corner_blob":
        return B.corner_blob(h, w)
    if name in ("corridor1", "corridor4"):
        return B.seam_corridors(h, w, int(name[-1]), seam)
    if name == "seam_morphology":
        return B.seam_morphology(h, w, seam)
    if name == "serpentine":
        return B.serpentine(h, w)
    if name == "serpentine_closed":
        return B.serpentine(h, w, closed_last=True)
    if name.startswith("bernoulli"):
        return B.bernoulli(h, w, float(name[9:]), seed=11)
    if name == "blocks0.3":
        return B.blocks(h, w, 0.3, seed=12)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _oracle_4k(name):
    return B.post(_plane_4k(name))


def _post(m, masks):
    """The labeller's post launch on bool masks [S][h][w] as one frame: (raw, filled, labels), each [S][..]."""
    labels = m.post_masks(np.stack([B.to_u8(x) for x in masks])[None])
    raw, filled = m.debug_masks()
    return raw[0], filled[0], labels[0]


# ------------------------------------------------------------------------------------------------ 1. banded against resident
def test_banded_equals_resident_at_960x540(ctx):
    planes = _planes_960()
    names = sorted(planes)
    masks = [planes[n] for n in names]
    m = mog.MogLabeler(ctx, 1920, 1080, streams=len(names), grid="macroblock")
    raw_r, fill_r, lab_r = _post(m, masks)
    for s, n in enumerate(names):
        assert (raw_r[s] == B.to_u8(planes[n])).all(), n
        f_o, l_o = B.post(planes[n])
        assert (fill_r[s] == f_o).all() and (lab_r[s] == l_o).all(), ("resident", n)
    assert fill_r[names.index("sealed_spiral")].sum() > planes["sealed_spiral"].sum()      # a fill happened
    for rows in (540, 270, 64, 37, 16):
        m.set_post_form(True, rows)
        raw_b, fill_b, lab_b = _post(m, masks)
        for s, n in enumerate(names):
            assert (raw_b[s] == raw_r[s]).all(), (rows, n)
            assert (fill_b[s] == fill_r[s]).all(), (rows, n)
            assert (lab_b[s] == lab_r[s]).all(), (rows, n)
    m.set_post_form(True, 0)                           # the automatic plan: one band
    assert (_post(m, masks)[1] == fill_r).all()
    m.set_post_form(False)
    assert (_post(m, masks)[1] == fill_r).all()
    lib = L.lib()
    for banded, rows in ((1, 15), (1, 541), (1, -1), (2, 0), (0, 64)):
        assert lib.covahip_dev_mog_set_post_form(m.handle, banded, rows) == 1, (banded, rows)
    m.close()
    for args in ((640, 360, "macroblock"), (1280, 720, "macroblock"), (1920, 1080, "reference")):
        small = mog.MogLabeler(ctx, args[0], args[1], grid=args[2])     # no banded kernel: 320x180, and the reference grid
        assert lib.covahip_dev_mog_set_post_form(small.handle, 1, 0) == 1
        assert lib.covahip_dev_mog_set_post_form(small.handle, 0, 0) == 0
        small.close()


# ------------------------------------------------------------------------------------------------ 2. seams at 1920x1080
@pytest.fixture(scope="module")
def labeler_4k(ctx):
    m = mog.MogLabeler(ctx, 3840, 2160, grid="macroblock")
    assert (m.work_w, m.work_h, m.label_h, m.label_w) == (W4K, H4K, 135, 240)
    yield m
    m.close()


@pytest.mark.parametrize("name", ["spiral", "sealed_spiral", "corner_blob", "corridor1", "corridor4", "seam_morphology",
                                  "serpentine", "serpentine_closed"])
def test_band_seams_at_1920x1080(labeler_4k, name):
    m = labeler_4k
    mask = _plane_4k(name)
    f_o, l_o = _oracle_4k(name)
    assert l_o.shape == (135, 240)
    for rows in (0, 64):
        m.set_post_form(True, rows)
        raw, filled, labels = _post(m, [mask])
        assert (raw[0] == B.to_u8(mask)).all(), rows
        assert (filled[0] == f_o).all(), (rows, int((filled[0] != f_o).sum()))
        assert (labels[0] == l_o).all(), rows
    m.set_post_form(True, 0)
    lib = L.lib()
    assert lib.covahip_dev_mog_set_post_form(m.handle, 0, 0) == 1            # no resident kernel at this size
    assert lib.covahip_dev_mog_set_post_form(m.handle, 1, 1080) == 1         # one band of 1080 rows does not fit LDS
    # what the planes are for, on the oracle (and so on the kernel)
    if name == "corner_blob":
        assert l_o[134, 239] == 1 and l_o[134].sum() > 1 and l_o[:, 239].sum() > 1
        assert f_o[1072, 1912] == 1 and not f_o[:1040].any()
    elif name in ("corridor1", "corridor4"):
        x0 = 64 * (W4K // 128) - 12
        seam = B.seams(H4K, B.band_plan(W4K, H4K)[0])
        assert len(seam) >= 1
        for s in seam:
            assert not mask[s, x0 - 15] and bool(f_o[s, x0 - 15]) == (name == "corridor1"), s
    elif name == "sealed_spiral":
        assert f_o.sum() > mask.sum()
    elif name in ("serpentine", "serpentine_closed"):
        ys, xs = B.last_lane(H4K, W4K)
        lane = f_o[ys, xs][4:-4, 4:-4]
        if name == "serpentine":
            assert not lane.any() and f_o.sum() == mask.sum()                # nothing is filled
        else:
            assert lane.all() and f_o.sum() == mask.sum() + (ys.stop - ys.start) * (xs.stop - xs.start)   # exactly that lane


# ------------------------------------------------------------------------------------------------ 3. random planes
@pytest.mark.parametrize("name", ["bernoulli0.02", "bernoulli0.2", "blocks0.3"])
def test_random_planes_at_1920x1080(labeler_4k, name):
    m = labeler_4k
    m.set_post_form(True, 0)
    mask = _plane_4k(name)
    f_o, l_o = _oracle_4k(name)
    raw, filled, labels = _post(m, [mask])
    assert (raw[0] == B.to_u8(mask)).all()
    assert (filled[0] == f_o).all(), int((filled[0] != f_o).sum())
    assert (labels[0] == l_o).all()


# ------------------------------------------------------------------------------------------------ 4. the full path
def test_full_path_3840x2160(ctx):
    n, hist = 3, 4
    vid = synth_video(n, 3840, 2160, seed=41)
    raw_r, fill_r, lab_r, mdl = G.label_video_grid(vid, history=hist)
    m = mog.MogLabeler(ctx, 3840, 2160, history=hist, grid="macroblock")
    labels = m.apply(vid[:, None])
    raw, filled = m.debug_masks()
    assert labels.shape == (n, 1, 135, 240) and raw.shape == (n, 1, H4K, W4K)
    assert (raw[:, 0] == raw_r).all() and (filled[:, 0] == fill_r).all() and (labels[:, 0] == lab_r).all()
    assert lab_r[1:].any() and not lab_r[1:].all()
    _state_equal(m.state(0), mdl)
    st = m.state(0)
    # the same call staged as one frame-step per update launch (a 24.9 MB frame exceeds the lowered budget)
    m.reset(0)
    m.set_stage_budget(1)
    ctx.profile(True)
    try:
        staged = m.apply(vid[:, None])
        prof = ctx.profile_read()
    finally:
        ctx.profile(False)
    assert {k: v[1] for k, v in prof.items()} == {"mog_band_update": n, "mog_band_post": 1}
    assert (staged == labels).all()
    for a, b in zip(m.debug_masks(), (raw, filled)):
        assert (a == b).all()
    _same_model(m.state(0), st)
    m.close()
    one = mog.MogLabeler(ctx, 3840, 2160, history=hist, grid="macroblock")
    for i in range(n):
        lab = one.apply(vid[i:i + 1, None])
        r1, f1 = one.debug_masks()
        assert (lab[0, 0] == lab_r[i]).all() and (r1[0, 0] == raw_r[i]).all() and (f1[0, 0] == fill_r[i]).all(), i
    _same_model(one.state(0), st)
    one.close()


def test_full_path_2560x1440_two_streams_staged_device_and_reset(ctx):
    n, S, hist = 4, 2, 4
    nv = np.array([4, 3], np.int32)
    vid = np.stack([synth_video(n, 2560, 1440, seed=50 + s) for s in range(S)], 1)
    ref = [G.label_video_grid(vid[:nv[s], s], history=hist) for s in range(S)]
    step = S * 2560 * 1440 * 3
    host = mog.MogLabeler(ctx, 2560, 1440, streams=S, history=hist, grid="macroblock")
    assert (host.work_w, host.work_h, host.label_h, host.label_w) == (1280, 720, 90, 160)
    host.set_stage_budget(step)                        # one frame-step per update launch
    pre = np.full((n, S, 90, 160), 77, np.uint8)
    lab_h = host.apply(vid, n_valid=nv, labels=pre)
    raw, filled = host.debug_masks()
    for s in range(S):
        k = int(nv[s])
        raw_r, fill_r, lab_r, mdl = ref[s]
        assert (raw[:k, s] == raw_r).all() and (filled[:k, s] == fill_r).all(), s
        assert (lab_h[:k, s] == lab_r).all() and (lab_h[k:, s] == 77).all(), s
        _state_equal(host.state(s), mdl)
    dev = mog.MogLabeler(ctx, 2560, 1440, streams=S, history=hist, grid="macroblock")
    d_f, d_l = ctx.malloc(vid.nbytes), ctx.malloc(pre.nbytes)
    try:
        ctx.h2d(d_f, vid)
        ctx.h2d(d_l, np.full((n, S, 90, 160), 77, np.uint8))
        dev.apply_device(d_f, n, d_l, n_valid=nv)
        lab_d = np.empty_like(lab_h)
        ctx.d2h(lab_d, d_l)
    finally:
        ctx.free(d_f)
        ctx.free(d_l)
    assert (lab_d == lab_h).all()
    for s in range(S):
        _same_model(dev.state(s), host.state(s), s)
    dev.close()
    # reset of stream 1, then one more frame: stream 1 starts over, stream 0 goes on
    host.reset(1)
    assert host.state(1)["n"] == 0 and not host.state(1)["nmodes"].any()
    nxt = np.stack([synth_video(1, 2560, 1440, seed=60 + s) for s in range(S)], 1)
    lab = host.apply(nxt)
    _, _, lab0, mdl0 = G.label_video_grid(nxt[:, 0], history=hist, model=ref[0][3])
    _, _, lab1, mdl1 = G.label_video_grid(nxt[:, 1], history=hist)
    assert (lab[:, 0] == lab0).all() and (lab[:, 1] == lab1).all() and lab1.all()
    _state_equal(host.state(0), mdl0)
    _state_equal(host.state(1), mdl1)
    host.close()


# ------------------------------------------------------------------------------------------------ 5. the labels are usable
def test_4k_labels_train_and_evaluate(ctx, labeler_4k):
    from cova_amd import train

    m = labeler_4k
    m.set_post_form(True, 0)
    masks = [B.blocks(H4K, W4K, 0.05, seed=s, size=40) for s in (1, 2)]
    labels = np.stack([_post(m, [x])[2][0] for x in masks])
    assert labels.shape == (2, 135, 240) and labels.any() and not labels.all()
    rng = np.random.default_rng(9)
    stacks = rng.integers(0, 7, (2, 4 * 135, 240, 4), dtype=np.uint8)
    stacks[..., 3] = 0
    tr = train.Trainer(ctx, 135, 240, max_batch=2, seed=0)
    loss = tr.step(stacks, labels)
    assert np.isfinite(loss)
    res = L.TrainEvalResult()                          # (the binding's dict has ratios; the counts are in the struct)
    L.check(tr._lib.covahip_train_eval(tr.handle, stacks.ctypes.data, labels.ctypes.data, 2, None, None, C.byref(res), L.MEM_HOST),
            "covahip_train_eval", ctx.handle)
    assert res.samples == 2 and np.isfinite(res.loss)
    assert int(res.tp) + int(res.fn) == int(labels.sum())
    ev = tr.evaluate((stacks, labels))
    assert ev["samples"] == 2 and np.isfinite(ev["loss"])
    tr.close()


# ------------------------------------------------------------------------------------------------ 6. nothing else moved
def test_1080p_macroblock_labeller_launches_what_it_did(ctx):
    """Without the developer switch a 1920x1080 macroblock labeller runs the resident kernels: one `mog_update` and one
    `mog_post` launch per call (the profile of this test body on the commit before the banded kernels), and its labels on the
    planted cases are the resident result."""
    cases = G.planted_cases(540, 960)
    names = sorted(cases)
    vid = G.plant([cases[n] for n in names], 2)
    m = mog.MogLabeler(ctx, 1920, 1080, streams=len(names), grid="macroblock")
    ctx.profile(True)
    try:
        labels = m.apply(vid)
        prof = ctx.profile_read()
    finally:
        ctx.profile(False)
    assert {k: v[1] for k, v in prof.items()} == {"mog_update": 1, "mog_post": 1}
    raw, filled = m.debug_masks()
    ctx.profile(True)
    try:
        lab_p = m.post_masks(raw[1:2])                 # the same planes through the developer entry: the resident kernel again
        prof_p = ctx.profile_read()
        m.set_post_form(True)
        lab_b = m.post_masks(raw[1:2])                 # and only the switch reaches the banded one
        prof_b = ctx.profile_read()
    finally:
        ctx.profile(False)
    assert {k: v[1] for k, v in prof_p.items()} == {"mog_post": 1}
    assert {k: v[1] for k, v in prof_b.items()} == {"mog_post": 1, "mog_band_post": 1}
    assert (lab_p[0] == labels[1]).all() and (lab_b[0] == labels[1]).all()
    for s, n in enumerate(names):
        assert (raw[1, s] == B.to_u8(cases[n])).all(), n
        f_o, l_o = B.post(cases[n])
        assert (filled[1, s] == f_o).all() and (labels[1, s] == l_o).all(), n
    m.close()
