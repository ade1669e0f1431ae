"""Per-model area threshold (covahip_blobnet_set_area): for a stack b that runs on model m
    eff(b) = area[m] >= 1 ? area[m] : the call's area_thresh,   boxes[b] = regionprops(mask[b], eff(b))
inside every kernel that runs bboxcc behind a BlobNet forward.  Every comparison is exact: the expected boxes are the CPU
reference's regionprops of the GPU's own mask at eff(b), byte for byte and in order, and logits and masks must equal those of a
ctx that never had an area.  Every case first checks, from the CPU reference alone, that for at least one frame of every model
with an area the box list at eff(b) is not empty and differs from the list at the call's scalar (_expected): neither a no-op nor
a dropped frame can pass.  The weights are noise-like (random_init with a negative foreground bias): many components of 1 - 10
macroblocks per frame.

Which kernel runs the tail of a (geometry, switch) pair: the table of tests/test_gpu_post.py, asserted here against
covahip_dev_blobnet_tail_form as well.  An area alone runs the POST = true instantiations: a batch of one
model gets its threshold by value, a mixed batch looks it up per stack through the model id (MS = true)."""
import ctypes as C

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import calibrate
from cova_amd import weights as W
from cova_amd.elements import BboxCc, BlobNetInfer, FilterPipe, pack_frames
from oracle import ref

pytestmark = pytest.mark.gpu

MAXB = 1024
ALONE, ROWS, BANDS = BlobNetInfer.TAIL_ALONE, BlobNetInfer.TAIL_ROWS, BlobNetInfer.TAIL_BANDS     # BANDS + 2 * WV + PART
AREAS3 = (0, 2, 7)            # model 0 unset, models 1 and 2 with a threshold of their own


@pytest.fixture(scope="module")
def models():
    return [W.random_init(33, fg_bias=-0.1), W.random_init(22, fg_bias=-0.1), W.random_init(11, fg_bias=-0.1)]


def _frames(rng, n, h, w):
    f = np.zeros((n, h, w, 4), np.uint8)
    f[..., 0] = rng.integers(0, 8, (n, h, w))
    f[..., 1:3] = rng.integers(0, 9, (n, h, w, 2))
    return f


def _own_frames_table(batch):
    return np.arange(batch * 4, dtype=np.int32).reshape(batch, 4)[:, ::-1].copy()


def _stack_of(frames, table):
    return np.ascontiguousarray(frames[table].reshape(table.shape[0], -1, frames.shape[2], 4))


def _eff(areas, ids, scalar):
    return np.array([areas[k] if areas[k] >= 1 else scalar for k in ids], np.int32)


def _expected(mask, eff, scalar, ids, max_boxes=MAXB):
    """The CPU reference's (boxes, counts) per frame at eff(b) -- after checking, from the reference alone, that the per-model
    thresholds matter: a model whose threshold differs from the scalar has a frame whose list is not empty and not the scalar's,
    any other model a frame with boxes."""
    rb = np.zeros((len(eff), max_boxes), ref.BOX_DTYPE)
    rc = np.zeros(len(eff), np.int32)
    sb, sc = ref.regionprops_batch(mask, scalar, max_boxes)
    for t in np.unique(eff):
        sel = eff == t
        rb[sel], rc[sel] = ref.regionprops_batch(mask[sel], int(t), max_boxes)
    for k in np.unique(ids):
        sel = np.flatnonzero(ids == k)
        if eff[sel[0]] == scalar:
            assert rc[sel].sum() > 0, k
        else:
            assert any(rc[i] > 0 and (rc[i] != sc[i] or rb[i, :min(rc[i], max_boxes)].tobytes() != sb[i, :min(sc[i], max_boxes)].tobytes())
                       for i in sel), f"model {k}: the threshold changes nothing"
    return rb, rc


def _eq(got, want, max_boxes=MAXB):
    boxes, counts = got[0], got[1]
    rb, rc = want
    assert np.array_equal(counts, rc), (counts.tolist(), rc.tolist())
    for i in range(len(rc)):
        n = min(int(rc[i]), max_boxes)
        assert boxes[i, :n].tobytes() == rb[i, :n].tobytes(), i


def _eq_runs(a, b):
    """Two runs: boxes up to their counts, counts, mask bytes, logits."""
    assert np.array_equal(a[1], b[1])
    for i in range(len(a[1])):
        n = min(int(a[1][i]), a[0].shape[1])
        assert a[0][i, :n].tobytes() == b[0][i, :n].tobytes(), i
    assert a[2].tobytes() == b[2].tobytes()
    assert a[3].tobytes() == b[3].tobytes()


def _run_packed(ctx, net, frames, table, scalar, ids, max_boxes=MAXB):
    """covahip_filter_forward_frames_packed_m: device pointers, two-byte records."""
    b, h, w = table.shape[0], net.h, net.w
    rec = pack_frames(frames)
    d = [ctx.malloc(rec.nbytes), ctx.malloc(b * max_boxes * 20), ctx.malloc(b * 4), ctx.malloc(b * h * w), ctx.malloc(b * h * w * 4)]
    try:
        ctx.h2d(d[0], rec)
        L.check(L.lib().covahip_memset(ctx.handle, d[1], 0, b * max_boxes * 20), "memset")
        net.filter_frames_device(d[0], frames.shape[0], table, b, scalar, d[1], d[2], max_boxes, d_mask=d[3], model_ids=ids, d_logits=d[4],
                                 packed=True)
        ctx.sync()
        out = (np.empty((b, max_boxes), L.BOX_DTYPE), np.empty(b, np.int32), np.empty((b, h, w), np.uint8), np.empty((b, h, w), np.float32))
        for a, p in zip(out, d[1:]):
            ctx.d2h(a, p)
        return out
    finally:
        for p in d:
            ctx.free(p)


def _three_entries(ctx, net, frames, table, scalar, ids):
    """The stacked, the carrier-frame and the packed entry: bit for bit the same; -> the carrier-frame entry's result."""
    got = net.filter_frames(frames, table, scalar, MAXB, True, True, model_ids=ids)
    form = net.tail_form()
    _eq_runs(net.filter_full(_stack_of(frames, table), scalar, MAXB, True, True, model_ids=ids), got)
    _eq_runs(_run_packed(ctx, net, frames, table, scalar, ids), got)
    return got, form


# ------------------------------------------------------------------------------------------------------------------ every tail form
def _tail_form(h, w, switch):
    wv = 0 if switch == "wave_cap" or w % 8 else 1
    if switch == "tail_skip_tensor":
        return BANDS + 2 * wv
    if switch == "mfma" and wv and (h, w) != (16, 16):
        return ROWS
    return BANDS + 2 * wv + 1


FORMS = [(16, 16, "mfma"), (16, 24, "mfma"), (18, 72, "mfma"), (20, 28, "mfma"), (45, 80, "tail_band_tiles"),
         (18, 72, "tail_skip_tensor"), (20, 28, "tail_skip_tensor"), (18, 72, "wave_cap"), (45, 80, "mfma")]


@pytest.mark.parametrize("h,w,switch", FORMS)
def test_every_tail_form(ctx, models, h, w, switch):
    b, scalar = 9, 1
    rng = np.random.default_rng(h * 1000 + w)
    frames, table = _frames(rng, 4 * b, h, w), _own_frames_table(b)
    cc = BboxCc(ctx, 1, MAXB)

    def load(ws):
        net = BlobNetInfer(ctx, ws, h, w, max_batch=b)
        if switch in ("tail_band_tiles", "tail_skip_tensor"):
            net.set_impl(switch)
        return net

    try:
        if switch == "wave_cap":
            cc.set_wave_cap(-1)
        ctx.profile(True)
        # one model: the threshold by value
        base = load(models[2]).filter_frames(frames, table, scalar, MAXB, True, True)        # a ctx that never had an area
        net = load(models[2])
        net.set_area(0, 3)
        want = _expected(base[2], np.full(b, 3, np.int32), scalar, np.zeros(b, np.uint8))
        got, form = _three_entries(ctx, net, frames, table, scalar, None)
        assert form == _tail_form(h, w, switch), (form, _tail_form(h, w, switch))
        assert got[2].tobytes() == base[2].tobytes() and got[3].tobytes() == base[3].tobytes()   # masks and logits are not affected
        _eq(got, want)
        # three models, stacks interleaved: the threshold through the model id
        ids = (np.arange(b) % 3).astype(np.uint8)
        base = load(models).filter_frames(frames, table, scalar, MAXB, True, True, model_ids=ids)
        net = load(models)
        for k, a in enumerate(AREAS3):
            if a:
                net.set_area(k, a)
        want = _expected(base[2], _eff(AREAS3, ids, scalar), scalar, ids)
        got, form = _three_entries(ctx, net, frames, table, scalar, ids)
        assert form == _tail_form(h, w, switch)
        assert got[2].tobytes() == base[2].tobytes() and got[3].tobytes() == base[3].tobytes()
        _eq(got, want)
        ctx.sync()
        names = ctx.profile_read()
        assert "dec3_bboxcc_fused" in names and not any(n.startswith("bboxcc") for n in names)   # no launch was added
    finally:
        ctx.profile(False)
        cc.set_wave_cap(0)


def test_more_frames_than_workgroups(ctx, models):
    """A workgroup of the row form takes several stacks of different models: the threshold is looked up per stack."""
    h, w, scalar = 16, 24, 1
    b = 2 * ctx.info()["num_cu"] + 5
    rng = np.random.default_rng(4)
    frames, table = _frames(rng, 4 * b, h, w), _own_frames_table(b)
    ids = (np.arange(b) % 3).astype(np.uint8)
    net = BlobNetInfer(ctx, models, h, w, max_batch=b)
    base = net.filter_frames(frames, table, scalar, MAXB, True, True, model_ids=ids)
    for k, a in enumerate(AREAS3):
        net.set_area(k, a)
    got = net.filter_frames(frames, table, scalar, MAXB, True, True, model_ids=ids)
    assert net.tail_form() == ROWS
    assert got[2].tobytes() == base[2].tobytes() and got[3].tobytes() == base[3].tobytes()
    _eq(got, _expected(base[2], _eff(AREAS3, ids, scalar), scalar, ids))


# ------------------------------------------------------------------------------------------------------------------ non-fused fallback
def test_fallback_135x240(ctx, models):
    """A frame that does not fit the fused tail: the last block alone, then the stand-alone bboxcc with the stacks' thresholds."""
    h, w, b, scalar = 135, 240, 2, 1
    rng = np.random.default_rng(9)
    frames, table = _frames(rng, 4 * b, h, w), _own_frames_table(b)
    net = BlobNetInfer(ctx, models[1:], h, w, max_batch=b)
    areas = (2, 6)
    # the same thresholds twice (nothing is uploaded the second time), swapped, one model by id, model 0 without ids
    cases = ([0, 1], [0, 1], [1, 0], [1, 1], None)
    plain = {str(ids): net.filter_frames(frames, table, scalar, MAXB, True, True, model_ids=ids) for ids in cases}
    assert net.tail_form() == ALONE
    for k, a in enumerate(areas):
        net.set_area(k, a)
    ctx.profile(True)
    try:
        for ids in cases:
            ids_a = np.zeros(b, np.uint8) if ids is None else np.array(ids, np.uint8)
            got = net.filter_frames(frames, table, scalar, MAXB, True, True, model_ids=ids)
            assert net.tail_form() == ALONE
            base = plain[str(ids)]
            assert got[2].tobytes() == base[2].tobytes() and got[3].tobytes() == base[3].tobytes()
            _eq(got, _expected(base[2], _eff(areas, ids_a, scalar), scalar, ids_a))
        ctx.sync()
        names = ctx.profile_read()
        assert "dec3_final_mfma" in names and "bboxcc_big_kernel" in names and "dec3_bboxcc_fused" not in names
    finally:
        ctx.profile(False)


# ------------------------------------------------------------------------------------------------------------------ interplay
def test_interplay_with_set_post(ctx, models):
    h, w, b, scalar = 45, 80, 8, 1
    rng = np.random.default_rng(21)
    frames, table = _frames(rng, 4 * b, h, w), _own_frames_table(b)
    ids = (np.arange(b) % 2).astype(np.uint8)
    keep = np.ones((h, w), np.uint8)
    keep[h // 2] = 0
    keep[:, w // 3] = 0
    plain = BlobNetInfer(ctx, models[1:], h, w, max_batch=b).filter_frames(frames, table, scalar, MAXB, True, True, model_ids=ids)
    net = BlobNetInfer(ctx, models[1:], h, w, max_batch=b)
    assert [net.get_area(k) for k in range(2)] == [0, 0]
    # threshold + keep map and an area on the same model
    net.set_post(1, logit_thresh=-0.25, keep=keep)
    net.set_area(1, 4)
    assert net.get_area(1) == 4 and net.post(1)[0] == -0.25
    got = net.filter_frames(frames, table, scalar, MAXB, True, True, model_ids=ids)
    mask = plain[2].copy()
    mask[ids == 1] = ((plain[3][ids == 1] > np.float32(-0.25)) & (keep != 0)).astype(np.uint8)
    assert not np.array_equal(mask, plain[2])
    assert got[2].tobytes() == mask.tobytes() and got[3].tobytes() == plain[3].tobytes()
    _eq(got, _expected(mask, _eff((0, 4), ids, scalar), scalar, ids))
    # set_post(NULL) leaves the area set; set_area leaves the post settings
    net.reset_post(1)
    assert net.get_area(1) == 4 and net.post(1) == (0.0, None)
    got = net.filter_frames(frames, table, scalar, MAXB, True, True, model_ids=ids)
    assert got[2].tobytes() == plain[2].tobytes() and got[3].tobytes() == plain[3].tobytes()
    _eq(got, _expected(plain[2], _eff((0, 4), ids, scalar), scalar, ids))
    net.set_post(0, logit_thresh=0.5)
    net.set_area(0, 2)
    assert net.post(0)[0] == 0.5 and net.get_area(0) == 2
    net.reset_post(0)
    # set_area(0): the call's scalar again -- whatever it is
    net.set_area(1, 0)
    assert net.get_area(1) == 0
    for sc in (1, 3):
        got = net.filter_frames(frames, table, sc, MAXB, True, True, model_ids=ids)
        _eq(got, _expected(plain[2], _eff((2, 0), ids, sc), sc, ids))
    # a model's own threshold wins over a LARGER scalar as well
    got = net.filter_frames(frames, table, 9, MAXB, True, True, model_ids=ids)
    _eq(got, _expected(plain[2], _eff((2, 0), ids, 9), 9, ids))
    # a reload resets every model
    net = BlobNetInfer(ctx, models[1:], h, w, max_batch=b)
    assert [net.get_area(k) for k in range(2)] == [0, 0]
    _eq_runs(net.filter_frames(frames, table, scalar, MAXB, True, True, model_ids=ids), plain)
    one = BlobNetInfer(ctx, models[1], h, w, max_batch=b)
    one.set_area(0, 5)
    one = BlobNetInfer(ctx, models[1], h, w, max_batch=b)            # covahip_blobnet_load as well
    assert one.get_area(0) == 0


# ------------------------------------------------------------------------------------------------------------------ defaults
@pytest.mark.parametrize("h,w", [(68, 120), (45, 80)])
def test_set_and_cleared_is_never_set(ctx, models, h, w):
    b, scalar = 12, 2
    rng = np.random.default_rng(h)
    frames, table = _frames(rng, 4 * b, h, w), _own_frames_table(b)
    fresh, net = BlobNetInfer(ctx, models[2], h, w, max_batch=b), None

    def profiled(n):
        ctx.profile(True)
        try:
            out = n.filter_frames(frames, table, scalar, MAXB, True, True)
            ctx.sync()
            return out, {k: v[1] for k, v in ctx.profile_read().items()}
        finally:
            ctx.profile(False)

    never, launches = profiled(fresh)
    assert never[1].sum() > 0 and "dec3_bboxcc_fused" in launches
    net = BlobNetInfer(ctx, models[2], h, w, max_batch=b)
    net.set_area(0, 6)
    changed = net.filter_frames(frames, table, scalar, MAXB, True, True)
    _eq(changed, _expected(never[2], np.full(b, 6, np.int32), scalar, np.zeros(b, np.uint8)))
    net.set_area(0, 0)
    again, launches2 = profiled(net)
    _eq_runs(again, never)
    assert launches2 == launches              # the same launches as a ctx that never had one


# ------------------------------------------------------------------------------------------------------------------ truncation
def test_truncation(ctx, models):
    """max_boxes below a frame's passing count: the count reports every passing component, the first max_boxes are written."""
    h, w, b, scalar, max_boxes = 45, 80, 9, 1, 12
    rng = np.random.default_rng(13)
    frames, table = _frames(rng, 4 * b, h, w), _own_frames_table(b)
    ids = (np.arange(b) % 3).astype(np.uint8)
    net = BlobNetInfer(ctx, models, h, w, max_batch=b)
    base = net.filter_frames(frames, table, scalar, max_boxes, True, True, model_ids=ids)
    for k, a in enumerate(AREAS3):
        net.set_area(k, a)
    want = _expected(base[2], _eff(AREAS3, ids, scalar), scalar, ids, max_boxes)
    assert (want[1][ids == 2] > max_boxes).any() and (want[1][ids == 1] > max_boxes).any()
    got = net.filter_frames(frames, table, scalar, max_boxes, True, True, model_ids=ids)
    _eq(got, want, max_boxes)


# ------------------------------------------------------------------------------------------------------------------ lanes and pipe
@pytest.mark.parametrize("packed", [False, True])
def test_pipe_three_lanes(ctx, models, packed):
    """Three lanes, three slots, mixed model ids per slot; a set_area between two submits: the batches submitted before it have
    the old value, the batch after it the new one."""
    h, w, b, scalar = 45, 80, 12, 1
    rng = np.random.default_rng(31 + packed)
    table = _own_frames_table(b)
    old_areas, new_areas = AREAS3, (5, 2, 0)
    old = ctx.lanes()
    ctx.set_lanes(3)
    try:
        net = BlobNetInfer(ctx, models, h, w, max_batch=b)
        for k, a in enumerate(old_areas):
            net.set_area(k, a)
        pipe = FilterPipe(net, max_batch=b, max_frames=4 * b, max_boxes=MAXB, n_slots=3, want_mask=True, packed=packed)
        pending = []
        try:
            for j in range(3):
                if j == 2:                                           # two batches are in flight
                    for k, a in enumerate(new_areas):
                        net.set_area(k, a)
                slot, fr, idx = pipe.acquire()
                frames = _frames(rng, 4 * b, h, w)
                ids = rng.permutation(np.arange(b) % 3).astype(np.uint8)
                fr[:4 * b] = pack_frames(frames) if packed else frames
                idx[:b] = table
                pipe.model_ids(slot)[:b] = ids
                pipe.submit(slot, 4 * b, b, scalar)
                pending.append((slot, frames, ids, old_areas if j < 2 else new_areas))
            results = []
            for slot, frames, ids, areas in pending:
                counts, offsets, boxes, mask = pipe.collect(slot)
                results.append((frames, ids, areas, counts.copy(), offsets.copy(), boxes.copy(), mask.copy()))
        finally:
            pipe.close()
        plain = BlobNetInfer(ctx, models, h, w, max_batch=b)
        for frames, ids, areas, counts, offsets, boxes, mask in results:
            pm = plain.filter_frames(frames, table, scalar, MAXB, True, False, model_ids=ids)[2]
            assert mask.tobytes() == pm.tobytes()
            rb, rc = _expected(pm, _eff(areas, ids, scalar), scalar, ids)
            assert np.array_equal(counts, rc)
            for j in range(b):
                n = min(int(rc[j]), MAXB)
                assert boxes[offsets[j]:offsets[j] + n].tobytes() == rb[j, :n].tobytes()
    finally:
        ctx.set_lanes(old)


def test_set_area_drains_the_lanes(ctx, models):
    """Device-pointer calls on three lanes with nothing synchronised in between, set_area, three more."""
    h, w, b, scalar = 45, 80, 16, 1
    rng = np.random.default_rng(77)
    table = _own_frames_table(b)
    frames = [_frames(rng, 4 * b, h, w) for _ in range(3)]
    old = ctx.lanes()
    ctx.set_lanes(3)
    bufs = []
    try:
        net = BlobNetInfer(ctx, models[2], h, w, max_batch=b)
        d_fr = []
        for f in frames:
            d = ctx.malloc(f.nbytes)
            bufs.append(d)
            ctx.h2d(d, f)
            d_fr.append(d)

        def submit(i):
            d = [ctx.malloc(b * MAXB * 20), ctx.malloc(b * 4), ctx.malloc(b * h * w)]
            bufs.extend(d)
            net.filter_frames_device(d_fr[i], 4 * b, table, b, scalar, d[0], d[1], MAXB, d_mask=d[2])
            return d

        net.set_area(0, 2)
        first = [submit(i) for i in range(3)]
        net.set_area(0, 7)
        later = [submit(i) for i in range(3)]
        ctx.sync()
        for handles, a in ((first, 2), (later, 7)):
            for d in handles:
                out = (np.empty((b, MAXB), L.BOX_DTYPE), np.empty(b, np.int32), np.empty((b, h, w), np.uint8))
                for arr, p in zip(out, d):
                    ctx.d2h(arr, p)
                _eq(out, _expected(out[2], np.full(b, a, np.int32), scalar, np.zeros(b, np.uint8)))
    finally:
        ctx.sync()
        for d in bufs:
            ctx.free(d)
        ctx.set_lanes(old)


# ------------------------------------------------------------------------------------------------------------------ calibration
def test_calibration_closes_the_loop(ctx, models):
    """What covahip_post_sweep counts in cell (t, a) is what serving emits with set_post(thr_t) and set_area(a)."""
    h, w, n, max_boxes = 45, 80, 16, 512
    rng = np.random.default_rng(55)
    frames, table = _frames(rng, 4 * n, h, w), _own_frames_table(n)
    stack = _stack_of(frames, table)
    thresholds, areas = [-0.5, 0.0, 0.75], [1, 2, 4, 8]
    net = BlobNetInfer(ctx, models[2], h, w, max_batch=n)
    logits, _ = net.infer(stack)
    res = calibrate.sweep(ctx, logits, np.zeros((n, h, w), np.uint8), thresholds, areas, max_boxes=max_boxes)
    assert (res["truncated"] == 0).all()
    pred = res["pred"]
    assert (pred[:, 0] > pred[:, 1]).all() and (pred[:, 2] > pred[:, 3]).all() and (pred[:, 3] > 0).all()   # every cell is its own
    for t, thr in enumerate(thresholds):
        net.set_post(0, logit_thresh=thr)
        for a, area in enumerate(areas):
            net.set_area(0, area)
            _, counts, _ = net.filter(stack, cc_threshold=1, max_boxes=max_boxes)
            assert int(counts.sum()) == int(pred[t, a]), (thr, area, int(counts.sum()), int(pred[t, a]))
    # the sidecar round trip applies both
    net.reset_post(0)
    net.set_area(0, 0)
    assert calibrate.apply_post(net, 0, ({"logit_thresh": 0.75, "keep": None}, 4)) == 4
    assert net.post(0) == (0.75, None) and net.get_area(0) == 4
    assert int(net.filter(stack, cc_threshold=1, max_boxes=max_boxes)[1].sum()) == int(pred[2, 2])


# ------------------------------------------------------------------------------------------------------------------ errors
def test_errors_leave_the_settings_alone(ctx, models):
    h, w, b = 20, 28, 6
    lib = L.lib()
    rng = np.random.default_rng(8)
    frames, table = _frames(rng, 4 * b, h, w), _own_frames_table(b)
    net = BlobNetInfer(ctx, models[:2], h, w, max_batch=b)
    net.set_area(1, 3)
    ids = np.ones(b, np.uint8)
    before = net.filter_frames(frames, table, 1, MAXB, True, True, model_ids=ids)
    _eq(before, _expected(before[2], np.full(b, 3, np.int32), 1, ids))
    v = C.c_int(-7)
    for model, area in ((1, -1), (1, -2 ** 31), (2, 4), (-1, 4)):
        assert lib.covahip_blobnet_set_area(ctx.handle, model, area) == 1, (model, area)
    assert lib.covahip_blobnet_set_area(None, 0, 1) == 1
    assert lib.covahip_blobnet_get_area(ctx.handle, 2, C.byref(v)) == 1 and lib.covahip_blobnet_get_area(ctx.handle, -1, C.byref(v)) == 1
    assert lib.covahip_blobnet_get_area(ctx.handle, 1, None) == 1 and lib.covahip_blobnet_get_area(None, 1, C.byref(v)) == 1
    assert v.value == -7
    assert [net.get_area(k) for k in range(2)] == [0, 3]
    _eq_runs(net.filter_frames(frames, table, 1, MAXB, True, True, model_ids=ids), before)
    # NULL threshold array of the stand-alone entry
    boxes, counts = np.zeros((b, 8), L.BOX_DTYPE), np.zeros(b, np.int32)
    assert lib.covahip_bboxcc_v(ctx.handle, before[2].ctypes.data, b, h, w, None, boxes.ctypes.data, counts.ctypes.data, 8, L.MEM_HOST) == 1
    # no model loaded: a failed load leaves the ctx without one
    blob = W.to_bytes(models[0])
    ptrs, sizes = (C.c_char_p * 1)(blob), (C.c_size_t * 1)(len(blob) - 4)
    assert lib.covahip_blobnet_load_set(ctx.handle, 1, ptrs, sizes, h, w, 4, b) == 6
    assert lib.covahip_blobnet_set_area(ctx.handle, 0, 2) == 4
    assert lib.covahip_blobnet_get_area(ctx.handle, 0, C.byref(v)) == 4
