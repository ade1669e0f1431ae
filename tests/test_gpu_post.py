"""Per-model post-processing (covahip_blobnet_set_post): for a stack b that runs on model m
    mask[b] = (logit[b] > logit_thresh[m]) & keep[m],   boxes[b] = regionprops(mask[b])
inside every kernel that turns logits into a mask.  Every comparison is exact: the expected mask is built on the host from the
GPU's own logits, the expected boxes are the CPU reference's regionprops of that mask (byte for byte, order included), and the
logits must equal those of a ctx that never had settings.  Each case also checks something that does not depend on the code
under test -- the expected mask differs from the default one and holds a box (unless the case is meant to be empty) -- so a
no-op cannot pass.

Which kernel ran the last decoder block of a (geometry, switch) pair, worked out from the planner's conditions in blobnet_mfma.hip
(run_tail_fused) and ASSERTED below against covahip_dev_blobnet_tail_form (the profile's launch names cannot tell the fused
forms apart: all of them launch as "dec3_bboxcc_fused"):
    switch             (16,16)            (18,72)            (20,28)            (45,80)            (68,120)
    mfma               dec3cc_mfma<1,1>   dec3cc_rows_mfma   dec3cc_mfma<0,1>   dec3cc_rows_mfma   dec3cc_rows_mfma
    tail_band_tiles    dec3cc_mfma<1,1>   dec3cc_mfma<1,1>   dec3cc_mfma<0,1>   dec3cc_mfma<1,1>   dec3cc_mfma<1,1>
    tail_skip_tensor   dec3cc_mfma<1,0>   dec3cc_mfma<1,0>   dec3cc_mfma<0,0>   dec3cc_mfma<1,0>   dec3cc_mfma<1,0>
    dec_separate       as mfma (the switch splits decoder blocks 0..2; the tail is unchanged)
    wave_cap -1        dec3cc_mfma<0,1>   dec3cc_mfma<0,1>   dec3cc_mfma<0,1>   dec3cc_mfma<0,1>   dec3cc_mfma<0,1>
    infer()            dec_mfma<16,0,16,FINAL> (launch "dec3_final_mfma"), mask only
(dec3cc_mfma<WV, PART>, WV = 1 the run-based bboxcc body, 0 the block-based one.  (20, 28) has W % 8 != 0, which neither the
row form nor the run-based body takes.  (16, 16) does not take the row form either: its parity planes, (2 * 8 + 2) * 16 = 288
bytes, do not fit the 256 bytes of the frame's mask region they would replace; the smallest grid of the row form is (16, 24),
which the frames-over-workgroups case runs beside (16, 16).)  A mixed batch runs the MS = true instantiation of the same kernel."""
import ctypes as C

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import weights as W
from cova_amd.elements import BboxCc, BlobNetInfer, FilterPipe, pack_frames
from oracle import ref

pytestmark = pytest.mark.gpu

MAXB = 256
LOG4 = np.float32(np.log(4.0))


def _frames(rng, n, h, w):
    f = np.zeros((n, h, w, 4), np.uint8)
    f[..., 0] = rng.integers(0, 8, (n, h, w))
    f[..., 1:3] = rng.integers(0, 9, (n, h, w, 2))
    return f


def _own_frames_table(batch):
    return np.arange(batch * 4, dtype=np.int32).reshape(batch, 4)[:, ::-1].copy()


def _stack_of(frames, table):
    """The stacked tensor [B][4 h][w][4] of a carrier-frame call."""
    return np.ascontiguousarray(frames[table].reshape(table.shape[0], -1, frames.shape[2], 4))


def _expect(logits, thr, keep):
    keep = np.ones(logits.shape[-2:], bool) if keep is None else keep != 0
    return ((logits > np.float32(thr)) & keep).astype(np.uint8)


def _eq_boxes(boxes, counts, mask, max_boxes=MAXB):
    """boxes / counts against the CPU reference's regionprops of `mask`, byte for byte."""
    rb, rc = ref.regionprops_batch(mask, 1, max_boxes)
    assert np.array_equal(counts, rc), (counts.tolist(), rc.tolist())
    for i in range(len(rc)):
        n = min(int(rc[i]), max_boxes)
        assert boxes[i, :n].tobytes() == rb[i, :n].tobytes(), i
    return rc


def _eq_runs(a, b):
    """Two runs: boxes up to their counts, counts, mask bytes, logits as floats."""
    assert np.array_equal(a[1], b[1])
    for i in range(len(a[1])):
        n = min(int(a[1][i]), a[0].shape[1])
        assert a[0][i, :n].tobytes() == b[0][i, :n].tobytes(), i
    assert a[2].tobytes() == b[2].tobytes()
    assert np.array_equal(a[3], b[3])


def _keeps(h, w, seed):
    yy, xx = np.mgrid[0:h, 0:w]
    corners = np.zeros((h, w), np.uint8)
    corners[[0, 0, -1, -1], [0, -1, 0, -1]] = 1
    cut = np.ones((h, w), np.uint8)
    cut[h // 2] = 0
    return {
        "corners": corners,
        "checker": ((yy + xx) & 1).astype(np.uint8),
        "stripes3": ((((xx + 2) // 3) & 1) == 0).astype(np.uint8),     # width-3 stripes with an edge at x = 63 | 64
        "cut": cut,
        "zero": np.zeros((h, w), np.uint8),
        "bernoulli": (np.random.default_rng(seed).random((h, w)) < 0.5).astype(np.uint8),
    }


def test_stripes_edge_at_64():
    k = _keeps(18, 72, 0)["stripes3"]
    assert k[0, 63] != k[0, 64] and k[0, 61:64].tolist() == [k[0, 63]] * 3 and k[0, 60] != k[0, 61]


# ------------------------------------------------------------------------------------------------------------------ 1. defaults
@pytest.mark.parametrize("h,w", [(68, 120), (45, 80)])
def test_defaults_are_the_parents_bits(ctx, h, w):
    b = 12
    rng = np.random.default_rng(h)
    frames, table = _frames(rng, 4 * b, h, w), _own_frames_table(b)
    m = W.blob_like(3)
    base = BlobNetInfer(ctx, m, h, w, max_batch=b).filter_frames(frames, table, 1, MAXB, True, True)
    assert base[1].sum() > 0
    net = BlobNetInfer(ctx, m, h, w, max_batch=b)              # a fresh load: the call was never made on it
    net.set_post(0, logit_thresh=0.0, keep=None)
    _eq_runs(net.filter_frames(frames, table, 1, MAXB, True, True), base)
    keep = _keeps(h, w, 1)["checker"]
    net.set_post(0, logit_thresh=0.7, keep=keep)
    changed = net.filter_frames(frames, table, 1, MAXB, True, True)
    assert changed[2].tobytes() != base[2].tobytes()           # (the non-default setting did something)
    assert np.array_equal(changed[2], _expect(base[3], 0.7, keep))
    net.reset_post(0)
    assert net.post(0) == (0.0, None)
    _eq_runs(net.filter_frames(frames, table, 1, MAXB, True, True), base)


# ------------------------------------------------------------------------------------------------------------------ 2. every tail form
GEOMS = [(16, 16), (18, 72), (20, 28), (45, 80), (68, 120)]
SWITCHES = ["mfma", "tail_band_tiles", "tail_skip_tensor", "dec_separate", "wave_cap", "infer"]
ALONE, ROWS, BANDS = BlobNetInfer.TAIL_ALONE, BlobNetInfer.TAIL_ROWS, BlobNetInfer.TAIL_BANDS     # BANDS + 2 * WV + PART


def _tail_form(h, w, switch):
    """The table of the module docstring."""
    if switch == "infer":
        return ALONE
    wv = 0 if switch == "wave_cap" or w % 8 else 1
    if switch == "tail_skip_tensor":
        return BANDS + 2 * wv
    if switch in ("mfma", "dec_separate") and wv and (h, w) != (16, 16):
        return ROWS
    return BANDS + 2 * wv + 1


def _settings(h, w, top):
    ks = _keeps(h, w, h * w)
    out = [(0.0, ks[name]) for name in ("corners", "checker", "stripes3", "cut", "zero", "bernoulli")]
    out += [(-1.5, None), (LOG4, None), (top + 1.0, None), (-1.5, ks["bernoulli"]), (LOG4, ks["cut"])]
    return out


@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("h,w", GEOMS)
def test_every_tail_form(ctx, h, w, switch):
    b = 6
    rng = np.random.default_rng(h * 1000 + w)
    frames, table = _frames(rng, 4 * b, h, w), _own_frames_table(b)
    stack = _stack_of(frames, table)
    m = W.random_init(h + w, fg_bias=0.2)
    cc = BboxCc(ctx, 1, MAXB)

    def load():
        net = BlobNetInfer(ctx, m, h, w, max_batch=b)
        if switch in ("tail_band_tiles", "tail_skip_tensor", "dec_separate"):
            net.set_impl(switch)
        return net

    def run(net):
        if switch == "infer":
            lg, mk = net.infer(stack)
            return None, None, mk, lg
        return net.filter_frames(frames, table, 1, MAXB, True, True)

    try:
        if switch == "wave_cap":
            cc.set_wave_cap(-1)
        base = run(load())                                        # a ctx that never had settings
        logits = base[3]
        default_mask = (logits > 0).astype(np.uint8)
        assert np.array_equal(base[2], default_mask)
        assert 0 < default_mask.mean() < 1                          # both classes occur: thresholds and keep maps can move the mask
        net = load()
        ctx.profile(True)
        for thr, keep in _settings(h, w, float(logits.max())):
            want = _expect(logits, thr, keep)
            empty = (keep is not None and not keep.any()) or thr > logits.max()
            assert not np.array_equal(want, default_mask)           # independent of the code under test
            assert bool(want.any()) != empty
            net.set_post(0, logit_thresh=thr, keep=keep)
            got = run(net)
            assert np.array_equal(got[2], want), (thr, None if keep is None else int(keep.sum()))
            assert np.array_equal(got[3], logits)                   # the logits output is not affected
            assert net.tail_form() == _tail_form(h, w, switch), (net.tail_form(), _tail_form(h, w, switch))
            if switch != "infer":
                rc = _eq_boxes(got[0], got[1], want)
                assert (rc.sum() == 0) == empty
        ctx.sync()
        names = ctx.profile_read()
        if switch == "infer":
            assert "dec3_final_mfma" in names and "dec3_bboxcc_fused" not in names
        else:
            assert "dec3_bboxcc_fused" in names and "dec3_final_mfma" not in names
            assert not any(n.startswith("bboxcc") for n in names)   # bboxcc ran inside the tail's launch
    finally:
        ctx.profile(False)
        cc.set_wave_cap(0)


# ------------------------------------------------------------------------------------------------------------------ 3. mixed batch
@pytest.fixture(scope="module")
def models():
    return [W.random_init(11, fg_bias=-0.1), W.random_init(22, fg_bias=0.3), W.blob_like(7), W.random_init(33, fg_bias=0.1)]


def _four_settings(h, w):
    """model 0: defaults, 1: keep only, 2: threshold only, 3: both."""
    ks = _keeps(h, w, 5)
    return [(0.0, None), (0.0, ks["stripes3"]), (float(LOG4), None), (-1.5, ks["bernoulli"])]


def _apply(net, settings, models_of=None):
    for k, (thr, keep) in enumerate(settings):
        if thr != 0.0 or keep is not None:
            net.set_post(k if models_of is None else models_of, logit_thresh=thr, keep=keep)


def _shared_frames_table(rng, b, n_streams=4):
    """Stacks of one stream (= one model) share carrier frames; stacks of all streams interleaved."""
    per = [b // n_streams + (1 if s < b % n_streams else 0) for s in range(n_streams)]
    rows, ids, base = [], [], 0
    for s, n in enumerate(per):
        for i in range(n):
            rows.append([base + i + 3, base + i + 2, base + i + 1, base + i])
            ids.append(s)
        base += n + 3
    order = rng.permutation(b)
    return np.array(rows, np.int32)[order], np.array(ids, np.uint8)[order], base


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("h,w", [(68, 120), (45, 80)])
def test_mixed_batch(ctx, models, h, w, shared, lanes):
    b = 40
    rng = np.random.default_rng(h + 7 * shared)
    if shared:
        table, ids, nf = _shared_frames_table(rng, b)
    else:
        table, nf = _own_frames_table(b), 4 * b
        ids = rng.permutation(np.arange(b) % 4).astype(np.uint8)
    frames = _frames(rng, nf, h, w)
    settings = _four_settings(h, w)
    old = ctx.lanes()
    ctx.set_lanes(lanes)
    try:
        net = BlobNetInfer(ctx, models, h, w, max_batch=b)
        _apply(net, settings)
        got = net.filter_frames(frames, table, 1, MAXB, True, True, model_ids=ids)
        assert net.tail_form() == ROWS                               # the row form's MS + POST instantiation
        for k in range(4):
            sel = ids == k
            thr, keep = settings[k]
            want = _expect(got[3][sel], thr, keep)
            assert np.array_equal(got[2][sel], want), k
            if k:
                assert not np.array_equal(want, (got[3][sel] > 0).astype(np.uint8)) and want.any()
            _eq_boxes(got[0][sel], got[1][sel], want)
            one = BlobNetInfer(ctx, models[k], h, w, max_batch=b)      # that model alone with that model's settings
            _apply(one, [settings[k]], models_of=0)
            r = one.filter_frames(frames, table, 1, MAXB, True, True)
            _eq_runs(tuple(x[sel] for x in got), tuple(x[sel] for x in r))
    finally:
        ctx.set_lanes(old)


# ------------------------------------------------------------------------------------------------------------------ 4. frames > workgroups
@pytest.mark.parametrize("h,w", [(16, 16), (16, 24)])
def test_more_frames_than_workgroups(ctx, models, h, w):
    """(16, 16) runs dec3cc_mfma<1, 1>, (16, 24) the row form: a workgroup of either takes several frames of different models."""
    b = 2 * ctx.info()["num_cu"] + 3
    rng = np.random.default_rng(4)
    frames, table = _frames(rng, 4 * b, h, w), _own_frames_table(b)
    ids = (np.arange(b) % 4).astype(np.uint8)
    ks = _keeps(h, w, 9)
    settings = [(0.0, ks["checker"]), (0.0, ks["stripes3"]), (-1.5, ks["cut"]), (0.5, ks["bernoulli"])]
    net = BlobNetInfer(ctx, models, h, w, max_batch=b)
    _apply(net, settings)
    got = net.filter_frames(frames, table, 1, MAXB, True, True, model_ids=ids)
    assert net.tail_form() == _tail_form(h, w, "mfma") == (ROWS if w == 24 else BANDS + 3)
    plain = BlobNetInfer(ctx, models, h, w, max_batch=b).filter_frames(frames, table, 1, MAXB, True, True, model_ids=ids)
    assert np.array_equal(got[3], plain[3])
    for k in range(4):
        sel = ids == k
        want = _expect(got[3][sel], *settings[k])
        assert want.any() and not np.array_equal(want, plain[2][sel])
        assert np.array_equal(got[2][sel], want), k
        _eq_boxes(got[0][sel], got[1][sel], want)


# ------------------------------------------------------------------------------------------------------------------ 5. pipe
@pytest.mark.parametrize("packed", [False, True])
def test_pipe(ctx, models, packed):
    h, w, b = 45, 80, 24
    rng = np.random.default_rng(31 + packed)
    table = _own_frames_table(b)
    settings = _four_settings(h, w)
    old = ctx.lanes()
    ctx.set_lanes(2)
    try:
        net = BlobNetInfer(ctx, models, h, w, max_batch=b)
        _apply(net, settings)
        pipe = FilterPipe(net, max_batch=b, max_frames=4 * b, max_boxes=MAXB, n_slots=2, want_mask=True, packed=packed)
        batches = []
        try:
            for _ in range(2):                                       # two rounds of two slots in flight
                pending = []
                for _ in range(2):
                    slot, fr, idx = pipe.acquire()
                    frames = _frames(rng, 4 * b, h, w)
                    ids = rng.integers(0, 4, b).astype(np.uint8)
                    fr[:4 * b] = pack_frames(frames) if packed else frames
                    idx[:b] = table
                    pipe.model_ids(slot)[:b] = ids
                    pipe.submit(slot, 4 * b, b, 1)
                    pending.append((slot, frames, ids))
                for slot, frames, ids in pending:
                    counts, offsets, boxes, mask = pipe.collect(slot)
                    batches.append((frames, ids, counts.copy(), offsets.copy(), boxes.copy(), mask.copy()))
        finally:
            pipe.close()
        for frames, ids, counts, offsets, boxes, mask in batches:
            rb, rc, rm, rl = net.filter_frames(frames, table, 1, MAXB, True, True, model_ids=ids)   # the direct _frames_m call
            assert not np.array_equal(rm, (rl > 0).astype(np.uint8)) and rc.sum() > 0
            for k in range(4):
                sel = ids == k
                assert np.array_equal(rm[sel], _expect(rl[sel], *settings[k]))
            assert np.array_equal(counts, rc) and np.array_equal(mask, rm)
            for j in range(b):
                n = min(int(rc[j]), MAXB)
                assert boxes[offsets[j]:offsets[j] + n].tobytes() == rb[j, :n].tobytes()
    finally:
        ctx.set_lanes(old)


# ------------------------------------------------------------------------------------------------------------------ 6. lifecycle, errors
def test_set_post_drains_the_lanes(ctx):
    """A batch on each of three lanes, set_post, three more: the first three have the old settings, the later ones the new."""
    h, w, b = 45, 80, 32
    rng = np.random.default_rng(77)
    m = W.random_init(5, fg_bias=0.2)
    table = _own_frames_table(b)
    frames = [_frames(rng, 4 * b, h, w) for _ in range(3)]
    ks = _keeps(h, w, 3)
    old_set, new_set = (0.0, ks["checker"]), (float(LOG4), ks["cut"])
    old = ctx.lanes()
    ctx.set_lanes(3)
    bufs = []
    try:
        net = BlobNetInfer(ctx, m, h, w, max_batch=b)
        d_fr = []
        for f in frames:
            d = ctx.malloc(f.nbytes)
            bufs.append(d)
            ctx.h2d(d, f)
            d_fr.append(d)

        def submit(i):
            d = [ctx.malloc(b * MAXB * L.BOX_DTYPE.itemsize), ctx.malloc(b * 4), ctx.malloc(b * h * w), ctx.malloc(b * h * w * 4)]
            bufs.extend(d)
            net.filter_frames_device(d_fr[i], 4 * b, table, b, 1, d[0], d[1], MAXB, d_mask=d[2], d_logits=d[3])
            return d

        def fetch(d):
            out = (np.empty((b, MAXB), L.BOX_DTYPE), np.empty(b, np.int32), np.empty((b, h, w), np.uint8), np.empty((b, h, w), np.float32))
            for a, p in zip(out, d):
                ctx.d2h(a, p)
            return out

        net.set_post(0, logit_thresh=old_set[0], keep=old_set[1])
        first = [submit(i) for i in range(3)]                          # nothing synchronised in between
        net.set_post(0, logit_thresh=new_set[0], keep=new_set[1])
        later = [submit(i) for i in range(3)]
        ctx.sync()
        for handles, (thr, keep) in ((first, old_set), (later, new_set)):
            for d in handles:
                boxes, counts, mask, logits = fetch(d)
                want = _expect(logits, thr, keep)
                assert want.any() and not np.array_equal(want, (logits > 0).astype(np.uint8))
                assert np.array_equal(mask, want)
                _eq_boxes(boxes, counts, want)
        a, c = _expect(fetch(first[0])[3], *old_set), _expect(fetch(later[0])[3], *new_set)
        assert not np.array_equal(a, c)                                 # (the two settings tell the batches apart)
    finally:
        ctx.sync()
        for d in bufs:
            ctx.free(d)
        ctx.set_lanes(old)


def test_get_post_round_trip_and_reload(ctx, models):
    h, w, b = 20, 28, 4
    net = BlobNetInfer(ctx, models[:3], h, w, max_batch=b)
    for k in range(3):
        assert net.post(k) == (0.0, None)
    keep = (np.random.default_rng(2).integers(0, 4, (h, w)) * 60).astype(np.uint8)     # values 0, 60, 120, 180
    net.set_post(1, logit_thresh=float(LOG4), keep=keep)
    lib = L.lib()
    raw = L.BlobNetPost(-0.25, keep.ctypes.data)                     # the C entry itself normalises non-zero bytes to 1
    assert lib.covahip_blobnet_set_post(ctx.handle, 2, C.byref(raw)) == 0
    thr, got = net.post(1)
    assert thr == float(LOG4) and got.dtype == np.uint8 and np.array_equal(got, (keep != 0).astype(np.uint8))
    thr, got = net.post(2)
    assert thr == -0.25 and np.array_equal(got, (keep != 0).astype(np.uint8)) and set(np.unique(got)) <= {0, 1}
    assert net.post(0) == (0.0, None)
    t, has = C.c_float(), C.c_int()
    ones = np.zeros((h, w), np.uint8)
    assert lib.covahip_blobnet_get_post(ctx.handle, 0, C.byref(t), ones.ctypes.data, C.byref(has)) == 0
    assert has.value == 0 and ones.all()
    assert lib.covahip_blobnet_get_post(ctx.handle, 1, None, None, None) == 0
    net.set_post(1, prob_thresh=0.8)                                 # a call replaces the model's settings as a whole
    assert net.post(1) == (float(LOG4), None)
    net = BlobNetInfer(ctx, models[:3], h, w, max_batch=b)           # reloading resets every model
    for k in range(3):
        assert net.post(k) == (0.0, None)
    net = BlobNetInfer(ctx, models[0], h, w, max_batch=b)
    net.set_post(0, logit_thresh=1.0)
    net = BlobNetInfer(ctx, models[0], h, w, max_batch=b)            # covahip_blobnet_load as well
    assert net.post(0) == (0.0, None)


def test_errors_leave_the_settings_alone(ctx, models):
    h, w, b = 20, 28, 6
    lib = L.lib()
    rng = np.random.default_rng(8)
    frames, table = _frames(rng, 4 * b, h, w), _own_frames_table(b)
    net = BlobNetInfer(ctx, models[:2], h, w, max_batch=b)
    keep = _keeps(h, w, 1)["checker"]
    net.set_post(1, logit_thresh=-1.5, keep=keep)
    ids = np.ones(b, np.uint8)
    before = net.filter_frames(frames, table, 1, MAXB, True, True, model_ids=ids)
    assert np.array_equal(before[2], _expect(before[3], -1.5, keep)) and before[1].sum() > 0
    assert not np.array_equal(before[2], (before[3] > 0).astype(np.uint8))
    zero = np.zeros((h, w), np.uint8)
    for model, thr in ((2, 0.5), (-1, 0.5), (1, float("nan")), (1, float("inf")), (1, float("-inf"))):
        post = L.BlobNetPost(thr, zero.ctypes.data)
        assert lib.covahip_blobnet_set_post(ctx.handle, model, C.byref(post)) == 1, (model, thr)
    assert lib.covahip_blobnet_set_post(ctx.handle, 2, None) == 1
    t = C.c_float()
    assert lib.covahip_blobnet_get_post(ctx.handle, 2, C.byref(t), None, None) == 1
    thr, got = net.post(1)
    assert thr == -1.5 and np.array_equal(got, keep)
    _eq_runs(net.filter_frames(frames, table, 1, MAXB, True, True, model_ids=ids), before)
    # no model loaded: a failed load leaves the ctx without one
    blob = W.to_bytes(models[0])
    ptrs, sizes = (C.c_char_p * 1)(blob), (C.c_size_t * 1)(len(blob) - 4)
    assert lib.covahip_blobnet_load_set(ctx.handle, 1, ptrs, sizes, h, w, 4, b) == 6
    post = L.BlobNetPost(0.5, None)
    assert lib.covahip_blobnet_set_post(ctx.handle, 0, C.byref(post)) == 4
    assert lib.covahip_blobnet_get_post(ctx.handle, 0, C.byref(t), None, None) == 4


# ------------------------------------------------------------------------------------------------------------------ 7. the caller's mask pointer
PAD, FILL = 64, 0xAA
MASK_CASES = ["frames_68x120", "frames_45x80_post", "frames_68x120_two_models_post", "stack_45x80", "stack_68x120_post", "infer_20x28"]


@pytest.mark.parametrize("case", MASK_CASES)
def test_mask_pointer_of_any_alignment(ctx, models, case):
    """d_mask 0, 1, 2 and 3 bytes into a buffer of 0xAA.  Off a 4-byte boundary the row form of the fused tail (whose ballots leave
    as words) is turned away for the band form, and the band form and the unfused last block store the mask byte by byte.  Mask,
    counts and boxes are the aligned call's, and no byte outside [d_mask, d_mask + batch * h * w) is written."""
    kind, geom = case.split("_")[:2]
    h, w = (int(v) for v in geom.split("x"))
    b = 5
    rng = np.random.default_rng(len(case) + h)
    frames, table = _frames(rng, 4 * b, h, w), _own_frames_table(b)
    src = frames if kind == "frames" else _stack_of(frames, table)
    two = "two_models" in case
    ids = np.array([0, 1, 1, 0, 1], np.uint8) if two else None
    net = BlobNetInfer(ctx, [models[1], models[3]] if two else models[1], h, w, max_batch=b)
    if "post" in case:
        net.set_post(1 if two else 0, logit_thresh=0.25, keep=_keeps(h, w, 6)["stripes3"])
    nbytes = b * h * w
    d_src, d_boxes, d_counts = ctx.malloc(src.nbytes), ctx.malloc(b * MAXB * L.BOX_DTYPE.itemsize), ctx.malloc(b * 4)
    d_buf = ctx.malloc(PAD + nbytes + PAD)
    runs = []
    try:
        assert d_buf % 16 == 0
        ctx.h2d(d_src, src)
        for shift in (0, 1, 2, 3):
            ctx.h2d(d_buf, np.full(PAD + nbytes + PAD, FILL, np.uint8))
            ctx.h2d(d_boxes, np.zeros(b * MAXB, L.BOX_DTYPE))
            ctx.h2d(d_counts, np.full(b, -1, np.int32))
            d_mask = d_buf + PAD + shift
            if kind == "frames":
                net.filter_frames_device(d_src, 4 * b, table, b, 1, d_boxes, d_counts, MAXB, d_mask=d_mask, model_ids=ids)
            elif kind == "stack":
                net.filter_device(d_src, b, 1, d_boxes, d_counts, MAXB, d_mask=d_mask, model_ids=ids)
            else:
                net.infer_device(d_src, b, None, d_mask, model_ids=ids)
            ctx.sync()
            form = net.tail_form()
            buf, boxes, counts = np.empty(PAD + nbytes + PAD, np.uint8), np.empty((b, MAXB), L.BOX_DTYPE), np.empty(b, np.int32)
            ctx.d2h(buf, d_buf)
            ctx.d2h(boxes, d_boxes)
            ctx.d2h(counts, d_counts)
            runs.append((shift, form, buf, boxes, counts))
    finally:
        ctx.sync()
        for d in (d_src, d_boxes, d_counts, d_buf):
            ctx.free(d)
    _, form0, buf0, boxes0, counts0 = runs[0]
    mask0 = buf0[PAD:PAD + nbytes].reshape(b, h, w)
    assert set(np.unique(mask0)) == {0, 1}                              # both classes, and every byte of the region was written
    if kind == "infer":
        assert form0 == ALONE
    else:
        assert form0 == ROWS and counts0.min() >= 0 and counts0.sum() > 0
        _eq_boxes(boxes0, counts0, mask0)
    for shift, form, buf, boxes, counts in runs:
        lo = PAD + shift
        assert (buf[:lo] == FILL).all() and (buf[lo + nbytes:] == FILL).all(), (shift, "a store outside the caller's mask")
        assert buf[lo:lo + nbytes].tobytes() == mask0.tobytes(), shift
        if kind == "infer":
            assert form == ALONE
            continue
        assert form == (ROWS if shift == 0 else BANDS + 3), (shift, form)   # dec3cc_mfma<WV = 1, PART = 1> where rows are turned away
        assert np.array_equal(counts, counts0), shift
        for i in range(b):
            n = min(int(counts0[i]), MAXB)
            assert boxes[i, :n].tobytes() == boxes0[i, :n].tobytes(), (shift, i)
