"""Model sets (covahip_blobnet_load_set + the _m forward entries): one ctx holds K models of one geometry and every stack of a
batch names its model.  The property checked throughout: a stack's result in a mixed batch equals, byte for byte (masks, counts,
boxes) and as floats (logits), the result of a ctx loaded with that stack's model alone running the same batch through the same
entry point, impl and lane count."""
import ctypes as C

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import weights as W
from cova_amd.elements import BlobNetInfer, pack_frames

pytestmark = pytest.mark.gpu

IMPLS = {1: "mfma", 4: "dec_separate", 5: "enc1_legacy", 6: "enc_general_tiles", 7: "enc23_separate", 8: "enc23_force",
         9: "tail_skip_tensor", 10: "tail_band_tiles"}


def _negated_gamma(flat: np.ndarray, level: int) -> np.ndarray:
    """A model whose encoder level `level` has some negative BN gammas (its allpos flag is false)."""
    t = W.unflatten(flat.copy())
    g = t[f"enc{level}.bn.gamma"]
    g[::3] = -np.abs(g[::3]) - 0.05
    return W.flatten(t)


@pytest.fixture(scope="module")
def models():
    """Four distinct models: two random, one blob-like, one with negative gammas at level 2 (so the set's allpos[2] is false
    while each of the other three models alone has it true)."""
    m0, m1, m2 = W.random_init(11, fg_bias=-0.5), W.random_init(22, fg_bias=0.3), W.blob_like(7)
    m3 = _negated_gamma(W.random_init(33, fg_bias=-0.2), 2)
    return [m0, m1, m2, m3]


def _frames(rng, n, h, w):
    f = np.zeros((n, h, w, 4), np.uint8)
    f[..., 0] = rng.integers(0, 8, (n, h, w))
    f[..., 1:3] = rng.integers(0, 9, (n, h, w, 2))
    return f


def _own_frames_table(batch):
    """Every stack has its own four carrier frames: any id per stack is legal."""
    return np.arange(batch * 4, dtype=np.int32).reshape(batch, 4)[:, ::-1].copy()


def _eq_boxes(boxes_a, counts_a, boxes_b, counts_b):
    """The boxes each stack reports (the slots behind its count hold nothing)."""
    assert np.array_equal(counts_a, counts_b)
    for i in range(len(counts_a)):
        n = min(int(counts_a[i]), boxes_a.shape[1])
        assert boxes_a[i, :n].tobytes() == boxes_b[i, :n].tobytes(), i


def _eq_logits(a, b):
    # equal as floats (a signed zero compares equal); NaNs never occur here
    assert np.array_equal(a, b), float(np.max(np.abs(a.astype(np.float64) - b)))


def _check_frames(ctx, models, ids, frames, table, h, w, impl=None, max_batch=None, max_boxes=64):
    b = table.shape[0]
    mb = max_batch or b
    net = BlobNetInfer(ctx, models, h, w, max_batch=mb)
    assert net.num_models == len(models)
    if impl:
        net.set_impl(IMPLS[impl])
    got = net.filter_frames(frames, table, 1, max_boxes=max_boxes, want_mask=True, want_logits=True, model_ids=ids)
    for k in sorted(set(ids.tolist())):
        ref_net = BlobNetInfer(ctx, models[k], h, w, max_batch=mb)
        if impl:
            ref_net.set_impl(IMPLS[impl])
        ref = ref_net.filter_frames(frames, table, 1, max_boxes=max_boxes, want_mask=True, want_logits=True)
        sel = ids == k
        _eq_boxes(got[0][sel], got[1][sel], ref[0][sel], ref[1][sel])
        assert np.array_equal(got[2][sel], ref[2][sel]), k                        # mask
        _eq_logits(got[3][sel], ref[3][sel])


@pytest.mark.parametrize("h,w", [(45, 80), (68, 120)])
def test_set_of_one_equals_load(ctx, h, w):
    m = W.blob_like(3)
    rng = np.random.default_rng(h)
    b = 24
    frames = _frames(rng, b + 3, h, w)
    stack = np.concatenate([frames[i:i + 4][::-1].reshape(4 * h, w, 4)[None] for i in range(b)])
    one = BlobNetInfer(ctx, m, h, w, max_batch=b)
    ref = (one.filter_full(stack, 1, 64, want_mask=True, want_logits=True), one.filter_frames(frames, None, 1, 64, True, True),
           one.infer(stack))
    s = BlobNetInfer(ctx, [m], h, w, max_batch=b)
    got = (s.filter_full(stack, 1, 64, want_mask=True, want_logits=True), s.filter_frames(frames, None, 1, 64, True, True),
           s.infer(stack))
    ids = np.zeros(b, np.uint8)
    got_ids = s.filter_frames(frames, None, 1, 64, True, True, model_ids=ids)
    for g, r in ((got[0], ref[0]), (got[1], ref[1]), (got_ids, ref[1])):
        _eq_boxes(g[0], g[1], r[0], r[1])
        assert g[2].tobytes() == r[2].tobytes() and g[3].tobytes() == r[3].tobytes()
    assert got[2][0].tobytes() == ref[2][0].tobytes() and got[2][1].tobytes() == ref[2][1].tobytes()


@pytest.mark.parametrize("h,w,b", [(45, 80, 40), (68, 120, 40), (67, 120, 24), (35, 60, 24), (135, 240, 6)])
def test_mixed_batch_equals_single_models_frames(ctx, models, h, w, b):
    rng = np.random.default_rng(h * w)
    ids = rng.integers(0, 4, b).astype(np.uint8)
    ids[:4] = [0, 1, 2, 3]
    _check_frames(ctx, models, ids, _frames(rng, 4 * b, h, w), _own_frames_table(b), h, w)


@pytest.mark.parametrize("impl", [1, 4, 5, 6, 7, 8, 9, 10])
@pytest.mark.parametrize("h,w", [(68, 120), (45, 80)])
def test_mixed_batch_every_impl(ctx, models, impl, h, w):
    rng = np.random.default_rng(impl * 7 + h)
    b = 36
    ids = rng.integers(0, 4, b).astype(np.uint8)
    _check_frames(ctx, models, ids, _frames(rng, 4 * b, h, w), _own_frames_table(b), h, w, impl=impl)


def test_mixed_batch_stacked_entries(ctx, models):
    """covahip_filter_forward_m and covahip_blobnet_forward_m (no bboxcc: the plain last decoder block)."""
    h, w, b = 45, 80, 30
    rng = np.random.default_rng(5)
    frames = _frames(rng, 4 * b, h, w)
    stack = frames.reshape(b, 4 * h, w, 4)
    ids = rng.integers(0, 4, b).astype(np.uint8)
    net = BlobNetInfer(ctx, models, h, w, max_batch=b)
    got_f = net.filter_full(stack, 1, 64, want_mask=True, want_logits=True, model_ids=ids)
    got_i = net.infer(stack, model_ids=ids)
    for k in range(4):
        one = BlobNetInfer(ctx, models[k], h, w, max_batch=b)
        ref_f = one.filter_full(stack, 1, 64, want_mask=True, want_logits=True)
        ref_i = one.infer(stack)
        sel = ids == k
        _eq_boxes(got_f[0][sel], got_f[1][sel], ref_f[0][sel], ref_f[1][sel])
        assert np.array_equal(got_f[2][sel], ref_f[2][sel])
        _eq_logits(got_f[3][sel], ref_f[3][sel])
        _eq_logits(got_i[0][sel], ref_i[0][sel])
        assert np.array_equal(got_i[1][sel], ref_i[1][sel])


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("b", [1, 255, 256, 257, 300])
def test_batch_sizes_streams(ctx, models, b, lanes):
    """Streams of carrier frames (each frame shared by up to four stacks of its stream's model), past the by-value table, on
    one lane and on three."""
    old = ctx.lanes() if callable(ctx.lanes) else ctx.lanes
    ctx.set_lanes(lanes)
    try:
        _batch_sizes_streams(ctx, models, b)
    finally:
        ctx.set_lanes(old)


def _batch_sizes_streams(ctx, models, b):
    h, w, mb = 45, 80, 300
    rng = np.random.default_rng(b)
    n_streams = 8
    per = [b // n_streams + (1 if s < b % n_streams else 0) for s in range(n_streams)]
    rows, ids, base = [], [], 0
    smodel = rng.integers(0, 4, n_streams)
    for s, n in enumerate(per):
        if n == 0:
            continue
        for i in range(n):
            rows.append([base + i + 3, base + i + 2, base + i + 1, base + i])
            ids.append(smodel[s])
        base += n + 3
    order = rng.permutation(len(rows))      # stacks of all streams interleaved, as a batching element produces them
    table = np.array(rows, np.int32)[order]
    ids = np.array(ids, np.uint8)[order]
    _check_frames(ctx, models, ids, _frames(rng, base, h, w), table, h, w, max_batch=mb)


@pytest.mark.parametrize("lanes", [1, 3])
def test_device_entries_lanes_and_id_cache(ctx, models, lanes):
    """Device-pointer calls on 1 and 3 lanes, unpacked and packed records; back-to-back calls with the SAME stack table and
    different ids (same lane with 1 lane, alternating lanes with 3) must not reuse stale ids."""
    h, w, b, mbx = 68, 120, 64, 64
    rng = np.random.default_rng(lanes)
    table = _own_frames_table(b)
    frames = _frames(rng, 4 * b, h, w)
    packed = pack_frames(frames)
    id_sets = [rng.integers(0, 4, b).astype(np.uint8) for _ in range(4)]
    old = ctx.lanes() if callable(ctx.lanes) else ctx.lanes
    ctx.set_lanes(lanes)
    bufs = []
    try:
        d_fr, d_pk = ctx.malloc(frames.nbytes), ctx.malloc(packed.nbytes)
        bufs += [d_fr, d_pk]
        ctx.h2d(d_fr, frames)
        ctx.h2d(d_pk, packed)

        def run(net, ids, pk):
            d_box, d_cnt = ctx.malloc(b * mbx * L.BOX_DTYPE.itemsize), ctx.malloc(b * 4)
            d_mask, d_log = ctx.malloc(b * h * w), ctx.malloc(b * h * w * 4)
            bufs.extend([d_box, d_cnt, d_mask, d_log])
            net.filter_frames_device(d_pk if pk else d_fr, 4 * b, table, b, 1, d_box, d_cnt, mbx, d_mask=d_mask, model_ids=ids,
                                     d_logits=d_log, packed=pk)
            return d_box, d_cnt, d_mask, d_log

        def fetch(d):
            d_box, d_cnt, d_mask, d_log = d
            box = np.empty((b, mbx), L.BOX_DTYPE); cnt = np.empty(b, np.int32)
            mask = np.empty((b, h, w), np.uint8); lg = np.empty((b, h, w), np.float32)
            ctx.d2h(box, d_box); ctx.d2h(cnt, d_cnt); ctx.d2h(mask, d_mask); ctx.d2h(lg, d_log)
            return box, cnt, mask, lg

        net = BlobNetInfer(ctx, models, h, w, max_batch=b)
        got = {}
        for pk in (False, True):
            handles = [run(net, ids, pk) for ids in id_sets]     # back to back, nothing synchronised in between
            ctx.sync()
            got[pk] = [fetch(d) for d in handles]
        for k in range(4):
            one = BlobNetInfer(ctx, models[k], h, w, max_batch=b)
            for pk in (False, True):
                d = run(one, None, pk)
                ctx.sync()
                ref = fetch(d)
                for ids, g in zip(id_sets, got[pk]):
                    sel = ids == k
                    _eq_boxes(g[0][sel], g[1][sel], ref[0][sel], ref[1][sel])
                    assert np.array_equal(g[2][sel], ref[2][sel]), (k, pk)
                    _eq_logits(g[3][sel], ref[3][sel])
    finally:
        ctx.sync()
        for d in bufs:
            ctx.free(d)
        ctx.set_lanes(old)


def test_all_positive_model_in_general_form(ctx, models):
    """A set whose allpos is false runs an all-positive model's stacks through the general (med3) pooling form: the results
    must equal that model alone (max form)."""
    h, w, b = 68, 120, 16
    rng = np.random.default_rng(9)
    ids = np.zeros(b, np.uint8)
    ids[::2] = 3                       # the negative-gamma model
    _check_frames(ctx, [models[2], models[0], models[1], models[3]], ids, _frames(rng, 4 * b, h, w), _own_frames_table(b), h, w)


def test_errors(ctx, models):
    lib = L.lib()
    h, w, b = 45, 80, 8
    rng = np.random.default_rng(1)
    frames = _frames(rng, b + 3, h, w)
    net = BlobNetInfer(ctx, models[:3], h, w, max_batch=b)
    n = C.c_int()
    assert lib.covahip_blobnet_num_models(ctx.handle, C.byref(n)) == 0 and n.value == 3
    boxes = np.zeros((b, 8), L.BOX_DTYPE); counts = np.zeros(b, np.int32)
    bad = np.zeros(b, np.uint8); bad[3] = 3                                   # id >= K
    assert lib.covahip_filter_forward_frames_m(ctx.handle, frames.ctypes.data, b + 3, None, bad.ctypes.data, b, 1,
                                               boxes.ctypes.data, counts.ctypes.data, 8, None, None, L.MEM_HOST) == 1
    stack = frames[:4][None].repeat(b, 0).reshape(b, 4 * h, w, 4)
    assert lib.covahip_filter_forward_m(ctx.handle, stack.ctypes.data, bad.ctypes.data, b, 1, boxes.ctypes.data,
                                        counts.ctypes.data, 8, None, None, L.MEM_HOST) == 1
    mask = np.zeros((b, h, w), np.uint8)
    assert lib.covahip_blobnet_forward_m(ctx.handle, stack.ctypes.data, bad.ctypes.data, b, None, mask.ctypes.data,
                                         L.MEM_HOST) == 1
    shared = np.zeros(b, np.uint8); shared[1] = 1                             # one stream in order: frames 1..4 shared by stacks 0, 1
    assert lib.covahip_filter_forward_frames_m(ctx.handle, frames.ctypes.data, b + 3, None, shared.ctypes.data, b, 1,
                                               boxes.ctypes.data, counts.ctypes.data, 8, None, None, L.MEM_HOST) == 1
    # the ctx still works after the rejected calls
    net.filter_frames(frames, None, 1, 8, model_ids=np.full(b, 2, np.uint8))
    blobs = [W.to_bytes(m) for m in models[:2]]
    ptrs = (C.c_char_p * 300)(*(blobs * 150))
    sizes = (C.c_size_t * 300)(*([len(blobs[0])] * 300))
    assert lib.covahip_blobnet_load_set(ctx.handle, 0, ptrs, sizes, h, w, 4, b) == 1
    assert lib.covahip_blobnet_load_set(ctx.handle, 257, ptrs, sizes, h, w, 4, b) == 1
    sizes_bad = (C.c_size_t * 3)(len(blobs[0]), len(blobs[0]) - 4, len(blobs[0]))
    ptrs3 = (C.c_char_p * 3)(blobs[0], blobs[1], blobs[0])
    assert lib.covahip_blobnet_load_set(ctx.handle, 3, ptrs3, sizes_bad, h, w, 4, b) == 6
    assert lib.covahip_blobnet_num_models(ctx.handle, C.byref(n)) == 4                 # no model left
    ids = np.zeros(b, np.uint8)
    assert lib.covahip_filter_forward_frames_m(ctx.handle, frames.ctypes.data, b + 3, None, ids.ctypes.data, b, 1,
                                               boxes.ctypes.data, counts.ctypes.data, 8, None, None, L.MEM_HOST) == 4
    assert lib.covahip_blobnet_forward_m(ctx.handle, stack.ctypes.data, ids.ctypes.data, b, None, mask.ctypes.data,
                                         L.MEM_HOST) == 4
    # K = 256 of one geometry loads
    sizes256 = (C.c_size_t * 300)(*([len(blobs[0])] * 300))
    assert lib.covahip_blobnet_load_set(ctx.handle, 256, ptrs, sizes256, h, w, 4, b) == 0
    assert lib.covahip_blobnet_num_models(ctx.handle, C.byref(n)) == 0 and n.value == 256
    ids255 = np.full(b, 255, np.uint8)
    assert lib.covahip_filter_forward_frames_m(ctx.handle, frames.ctypes.data, b + 3, None, ids255.ctypes.data, b, 1,
                                               boxes.ctypes.data, counts.ctypes.data, 8, None, None, L.MEM_HOST) == 0


@pytest.mark.parametrize("packed", [False, True])
def test_pipe_model_ids(ctx, models, packed):
    """FilterPipe with three slots: the slot's model id view is zeroed by acquire, filled in place, read by submit; ids change
    every batch."""
    from cova_amd.elements import FilterPipe
    h, w, b, mbx = 45, 80, 32, 256
    rng = np.random.default_rng(17 + packed)
    net = BlobNetInfer(ctx, models, h, w, max_batch=b)
    pipe = FilterPipe(net, max_batch=b, max_frames=4 * b, max_boxes=mbx, n_slots=3, want_mask=True, packed=packed)
    table = _own_frames_table(b)
    batches = []
    try:
        pending = []
        for i in range(6):
            slot, fr, idx = pipe.acquire()
            ids_view = pipe.model_ids(slot)
            assert ids_view.shape == (b,) and not ids_view.any()          # acquire zeroes it
            frames = _frames(rng, 4 * b, h, w)
            ids = rng.integers(0, 4, b).astype(np.uint8)
            fr[:4 * b] = pack_frames(frames) if packed else frames
            idx[:b] = table
            ids_view[:] = ids
            pipe.submit(slot, 4 * b, b, 1)
            pending.append((slot, frames, ids))
            if len(pending) == 3 or i == 5:
                for slot_, frames_, ids_ in pending:
                    counts, offsets, boxes, mask = pipe.collect(slot_)
                    batches.append((frames_, ids_, counts.copy(), offsets.copy(), boxes.copy(), mask.copy()))
                pending = []
    finally:
        pipe.close()
    for k in range(4):
        one = BlobNetInfer(ctx, models[k], h, w, max_batch=b)
        for frames, ids, counts, offsets, boxes, mask in batches:
            rb, rc, rm, _ = one.filter_frames(frames, table, 1, max_boxes=mbx, want_mask=True)
            for j in np.flatnonzero(ids == k):
                assert counts[j] == rc[j]
                n = min(int(rc[j]), mbx)
                assert boxes[offsets[j]:offsets[j] + n].tobytes() == rb[j, :n].tobytes()
                assert np.array_equal(mask[j], rm[j])
