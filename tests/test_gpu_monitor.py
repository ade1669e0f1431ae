"""covahip_monitor_* on the GPU against its numpy restatement (tests/monitor_ref.py): every table must be EQUAL -- all quantities are
integer counts.  Stand-alone the monitor is fed seeded masks with the boxes covahip_bboxcc finds in them; attached it must equal
the restatement on what the filter calls themselves returned."""
import ctypes as C
import json

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import calibrate as cal
from cova_amd import monitor as mon
from cova_amd import synth
from cova_amd import weights as W
from cova_amd.elements import BboxCc, BlobNetInfer, Context, FilterPipe, tfrecord_example
from tests.monitor_ref import FIELDS, empty, monitor_ref, same
from tests.sweep_ref import smooth_field

pytestmark = pytest.mark.gpu

# (1,1), (5,7): under a wave, the byte path; (17,16): one word over a 256-macroblock tile; (16,64): exact tile multiples;
# (67,120): not a multiple of the tile
GRIDS = [(1, 1), (5, 7), (17, 16), (16, 64), (67, 120)]
NS = [1, 37, 257, 300]
N_MAX = 300
MAX_BOXES = 4                                             # small, so that some frames truncate
INVALID, NOT_LOADED, UNSUPPORTED = 1, 4, 5


def _ids(kind, n):
    """-> (model ids u8 [n] or None, n_models)"""
    if kind == "one":
        return None, 1
    if kind == "robin3":
        return (np.arange(n) % 3).astype(np.uint8), 3
    if kind == "blocks":                                  # blocks of unequal length: 1, 2, 3, ... samples of models 0, 1, 2, 0, ...
        ids, k = [], 0
        while len(ids) < n:
            ids += [k % 3] * (k + 1)
            k += 1
        return np.asarray(ids[:n], np.uint8), 3
    if kind == "shuffle5":                                # model 3 absent: its rows stay zero
        rng = np.random.default_rng(n)
        return rng.choice(np.asarray([0, 1, 2, 4], np.uint8), n), 5
    if kind == "ends256":
        return np.where(np.arange(n) % 3 == 1, 255, 0).astype(np.uint8), 256
    raise KeyError(kind)


ID_KINDS = ["one", "robin3", "blocks", "shuffle5", "ends256"]


@pytest.fixture(scope="module")
def cases(ctx):
    """Per grid: 300 seeded masks with values in {0, 1, 255}, the last macroblock forced on and the first forced off in every
    sample, and their boxes and counts from covahip_bboxcc with max_boxes = 4; per (grid, n, ids) the restatement."""
    data, refs = {}, {}

    def get(h, w, n, kind):
        if (h, w) not in data:
            rng = np.random.default_rng(77 * h + w)
            field = smooth_field(rng, N_MAX, h, w, 3)
            mask = (field > 0.8).astype(np.uint8) * rng.choice(np.asarray([1, 255], np.uint8), field.shape)
            mask[:, h - 1, w - 1] = rng.choice(np.asarray([1, 255], np.uint8), N_MAX)
            if h * w > 1:
                mask[:, 0, 0] = 0
            boxes, counts = BboxCc(ctx, 1, MAX_BOXES).regionprops(mask)
            # a grid of 256 macroblocks or more has frames that truncate at 4 boxes; (1,1) and (5,7) cannot hold that many blobs
            if h * w >= 256:
                assert (counts > MAX_BOXES).any(), counts.max()
            assert counts.min() >= 1
            data[(h, w)] = (mask, counts, boxes)
        mask, counts, boxes = data[(h, w)]
        ids, n_models = _ids(kind, n)
        if (h, w, n, kind) not in refs:
            refs[(h, w, n, kind)] = monitor_ref(mask[:n], counts[:n], boxes[:n], ids, MAX_BOXES, n_models)
        return mask[:n], counts[:n], boxes[:n], ids, n_models, refs[(h, w, n, kind)]
    return get


class _OnDevice:
    """mask (at `shift` bytes past an allocation one byte longer), counts and boxes of a case on the device."""

    def __init__(self, ctx, mask, counts, boxes, shift=0):
        self.ctx = ctx
        self.ptrs = [ctx.malloc(mask.nbytes + 1), ctx.malloc(counts.nbytes), ctx.malloc(max(1, boxes.nbytes))]
        self.mask = self.ptrs[0] + shift
        ctx.h2d(self.mask, mask)
        ctx.h2d(self.ptrs[1], counts)
        ctx.h2d(self.ptrs[2], boxes)
        self.hw, self.row = mask.shape[1] * mask.shape[2], boxes.shape[1] * boxes.dtype.itemsize

    def at(self, s0):
        return self.mask + s0 * self.hw, self.ptrs[1] + 4 * s0, self.ptrs[2] + s0 * self.row

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)


# ------------------------------------------------------------------------------------------------------------------ 1. stand-alone add
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("h,w", GRIDS)
def test_add_equals_the_restatement(ctx, cases, h, w, n):
    mask, counts, boxes = cases(h, w, n, "one")[:3]
    dev = [_OnDevice(ctx, mask, counts, boxes, shift) for shift in (0, 1)]     # shift 1: the unaligned path
    try:
        for kind in ID_KINDS:
            _, _, _, ids, n_models, want = cases(h, w, n, kind)
            assert want["frames"].sum() == n and want["area_hist"].sum() == np.minimum(counts, MAX_BOXES).sum()
            if kind == "shuffle5":
                assert want["frames"][3] == 0 and (n < 37 or (want["frames"][[0, 1, 2, 4]] > 0).all())
            got = []
            mon.begin(ctx, h, w, n_models, MAX_BOXES)
            mon.add(ctx, mask, counts, boxes, ids)
            got.append(mon.read(ctx, reset=True))
            for d in dev:
                mon.add_device(ctx, *d.at(0), n, ids)
                got.append(mon.read(ctx, reset=True))
            mon.end(ctx)
            for g in got:
                same(g, want)
                assert g["batches_seen"] == 0 and g["batches_counted"] == 0        # stand-alone: no filter batch
            if kind == "one":
                assert got[0]["fire"][0, h - 1, w - 1] == n and (h * w == 1 or got[0]["fire"][0, 0, 0] == 0)
    finally:
        for d in dev:
            d.free()


@pytest.mark.parametrize("h,w", GRIDS)
def test_a_slice_longer_than_255_samples_is_exact(ctx, cases, h, w):
    """The automatic slices stay short at these sizes (enough workgroups for every CU); with the developer's slice length the 300
    samples of one model are ONE slice, so the kernel's packed byte counters must spill: the always-on macroblock reads 300."""
    n = 300
    mask, counts, boxes = cases(h, w, n, "one")[:3]
    dev = [_OnDevice(ctx, mask, counts, boxes, shift) for shift in (0, 1)]
    try:
        mon.set_slice(ctx, 512)
        for kind in ("one", "blocks", "ends256"):
            _, _, _, ids, n_models, want = cases(h, w, n, kind)
            mon.begin(ctx, h, w, n_models, MAX_BOXES)
            for d in dev:
                mon.add_device(ctx, *d.at(0), n, ids)
                got = mon.read(ctx, reset=True)
                same(got, want)
                if kind == "one":
                    assert got["fire"][0, h - 1, w - 1] == 300
            mon.end(ctx)
    finally:
        mon.set_slice(ctx, 0)
        for d in dev:
            d.free()


def test_an_add_longer_than_one_launch(ctx, cases):
    """A stand-alone add takes 16384 samples per launch: 16384 + 5 samples are two launches from device memory, and from host
    memory two staged pieces, the second from the arrays' offsets (model ids included)."""
    h, w, n = 5, 7, 16384 + 5
    m300, c300, b300 = cases(h, w, N_MAX, "one")[:3]
    pick = np.random.default_rng(3).integers(0, N_MAX, n)
    mask, counts, boxes = np.ascontiguousarray(m300[pick]), np.ascontiguousarray(c300[pick]), np.ascontiguousarray(b300[pick])
    dev = _OnDevice(ctx, mask, counts, boxes)
    try:
        for kind in ("one", "robin3"):
            ids, n_models = _ids(kind, n)
            want = monitor_ref(mask, counts, boxes, ids, MAX_BOXES, n_models)
            tail = monitor_ref(mask[16384:], counts[16384:], boxes[16384:], None if ids is None else ids[16384:], MAX_BOXES, n_models)
            assert tail["fire"].any() and tail["area_hist"].any()          # the second launch's share is visible in the tables
            mon.begin(ctx, h, w, n_models, MAX_BOXES)
            mon.add_device(ctx, *dev.at(0), n, ids)
            same(mon.read(ctx, reset=True), want)
            mon.add(ctx, mask, counts, boxes, ids)
            same(mon.read(ctx, reset=True), want)
            mon.end(ctx)
    finally:
        dev.free()


# ------------------------------------------------------------------------------------------------------------------ 2. additivity, state
def test_additivity_and_state(ctx, cases):
    h, w, n = 17, 16, 257
    mask, counts, boxes, ids, n_models, want = cases(h, w, n, "blocks")

    def split(*parts):
        s0 = 0
        for c in parts:
            sl = slice(s0, s0 + c)
            mon.add(ctx, mask[sl], counts[sl], boxes[sl], ids[sl])
            s0 += c
        assert s0 == n

    mon.begin(ctx, h, w, n_models, MAX_BOXES)
    split(257)
    a = mon.read(ctx)
    same(a, want)
    same(mon.read(ctx), want)                                            # read(reset=False) twice returns the same
    same(mon.read(ctx, reset=True), want)
    zero = empty(n_models, h, w)
    same(mon.read(ctx), zero)                                            # ... and after a reset zeros
    split(1, 256)
    same(mon.read(ctx, reset=True), want)
    split(100, 0, 100, 57)                                               # n == 0 changes nothing
    same(mon.read(ctx), want)
    mon.add_device(ctx, None, None, None, 0)                             # null pointers are fine with n == 0
    same(mon.read(ctx), want)
    mon.begin(ctx, h, w, n_models, MAX_BOXES)                            # begin while open starts from zero
    same(mon.read(ctx), zero)
    split(257)
    mon.end(ctx)
    # a second bracket at another grid and n_models
    m2, c2, b2, i2, nm2, want2 = cases(5, 7, 37, "shuffle5")
    mon.begin(ctx, 5, 7, nm2, MAX_BOXES)
    mon.add(ctx, m2, c2, b2, i2)
    same(mon.read(ctx), want2)
    mon.end(ctx)
    with pytest.raises(L.CovahipError):
        mon.read(ctx)
    # max_boxes = 0: no boxes array, every frame with a box truncates
    mon.begin(ctx, h, w, n_models, 0)
    mon.add(ctx, mask, counts, None, ids)
    same(mon.read(ctx), monitor_ref(mask, counts, None, ids, 0, n_models))
    mon.end(ctx)


# ------------------------------------------------------------------------------------------------------------------ 3. attached
def _models(n_models):
    return [W.blob_like()] + [W.random_init(4321 + k) for k in range(1, n_models)]


def _serving_net(ctx, h, w, b, n_models):
    """A set of 1 or 3 models; model 1 with a threshold, a rectangle removed and an area threshold of its own; on the 16 x 16 grid
    the last model with a threshold so low that its mask is all ones."""
    net = BlobNetInfer(ctx, _models(n_models) if n_models > 1 else W.blob_like(), h, w, max_batch=b)
    keep = np.ones((h, w), np.uint8)
    keep[2:7, 3:11] = 0
    if n_models > 1:
        net.set_post(1, logit_thresh=-0.5, keep=keep)
        net.set_area(1, 3)
    if (h, w) == (16, 16):
        net.set_post(n_models - 1, logit_thresh=-1e30)
    return net, keep


def _call_ids(k, b, n_models):
    if n_models == 1:
        return None
    if k % 2 == 0:
        return (np.arange(b) % n_models).astype(np.uint8)                       # round robin
    return np.minimum(np.arange(b) * n_models // b, n_models - 1).astype(np.uint8)[::-1].copy()   # blocks, last model first


def _same_boxes(a, b, counts):
    """The boxes a call wrote: the first min(count, max_boxes) of every frame (what lies behind them is not the call's)."""
    return all(a[i, :min(int(c), a.shape[1])].tobytes() == b[i, :min(int(c), b.shape[1])].tobytes() for i, c in enumerate(counts))


def _as_frames(stack, h):
    """A stacked batch as carrier frames no two stacks share: row block t of stack i is frame 4 i + t."""
    b = stack.shape[0]
    return np.ascontiguousarray(stack.reshape(b * 4, h, stack.shape[2], 4)), np.arange(4 * b, dtype=np.int32).reshape(b, 4)


@pytest.mark.parametrize("h,w,b", [(16, 16, 8), (45, 80, 40)])
@pytest.mark.parametrize("n_models", [1, 3])
def test_attached_equals_the_calls_own_outputs(ctx, h, w, b, n_models):
    max_boxes, cc = 16, 1
    net, keep = _serving_net(ctx, h, w, b, n_models)
    stacks = [synth.stacked_batch(b - (k == 4), h, w, seed=50 + k, streams=2) for k in range(6)]      # call 4: a partial batch
    ids = [_call_ids(k, s.shape[0], n_models) for k, s in enumerate(stacks)]
    net.monitor_begin()
    want = empty(n_models, h, w)
    outs = []
    for s, i in zip(stacks, ids):
        boxes, counts, mask, _ = net.filter_full(s, cc, max_boxes, want_mask=True, model_ids=i)
        outs.append((boxes, counts, mask))
        monitor_ref(mask, counts, boxes, i, max_boxes, n_models, into=want)
    got = net.monitor_read(reset=True)
    assert got["batches_seen"] == 6 and got["batches_counted"] == 6
    same(got, want)
    # the comparison is not between empty tables, the served mask is what is counted, and some frame truncates
    assert want["boxes"].sum() > 0 and want["area_hist"].sum() > 0 and want["frames"].sum() == 6 * b - 1
    if n_models > 1:
        assert not want["fire"][1][keep == 0].any() and want["fire"][1].any()
        assert (h, w) == (16, 16) or want["truncated"].sum() > 0
    if (h, w) == (16, 16):
        assert (want["fire"][n_models - 1] == want["frames"][n_models - 1]).all() and want["frames"][n_models - 1] > 0

    # the same batches as carrier frames, and with the mask left in the lane's scratch
    for s, i, (boxes, counts, mask) in zip(stacks, ids, outs):
        fr, index = _as_frames(s, h)
        fb, fc, fm, _ = net.filter_frames(fr, index, cc, max_boxes, want_mask=True, model_ids=i)
        assert np.array_equal(fc, counts) and np.array_equal(fm, mask) and _same_boxes(fb, boxes, counts)
    same(net.monitor_read(reset=True), want)
    for s, i in zip(stacks, ids):
        net.filter_full(s, cc, max_boxes, want_mask=False, model_ids=i)
    same(net.monitor_read(reset=True), want)

    # device pointers back to back, on one lane and on three
    d_in = []
    for s in stacks:
        d_in.append(ctx.malloc(s.nbytes))
        ctx.h2d(d_in[-1], s)
    d_out = [(ctx.malloc(b * max_boxes * 20), ctx.malloc(b * 4), ctx.malloc(b * h * w)) for _ in stacks]
    try:
        for lanes in (1, 3):
            ctx.set_lanes(lanes)
            for rnd in range(2):
                for k, s in enumerate(stacks):
                    # the second round leaves the mask to the lane's scratch
                    net.filter_device(d_in[k], s.shape[0], cc, d_out[k][0], d_out[k][1], max_boxes, d_out[k][2] if rnd == 0 else None, ids[k])
            got = net.monitor_read(reset=True)
            assert got["batches_seen"] == 12 and got["batches_counted"] == 12
            same(got, {k: 2 * want[k] for k in FIELDS})
    finally:
        ctx.set_lanes(1)
        for p in d_in + [p for o in d_out for p in o]:
            ctx.free(p)
    net.monitor_end()


def test_attached_table_from_the_device_for_a_mixed_batch_above_256(ctx):
    """A mixed batch of more than 256 stacks takes its order and slices from the lane's device table instead of the kernel
    arguments; a repeated batch does not upload it again, a changed one does."""
    h, w, b, max_boxes = 16, 16, 300, 8
    net = BlobNetInfer(ctx, _models(3), h, w, max_batch=b)
    stack = synth.stacked_batch(b, h, w, seed=9, streams=3)
    id_a, id_b = (np.arange(b) % 3).astype(np.uint8), (np.arange(b) // 100).astype(np.uint8)
    net.monitor_begin()
    want = empty(3, h, w)
    for i in (id_a, id_a, id_b, id_a):
        boxes, counts, mask, _ = net.filter_full(stack, 1, max_boxes, want_mask=True, model_ids=i)
        monitor_ref(mask, counts, boxes, i, max_boxes, 3, into=want)
    assert want["boxes"].sum() > 0
    same(net.monitor_read(), want)
    net.monitor_end()


# ------------------------------------------------------------------------------------------------------------------ 4. every
def test_every_third_batch(ctx):
    h, w, b, max_boxes = 16, 16, 8, 16
    net = BlobNetInfer(ctx, _models(3), h, w, max_batch=b)
    net.monitor_begin(every=3)
    want = empty(3, h, w)
    for k in range(7):
        ids = _call_ids(k, b, 3)
        boxes, counts, mask, _ = net.filter_full(synth.stacked_batch(b, h, w, seed=70 + k, streams=2), 1, max_boxes, want_mask=True, model_ids=ids)
        if k % 3 == 0:
            monitor_ref(mask, counts, boxes, ids, max_boxes, 3, into=want)
        net.infer(synth.stacked_batch(2, h, w, seed=1), model_ids=[0, 1])      # makes no boxes: neither seen nor counted
    got = net.monitor_read()
    assert got["batches_seen"] == 7 and got["batches_counted"] == 3 and want["frames"].sum() == 3 * b and want["boxes"].sum() > 0
    same(got, want)
    # a failed call and an empty one are neither seen nor counted
    lib = L.lib()
    bad = np.full(b, 3, np.uint8)
    st = synth.stacked_batch(b, h, w, seed=70, streams=2)
    boxes, counts = np.zeros((b, max_boxes), L.BOX_DTYPE), np.zeros(b, np.int32)
    assert lib.covahip_filter_forward_m(ctx.handle, st.ctypes.data, bad.ctypes.data, b, 1, boxes.ctypes.data, counts.ctypes.data, max_boxes,
                                        None, None, L.MEM_HOST) == INVALID
    assert lib.covahip_filter_forward_m(ctx.handle, st.ctypes.data, None, 0, 1, boxes.ctypes.data, counts.ctypes.data, max_boxes,
                                        None, None, L.MEM_HOST) == 0
    again = net.monitor_read()
    assert again["batches_seen"] == 7 and again["batches_counted"] == 3
    same(again, want)
    net.monitor_end()


# ------------------------------------------------------------------------------------------------------------------ 5. the pipe
def test_the_pipe_is_counted(ctx):
    h, w, b, max_boxes = 45, 80, 24, 32
    ctx.set_lanes(2)
    pipe = None
    try:
        net, _ = _serving_net(ctx, h, w, b, 3)
        pipe = FilterPipe(net, max_batch=b, max_frames=4 * b, max_boxes=max_boxes, n_slots=3, want_mask=True)
        net.monitor_begin()
        want = empty(3, h, w)
        in_flight = []

        def collect():
            slot, ids = in_flight.pop(0)
            c, o, bx, m = pipe.collect(slot)
            rows = np.zeros((len(c), max_boxes), L.BOX_DTYPE)
            for i in range(len(c)):
                rows[i, :o[i + 1] - o[i]] = bx[o[i]:o[i + 1]]
            monitor_ref(m, c, rows, ids, max_boxes, 3, into=want)

        for k in range(5):
            fr, index = _as_frames(synth.stacked_batch(b, h, w, seed=90 + k, streams=2), h)
            acq = pipe.acquire()
            while acq is None:
                collect()
                acq = pipe.acquire()
            slot, pf, pi = acq
            ids = _call_ids(k, b, 3)
            pf[:fr.shape[0]] = fr
            pi[:b] = index
            pipe.model_ids(slot)[:b] = ids
            pipe.submit(slot, fr.shape[0], b, 2)
            in_flight.append((slot, ids))
        while in_flight:
            collect()
        got = net.monitor_read()
        assert got["batches_seen"] == 5 and got["batches_counted"] == 5 and want["boxes"].sum() > 0 and want["frames"].sum() == 5 * b
        same(got, want)
        net.monitor_end()
    finally:
        if pipe is not None:
            pipe.close()
        ctx.set_lanes(1)


# ------------------------------------------------------------------------------------------------------------------ 6. serving is not disturbed
def test_serving_is_not_disturbed_and_a_closed_monitor_is_free(ctx):
    h, w, b, max_boxes = 45, 80, 8, 64
    stacks = [synth.stacked_batch(b, h, w, seed=20 + k, streams=2) for k in range(3)]
    ids = [_call_ids(k, b, 3) for k in range(3)]

    def serve(c, net):
        c.profile(True)
        outs = [net.filter_full(s, 2, max_boxes, True, True, model_ids=i) for s, i in zip(stacks, ids)]
        prof = {k: v[1] for k, v in c.profile_read().items()}
        c.profile(False)
        return outs, prof

    fresh = Context(0)                                                    # a ctx that never opens a monitor
    try:
        base_outs, base_prof = serve(fresh, _serving_net(fresh, h, w, b, 3)[0])
    finally:
        fresh.close()
    assert "monitor_count" not in base_prof and sum(o[1].sum() for o in base_outs) > 0
    net, _ = _serving_net(ctx, h, w, b, 3)
    never, prof_never = serve(ctx, net)
    net.monitor_begin(every=2)
    during, prof_during = serve(ctx, net)
    counted = net.monitor_read()["batches_counted"]
    mon.begin(ctx, h, w, 3, max_boxes)                                    # a stand-alone monitor takes no part in a filter step
    alone, prof_alone = serve(ctx, net)
    net.monitor_end()
    after, prof_after = serve(ctx, net)
    for outs in (never, during, alone, after):
        for o, want in zip(outs, base_outs):
            assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(o[1:], want[1:])) and _same_boxes(o[0], want[0], want[1])
    assert prof_never == base_prof and prof_after == base_prof and prof_alone == base_prof
    assert counted == 2 and prof_during.pop("monitor_count") == counted and prof_during == base_prof


# ------------------------------------------------------------------------------------------------------------------ 7. lifecycle, errors
def test_lifecycle_and_errors(ctx, cases):
    lib = L.lib()
    h, w, n = 5, 7, 37
    mask, counts, boxes, ids, n_models, want = cases(h, w, n, "robin3")
    begin, add, read, end = lib.covahip_monitor_begin, lib.covahip_monitor_add, lib.covahip_monitor_read, lib.covahip_monitor_end

    def cfg(hh=h, ww=w, m=n_models, mb=MAX_BOXES, attach=0, every=1):
        return C.byref(L.MonitorCfg(hh, ww, m, mb, attach, every))

    def do_add(m=mask.ctypes.data, c=counts.ctypes.data, b=boxes.ctypes.data, i=ids.ctypes.data, k=n, kind=L.MEM_HOST, handle=ctx.handle):
        return add(handle, m, c, b, i, k, kind)

    nulls = (None,) * 8
    # add, read and end without begin (whatever earlier tests left open is closed first)
    begin(ctx.handle, cfg())
    assert end(ctx.handle) == 0
    assert do_add() == INVALID and read(ctx.handle, 0, *nulls) == INVALID and end(ctx.handle) == INVALID
    assert begin(ctx.handle, cfg()) == 0 and do_add() == 0
    # every refused call below leaves the open monitor's counts as they are
    assert begin(None, cfg()) == INVALID and begin(ctx.handle, None) == INVALID
    for bad in (dict(hh=0), dict(ww=0), dict(hh=-1), dict(m=0), dict(m=257), dict(mb=-1), dict(attach=2), dict(attach=-1)):
        assert begin(ctx.handle, cfg(**bad)) == INVALID, bad
    assert begin(ctx.handle, cfg(hh=4097, ww=4096)) == UNSUPPORTED
    assert do_add(handle=None) == INVALID and read(None, 0, *nulls) == INVALID and end(None) == INVALID
    assert do_add(k=-1) == INVALID and do_add(m=None) == INVALID and do_add(c=None) == INVALID and do_add(b=None) == INVALID
    assert do_add(kind=2) == INVALID and do_add(kind=-1) == INVALID
    bad_ids = ids.copy()
    bad_ids[-1] = n_models
    assert do_add(i=bad_ids.ctypes.data) == INVALID
    assert do_add(m=None, c=None, b=None, i=None, k=0) == 0               # n == 0 is OK and changes nothing
    ctx._monitor_shape = (h, w, n_models)                                 # (opened through the raw call: what mon.read sizes its arrays by)
    same(mon.read(ctx), want)
    # read takes NULL outputs
    seen = C.c_int64(-1)
    assert read(ctx.handle, 0, None, None, None, None, None, None, C.byref(seen), None) == 0 and seen.value == 0

    # attached: needs a loaded model of the cfg's grid and n_models
    net = BlobNetInfer(ctx, _models(3), 16, 16, max_batch=4)
    same(mon.read(ctx), want)                                            # a stand-alone monitor survives a load
    for bad in (dict(hh=16, ww=17), dict(hh=17, ww=16), dict(hh=16, ww=16, m=2), dict(hh=16, ww=16, m=3, every=0)):
        assert begin(ctx.handle, cfg(attach=1, **bad)) == INVALID, bad
    same(mon.read(ctx), want)                                            # the failed begins left it open
    net.monitor_begin()
    assert do_add() == INVALID                                            # add on an attached monitor
    stack = synth.stacked_batch(4, 16, 16, seed=3)
    net.filter(stack, 1, 8)
    assert net.monitor_read()["batches_seen"] == 1
    net2 = BlobNetInfer(ctx, W.blob_like(), 16, 16, max_batch=4)          # a load closes an attached monitor
    with pytest.raises(L.CovahipError):
        net2.monitor_read()
    assert end(ctx.handle) == INVALID
    net2.filter(stack, 1, 8)                                              # ... and serving goes on without one
    net2.monitor_begin()
    junk = b"x" * 100                                                     # a set load drops the model before it finds the blob bad
    assert lib.covahip_blobnet_load_set(ctx.handle, 1, (C.c_char_p * 1)(junk), (C.c_size_t * 1)(len(junk)), 16, 16, 4, 4) == 6
    assert begin(ctx.handle, cfg(hh=16, ww=16, m=1, attach=1)) == NOT_LOADED
    assert end(ctx.handle) == INVALID                                     # the monitor went with the model


# ------------------------------------------------------------------------------------------------------------------ 8. command line
def test_command_line(ctx, tmp_path, capsys):
    from cova_amd import train
    h, w, n = 45, 80, 40
    block = np.zeros((h, w), bool)
    block[2:5, 66:78] = True
    flats = [W.blob_like(), W.blob_like(seed=8)]
    cams = []
    for k in range(2):
        fr = synth.carrier_frames(4 * n, h, w, seed=31 + k, n_objects=5)
        fr[..., 3] = 0
        if k == 1:                                                        # a block that moves in every frame
            fr[:, block, 0] = 1
            fr[:, block, 1:3] = 6
        cams.append(fr)
    # precondition: camera 1's model fires on the block in every sample, camera 0's in none
    net = BlobNetInfer(ctx, flats, h, w, max_batch=n)
    own = [net.infer(train.slide(cams[k], np.zeros((4 * n, h, w), np.uint8))[0], model_ids=np.full(n, k, np.uint8))[1] for k in range(2)]
    assert (own[1][:, block] != 0).all() and not own[0][:, block].all(axis=0).any()

    # the restatement on a separate pass over the command line's batches, served as the sidecars say: cc-threshold 2
    posts = [({"logit_thresh": 0.0, "keep": None}, 2)] * 2
    net = BlobNetInfer(ctx, flats, h, w, max_batch=16)
    for k in range(2):
        cal.apply_post(net, k, posts[k])
    want = empty(2, h, w)
    n_batches = 0
    for fr, index, ids in mon.mixed_batches(cams, 16):
        boxes, counts, mask, _ = net.filter_frames(fr, index, 30, 256, want_mask=True, model_ids=ids)
        monitor_ref(mask, counts, boxes, ids, 256, 2, into=want)
        n_batches += 1
    assert n_batches == 5 and want["frames"].tolist() == [n, n] and (want["fire"][1][block] == n).all() and want["boxes"][1] >= n
    hot = 2 * want["fire"][1] >= n
    assert not (2 * want["fire"][0] >= n).any()
    rects = cal.rects_from_keep((~hot).astype(np.uint8))

    paths = {"rec": [], "wts": [], "post": []}
    for k in range(2):
        rec, wts, post = tmp_path / f"cam{k}.tfrecord", tmp_path / f"cam{k}.cvhw", tmp_path / f"cam{k}.json"
        with open(rec, "wb") as f:
            for i in range(0, 4 * n, 8):
                f.write(tfrecord_example(cams[k][i:i + 8], np.zeros((8, h, w), np.uint8), gop=8))
        wts.write_bytes(W.to_bytes(flats[k]))
        # camera 0's baseline is what it does; camera 1's a tenth of what the block produces
        pred = int(want["boxes"][0]) if k == 0 else max(1, int(want["boxes"][1]) // 10)
        post.write_text(json.dumps({"format": "covahip-post-1", "logit_thresh": 0.0, "cc_threshold": 2, "ignore_rects": [],
                                    "scores": {"pred": pred, "samples": n}}))
        for key, p in zip(("rec", "wts", "post"), (rec, wts, post)):
            paths[key].append(str(p))
    npz = tmp_path / "snapshot.npz"
    assert mon.main(paths["rec"] + ["--weights"] + paths["wts"] + ["--post"] + paths["post"] +
                    ["--h-mb", str(h), "--w-mb", str(w), "--batch", "16", "--persistent", "0.5", "--out", str(npz)]) == 0
    lines = capsys.readouterr().out.splitlines()
    cam = {k: next(i for i, ln in enumerate(lines) if ln.startswith(f"camera {k} ")) for k in range(2)}
    assert "no drift" in lines[cam[0]] and "DRIFT" not in lines[cam[0]]
    assert "DRIFT" in lines[cam[1]] and "no drift" not in lines[cam[1]]
    hints = [ln.strip() for ln in lines if "pad-ignore-rects" in ln]
    assert hints == ["persistent: " + mon.ignore_hint(1, rects)] and lines.index("  " + hints[0]) > cam[1]
    assert "batches seen 5, counted 5" in lines[0]
    saved = np.load(npz)
    same({k: saved[k] for k in FIELDS}, want)
    assert int(saved["batches_seen"]) == 5 and int(saved["batches_counted"]) == 5
