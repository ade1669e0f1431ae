"""covahip_monitor_set_inputs / add_inputs / read_inputs and the attached input counting on the GPU against the numpy restatement
(tests/input_stats_ref.py): every table must be EQUAL -- all quantities are integer counts -- whatever the input form, the
pointer alignment, the slicing, the flush cadence and the lanes."""
import ctypes as C

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import monitor as mon
from cova_amd import synth
from cova_amd import weights as W
from cova_amd.elements import BlobNetInfer, Context, FilterPipe, pack_frames, tfrecord_example
from tests import input_stats_ref as ref
from tests import monitor_ref

pytestmark = pytest.mark.gpu

# (5,7): under a wave, h * w % 4 != 0; (16,16): exactly one 256-macroblock tile; (17,16): one row over it; (45,80): 3600, two
# 2048-macroblock workgroup tiles, the second partial; (67,120): 8040, the last lanes' eight macroblocks end inside the frame
GRIDS = [(5, 7), (16, 16), (17, 16), (45, 80), (67, 120)]
NS = [1, 3, 64, 300]                                     # 300 passes a 255-sample spill
CONTENTS = ["zero", "const", "uniform", "sparse", "special"]
INVALID = 1


def make_frames(kind, f, h, w, seed):
    """u8 [f][h][w][4]; byte 3 is random throughout and must be ignored."""
    rng = np.random.default_rng(seed)
    fr = np.zeros((f, h, w, 4), np.uint8)
    if kind == "const":                                  # every record the same non-zero value
        fr[..., 0], fr[..., 1] = 1, 2
    elif kind == "uniform":                              # bytes 0 .. 255: the clip at 6, class 7 -> 6
        fr = rng.integers(0, 256, fr.shape).astype(np.uint8)
    elif kind in ("sparse", "special"):                  # 2 % non-zero
        hit = rng.random((f, h, w)) < 0.02
        fr[hit, :3] = rng.integers(0, 256, (int(hit.sum()), 3)).astype(np.uint8)
    if kind == "special" and f > 3:
        hw = h * w
        at = 3                                           # the first counted frame of a NULL stack_index

        def put(frame):
            nonlocal at
            if at < f:
                fr[at] = frame
            at += 1
        intra_f = np.zeros((h, w, 4), np.uint8)          # one frame all intra among inter frames
        intra_f[..., 0] = rng.choice(np.asarray([5, 6, 7, 200], np.uint8), (h, w))
        intra_f[..., 1] = rng.integers(0, 3, (h, w))
        put(intra_f)
        for count in [1] + [1 << k for k in (1, 2, 5, 8, 11, 12) if (1 << k) <= hw] + [hw - 1, hw]:
            one = np.zeros((hw, 4), np.uint8)            # exactly `count` moving macroblocks; classes alone do not move
            one[:, 0] = rng.integers(0, 5, hw)
            one[rng.choice(hw, count, replace=False), 1 + int(rng.integers(0, 2))] = rng.integers(1, 256)
            put(one.reshape(h, w, 4))
    fr[..., 3] = rng.integers(0, 256, fr.shape[:3])
    return fr


def stacked_of(frames, n):
    """u8 [n][4h][w][4]: row block t of stack b is frame b + 3 - t, so row block 0 is the frame a NULL stack_index counts."""
    return np.ascontiguousarray(np.concatenate([frames[3 - t:3 - t + n] for t in range(4)], axis=1))


class Dev:
    """An array on the device, `shift` bytes past an allocation."""

    def __init__(self, ctx, arr, shift=0):
        self.ctx, self.base = ctx, ctx.malloc(arr.nbytes + 16)
        self.ptr = self.base + shift
        ctx.h2d(self.ptr, arr)

    def free(self):
        self.ctx.free(self.base)


def read_reset(ctx):
    return mon.read_inputs(ctx, reset=True)


# ------------------------------------------------------------------------------------------------------------------ 1. stand-alone
@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("h,w", GRIDS)
def test_three_forms_equal_the_restatement(ctx, h, w, kind):
    frames = make_frames(kind, max(NS) + 3, h, w, 11 * h + w)
    r_all = ref.records(frames, False)
    packed = pack_frames(frames)
    assert np.array_equal(ref.records(packed, True), r_all)
    d_frames, d_packed = Dev(ctx, frames), Dev(ctx, packed)
    mon.begin(ctx, h, w, 1, 0)
    mon.set_inputs(ctx, True)
    assert mon.get_inputs(ctx)
    try:
        for n in NS:
            want = ref.input_ref(r_all[3:3 + n])
            assert want["in_frames"][0] == n and want["hist"].sum() == n * h * w
            stk = stacked_of(frames, n)
            d_stk = Dev(ctx, stk)
            try:
                got = []
                mon.add_inputs(ctx, stk, "stacked")
                got.append(read_reset(ctx))
                mon.add_inputs(ctx, frames[:n + 3], "frames")
                got.append(read_reset(ctx))
                mon.add_inputs(ctx, packed[:n + 3], "packed")
                got.append(read_reset(ctx))
                mon.add_inputs_device(ctx, d_stk.ptr, "stacked", 0, None, n)
                got.append(read_reset(ctx))
                mon.add_inputs_device(ctx, d_frames.ptr, "frames", n + 3, None, n)
                got.append(read_reset(ctx))
                mon.add_inputs_device(ctx, d_packed.ptr, "packed", n + 3, None, n)
                got.append(read_reset(ctx))
            finally:
                d_stk.free()
            for g in got:
                ref.same(g, want)
            if kind == "zero":
                assert want["still_frames"][0] == n and want["hist"][0, 0] == n * h * w and want["move_hist"][0, 0] == n
            if kind == "const":
                assert want["hist"][0, 1 | 2 << 3] == n * h * w and (want["moving"][0] == n).all()
            if kind == "special" and n >= 64:
                assert want["intra_frames"][0] == 1 and want["move_hist"][0, 1] >= 1 and (want["move_hist"][0, 2:4] >= 1).all()
                assert want["move_hist"][0, ref.move_bin(h * w)] >= 1
    finally:
        mon.end(ctx)
        d_frames.free()
        d_packed.free()


@pytest.mark.parametrize("h,w", GRIDS)
def test_device_pointers_off_their_boundaries(ctx, h, w):
    n = 67
    frames = make_frames("uniform", n + 3, h, w, 5 * h + w)
    packed = pack_frames(frames)
    stk = stacked_of(frames, n)
    want = ref.input_ref(ref.records(frames[3:], False))
    mon.begin(ctx, h, w, 1, 0)
    mon.set_inputs(ctx, True)
    try:
        for shift in (1, 2, 4, 8):
            devs = [Dev(ctx, a, shift) for a in (stk, frames, packed)]
            try:
                for d, form, nf in zip(devs, ("stacked", "frames", "packed"), (0, n + 3, n + 3)):
                    mon.add_inputs_device(ctx, d.ptr, form, nf, None, n)
                    ref.same(read_reset(ctx), want)
            finally:
                for d in devs:
                    d.free()
    finally:
        mon.end(ctx)


@pytest.mark.parametrize("h,w", [(5, 7), (45, 80)])
def test_packed_data_with_high_bits_and_fields_of_seven(ctx, h, w):
    n = 40
    rng = np.random.default_rng(h)
    packed = rng.integers(0, 65536, (n + 3, h, w)).astype(np.uint16)
    assert (packed >> 9).any() and ((packed & 7) == 7).any() and ((packed >> 3 & 7) == 7).any()
    want = ref.input_ref(ref.records(packed[3:], True))
    assert want["hist"][0][(np.arange(512) & 7) == 7].sum() > 0
    d = Dev(ctx, packed)
    mon.begin(ctx, h, w, 1, 0)
    mon.set_inputs(ctx, True)
    try:
        mon.add_inputs_device(ctx, d.ptr, "packed", n + 3, None, n)
        ref.same(read_reset(ctx), want)
        mon.add_inputs(ctx, packed, "packed")
        ref.same(read_reset(ctx), want)
    finally:
        mon.end(ctx)
        d.free()


@pytest.mark.parametrize("h,w", [(17, 16), (45, 80)])
def test_a_stack_index_that_names_a_frame_twice(ctx, h, w):
    f = 40
    frames = make_frames("special", f, h, w, 3)
    packed = pack_frames(frames)
    r_all = ref.records(frames, False)
    rng = np.random.default_rng(8)
    for batch in (31, 300):                                # 300: the frame list no longer travels in the kernel arguments
        index = rng.integers(0, f, (batch, 4)).astype(np.int32)
        index[1, 0] = index[0, 0] = 3                       # the all-intra frame is the newest slice of two stacks
        index[2, 0], index[2, 1:] = 0, 3                    # ... and an older slice of a third: not counted there
        want = ref.input_ref(r_all[ref.counted_frames("frames", batch, index)])
        assert ref.all_intra(r_all[3]) and want["intra_frames"][0] == 2 + int((index[3:, 0] == 3).sum())
        devs = [Dev(ctx, frames), Dev(ctx, packed)]
        mon.begin(ctx, h, w, 1, 0)
        mon.set_inputs(ctx, True)
        try:
            mon.add_inputs(ctx, frames, "frames", index)
            ref.same(read_reset(ctx), want)
            mon.add_inputs(ctx, packed, "packed", index)
            ref.same(read_reset(ctx), want)
            mon.add_inputs_device(ctx, devs[0].ptr, "frames", f, index, batch)
            ref.same(read_reset(ctx), want)
            mon.add_inputs_device(ctx, devs[1].ptr, "packed", f, index, batch)
            ref.same(read_reset(ctx), want)
        finally:
            mon.end(ctx)
            for d in devs:
                d.free()


# ------------------------------------------------------------------------------------------------------------------ 2. models and tables
@pytest.mark.parametrize("h,w", [(16, 16), (45, 80)])
def test_models_and_tables(ctx, h, w):
    frames = make_frames("special", 303, h, w, 21)
    packed = pack_frames(frames)
    r_all = ref.records(frames, False)
    d = Dev(ctx, packed)
    try:
        for n in (64, 256, 300):                           # 300: the order / slice table comes from the device
            ids = np.random.default_rng(n).permutation(np.arange(n) % 3).astype(np.uint8)
            ids = np.asarray([2, 0, 1], np.uint8)[ids]      # permuted ids
            want = ref.input_ref(r_all[3:3 + n], ids, 3)
            assert (want["in_frames"] > 0).all() and want["in_frames"].sum() == n
            mon.begin(ctx, h, w, 3, 0)
            mon.set_inputs(ctx, True)
            mon.add_inputs_device(ctx, d.ptr, "packed", n + 3, None, n, ids)
            ref.same(read_reset(ctx), want)
            mon.add_inputs(ctx, frames[:n + 3], "frames", None, ids)
            ref.same(read_reset(ctx), want)
            mon.add_inputs(ctx, stacked_of(frames, n), "stacked", None, ids)
            ref.same(read_reset(ctx), want)
            one = np.full(n, 2, np.uint8)                   # a one-model batch
            mon.add_inputs_device(ctx, d.ptr, "packed", n + 3, None, n, one)
            got = read_reset(ctx)
            ref.same(got, ref.input_ref(r_all[3:3 + n], one, 3))
            assert got["in_frames"].tolist() == [0, 0, n]
            bad = ids.copy()
            bad[-1] = 3                                     # an id >= n_models is refused, and nothing is counted
            with pytest.raises(L.CovahipError):
                mon.add_inputs_device(ctx, d.ptr, "packed", n + 3, None, n, bad)
            ref.same(mon.read_inputs(ctx), ref.empty(3, h, w))
            mon.end(ctx)
    finally:
        d.free()


# ------------------------------------------------------------------------------------------------------------------ 3. additivity, cadence
@pytest.mark.parametrize("h,w", [(5, 7), (45, 80)])
def test_additivity_and_flush_cadence(ctx, h, w):
    n = 300
    frames = make_frames("uniform", n + 3, h, w, 2)
    frames[100:200] = make_frames("special", 100, h, w, 4)
    packed = pack_frames(frames)
    ids = (np.arange(n) % 3).astype(np.uint8)
    r_all = ref.records(frames, False)
    want = {"one": ref.input_ref(r_all[3:]), "three": ref.input_ref(r_all[3:], ids, 3)}
    d = Dev(ctx, packed)
    try:
        mon.begin(ctx, h, w, 3, 0)
        mon.set_inputs(ctx, True)
        mon.add_inputs_device(ctx, d.ptr, "packed", n + 3, None, n, ids)
        ref.same(mon.read_inputs(ctx), want["three"])
        ref.same(read_reset(ctx), want["three"])             # read(reset=False) twice returns the same
        s0 = 0
        for c in (1, 44, 0, 255):                            # one call of 300 equals calls of 1, 44 and 255; 0 changes nothing
            mon.add_inputs_device(ctx, d.ptr + 2 * s0 * h * w, "packed", c + 3, None, c, ids[s0:s0 + c])
            s0 += c
        ref.same(read_reset(ctx), want["three"])
        # the developer's slice length and flush cadence: one slice of 300 (or short ones) flushed every 1, 255, 256 samples
        try:
            for slice_len in (0, 7, 512):
                mon.set_slice(ctx, slice_len)
                for flush in (1, 255, 256, 0):
                    mon.set_input_flush(ctx, flush)
                    mon.add_inputs_device(ctx, d.ptr, "packed", n + 3, None, n, ids)
                    ref.same(read_reset(ctx), want["three"])
                    mon.add_inputs_device(ctx, d.ptr, "packed", n + 3, None, n, None)
                    got = read_reset(ctx)
                    ref.same({k: v[:1] for k, v in got.items()}, want["one"])
        finally:
            mon.set_slice(ctx, 0)
            mon.set_input_flush(ctx, 0)
        assert L.lib().covahip_dev_input_flush(ctx.handle, -1) == INVALID and L.lib().covahip_dev_input_flush(None, 1) == INVALID
        mon.end(ctx)
    finally:
        d.free()


# ------------------------------------------------------------------------------------------------------------------ 4. attached
def _as_frames(stack, h):
    """A stacked batch as carrier frames no two stacks share: row block t of stack i is frame 4 i + t."""
    b = stack.shape[0]
    return np.ascontiguousarray(stack.reshape(b * 4, h, stack.shape[2], 4)), np.arange(4 * b, dtype=np.int32).reshape(b, 4)


def _net(ctx, h, w, b, n_models):
    flats = [W.blob_like()] + [W.random_init(4321 + k) for k in range(1, n_models)]
    return BlobNetInfer(ctx, flats if n_models > 1 else flats[0], h, w, max_batch=b)


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("h,w,b,n_models", [(16, 16, 8, 2), (45, 80, 12, 1)])
def test_attached_counts_the_inputs_of_the_counted_batches(ctx, h, w, b, n_models, every, lanes):
    max_boxes = 16
    net = _net(ctx, h, w, b, n_models)
    stacks = [synth.stacked_batch(b - (k == 2), h, w, seed=60 + k, streams=2) for k in range(4)]   # call 2: a partial batch
    ids = [None if n_models == 1 else ((np.arange(s.shape[0]) + k) % n_models).astype(np.uint8) for k, s in enumerate(stacks)]
    as_fr = [_as_frames(s, h) for s in stacks]
    devs = [Dev(ctx, stacks[0]), Dev(ctx, as_fr[1][0]), Dev(ctx, pack_frames(as_fr[2][0]))]
    outs = (ctx.malloc(b * max_boxes * 20), ctx.malloc(b * 4))

    def call(k):
        n = stacks[k].shape[0]
        if k == 0:
            net.filter_device(devs[0].ptr, n, 1, outs[0], outs[1], max_boxes, None, ids[k])
        elif k == 1:
            net.filter_frames_device(devs[1].ptr, 4 * n, as_fr[1][1], n, 1, outs[0], outs[1], max_boxes, None, ids[k])
        elif k == 2:
            net.filter_frames_device(devs[2].ptr, 4 * n, as_fr[2][1], n, 1, outs[0], outs[1], max_boxes, None, ids[k], packed=True)
        else:                                               # host pointers: stacked and carrier frames in turn
            net.filter_frames(as_fr[3][0], as_fr[3][1], 1, max_boxes, model_ids=ids[k])

    order = [0, 1, 2, 3, 1, 2, 3, 0, 0]                      # with every = 2 each entry is counted at least once
    try:
        ctx.set_lanes(lanes)
        net.monitor_begin(every=every)
        net.monitor_set_inputs(True)
        want = ref.empty(n_models, h, w)
        for i, k in enumerate(order):
            call(k)
            if i % every == 0:
                ref.input_ref(ref.records(ref.newest(stacks[k], h), False), ids[k], n_models, into=want)
        got = net.monitor_read_inputs()
        ref.same(got, want)
        counted = (len(order) + every - 1) // every
        assert want["in_frames"].sum() > 0 and want["hist"][:, 1:].sum() > 0
        outputs_on = net.monitor_read()
        assert outputs_on["batches_counted"] == counted and outputs_on["batches_seen"] == len(order)
        # the same run with inputs off: the monitor's own tables are what they were
        net.monitor_begin(every=every)
        for k in order:
            call(k)
        outputs_off = net.monitor_read()
        monitor_ref.same(outputs_on, outputs_off)
        assert outputs_off["batches_counted"] == counted and outputs_off["frames"].sum() > 0
        with pytest.raises(L.CovahipError):
            net.monitor_read_inputs()                       # begin discarded the setting
        net.monitor_end()
    finally:
        ctx.set_lanes(1)
        for d in devs:
            d.free()
        for p in outs:
            ctx.free(p)


def test_attached_stacked_host_entry_and_a_mixed_batch_above_256(ctx):
    """filter_full on host stacks, and a mixed batch of 300 stacks, whose order / slice table monitor_count uploads and the
    input kernel shares."""
    h, w, b = 16, 16, 300
    net = _net(ctx, h, w, b, 3)
    stack = synth.stacked_batch(b, h, w, seed=9, streams=3)
    fr, index = _as_frames(stack, h)
    r_new = ref.records(ref.newest(stack, h), False)
    net.monitor_begin()
    net.monitor_set_inputs(True)
    want = ref.empty(3, h, w)
    for ids in ((np.arange(b) % 3).astype(np.uint8), (np.arange(b) // 100).astype(np.uint8), None):
        net.filter_full(stack, 1, 8, model_ids=ids)
        net.filter_frames(fr, index, 1, 8, model_ids=ids)
        ref.input_ref(r_new, ids, 3, into=want)
        ref.input_ref(r_new, ids, 3, into=want)
    ref.same(net.monitor_read_inputs(), want)
    net.monitor_end()


def test_the_pipe_counts_its_inputs(ctx):
    h, w, b, max_boxes = 45, 80, 24, 32
    ctx.set_lanes(2)
    pipe = None
    try:
        net = _net(ctx, h, w, b, 3)
        pipe = FilterPipe(net, max_batch=b, max_frames=4 * b, max_boxes=max_boxes, n_slots=3, want_mask=False)
        net.monitor_begin()
        net.monitor_set_inputs(True)
        want = ref.empty(3, h, w)
        in_flight = []
        for k in range(5):
            stack = synth.stacked_batch(b, h, w, seed=90 + k, streams=2)
            fr, index = _as_frames(stack, h)
            acq = pipe.acquire()
            while acq is None:
                pipe.collect(in_flight.pop(0))
                acq = pipe.acquire()
            slot, pf, pi = acq
            ids = ((np.arange(b) + k) % 3).astype(np.uint8)
            pf[:fr.shape[0]] = fr
            pi[:b] = index
            pipe.model_ids(slot)[:b] = ids
            pipe.submit(slot, fr.shape[0], b, 2)
            in_flight.append(slot)
            ref.input_ref(ref.records(ref.newest(stack, h), False), ids, 3, into=want)
        while in_flight:
            pipe.collect(in_flight.pop(0))
        ref.same(net.monitor_read_inputs(), want)
        assert net.monitor_read()["batches_counted"] == 5 and want["in_frames"].sum() == 5 * b
        net.monitor_end()
    finally:
        if pipe is not None:
            pipe.close()
        ctx.set_lanes(1)


def test_inputs_off_launches_what_a_monitor_without_input_tables_launches(ctx):
    h, w, b, max_boxes = 45, 80, 8, 64
    stacks = [synth.stacked_batch(b, h, w, seed=20 + k, streams=2) for k in range(3)]
    ids = [((np.arange(b) + k) % 3).astype(np.uint8) for k in range(3)]

    def serve(c, net):
        c.profile(True)
        outs = [net.filter_full(s, 2, max_boxes, True, True, model_ids=i) for s, i in zip(stacks, ids)]
        outs += [net.filter_frames(*_as_frames(s, h), 2, max_boxes, True, True, model_ids=i) for s, i in zip(stacks, ids)]
        prof = {k: v[1] for k, v in c.profile_read().items()}
        c.profile(False)
        return outs, prof

    fresh = Context(0)                                       # a ctx on which no input tables are ever created
    try:
        net0 = _net(fresh, h, w, b, 3)
        net0.monitor_begin()
        base_outs, base_prof = serve(fresh, net0)
    finally:
        fresh.close()
    assert base_prof["monitor_count"] == 6 and "input_count" not in base_prof and "input_finish" not in base_prof
    net = _net(ctx, h, w, b, 3)
    net.monitor_begin()
    default_outs, default_prof = serve(ctx, net)             # off is the default
    net.monitor_set_inputs(True)
    on_outs, on_prof = serve(ctx, net)
    net.monitor_set_inputs(False)
    off_outs, off_prof = serve(ctx, net)
    net.monitor_end()
    assert default_prof == base_prof and off_prof == base_prof
    assert on_prof.pop("input_count") == 6 and on_prof.pop("input_finish") == 6 and on_prof == base_prof
    for outs in (default_outs, on_outs, off_outs):
        for o, want in zip(outs, base_outs):
            assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(o[1:], want[1:]))


# ------------------------------------------------------------------------------------------------------------------ 5. read, reset, refusals
def test_read_reset_and_refusals(ctx):
    lib = L.lib()
    h, w, n = 16, 16, 10
    frames = make_frames("sparse", n + 3, h, w, 1)
    ids = (np.arange(n) % 2).astype(np.uint8)
    want = ref.input_ref(ref.records(frames[3:], False), ids, 2)
    index = np.asarray([[b + 3, b + 2, b + 1, b] for b in range(n)], np.int32)
    set_in, get_in, add_in, read_in = (lib.covahip_monitor_set_inputs, lib.covahip_monitor_get_inputs, lib.covahip_monitor_add_inputs,
                                       lib.covahip_monitor_read_inputs)
    nulls = (None,) * 6

    def do_add(src=frames.ctypes.data, form=L.INPUT_FRAMES, nf=n + 3, idx=index.ctypes.data, batch=n, i=ids.ctypes.data, kind=L.MEM_HOST,
               handle=ctx.handle):
        return add_in(handle, src, form, nf, idx, batch, i, kind)

    mon.begin(ctx, h, w, 2, 4)
    mon.end(ctx)                                            # whatever earlier tests left open is closed
    on = C.c_int(-1)
    assert set_in(ctx.handle, 1) == INVALID and get_in(ctx.handle, C.byref(on)) == INVALID and read_in(ctx.handle, 0, *nulls) == INVALID
    assert do_add() == INVALID
    mon.begin(ctx, h, w, 2, 4)
    assert get_in(ctx.handle, C.byref(on)) == 0 and on.value == 0       # off is the default
    assert do_add() == INVALID and read_in(ctx.handle, 0, *nulls) == INVALID   # inputs not switched on
    assert set_in(None, 1) == INVALID and set_in(ctx.handle, 2) == INVALID and set_in(ctx.handle, -1) == INVALID
    assert get_in(ctx.handle, None) == INVALID and get_in(None, C.byref(on)) == INVALID
    assert set_in(ctx.handle, 1) == 0 and get_in(ctx.handle, C.byref(on)) == 0 and on.value == 1
    assert do_add() == 0
    ref.same(mon.read_inputs(ctx), want)
    assert set_in(ctx.handle, 1) == 0                                   # on while on keeps the tables
    ref.same(mon.read_inputs(ctx), want)
    # every refused call leaves the tables as they are
    assert do_add(handle=None) == INVALID and do_add(form=3) == INVALID and do_add(form=-1) == INVALID and do_add(batch=-1) == INVALID
    assert do_add(src=None) == INVALID and do_add(kind=2) == INVALID and do_add(kind=-1) == INVALID
    bad_ids = ids.copy()
    bad_ids[3] = 2
    assert do_add(i=bad_ids.ctypes.data) == INVALID
    assert do_add(nf=3) == INVALID and do_add(idx=None, batch=n - 1) == INVALID      # NULL stack_index: batch must be n_frames - 3
    for v in (-1, n + 3):
        bad_index = index.copy()
        bad_index[4, 2] = v                                             # an older slice outside the frames is refused too
        assert do_add(idx=bad_index.ctypes.data) == INVALID
    assert do_add(src=None, batch=0) == 0                               # batch == 0 is OK and changes nothing
    assert read_in(None, 0, *nulls) == INVALID
    ref.same(mon.read_inputs(ctx), want)
    assert read_in(ctx.handle, 0, *nulls) == 0                          # NULL outputs are fine
    # read_inputs(reset) zeroes the input tables only; monitor_read(reset) zeroes both
    mask = np.ones((n, h, w), np.uint8)
    counts = np.zeros(n, np.int32)
    boxes = np.zeros((n, 4), L.BOX_DTYPE)
    mon.add(ctx, mask, counts, boxes, ids)
    out_want = monitor_ref.monitor_ref(mask, counts, boxes, ids, 4, 2)
    ref.same(mon.read_inputs(ctx, reset=True), want)
    ref.same(mon.read_inputs(ctx), ref.empty(2, h, w))
    monitor_ref.same(mon.read(ctx), out_want)
    assert do_add() == 0
    monitor_ref.same(mon.read(ctx, reset=True), out_want)
    ref.same(mon.read_inputs(ctx), ref.empty(2, h, w))
    monitor_ref.same(mon.read(ctx), monitor_ref.empty(2, h, w))
    # off frees the tables, on again starts from zero; begin discards the setting
    assert do_add() == 0 and set_in(ctx.handle, 0) == 0 and read_in(ctx.handle, 0, *nulls) == INVALID
    assert set_in(ctx.handle, 1) == 0
    ref.same(mon.read_inputs(ctx), ref.empty(2, h, w))
    mon.begin(ctx, h, w, 2, 4)
    assert get_in(ctx.handle, C.byref(on)) == 0 and on.value == 0 and do_add() == INVALID
    mon.end(ctx)
    # an attached monitor takes no add_inputs
    net = _net(ctx, h, w, 4, 2)
    net.monitor_begin()
    net.monitor_set_inputs(True)
    assert do_add() == INVALID
    ref.same(net.monitor_read_inputs(), ref.empty(2, h, w))
    net.monitor_end()


# ------------------------------------------------------------------------------------------------------------------ 6. command line
def test_command_line_inputs(ctx, tmp_path, capsys):
    h, w, n = 45, 80, 10
    cams = [make_frames("special" if k else "sparse", 4 * n, h, w, 70 + k) for k in range(2)]
    args, saved = [], []
    for k in range(2):
        rec, wts = tmp_path / f"cam{k}.tfrecord", tmp_path / f"cam{k}.cvhw"
        with open(rec, "wb") as f:
            for i in range(0, 4 * n, 8):
                f.write(tfrecord_example(cams[k][i:i + 8], np.zeros((8, h, w), np.uint8), gop=8))
        wts.write_bytes(W.to_bytes(W.blob_like(seed=8 + k)))
        args.append((str(rec), str(wts)))
        saved.append(str(tmp_path / f"cam{k}.inputs.json"))
    base = [a[0] for a in args] + ["--weights"] + [a[1] for a in args] + ["--h-mb", str(h), "--w-mb", str(w), "--batch", "16"]
    assert mon.main(base + ["--save-inputs"] + saved) == 0
    out = capsys.readouterr().out
    # a sample is frames 4 j .. 4 j + 3 of its camera, the newest slice 4 j + 3
    want = [ref.input_ref(ref.records(c[3::4], False)) for c in cams]
    for k in range(2):
        got = mon.load_inputs(saved[k])
        ref.same(got, {f: v[0] for f, v in want[k].items()})
        assert mon.format_input_report(mon.input_report(got, None) | {"model": k}, args[k][0]) in out
    assert out.count(" inputs: frames 10 ") == 2
    # against its own counts a camera is at distance 0; against the other camera's it is not
    assert mon.main(base + ["--input-baseline"] + saved + ["--input-drift", "0.5"]) == 0
    out = capsys.readouterr().out
    assert out.count("tv 0.0000") == 2 and out.count("no input drift (tv at most 0.5)") == 2
    assert mon.main(base + ["--input-baseline"] + saved[::-1] + ["--input-drift", "0.000001"]) == 0
    out = capsys.readouterr().out
    cross = mon.input_report(mon.load_inputs(saved[0]), None, mon.load_inputs(saved[1]))["tv"]
    assert cross > 0 and out.count("INPUT DRIFT (tv above 1e-06)") == 2 and f"tv {cross:.4f}" in out
