"""covahip_bboxcc_v: bboxcc with an area threshold per frame, against the CPU oracle frame by frame.

Frame b of a call must give what oracle.ref.regionprops_batch gives for that frame alone at area_thresh[b], byte for byte and
in order.  The masks are Bernoulli noise of density 0.3 (below the 8-connected percolation threshold: components of every
area from 1 up), so a frame's box list is different at every threshold used; each case first checks that from the oracle
alone, so a kernel that ignores the array, or reads another frame's entry, cannot pass.  Every stand-alone kernel is driven:
the wave kernel's first pass, its persistent second-chance pass and the persistent workgroup pass (both take their frames from
an overflow list and must index the thresholds by the FRAME, not by the list position), the workgroup kernel with the
run-based and with the block-based body, and the kernel for frames whose state does not fit LDS (135x240)."""
import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd.elements import BboxCc, Context
from oracle import ref
from tests.cc_runs import run_counts

pytestmark = pytest.mark.gpu

THRS = (1, 2, 3, 5, 8)


@pytest.fixture
def own_ctx(ctx):
    """A context of the test's own: lane 0's bboxcc plan state starts empty (the session `ctx` tells whether there is a device)."""
    c = Context(0)
    try:
        yield c
    finally:
        c.close()


def _noise(rng, n, h, w, density=0.3):
    return (rng.random((n, h, w)) < density).astype(np.uint8)


def _oracle(uniq, max_boxes):
    """{threshold: (boxes, counts)} of the unique frames."""
    return {t: ref.regionprops_batch(uniq, t, max_boxes) for t in THRS}


def _check(boxes, counts, table, idx, thr, max_boxes, what):
    for i, (u, t) in enumerate(zip(idx, thr)):
        rb, rc = table[int(t)]
        assert counts[i] == rc[u], f"{what}: frame {i} (threshold {t}): count {counts[i]} != {rc[u]}"
        n = min(int(rc[u]), max_boxes)
        assert boxes[i, :n].tobytes() == rb[u, :n].tobytes(), f"{what}: frame {i} (threshold {t}): boxes differ"


def _thresholds_matter(table, frames):
    """From the oracle alone: every threshold gives each of these frames another, non-empty box list."""
    for u in frames:
        c = [int(table[t][1][u]) for t in THRS]
        assert all(a > b for a, b in zip(c, c[1:])) and c[-1] > 0, (u, c)


def _device_call(ctx, cc, masks, thr, fn=None, shift=0):
    """shift: the mask starts that many bytes past its (longer) allocation."""
    b, h, w = masks.shape
    d_m0, d_b, d_c = ctx.malloc(masks.nbytes + 8), ctx.malloc(max(1, b * cc.max_boxes) * 20), ctx.malloc(b * 4)
    d_m = d_m0 + shift
    lib = L.lib()
    try:
        assert d_m0 % 8 == 0
        ctx.h2d(d_m, masks)
        L.check(lib.covahip_memset(ctx.handle, d_c, 0xA5, b * 4), "memset")          # poisoned: a frame no pass labels cannot pass
        L.check(lib.covahip_memset(ctx.handle, d_b, 0x5A, b * cc.max_boxes * 20), "memset")
        if fn is None:
            cc.regionprops_v_device(d_m, b, h, w, thr, d_b, d_c)
        else:
            fn(d_m, b, h, w, d_b, d_c)
        stats = cc.overflow_stats()   # synchronises the ctx
        boxes, counts = np.zeros((b, cc.max_boxes), L.BOX_DTYPE), np.zeros(b, np.int32)
        ctx.d2h(boxes, d_b)
        ctx.d2h(counts, d_c)
        return boxes, counts, stats
    finally:
        for p in (d_m0, d_b, d_c):
            ctx.free(p)


# (h, w, developer wave capacity, kernels the profile must show)
CHOICES = [
    (68, 120, 0, {"bboxcc_kernel"}),                                                  # small batch: workgroup kernel, run-based body
    (68, 120, -1, {"bboxcc_kernel"}),                                                 # ... block-based body
    (20, 28, 0, {"bboxcc_kernel"}),                                                   # W % 8 != 0: block-based body
    (20, 32, 160, {"bboxcc_wave_kernel"}),                                            # wave kernel at full capacity (160 blocks): nothing overflows
    (68, 120, 24, {"bboxcc_wave_kernel", "bboxcc_wave_kernel_2", "bboxcc_kernel"}),   # every frame through both overflow lists
    (135, 240, 0, {"bboxcc_big_kernel"}),                                             # state in global memory
]


@pytest.mark.parametrize("h,w,cap,kernels", CHOICES)
def test_every_kernel_choice(own_ctx, h, w, cap, kernels):
    ctx = own_ctx
    b, max_boxes = 11, 2048
    rng = np.random.default_rng(h * w + cap + 7)
    masks = _noise(rng, b, h, w)
    thr = np.array([THRS[(3 * i + 1) % 5] for i in range(b)], np.int32)   # neighbours always differ
    table = _oracle(masks, max_boxes)
    _thresholds_matter(table, range(b))
    idx = np.arange(b)
    cc = BboxCc(ctx, 99, max_boxes)          # (the element's own scalar threshold plays no part)
    cc.set_wave_cap(cap)
    ctx.profile(True)
    try:
        boxes, counts = cc.regionprops_v(masks, thr)                       # host pointers
        _check(boxes, counts, table, idx, thr, max_boxes, "host")
        boxes, counts, _ = _device_call(ctx, cc, masks, thr)               # device pointers
        _check(boxes, counts, table, idx, thr, max_boxes, "device")
        assert set(ctx.profile_read()) == kernels
        # the same threshold everywhere is covahip_bboxcc
        for t in (1, 5):
            one = BboxCc(ctx, t, max_boxes)
            sb, sc = one.regionprops(masks)
            vb, vc = cc.regionprops_v(masks, np.full(b, t, np.int32))
            assert np.array_equal(sc, vc) and sc.tobytes() == table[t][1].tobytes()
            for i in range(b):
                assert vb[i, :vc[i]].tobytes() == sb[i, :sc[i]].tobytes()
            db, dc, _ = _device_call(ctx, one, masks, None, fn=one.regionprops_device)
            ub, uc, _ = _device_call(ctx, cc, masks, np.full(b, t, np.int32))
            assert ub.tobytes() == db.tobytes() and uc.tobytes() == dc.tobytes()   # poisoned alike: the whole buffers
    finally:
        ctx.profile(False)
        cc.set_wave_cap(0)


@pytest.mark.parametrize("density", [0.05, 0.5])
@pytest.mark.parametrize("cap", [0, 24, -1])
@pytest.mark.parametrize("h,w", [(68, 120), (16, 64)])
def test_mask_pointer_off_an_8_byte_boundary(own_ctx, h, w, cap, density):
    """h * w and W are multiples of 8 here, so only the caller's pointer keeps the frames off 8-byte boundaries: the wave kernel
    and the run-based body are turned away (both load 8 mask bytes at a time) and the block-based body reads byte by byte.  Both
    device entries, against the oracle."""
    ctx = own_ctx
    b, max_boxes = 11, 2048
    masks = _noise(np.random.default_rng(h + w + cap), b, h, w, density)
    thr = np.array([THRS[(3 * i + 1) % 5] for i in range(b)], np.int32)
    table = _oracle(masks, max_boxes)
    assert all(table[1][1][u] > table[8][1][u] for u in range(b))      # from the oracle alone: the thresholds matter
    idx = np.arange(b)
    cc, one = BboxCc(ctx, 99, max_boxes), BboxCc(ctx, 2, max_boxes)
    cc.set_wave_cap(cap)
    ctx.profile(True)
    try:
        for shift in (1, 4, 7):
            boxes, counts, _ = _device_call(ctx, cc, masks, thr, shift=shift)
            _check(boxes, counts, table, idx, thr, max_boxes, f"bboxcc_v, mask + {shift}")
            boxes, counts, _ = _device_call(ctx, one, masks, None, fn=one.regionprops_device, shift=shift)
            _check(boxes, counts, table, idx, np.full(b, 2), max_boxes, f"bboxcc, mask + {shift}")
        assert set(ctx.profile_read()) == {"bboxcc_kernel"}
    finally:
        ctx.profile(False)
        cc.set_wave_cap(0)


def test_large_batch_plan_declines_an_unaligned_mask(own_ctx):
    """More than 3 x num_cu frames ask for the wave kernel's large-batch plan; a mask 4 bytes off has to be declined by it."""
    ctx = own_ctx
    h, w, max_boxes = 16, 64, 512
    rng = np.random.default_rng(21)
    uniq = np.concatenate([_noise(rng, 6, h, w, 0.05), _noise(rng, 6, h, w, 0.5)])
    table = _oracle(uniq, max_boxes)
    assert all(table[1][1][u] > table[8][1][u] for u in range(12))
    b = 3 * ctx.info()["num_cu"] + 8
    idx = rng.integers(0, 12, b)
    thr = rng.choice(THRS, b).astype(np.int32)
    cc = BboxCc(ctx, 99, max_boxes)
    masks = np.ascontiguousarray(uniq[idx])
    ctx.profile(True)
    try:
        boxes, counts, stats = _device_call(ctx, cc, masks, thr, shift=4)
        assert set(ctx.profile_read()) == {"bboxcc_kernel"} and stats["batch"] == 0
        _check(boxes, counts, table, idx, thr, max_boxes, "large batch, mask + 4")
        boxes, counts, stats = _device_call(ctx, cc, masks, thr)           # aligned: the plan it declined
        assert "bboxcc_wave_kernel" in set(ctx.profile_read())
        _check(boxes, counts, table, idx, thr, max_boxes, "large batch, aligned")
    finally:
        ctx.profile(False)


def test_truncation_per_frame(own_ctx):
    """max_boxes below a frame's count: the count reports every passing component, the first max_boxes are written."""
    h, w, b, max_boxes = 45, 80, 6, 16
    masks = _noise(np.random.default_rng(5), b, h, w)
    thr = np.array([1, 8, 2, 5, 1, 3], np.int32)
    table = _oracle(masks, max_boxes)
    assert all(table[int(t)][1][i] > max_boxes for i, t in enumerate(thr))
    boxes, counts = BboxCc(own_ctx, 1, max_boxes).regionprops_v(masks, thr)
    _check(boxes, counts, table, np.arange(b), thr, max_boxes, "truncated")


def test_large_batch_overflow_lists(own_ctx):
    """The automatic large-batch plan on an empty lane: pass 1 at 128 runs, the second chance at 512, the workgroup pass for the
    rest.  Sparse, medium and dense frames interleaved, a random threshold per frame: the listed frames' thresholds differ from
    their neighbours' and from those at their list positions."""
    ctx = own_ctx
    h, w, max_boxes = 68, 120, 1024
    rng = np.random.default_rng(12)
    uniq = np.concatenate([_noise(rng, 6, h, w, 0.004), _noise(rng, 6, h, w, 0.04), _noise(rng, 6, h, w, 0.3)])
    runs = run_counts(uniq)
    assert (runs[:6] <= 128).all() and ((runs[6:12] > 128) & (runs[6:12] <= 512)).all() and (runs[12:] > 512).all(), runs.tolist()
    table = _oracle(uniq, max_boxes)
    _thresholds_matter(table, range(12, 18))                       # the dense frames: every threshold changes their lists
    assert all(table[1][1][u] > table[8][1][u] for u in range(6, 12))
    b = 3 * ctx.info()["num_cu"] + 40
    idx = rng.integers(0, 18, b)
    thr = rng.choice(THRS, b).astype(np.int32)
    listed = np.flatnonzero(runs[idx] > 128)
    assert len(listed) > 64 and (thr[listed] != thr[np.arange(len(listed))]).sum() > len(listed) // 2   # position != frame
    assert (thr[listed] != thr[listed - 1]).sum() > len(listed) // 2
    cc = BboxCc(ctx, 99, max_boxes)
    masks = np.ascontiguousarray(uniq[idx])
    ctx.profile(True)
    try:
        boxes, counts, stats = _device_call(ctx, cc, masks, thr)
        names = set(ctx.profile_read())
    finally:
        ctx.profile(False)
    assert names == {"bboxcc_wave_kernel", "bboxcc_wave_kernel_2", "bboxcc_kernel"}
    assert stats == {"batch": b, "overflow_pass1": len(listed), "overflow_pass2": int((runs[idx] > 512).sum()), "cap_pass1": 128}
    _check(boxes, counts, table, idx, thr, max_boxes, "large batch")
    boxes, counts = cc.regionprops_v(masks, thr)                   # host pointers, the plan of the statistics just collected
    _check(boxes, counts, table, idx, thr, max_boxes, "large batch, host")


def test_threshold_table_grows_repeats_changes_and_shrinks(own_ctx):
    """One ctx, calls of 3, 8, 8, 8 and 5 frames: the ctx's threshold table is made, grows, is asked for the thresholds it holds,
    for others of the same length, and for a shorter list.  Device pointers (the kernels read the table while the host goes on)
    and host pointers, each call against the oracle."""
    ctx = own_ctx
    h, w, max_boxes = 16, 16, 64
    rng = np.random.default_rng(33)
    uniq = _noise(rng, 8, h, w)
    table = _oracle(uniq, max_boxes)
    assert all(table[1][1][u] > table[8][1][u] for u in range(8))          # from the oracle alone: the thresholds matter
    cc = BboxCc(ctx, 99, max_boxes)
    thr8 = np.array([THRS[(3 * i + 1) % 5] for i in range(8)], np.int32)
    other8 = np.array([THRS[(3 * i + 2) % 5] for i in range(8)], np.int32)
    assert (thr8 != other8).all()
    for b, thr, what in ((3, thr8[:3], "first"), (8, thr8, "grown"), (8, thr8, "repeated"), (8, other8, "changed"), (5, thr8[3:], "shrunk")):
        idx = np.arange(8 - b, 8) if what == "shrunk" else np.arange(b)
        masks = np.ascontiguousarray(uniq[idx])
        boxes, counts, _ = _device_call(ctx, cc, masks, thr)
        _check(boxes, counts, table, idx, thr, max_boxes, f"{what}, device")
        boxes, counts = cc.regionprops_v(masks, thr)
        _check(boxes, counts, table, idx, thr, max_boxes, f"{what}, host")


def test_errors(own_ctx):
    lib = L.lib()
    masks = _noise(np.random.default_rng(1), 2, 16, 16)
    boxes, counts = np.zeros((2, 8), L.BOX_DTYPE), np.zeros(2, np.int32)
    thr = np.array([1, 2], np.int32)
    args = (masks.ctypes.data, 2, 16, 16)
    out = (boxes.ctypes.data, counts.ctypes.data, 8, L.MEM_HOST)
    assert lib.covahip_bboxcc_v(own_ctx.handle, *args, None, *out) == 1                      # NULL array
    assert lib.covahip_bboxcc_v(None, *args, thr.ctypes.data, *out) == 1
    assert lib.covahip_bboxcc_v(own_ctx.handle, *args, thr.ctypes.data, boxes.ctypes.data, counts.ctypes.data, 8, 7) == 1
    assert lib.covahip_bboxcc_v(own_ctx.handle, *args, thr.ctypes.data, *out) == 0
    with pytest.raises(ValueError):
        BboxCc(own_ctx, 1, 8).regionprops_v(masks, [1, 2, 3])
