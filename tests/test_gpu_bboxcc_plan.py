"""bboxcc's automatic large-batch plan (covahip_bboxcc_launch, cova_amd/csrc/bboxcc.hip) against the CPU oracle.

Above 3 x num_cu frames the automatic mode runs the wave kernel at a capacity chosen from the previous call's sampled run
statistics, a second-chance pass, a persistent workgroup pass and two alternating counter sets.  Every test here runs on a
context of its own (lane 0's plan state starts empty), and every call is checked twice: its boxes against
oracle.ref.regionprops_batch bit for bit, and its plan -- overflow_stats() and the kernels the profile saw -- against
tests/cc_runs.PlanModel.  Calls go through the device entry with poisoned outputs, so a frame that no pass labels cannot pass
on an earlier call's results; overflow_stats() synchronises the context after each call, so the next plan reads complete
statistics, as after the synchronous host entry."""
import ctypes as C

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd.elements import BboxCc, Context
from oracle import ref
from tests.cc_runs import LaneState, PlanModel, masks_with_runs, run_counts

pytestmark = pytest.mark.gpu

FIELDS = (("left", "left"), ("top", "top"), ("width", "width"), ("height", "height"), ("area_px", "area"))


@pytest.fixture
def own_ctx(ctx):
    """A context of the test's own (the session `ctx` only tells whether there is a device)."""
    c = Context(0)
    try:
        yield c
    finally:
        c.close()


def _nb(h, w):
    return ((h + 1) // 2) * ((w + 1) // 2)


def _expected(uniq, idx, thresh, max_boxes):
    """Oracle of the unique frames, spread to the batch."""
    rb, rc = ref.regionprops_batch(uniq, thresh, max_boxes)
    return rb[idx], rc[idx]


def _assert_boxes(boxes, counts, rboxes, rcounts, max_boxes, what):
    bad = np.flatnonzero(counts != rcounts)
    assert not len(bad), f"{what}: counts differ in {len(bad)} frames, first {bad[0]}: {counts[bad[0]]} != {rcounts[bad[0]]}"
    if max_boxes == 0:
        return
    valid = np.arange(max_boxes)[None, :] < np.minimum(counts, max_boxes)[:, None]
    for f, g in FIELDS:
        bad = np.argwhere((boxes[f] != rboxes[g]) & valid)
        assert not len(bad), f"{what}: field {f} differs in {len(bad)} boxes, first frame {bad[0][0]} box {bad[0][1]}"


class Runner:
    """Device-pointer bboxcc on one context, with the plan model of lane 0 alongside."""

    def __init__(self, ctx, max_mask_bytes, max_box_slots, max_frames):
        self.ctx = ctx
        self.lib = L.lib()
        self.num_cu = ctx.info()["num_cu"]
        self.model = PlanModel(self.num_cu)
        self.state = LaneState()
        self.d_m = ctx.malloc(max_mask_bytes + 8)
        self.d_b = ctx.malloc(max(max_box_slots, 1) * 20)
        self.d_c = ctx.malloc(max_frames * 4)
        self.caps = (max_mask_bytes, max_box_slots, max_frames)
        self.plans = []

    def close(self):
        for p in (self.d_m, self.d_b, self.d_c):
            self.ctx.free(p)

    def _poison(self, b, max_boxes):
        L.check(self.lib.covahip_memset(self.ctx.handle, C.c_void_p(self.d_c), 0xA5, b * 4), "memset")
        if max_boxes:
            L.check(self.lib.covahip_memset(self.ctx.handle, C.c_void_p(self.d_b), 0x5A, b * max_boxes * 20), "memset")

    def run(self, uniq, idx, thresh, max_boxes, cap=0, offset=0, runs=None):
        """One call on frames uniq[idx]; checks boxes and plan, returns the model's plan."""
        b = len(idx)
        h, w = uniq.shape[1:]
        masks = np.ascontiguousarray(uniq[idx])
        assert masks.nbytes + offset <= self.caps[0] + 8 and b * max_boxes <= self.caps[1] and b <= self.caps[2]
        self.ctx.h2d(self.d_m + offset, masks)
        self._poison(b, max_boxes)
        cc = BboxCc(self.ctx, cc_threshold=thresh, max_boxes=max_boxes)
        cc.set_wave_cap(cap)
        self.ctx.profile(True)
        try:
            cc.regionprops_device(self.d_m + offset, b, h, w, self.d_b, self.d_c)
            got = cc.overflow_stats()   # synchronises the ctx
            prof = self.ctx.profile_read()
        finally:
            self.ctx.profile(False)
            cc.set_wave_cap(0)
        runs = run_counts(uniq)[idx] if runs is None else runs
        plan = self.model.call(self.state, runs, h, w, forced_cap=cap, aligned=offset % 8 == 0)
        what = f"{b}x{h}x{w} thresh {thresh} max_boxes {max_boxes} cap {cap} offset {offset} (plan {plan.cap}/{plan.pass3})"
        boxes = np.zeros((b, max_boxes), L.BOX_DTYPE)
        counts = np.zeros(b, np.int32)
        if max_boxes:
            self.ctx.d2h(boxes, self.d_b)
        self.ctx.d2h(counts, self.d_c)
        _assert_boxes(boxes, counts, *_expected(uniq, idx, thresh, max_boxes), max_boxes, what)
        assert {k: v[1] for k, v in prof.items()} == plan.kernels, what
        exp = plan.overflow
        if exp["batch"]:
            assert got == exp, what
        else:
            assert (got["batch"], got["overflow_pass1"], got["overflow_pass2"]) == (0, 0, 0), what
        self.state = plan.state
        self.plans.append((plan, runs))
        return plan


@pytest.fixture
def runner_factory(own_ctx):
    made = []

    def make(*a):
        r = Runner(own_ctx, *a)
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


def _bank(h, w, classes, variants, seed):
    """[len(classes) * variants] frames with exactly the given run counts, class k at k * variants ..."""
    rng = np.random.default_rng(seed)
    return np.stack([masks_with_runs(n, h, w, rng) for n in classes for _ in range(variants)])


def _pick(classes, variants, want, rng):
    """Frame indices of the bank _bank(classes, variants) for run counts `want` (one per frame)."""
    pos = {n: k for k, n in enumerate(classes)}
    return np.array([pos[n] * variants + rng.integers(variants) for n in want])


# ------------------------------------------------------------------------------------------------------------------------- tests
H, W = 68, 120
NB = _nb(H, W)   # 2040
CLASSES = (0, 1, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 1000, NB)


def test_class_mix(runner_factory):
    """4,096 frames of every run class around the capacity edges; the sampled slots (index % 16 == 0) walk through the classes.
    Thresholds 1 and 30, max_boxes nb / 64 / 0; forced capacities 24, 128, 512, the workgroup kernel alone and the automatic
    plan all give the oracle's boxes."""
    rng = np.random.default_rng(1)
    bank = _bank(H, W, CLASSES, 2, 11)
    want = rng.choice(CLASSES, 4096)
    want[::16] = np.resize(CLASSES, 256)
    idx = _pick(CLASSES, 2, want, rng)
    r = runner_factory(4096 * H * W, 4096 * NB, 4096)
    for thresh, max_boxes in ((1, NB), (30, 64), (1, 0)):
        for cap in (0, 24, 128, 512, -1, 0):
            r.run(bank, idx, thresh, max_boxes, cap)
    # the automatic calls: 128 on the empty lane, then what the last forced call's statistics say (6 of 16 sampled classes > 256)
    assert [p.cap for p, _ in r.plans[::6]] == [128, 512, 512]


def _sampled(rng, n_hit, hit_classes, rest_classes, b=4096):
    """Run counts of a batch whose sampled slots hold exactly n_hit frames of hit_classes, the others rest_classes."""
    want = rng.choice(rest_classes, b)
    slots = np.arange(0, b, 16)
    pick = rng.permutation(len(slots))[:n_hit]
    want[slots] = rng.choice(rest_classes, len(slots))
    want[slots[pick]] = rng.choice(hit_classes, n_hit)
    return want


def test_state_sequence(runner_factory):
    """One context, sparse -> dense -> ... -> sparse with statistics on every capacity edge, batch 4,096 -> 800 -> 5,000 and the
    shape 68x120 -> 45x80 -> 128x128.  Covers (cc_runs.PlanModel names the branch, overflow_stats() and the profile prove it):
    capacities 128 / 192 / 256 / 512, pass 2 run / skipped / not planned / at full capacity, pass 3 quiet / full / one, the
    counters reallocated, and persistent loops that iterate (more listed frames than waves or workgroups)."""
    rng = np.random.default_rng(2)
    bank = _bank(H, W, CLASSES, 3, 21)
    r = runner_factory(4096 * 128 * 128, 5000 * NB, 5000)
    low = (0, 1, 127, 128)                      # never counted by the statistics (> 128 is)
    dense = (1000, NB, 513)
    small = 3 * r.num_cu + 32                   # 800 at 256 CUs: still the large-batch plan

    def call(want, **kw):
        return r.run(bank, _pick(CLASSES, 3, want, rng), 1, NB, **kw)

    def mixed(n_hit, hit, b=4096):
        want = _sampled(rng, n_hit, hit, low, b)
        body = np.ones(b, bool)
        body[::16] = False
        want[body] = rng.choice(dense + (129, 256, 257), body.sum())
        return want

    seq = []
    seq.append(call(rng.choice(low, 4096)))                      # empty lane: 128, pass 2 runs, full grid, nothing overflows
    seq.append(call(rng.choice(dense, 4096)))                    # last call had no overflow: pass 2 skipped, quiet 32 drain 4,096
    seq.append(call(mixed(65, (257, 511, 513, 1000, NB))))       # 512 (c3 = 256): pass 2 not planned, full grid; c3 = 65
    seq.append(call(mixed(64, (257, 511, 513, 1000, NB))))       # 512 (65 > a quarter); c3 = 64
    seq.append(call(mixed(65, (193, 255, 256))))                 # 128 (64 = a quarter); pass 2 over > 3,072 frames; c2 = 65
    seq.append(call(mixed(64, (193, 255, 256))))                 # 256; pass 2 at 1,024; c2 = 64
    seq.append(call(mixed(65, (129, 191, 192))))                 # 128; c1 = 65
    seq.append(call(mixed(64, (129, 191, 192))))                 # 192; pass 2 at 768; c1 = 64
    seq.append(call(rng.choice(low, 4096)))                      # 128; pass 2 runs, nothing overflows
    seq.append(call(rng.choice(dense, small)))                   # 800: buffer kept; 128, pass 2 skipped, quiet 32 drain 800
    seq.append(call(mixed(200, (513, 1000, NB), b=5000)))        # 5,000: reallocated, turn reset; 512 from the 800 dense frames
    assert [p.cap for p in seq] == [128, 128, 512, 512, 128, 256, 128, 192, 128, 128, 512]
    assert [p.second_runs for p in seq] == [True, False, False, False, True, True, True, True, True, False, False]
    assert [p.second_planned for p in seq] == [True, True, False, False, True, True, True, True, True, True, False]
    assert [p.pass3 for p in seq] == ["full", "quiet", "full", "full", "full", "full", "full", "full", "full", "quiet", "full"]
    assert [p.realloc for p in seq] == [True] + [False] * 9 + [True]
    assert seq[2].overflow["overflow_pass2"] == seq[2].overflow["overflow_pass1"] > 0   # pass 3 took pass 1's list

    # 45x80 (nb = 920): 512 from the last statistics, four times that covers nb -> pass 2 leaves nothing, pass 3 grid of one
    nb2 = _nb(45, 80)
    cls2 = (0, 128, 129, 300, 600, nb2)
    bank2 = _bank(45, 80, cls2, 2, 22)
    p = r.run(bank2, _pick(cls2, 2, rng.choice(cls2, 4096), rng), 1, nb2)
    assert (p.cap, p.second_runs, p.pass3) == (512, True, "one") and p.overflow["overflow_pass1"] > 0
    r.run(bank2, _pick(cls2, 2, _sampled(rng, 0, (129,), (0, 128), 4096), rng), 30, 64)   # nothing overflows: the next call is quiet
    # 128x128 (nb = 4096, BH = 64: no helper lanes): 128 with a quiet drain, then 512 where pass 2 (4 x 2,048) does not fit
    nb3 = _nb(128, 128)
    cls3 = (0, 128, 129, 300, 513, 1000, 2049, nb3)
    bank3 = _bank(128, 128, cls3, 1, 23)
    want3 = rng.choice(cls3, 4096)
    want3[::16] = rng.choice((300, 513, 1000, nb3), 256)
    p = r.run(bank3, _pick(cls3, 1, want3, rng), 1, 1024)
    assert (p.cap, p.second_planned, p.second_runs, p.pass3) == (128, True, False, "quiet")   # the 45x80 call had no overflow
    p = r.run(bank3, _pick(cls3, 1, want3, rng), 1, 1024)
    assert (p.cap, p.second_planned, p.pass3) == (512, False, "full")
    assert p.overflow["overflow_pass2"] == p.overflow["overflow_pass1"] > 512

    # the persistent loops went round: more frames in a list than the launch has waves / workgroups
    num_cu = r.num_cu
    pass2_waves = {128: 4 * min(1024, 3 * num_cu), 256: 4 * min(1024, num_cu)}   # 68x120: 3 / 1 workgroups per CU at 4 x cap
    assert seq[4].overflow["overflow_pass1"] > pass2_waves[128]
    assert seq[5].overflow["overflow_pass1"] > pass2_waves[256]
    assert seq[2].overflow["overflow_pass1"] > 2 * num_cu
    assert seq[1].overflow["overflow_pass1"] > 32 and seq[9].overflow["overflow_pass1"] > 32


def test_no_sync_between_calls(own_ctx):
    """Device-pointer calls back to back, sparse and dense in turn, no synchronisation: the plan may read statistics that have
    not arrived.  Whatever it decides, no box may change."""
    rng = np.random.default_rng(3)
    bank = _bank(H, W, CLASSES, 2, 31)
    num_cu = own_ctx.info()["num_cu"]
    b, max_boxes = 4 * num_cu, 256
    batches = []
    for k in range(8):
        want = rng.choice((0, 1, 127, 128) if k % 2 == 0 else (257, 513, 1000, NB), b)
        batches.append(_pick(CLASSES, 2, want, rng))
    cc = BboxCc(own_ctx, cc_threshold=1, max_boxes=max_boxes)
    ptrs = []
    try:
        for idx in batches:
            d_m, d_b, d_c = own_ctx.malloc(b * H * W), own_ctx.malloc(b * max_boxes * 20), own_ctx.malloc(b * 4)
            ptrs += [d_m, d_b, d_c]
            own_ctx.h2d(d_m, np.ascontiguousarray(bank[idx]))
        for k in range(len(batches)):
            cc.regionprops_device(ptrs[3 * k], b, H, W, ptrs[3 * k + 1], ptrs[3 * k + 2])
        own_ctx.sync()
        for k, idx in enumerate(batches):
            boxes = np.zeros((b, max_boxes), L.BOX_DTYPE)
            counts = np.zeros(b, np.int32)
            own_ctx.d2h(boxes, ptrs[3 * k + 1])
            own_ctx.d2h(counts, ptrs[3 * k + 2])
            _assert_boxes(boxes, counts, *_expected(bank, idx, 1, max_boxes), max_boxes, f"call {k}")
    finally:
        for p in ptrs:
            own_ctx.free(p)


def test_bench_leg(runner_factory):
    """bench.py's bboxcc leg: 65,536 tiled blob frames (cc-threshold 1, 64 boxes), then 16,384 frames of thresholded noise,
    twice each (the second call plans from the first one's statistics)."""
    from tools.bboxcc_sweep import make_masks
    r = runner_factory(65536 * H * W, 65536 * 64, 65536)
    blobs, noise = make_masks("blobs", 256), make_masks("noise", 256)
    idx = np.tile(np.arange(256), 65536 // 256)
    for _ in range(2):
        r.run(blobs, idx, 1, 64)
    idx = np.tile(np.arange(256), 16384 // 256)
    for _ in range(2):
        r.run(noise, idx, 1, 256)
    assert [p.cap for p, _ in r.plans] == [128, 128, 128, 512]


def test_fallback_route(runner_factory):
    """Masks 4 bytes off 8-byte alignment, and W % 8 != 0, at a large batch: the block-based workgroup body alone (no wave
    kernel, no overflow statistics), exact."""
    rng = np.random.default_rng(4)
    bank = _bank(H, W, CLASSES, 1, 41)
    bank118 = np.stack([masks_with_runs(n, 68, 118, rng) for n in (0, 1, 128, 129, 257, 513, 1000, _nb(68, 118))])
    r = runner_factory(1024 * H * W, 1024 * NB, 1024)
    b = 3 * r.num_cu + 32
    idx = rng.integers(0, len(bank), b)
    r.run(bank, idx, 1, NB)                                    # aligned: the wave kernel (statistics for the next call)
    p = r.run(bank, idx, 1, NB, offset=4)
    assert p.cap is None and p.kernels == {"bboxcc_kernel": 1}
    p = r.run(bank118, rng.integers(0, len(bank118), b), 1, _nb(68, 118))
    assert p.cap is None and p.kernels == {"bboxcc_kernel": 1}
    p = r.run(bank118, rng.integers(0, len(bank118), b), 30, 16, offset=4)
    assert p.cap is None


def _adversarial(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    serp = np.zeros((h, w), np.uint8)
    serp[::2, :] = 1
    for k, r in enumerate(range(1, h, 2)):
        serp[r, w - 1 if k % 2 == 0 else 0] = 1
    return [np.ones((h, w), np.uint8), np.zeros((h, w), np.uint8), ((yy + xx) % 2).astype(np.uint8), serp,
            (xx % 2 == 0).astype(np.uint8), (xx % 2 == 1).astype(np.uint8),            # half blocks: nb runs
            ((xx % 2 == 0) & (yy % 4 < 2)).astype(np.uint8)]


GEOMETRY = [(1, 8), (2, 8), (3, 16), (2, 128), (63, 64), (64, 120), (65, 8), (64, 16), (127, 128), (128, 128), (128, 64), (65, 120)]


@pytest.mark.parametrize("hw", GEOMETRY, ids=[f"{h}x{w}" for h, w in GEOMETRY])
def test_wave_geometry(runner_factory, hw):
    """The wave kernel at its geometry edges (wv_plan: W <= 128, W % 8 == 0, H <= 128): BW = 64 (a full plane word), NXB = 1,
    BH = 64 (no helper lanes), BH = 32 (every row split), one block row.  Random and adversarial frames and exact run counts,
    under forced capacities 24 and nb and the automatic plan at a large batch (twice: the second plans from the first)."""
    h, w = hw
    nb = _nb(h, w)
    rng = np.random.default_rng(h * 1000 + w)
    frames = _adversarial(h, w)
    frames += [(rng.random((h, w)) < p).astype(np.uint8) for p in (0.05, 0.3, 0.6)]
    frames += [masks_with_runs(n, h, w, rng) for n in sorted({1, min(24, nb), min(25, nb), nb // 3, nb // 2, nb})]
    bank = np.stack(frames)
    r = runner_factory(2048 * h * w, 2048 * nb, 2048)
    idx = np.resize(np.arange(len(bank)), 64)
    for cap in (24, nb):
        r.run(bank, idx, 1, nb, cap)
        r.run(bank, idx, 2, 8, cap)
    big = rng.integers(0, len(bank), 3 * r.num_cu + 32)
    big[:len(bank)] = np.arange(len(bank))
    for _ in range(2):
        assert r.run(bank, big, 1, nb).cap is not None   # the wave kernel
