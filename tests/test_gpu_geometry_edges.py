"""The BlobNet forward at the edges of the geometry covahip_blobnet_load admits (include/covahip.h): the smallest grid, grids that
are odd at every level, the tallest and the widest grid that load, and every batch between 1 and max_batch on them.

1. test_stages_at_edge_shapes: the whole per-stage comparison of tests/stage_check.py (float64 references and bound of
   tests/blobnet_stages.py, K = 16 / 2K = 32; tests/test_stage_bounds.py holds the CPU justification at 16x16, 17x20 and 33x36 with
   the 3x margins -- no stage is left out at any shape) with the kernels of every case pinned through the profile.
2. test_admitted_widths_probed_at_load: which widths load at heights 16, 17, 135 and 1024 (loads only); the edge is WIDTH_EDGE.
3. test_every_batch_runs_and_agrees_with_batch_1: "every limit is checked at load, never at forward time" -- every entry at batches
   1 .. 64 of a model loaded with max_batch 64, and every stack's logits bit-identical to that stack's at batch 1.

Worst ratio |hip - ref| / (u * (rms(ref) + |ref|)) per stage over the cases of (1) on MI355X (the STAGE_RATIOS print):
E0 4.53, E1 5.40, E2 3.39, E3 3.35, D0 2.76, D1 2.75, D2 2.82, D012 5.48, T 1.18 -- at least 3.5x below K = 16 (5.8x below 2K = 32
for E1 and D012).  The fp16 emulation of tests/test_stage_bounds.py reaches, at its three small shapes: E0 3.4, E1 3.6, E2 3.7, E3 5.1,
D0 3.3, D1 3.1, D2 2.7, D012 4.6, T 1.6.  No case here takes enc23_mfma: the default chain wants a batch that fills the chip.
"""

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import synth, weights as W
from cova_amd.elements import BlobNetInfer
from tests import stage_check
from tests.stage_check import DEC012, DEC0_2, ENC2_3, TAIL, TAIL_CC

pytestmark = pytest.mark.gpu

OK, ERR_NOT_LOADED, ERR_UNSUPPORTED = 0, 4, 5

# The widest grid that loads, in macroblocks, at every height.  Set by run_enc_level's band planner for level 1 in
# cova_amd/csrc/blobnet_mfma.hip (`lds_cap = (wgs_per_cu == 1 ? 150 * 1024 : 80 * 1024) - scr_bytes` with plan_bands' fit
# `BN_T * (2 * rb + 2) * TC * px_bytes <= lds_cap`): the one-window-row band of the round-1..3 level-1 kernel, 4 slices x 4 rows x
# (W1 + 2) pixels x 32 bytes, has to fit 80 KB less 16 KB of transpose scratch, so W1 <= 126 and w_mb <= 252.
WIDTH_EDGE = 252

WMAX = "Wmax"    # in a case: the widest multiple of 4 that loads at the case's height (probed, _w_max)
_RATIOS = {}     # stage -> worst ratio over the module
_accepted = {}   # (h, max_batch) -> {w: status}


def _load(ctx, blob, h, w, max_batch):
    return L.lib().covahip_blobnet_load(ctx.handle, blob, len(blob), h, w, 4, max_batch)


def _probe(ctx, h, max_batch, widths):
    """{w: status of covahip_blobnet_load(h, w, max_batch)}, remembered for the session."""
    st = _accepted.setdefault((h, max_batch), {})
    blob = None
    for w in widths:
        if w not in st:
            blob = blob or W.to_bytes(W.random_init(1234))
            st[w] = _load(ctx, blob, h, w, max_batch)
    return {w: st[w] for w in widths}


ALL_WIDTHS = tuple(range(16, 1025, 4))


def _w_max(ctx, h):
    """The widest multiple of 4 that loads at height h: every width from 1024 downwards until one loads."""
    for w in reversed(ALL_WIDTHS):
        if _probe(ctx, h, 1, (w,))[w] == OK:
            return w
    raise AssertionError(f"no width loads at h_mb = {h}")


# (h, w, batch, impl, weights, entry, the kernels that launch beside enc0p_mfma and enc1_mfma -- as the first run on MI355X showed
# them: the profile must show exactly these, so a planner change that reroutes an edge shape fails here).  Level 1 runs under the
# profile name enc1_mfma on either kernel; past BN_E1_MAXW = 62 level-1 columns (the Wmax cases) it is the round-1..3 kernel, which
# writes the level-0 skip tensor act[1] instead of the partial logits, and stage_check.run checks that tensor then.
CC = {"bboxcc_kernel"}            # the carrier-frame entry's bboxcc as a launch of its own, where the fused tail does not fit
CC_BIG = {"bboxcc_big_kernel"}    # ... and with its state in global memory
CASES = [
    # every level at its minimum: 16 -> 8 -> 4 -> 2 -> 1, Hp3 = Wp3 = 1, decoder block 0 starts from a 1x1 tensor
    (16, 16, 3, "mfma", "seed", "stack", ENC2_3 | DEC012 | TAIL),
    (16, 16, 3, "mfma", "mixed", "frames", ENC2_3 | DEC012 | TAIL_CC),
    (16, 16, 3, "dec_separate", "smallvar", "frames", ENC2_3 | DEC0_2 | TAIL_CC),
    (16, 16, 3, "enc1_legacy", "mixed", "stack", ENC2_3 | DEC012 | TAIL),
    # odd at every level on both axes: 17 -> 9 -> 5 -> 3 -> 2, 20 -> 10 -> 5 -> 3 -> 2
    (17, 20, 3, "mfma", "mixed", "frames", ENC2_3 | DEC012 | TAIL_CC),
    (17, 20, 3, "dec_separate", "seed", "frames", ENC2_3 | DEC0_2 | TAIL_CC),
    (17, 20, 3, "enc1_legacy", "smallvar", "frames", ENC2_3 | DEC012 | TAIL_CC),
    # 33 -> 17 -> 9 -> 5 -> 3: odd height at every level with more than one window row
    (33, 36, 3, "mfma", "smallvar", "stack", ENC2_3 | DEC012 | TAIL),
    (33, 36, 3, "dec_separate", "mixed", "stack", ENC2_3 | DEC0_2 | TAIL),
    (33, 36, 3, "enc1_legacy", "seed", "stack", ENC2_3 | DEC012 | TAIL),
    # the widest admitted grid with one band per level (the fused decoder and the fused tail still fit at 16 rows)
    (16, WMAX, 2, "mfma", "seed", "frames", ENC2_3 | DEC012 | TAIL_CC),
    (16, WMAX, 2, "dec_separate", "mixed", "frames", ENC2_3 | DEC0_2 | TAIL_CC),
    # the tallest grid: the largest band counts on the narrowest row; 20: odd level-2 width.  The fused decoder and the fused
    # tail of the default chain do not fit 1024 rows, so the default chain is already the one of "dec_separate"
    (1024, 16, 1, "mfma", "mixed", "stack", ENC2_3 | DEC0_2 | TAIL),
    (1024, 20, 1, "mfma", "smallvar", "frames", ENC2_3 | DEC0_2 | TAIL | CC),
    # (without the partial logits beside the mask the fused tail fits even 1024 rows: its band form, 1024 rows of mask in LDS)
    (1024, 20, 1, "enc1_legacy", "seed", "frames", ENC2_3 | DEC0_2 | TAIL_CC),
    # large on both axes: the largest divisor operands the kernels see (level 1: 75 bands of 126 columns)
    (300, WMAX, 1, "mfma", "seed", "frames", ENC2_3 | DEC0_2 | TAIL | CC_BIG),
]


def _id(c):
    return f"{c[0]}x{c[1]}-b{c[2]}-{c[3]}-{c[4]}-{c[5]}"


@pytest.mark.parametrize("h,w,b,impl,wname,entry,kernels", CASES, ids=[_id(c) for c in CASES])
def test_stages_at_edge_shapes(ctx, h, w, b, impl, wname, entry, kernels):
    if w == WMAX:
        w = _w_max(ctx, h)
        assert w > 2 * 62, w    # level 1 past BN_E1_MAXW
    stage_check.run(ctx, h, w, b, impl, wname, entry, kernels, set(), _RATIOS, exact=True)


@pytest.mark.parametrize("h", [16, 17, 135, 1024])
def test_admitted_widths_probed_at_load(ctx, h):
    """Loads only.  A refused load takes milliseconds whatever the grid; the first load of an accepted grid runs the host-side
    swizzle search of every level (choose_swz), 20 ms at 16 rows but 0.2 - 5 s per width at 135 and 1024 rows.  So:
    heights 16 and 17: every multiple of 4 from 16 to 1024 with max_batch 1; with max_batch 64 every multiple of 4 within 32 of
    the edge and every 32nd elsewhere.  Heights 135 and 1024: every multiple of 4 above the edge (all refused), the edge, and of
    the accepted widths below it 16 (and 128 and the two next to the edge at 135 rows); the same with max_batch 64.  No planner's
    fit of a one-row band depends on the height, which is why the interval is swept in full at the two small heights only."""
    blob = W.to_bytes(W.random_init(1234))
    lib = L.lib()
    edge = _w_max(ctx, h)
    if h < 100:
        widths = ALL_WIDTHS
        widths64 = tuple(w for w in ALL_WIDTHS if abs(w - edge) <= 32 or w % 32 == 16 or w == 1024)
    else:
        below = (16, 128, edge - 8, edge - 4) if h == 135 else (16,)
        widths = widths64 = tuple(sorted(set(below) | set(range(edge, 1025, 4))))
    st = _probe(ctx, h, 1, widths)
    bad = {w: rc for w, rc in st.items() if rc not in (OK, ERR_UNSUPPORTED)}
    assert not bad, (h, bad)                                          # never COVAHIP_ERR_HIP
    ok = [w for w in widths if st[w] == OK]
    print(f"\nh_mb = {h}: widths 16 .. {edge} load ({len(ok)} of the {len(widths)} probed)")
    assert ok == [w for w in widths if w <= edge], (h, ok)            # one interval that starts at 16
    assert edge == WIDTH_EDGE, (h, edge)
    st64 = _probe(ctx, h, 64, widths64)
    assert st64 == {w: st[w] for w in widths64}, (h, {w: (st[w], st64[w]) for w in widths64 if st[w] != st64[w]})
    # a refused load leaves the ctx without a model
    stack = synth.stacked_batch(1, 16, 16, seed=1)
    mask = np.zeros((1, 16, 16), np.uint8)
    assert _load(ctx, blob, 16, 16, 1) == OK
    assert lib.covahip_blobnet_forward(ctx.handle, stack.ctypes.data, 1, None, mask.ctypes.data, L.MEM_HOST) == OK
    assert _load(ctx, blob, h, edge + 4, 1) == ERR_UNSUPPORTED
    assert lib.covahip_blobnet_forward(ctx.handle, stack.ctypes.data, 1, None, mask.ctypes.data, L.MEM_HOST) == ERR_NOT_LOADED


BATCHES = (1, 2, 3, 5, 17, 33, 63, 64)
MAXB = 64
# (h, w, lanes)
BATCH_CASES = [(16, 16, 1), (17, 20, 1), (16, WMAX, 1), (1024, 16, 1), (135, 240, 1), (17, 20, 3), (16, WMAX, 3)]


def _frames_of(frames, index, b):
    """The carrier frames that stacks 0 .. b-1 use, shuffled, and their table."""
    used = np.unique(index[:b])
    used = used[np.random.default_rng(b).permutation(len(used))]
    where = np.full(len(frames), -1, np.int32)
    where[used] = np.arange(len(used), dtype=np.int32)
    return np.ascontiguousarray(frames[used]), np.ascontiguousarray(where[index[:b]])


@pytest.mark.parametrize("h,w,lanes", BATCH_CASES, ids=[f"{c[0]}x{c[1]}-lanes{c[2]}" for c in BATCH_CASES])
def test_every_batch_runs_and_agrees_with_batch_1(ctx, h, w, lanes):
    """One lane: host pointers (synchronous calls).  Three lanes: device pointers, so that consecutive filter calls of different
    batches overlap on the lanes' own workspaces; every call writes buffers of its own and one sync ends the run."""
    if w == WMAX:
        w = _w_max(ctx, h)
    lib = L.lib()
    if ctx.lanes() != 1:
        ctx.set_lanes(1)
    BlobNetInfer(ctx, W.random_init(1234), h, w, max_batch=MAXB)
    stacks = synth.stacked_batch(MAXB, h, w, seed=21, streams=4)
    frames, index = synth.carrier_batch(MAXB, h, w, seed=21, streams=4)
    hw = h * w
    want = np.empty((MAXB, h, w), np.float32)    # every stack alone: batch 1
    for i in range(MAXB):
        one = np.ascontiguousarray(stacks[i:i + 1])
        assert lib.covahip_blobnet_forward(ctx.handle, one.ctypes.data, 1, want[i:i + 1].ctypes.data, None, L.MEM_HOST) == OK, i
    assert np.isfinite(want).all() and want.std() > 0
    mb = 64
    got = {}     # (entry, batch) -> logits
    if lanes == 1:
        for b in BATCHES:
            fr, tab = _frames_of(frames, index, b)
            boxes = np.zeros((b, mb), dtype=L.BOX_DTYPE)
            counts = np.zeros(b, np.int32)
            for entry in ("forward", "filter", "frames"):
                lg = np.full((b, h, w), np.nan, np.float32)
                if entry == "forward":
                    rc = lib.covahip_blobnet_forward(ctx.handle, stacks.ctypes.data, b, lg.ctypes.data, None, L.MEM_HOST)
                elif entry == "filter":
                    rc = lib.covahip_filter_forward(ctx.handle, stacks.ctypes.data, b, 2, boxes.ctypes.data, counts.ctypes.data, mb,
                                                    lg.ctypes.data, None, L.MEM_HOST)
                else:
                    rc = lib.covahip_filter_forward_frames(ctx.handle, fr.ctypes.data, len(fr), tab.ctypes.data, b, 2, boxes.ctypes.data,
                                                           counts.ctypes.data, mb, lg.ctypes.data, None, L.MEM_HOST)
                assert rc == OK, (entry, b, rc)    # (no admitted grid is wider than bboxcc's 256: no refusal applies)
                got[entry, b] = lg
    else:
        held = []

        def dev(nbytes, src=None):
            p = ctx.malloc(nbytes)
            held.append(p)
            if src is not None:
                ctx.h2d(p, src)
            return p

        try:
            d_stacks = dev(stacks.nbytes, stacks)
            calls = []
            for b in BATCHES:
                fr, tab = _frames_of(frames, index, b)
                calls.append((b, fr, tab, dev(fr.nbytes, fr), [dev(b * hw * 4) for _ in range(2)],
                              [dev(b * mb * 20) for _ in range(2)], [dev(b * 4) for _ in range(2)]))
            ctx.set_lanes(lanes)
            for b, fr, tab, d_fr, d_lg, d_boxes, d_counts in calls:
                rc = lib.covahip_filter_forward(ctx.handle, d_stacks, b, 2, d_boxes[0], d_counts[0], mb, d_lg[0], None, L.MEM_DEVICE)
                assert rc == OK, ("filter", b, rc)
                rc = lib.covahip_filter_forward_frames(ctx.handle, d_fr, len(fr), tab.ctypes.data, b, 2, d_boxes[1], d_counts[1], mb, d_lg[1],
                                                       None, L.MEM_DEVICE)
                assert rc == OK, ("frames", b, rc)
            ctx.sync()
            for b, fr, tab, d_fr, d_lg, d_boxes, d_counts in calls:
                for entry, p in zip(("filter", "frames"), d_lg):
                    got[entry, b] = np.empty((b, h, w), np.float32)
                    ctx.d2h(got[entry, b], p)
        finally:
            ctx.sync()
            ctx.set_lanes(1)
            for p in held:
                ctx.free(p)
    for (entry, b), lg in got.items():
        np.testing.assert_array_equal(lg, want[:b], err_msg=f"{h}x{w} {entry} batch {b}")
