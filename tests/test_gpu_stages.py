"""Every kernel stage of the HIP BlobNet path against its float64 reference (tests/blobnet_stages.py), on the kernel's own input.

The oracle test of the whole network (tests/test_gpu_blobnet.py) spends most of its tolerance on legitimate fp16 noise and lets
a kernel that drops a 3x3 tap of a level-2 channel pass; a check per stage is about 30x more sensitive.  After each forward the
workspace is read back (include/covahip_dev.h, covahip_dev_blobnet_buffer) and every stage output is checked with
|hip - ref| <= K * u * (rms(ref) + |ref|), u = 2^-11, 2K for the stages that span two levels (blobnet_stages.K).

K = 16 (2K = 32 for E1 / E23 / D012).  Worst ratio |hip - ref| / (u * (rms(ref) + |ref|)) per stage over this module's cases on
MI355X: E0 4.69, E1 9.87, E2 3.98, E3 4.08, E23 8.38, D0 3.75, D1 3.03, D2 2.30, D012 8.18, T 1.59 -- at least 3.2x below the
bound; the fp16 emulation of tests/test_stage_bounds.py reaches 2.3 - 4.4 (9.8 fused), its planted bugs 148 and more.
"""
import json
import os
import re

import numpy as np
import pytest

from cova_amd import synth, weights as W
from cova_amd.elements import BlobNetInfer
from oracle import ref
from tests import blobnet_stages as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AREA, MAX_BOXES = 2, 2048


_WEIGHTS = {"seed": lambda: W.random_init(1234), "mixed": lambda: S.mixed_gamma_weights(77), "smallvar": lambda: S.small_var_weights(5)}

ENC23 = {"enc23_mfma"}
ENC2_3 = {"enc2_mfma", "enc3_mfma"}
DEC012 = {"dec012_mfma"}
DEC0_2 = {"dec0_mfma", "dec1_mfma", "dec2_mfma"}
ALWAYS = {"enc0p_mfma", "enc1_mfma"}

# (h, w, batch, impl, weights, entry, kernels that must launch, kernels that must not).  entry "stack": the stacked tensor through
# covahip_blobnet_forward (unfused tail); "frames": carrier frames with a shuffled stack table through covahip_filter_forward_frames
# (fused tail where it fits).  Every stage is checked at every shape; the sets pin the path of each case.
CASES = [
    (68, 120, 20, "mfma", "seed", "stack", ENC2_3 | DEC012 | {"dec3_final_mfma"}, ENC23),
    (68, 120, 256, "mfma", "seed", "frames", ENC23 | DEC012 | {"dec3_bboxcc_fused"}, ENC2_3),
    (68, 120, 256, "mfma", "smallvar", "stack", ENC23, ENC2_3),
    (67, 120, 16, "mfma", "seed", "stack", {"dec3_final_mfma"}, set()),
    (67, 120, 16, "mfma", "mixed", "frames", {"dec3_bboxcc_fused"}, set()),
    (45, 80, 8, "mfma", "seed", "frames", {"dec3_bboxcc_fused"}, set()),
    (35, 60, 8, "mfma", "mixed", "stack", set(), set()),
    (61, 100, 8, "mfma", "seed", "frames", set(), set()),
    (66, 116, 8, "mfma", "smallvar", "frames", set(), set()),
    (36, 64, 8, "mfma", "seed", "stack", set(), set()),
    (24, 32, 8, "mfma", "seed", "frames", set(), set()),
    (128, 120, 4, "mfma", "seed", "frames", set(), set()),
    (124, 124, 4, "mfma", "mixed", "stack", set(), set()),
    (128, 128, 4, "mfma", "seed", "frames", set(), set()),
    (135, 240, 2, "mfma", "seed", "frames", DEC0_2 | {"dec3_final_mfma"}, DEC012 | {"dec3_bboxcc_fused"}),
    (68, 120, 20, "dec_separate", "mixed", "frames", DEC0_2, DEC012),
    (35, 60, 8, "dec_separate", "smallvar", "stack", DEC0_2, DEC012),
    (67, 120, 16, "enc1_legacy", "seed", "frames", set(), set()),
    (35, 60, 8, "enc1_legacy", "mixed", "stack", set(), set()),
    (68, 120, 20, "enc_general_tiles", "mixed", "stack", ENC2_3, ENC23),
    (45, 80, 8, "enc_general_tiles", "seed", "frames", ENC2_3, ENC23),
    (68, 120, 20, "enc23_force", "mixed", "frames", ENC23, ENC2_3),
    (67, 120, 16, "enc23_force", "smallvar", "stack", ENC23, ENC2_3),
    (68, 120, 256, "enc23_separate", "seed", "frames", ENC2_3, ENC23),
    (68, 120, 20, "tail_skip_tensor", "mixed", "frames", {"dec3_bboxcc_fused"}, set()),
    (67, 120, 16, "tail_skip_tensor", "seed", "stack", {"dec3_final_mfma"}, set()),
    (68, 120, 20, "tail_band_tiles", "seed", "frames", {"dec3_bboxcc_fused"}, set()),
]

_RATIOS = {}   # stage -> worst ratio over the module (printed at the end for the record in the docstring)


PROF_SCOPES = {"enc0p_mfma", "enc1_mfma", "enc2_mfma", "enc3_mfma", "enc23_mfma", "dec012_mfma", "dec0_mfma", "dec1_mfma", "dec2_mfma",
               "dec3_final_mfma", "dec3_bboxcc_fused"}


def _prof_scopes():
    """The profile names blobnet_mfma.hip launches under: the second argument of its launch helper."""
    src = open(os.path.join(ROOT, "cova_amd", "csrc", "blobnet_mfma.hip")).read()
    return set(re.findall(r'\blaunch\(f, "([a-z0-9_]+)"', src))


def test_cases_cover_every_profile_scope():
    """Across the module every kernel of blobnet_mfma.hip's ProfScopes is REQUIRED to launch by some case."""
    assert _prof_scopes() == PROF_SCOPES, sorted(_prof_scopes() ^ PROF_SCOPES)   # (an extraction that finds nothing proves nothing)
    must = ALWAYS.union(*(c[6] for c in CASES))
    assert _prof_scopes() <= must, sorted(_prof_scopes() - must)


def _sel(b):
    """Stacks whose references are computed (all of a small batch; first, middle and last ones of a large one)."""
    return np.arange(b) if b <= 24 else np.unique(np.r_[0:4, b // 2 - 2:b // 2 + 2, b - 4:b])


def _record(case, stage, r, k, what):
    case[stage] = max(case.get(stage, 0.0), r)
    _RATIOS[stage] = max(_RATIOS.get(stage, 0.0), r)
    assert r <= S.stage_k(stage, k), f"{what}: stage {stage} worst ratio {r:.3g} > {S.stage_k(stage, k)}"


@pytest.mark.parametrize("h,w,b,impl,wname,entry,must,mustnot", CASES,
                         ids=[f"{c[0]}x{c[1]}-b{c[2]}-{c[3]}-{c[4]}-{c[5]}" for c in CASES])
def test_stages_against_float64(ctx, h, w, b, impl, wname, entry, must, mustnot):
    if ctx.lanes() != 1:
        ctx.set_lanes(1)     # the read-back shows lane 0's workspace
    flat = _WEIGHTS[wname]()
    wt = S.weights(flat)
    lv = S.geometry(h, w)
    net = BlobNetInfer(ctx, flat, h, w, max_batch=b)
    net.set_impl(impl)
    what = f"{h}x{w} b={b} {impl} {wname} {entry}"
    streams = 3 if b > 2 else 1   # (streams * (ceil(b / streams) + 3) carrier frames must fit the 4 * max_batch of P)

    # stale-buffer guard: a forward on another input first, so that a buffer the measured forward does not rewrite fails its stage
    if entry == "stack":
        net.infer(synth.stacked_batch(b, h, w, seed=901, streams=streams))
        stack = synth.stacked_batch(b, h, w, seed=11, streams=streams)
        frames = stack.reshape(b, 4, h, w, 4).reshape(b * 4, h, w, 4)
        table = np.arange(4 * b, dtype=np.int32).reshape(b, 4)
        ctx.profile(True)
        logits, mask = net.infer(stack)
        boxes = counts = None
    else:
        gf, gi = synth.carrier_batch(b, h, w, seed=902, streams=streams)
        net.filter_frames(gf, gi, AREA, max_boxes=MAX_BOXES, want_mask=True, want_logits=True)
        frames, table = synth.carrier_batch(b, h, w, seed=12, streams=streams)
        table = table[np.random.default_rng(b).permutation(b)]
        ctx.profile(True)
        boxes, counts, mask, logits = net.filter_frames(frames, table, AREA, max_boxes=MAX_BOXES, want_mask=True, want_logits=True)
    prof = ctx.profile_read()
    ctx.profile(False)
    launched = {k for k, (_, n) in prof.items() if n > 0}
    print(f"\n{what}: {sorted(launched)}")
    assert must <= launched and not (mustnot & launched), (what, sorted(launched))
    assert ALWAYS <= launched
    assert len(launched & ENC23) + (ENC2_3 <= launched) == 1 and len(launched & DEC012) + (DEC0_2 <= launched) == 1
    assert len(launched & {"dec3_final_mfma", "dec3_bboxcc_fused"}) == 1

    rd = {"P": net.read_buffer(0), "part": net.read_buffer(3)}
    for i in range(1, 5):
        rd[f"act{i}"] = net.read_buffer(1, i)
    for j in range(3):
        rd[f"dact{j}"] = net.read_buffer(2, j)
    sel = _sel(b)
    tsel = table[sel]
    fsel = np.unique(tsel)
    k = S.K
    cw = {}   # this case's worst ratio per stage

    # E0: the carrier frames the checked stacks use
    P = rd["P"][:len(frames)].astype(np.float64)
    ref0 = S.e0(frames[fsel], wt)
    assert S.pad_zero(P[fsel], lv[0]), what
    _record(cw, "E0", S.worst(P[fsel], ref0), k, what)
    # E1 on the HIP path's P, gathered by the (shuffled) table
    r1 = S.e1(P, tsel, wt)
    a2 = rd["act2"][sel].astype(np.float64)
    assert S.pad_zero(a2, lv[1]), what
    _record(cw, "E1", S.worst(a2, r1["act2"]), k, what)
    part_on = impl not in ("tail_skip_tensor", "enc1_legacy") and lv[1][1] <= 62
    if part_on:
        _record(cw, "E1", S.worst(rd["part"][sel], r1["part"]), k, what + " part")
    else:
        a1 = rd["act1"][sel, 0].astype(np.float64)
        assert S.pad_zero(a1, lv[0]), what
        _record(cw, "E1", S.worst(a1, r1["act1"]), k, what + " act1")
    # encoder levels 2 + 3
    a3 = rd["act3"][sel].astype(np.float64)
    a4 = rd["act4"][sel].astype(np.float64)
    assert S.pad_zero(a4, lv[3]), what
    if "enc23_mfma" in launched:
        r3 = S.enc(a2, wt, 2)
        assert S.pad_zero(a3[:, 0], lv[2]), what
        _record(cw, "E23", S.worst(a3[:, 0], r3[:, 0]), k, what + " act3 t=0")
        _record(cw, "E23", S.worst(a4, S.enc(r3, wt, 3)), k, what)
    else:
        assert S.pad_zero(a3, lv[2]), what
        _record(cw, "E2", S.worst(a3, S.enc(a2, wt, 2)), k, what)
        _record(cw, "E3", S.worst(a4, S.enc(a3, wt, 3)), k, what)
    # decoder blocks 0..2
    d2 = rd["dact2"][sel].astype(np.float64)
    if "dec012_mfma" in launched:
        x0 = S.dec(None, a4, wt, 0, lv[3])
        x1 = S.dec(x0, a3, wt, 1, lv[2])
        _record(cw, "D012", S.worst(d2, S.dec(x1, a2, wt, 2, lv[1])), k, what)
    else:
        d0 = rd["dact0"][sel].astype(np.float64)
        d1 = rd["dact1"][sel].astype(np.float64)
        _record(cw, "D0", S.worst(d0, S.dec(None, a4, wt, 0, lv[3])), k, what)
        _record(cw, "D1", S.worst(d1, S.dec(d0, a3, wt, 1, lv[2])), k, what)
        _record(cw, "D2", S.worst(d2, S.dec(d1, a2, wt, 2, lv[1])), k, what)
    # the tail: fp32 logits, the mask, the boxes of that mask
    if part_on:
        rl = S.tail(d2, wt, lv[0], part=rd["part"][sel])
    else:
        rl = S.tail(d2, wt, lv[0], act1=rd["act1"][sel])
    lg = logits[sel].astype(np.float64)
    _record(cw, "T", S.worst(lg, rl), k, what)
    np.testing.assert_array_equal(mask, (logits > 0).astype(np.uint8), err_msg=what)
    rms = float(np.sqrt(np.mean(np.square(rl))))
    off = (mask[sel] != (rl > 0)) & (np.abs(rl) > k * S.U * (rms + np.abs(rl)))
    assert not off.any(), f"{what}: mask differs from ref > 0 beyond the bound at {np.argwhere(off)[:5].tolist()}"
    if boxes is not None:
        rb, rc = ref.regionprops_batch(mask, AREA, MAX_BOXES)
        np.testing.assert_array_equal(counts, rc, err_msg=what)
        for i in range(b):
            n = int(counts[i])
            for f, g in (("left", "left"), ("top", "top"), ("width", "width"), ("height", "height"), ("area_px", "area")):
                np.testing.assert_array_equal(boxes[i, :n][f], rb[i, :n][g], err_msg=what)
    print("STAGE_RATIOS " + json.dumps({"case": what, "kernels": sorted(launched), "worst": {s: round(v, 3) for s, v in cw.items()},
                                         "module_worst": {s: round(v, 3) for s, v in _RATIOS.items()}}))
