"""The per-stage check of a HIP BlobNet forward against tests/blobnet_stages.py (test helper; the GPU modules call run()).

One call loads a geometry, runs a forward on another input first (the stale-buffer guard), runs the measured forward under the
profile, reads lane 0's workspace back (include/covahip_dev.h, covahip_dev_blobnet_buffer) and checks every stage output on the
kernel's own input with |hip - ref| <= K * u * (rms(ref) + |ref|) (blobnet_stages.K, 2K for the stages that span two levels):
E0, E1 and the `part` / act[1] skip, E2 / E3 or E23, D0 .. D2 or D012, T, the pad rows and columns, mask == (logits > 0), the mask
against ref > 0 outside the bound, and the boxes of the fused entry against oracle.ref.regionprops_batch.
"""
import json

import numpy as np

from cova_amd import synth, weights as W
from cova_amd.elements import BlobNetInfer
from oracle import ref
from tests import blobnet_stages as S

AREA, MAX_BOXES = 2, 2048

WEIGHTS = {"seed": lambda: W.random_init(1234), "mixed": lambda: S.mixed_gamma_weights(77), "smallvar": lambda: S.small_var_weights(5)}

ENC23 = {"enc23_mfma"}
ENC2_3 = {"enc2_mfma", "enc3_mfma"}
DEC012 = {"dec012_mfma"}
DEC0_2 = {"dec0_mfma", "dec1_mfma", "dec2_mfma"}
ALWAYS = {"enc0p_mfma", "enc1_mfma"}
TAIL = {"dec3_final_mfma"}
TAIL_CC = {"dec3_bboxcc_fused"}


def picked(b):
    """Stacks whose references are computed (all of a small batch; first, middle and last ones of a large one)."""
    return np.arange(b) if b <= 24 else np.unique(np.r_[0:4, b // 2 - 2:b // 2 + 2, b - 4:b])


def _record(ratios, case, stage, r, k, what):
    case[stage] = max(case.get(stage, 0.0), r)
    ratios[stage] = max(ratios.get(stage, 0.0), r)
    assert r <= S.stage_k(stage, k), f"{what}: stage {stage} worst ratio {r:.3g} > {S.stage_k(stage, k)}"


def run(ctx, h, w, b, impl, wname, entry, must, mustnot, ratios, exact=False):
    """The whole comparison of one case.  entry "stack": the stacked tensor through covahip_blobnet_forward (unfused tail);
    "frames": carrier frames with a shuffled stack table through covahip_filter_forward_frames (fused tail where it fits).
    must / mustnot: kernels that have to / must not launch (exact: `must` plus ALWAYS is the whole set that launched).
    ratios: the calling module's worst ratio per stage, updated.  Returns (this case's worst ratios, the kernels that launched)."""
    _record_ = lambda *a: _record(ratios, *a)   # noqa: E731
    if ctx.lanes() != 1:
        ctx.set_lanes(1)     # the read-back shows lane 0's workspace
    flat = WEIGHTS[wname]()
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
    assert not exact or launched == must | ALWAYS, (what, sorted(launched))
    assert len(launched & ENC23) + (ENC2_3 <= launched) == 1 and len(launched & DEC012) + (DEC0_2 <= launched) == 1
    assert len(launched & {"dec3_final_mfma", "dec3_bboxcc_fused"}) == 1

    rd = {"P": net.read_buffer(0), "part": net.read_buffer(3)}
    for i in range(1, 5):
        rd[f"act{i}"] = net.read_buffer(1, i)
    for j in range(3):
        rd[f"dact{j}"] = net.read_buffer(2, j)
    sel = picked(b)
    tsel = table[sel]
    fsel = np.unique(tsel)
    k = S.K
    cw = {}   # this case's worst ratio per stage

    # E0: the carrier frames the checked stacks use
    P = rd["P"][:len(frames)].astype(np.float64)
    ref0 = S.e0(frames[fsel], wt)
    assert S.pad_zero(P[fsel], lv[0]), what
    _record_(cw, "E0", S.worst(P[fsel], ref0), k, what)
    # E1 on the HIP path's P, gathered by the (shuffled) table
    r1 = S.e1(P, tsel, wt)
    a2 = rd["act2"][sel].astype(np.float64)
    assert S.pad_zero(a2, lv[1]), what
    _record_(cw, "E1", S.worst(a2, r1["act2"]), k, what)
    part_on = impl not in ("tail_skip_tensor", "enc1_legacy") and lv[1][1] <= 62
    if part_on:
        _record_(cw, "E1", S.worst(rd["part"][sel], r1["part"]), k, what + " part")
    else:
        a1 = rd["act1"][sel, 0].astype(np.float64)
        assert S.pad_zero(a1, lv[0]), what
        _record_(cw, "E1", S.worst(a1, r1["act1"]), k, what + " act1")
    # encoder levels 2 + 3
    a3 = rd["act3"][sel].astype(np.float64)
    a4 = rd["act4"][sel].astype(np.float64)
    assert S.pad_zero(a4, lv[3]), what
    if "enc23_mfma" in launched:
        r3 = S.enc(a2, wt, 2)
        assert S.pad_zero(a3[:, 0], lv[2]), what
        _record_(cw, "E23", S.worst(a3[:, 0], r3[:, 0]), k, what + " act3 t=0")
        _record_(cw, "E23", S.worst(a4, S.enc(r3, wt, 3)), k, what)
    else:
        assert S.pad_zero(a3, lv[2]), what
        _record_(cw, "E2", S.worst(a3, S.enc(a2, wt, 2)), k, what)
        _record_(cw, "E3", S.worst(a4, S.enc(a3, wt, 3)), k, what)
    # decoder blocks 0..2
    d2 = rd["dact2"][sel].astype(np.float64)
    if "dec012_mfma" in launched:
        x0 = S.dec(None, a4, wt, 0, lv[3])
        x1 = S.dec(x0, a3, wt, 1, lv[2])
        _record_(cw, "D012", S.worst(d2, S.dec(x1, a2, wt, 2, lv[1])), k, what)
    else:
        d0 = rd["dact0"][sel].astype(np.float64)
        d1 = rd["dact1"][sel].astype(np.float64)
        _record_(cw, "D0", S.worst(d0, S.dec(None, a4, wt, 0, lv[3])), k, what)
        _record_(cw, "D1", S.worst(d1, S.dec(d0, a3, wt, 1, lv[2])), k, what)
        _record_(cw, "D2", S.worst(d2, S.dec(d1, a2, wt, 2, lv[1])), k, what)
    # the tail: fp32 logits, the mask, the boxes of that mask
    if part_on:
        rl = S.tail(d2, wt, lv[0], part=rd["part"][sel])
    else:
        rl = S.tail(d2, wt, lv[0], act1=rd["act1"][sel])
    lg = logits[sel].astype(np.float64)
    _record_(cw, "T", S.worst(lg, rl), k, what)
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
    print("STAGEratios " + json.dumps({"case": what, "kernels": sorted(launched), "worst": {s: round(v, 3) for s, v in cw.items()},
                                         "module_worst": {s: round(v, 3) for s, v in ratios.items()}}))
    return cw, launched
