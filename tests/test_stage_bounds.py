"""The per-stage bound of tests/blobnet_stages.py is neither vacuous nor too tight (CPU, float64 torch, no GPU).

Every stage is fed the float64 network's checkpoint of its input rounded to fp16 (what a kernel reads) and compared with its
float64 reference on that input:
  (a) an fp16 emulation of the stage -- weights, stage input, post-BN pre-pool value, tmix operands and output rounded to fp16 --
      passes at the committed K with at least a 3x margin;
  (b) every planted bug fails at the committed K by at least 3x, at every shape below: a missing 3x3 tap of one output channel in
      every encoder level and decoder block, a pad row / column on the wrong side, a crop offset off by one in each odd-size
      decoder block, a level-0 / level-1 tmix row zeroed, a decoder skip dropped, BN eps = 1e-5 (on the weights with BN
      variances of 1e-3 .. 1e-2, where eps is not lost in the variance).  Mutations that are inert at a shape are left out.

Shapes: 67x120 and 35x60, and the smallest and all-odd grids of tests/test_gpu_geometry_edges.py -- 16x16 (level sizes 16 -> 8 -> 4 ->
2 -> 1: act4 is 1x1x128 per stack, so rms(ref) of E3 / E23 is taken over 384 values), 17x20 (odd at every level on both axes) and
33x36.  The bound holds there with the same margins: the emulation reaches at most 0.95 of K / 3 (E3 at 17x20, negative gammas), and
the weakest planted bug (the missing tap of the last block at 17x20) is at 221 against 3K = 48.  No stage is left out at any shape.
"""
import numpy as np
import pytest
import torch

from cova_amd import synth, weights as W
from tests import blobnet_stages as S

SHAPES = [(67, 120), (35, 60), (16, 16), (17, 20), (33, 36)]
MARGIN = 3.0
_WEIGHTS = {"seed": lambda: W.random_init(1234), "mixed": lambda: S.mixed_gamma_weights(77), "smallvar": lambda: S.small_var_weights(5)}
_cache = {}


def _case(hw, wname):
    """(fp16-rounded stage inputs, exact float64 weights, level geometry) of the float64 network on synth.stacked_batch(3, ...)."""
    key = (hw, wname)
    if key not in _cache:
        flat = _WEIGHTS[wname]()
        c = S.checkpoints(flat, synth.stacked_batch(3, *hw, seed=11), *hw)
        c16 = dict(c)
        for k in ("P", "act1", "act2", "act3", "act4", "dact0", "dact1", "dact2"):
            c16[k] = _r16(c[k])
        c16["part"] = c["part"].astype(np.float32).astype(np.float64)
        _cache[key] = (c16, S.weights(flat), S.geometry(*hw))
    return _cache[key]


def _r16(a):
    return np.asarray(a).astype(np.float16).astype(np.float64)


def _stage(st, c, wt, lv, q=None, **mut):
    """Outputs of stage `st` on the rounded inputs c: a list of arrays (fp16 emulation when q is given)."""
    kw = {} if q is None else {"q": q}
    out = lambda a: _r16(a) if q is not None else a      # noqa: E731  (the kernels store fp16)
    if st == "E0":
        return [out(S.e0(c["frames"], wt, **kw, **mut))]
    if st == "E1":
        r = S.e1(c["P"], c["table"], wt, **kw, **mut)
        return [out(r["act2"]), r["part"]]
    if st == "E2":
        return [out(S.enc(c["act2"], wt, 2, **kw, **mut))]
    if st == "E3":
        return [out(S.enc(c["act3"], wt, 3, **kw, **mut))]
    if st == "E23":
        a3 = out(S.enc(c["act2"], wt, 2, **kw))
        return [a3[:, 0], out(S.enc(a3, wt, 3, **kw))]
    if st == "D0":
        return [out(S.dec(None, c["act4"], wt, 0, lv[3], **kw, **mut))]
    if st == "D1":
        return [out(S.dec(c["dact0"], c["act3"], wt, 1, lv[2], **kw, **mut))]
    if st == "D2":
        return [out(S.dec(c["dact1"], c["act2"], wt, 2, lv[1], **kw, **mut))]
    if st == "D012":
        x0 = out(S.dec(None, c["act4"], wt, 0, lv[3], **kw))
        x1 = out(S.dec(x0, c["act3"], wt, 1, lv[2], **kw))
        return [out(S.dec(x1, c["act2"], wt, 2, lv[1], **kw))]
    if st == "T":
        return [S.tail(c["dact2"], wt, lv[0], part=c["part"], **kw, **mut)]
    raise AssertionError(st)


def _worst(st, c, wt_ref, wt_cand, lv, q=None, **mut):
    ref = _stage(st, c, wt_ref, lv)
    cand = _stage(st, c, wt_cand, lv, q=q, **mut)
    return max(S.worst(h, r) for h, r in zip(cand, ref))


def _fp16_weights(wt):
    rounded = ("conv.kernel", "up.kernel", "tmix.w1", "tmix.w2", "final.kernel")
    return {k: (S.round16(v) if k.endswith(rounded) else v) for k, v in wt.items()}


STAGES = ["E0", "E1", "E2", "E3", "E23", "D0", "D1", "D2", "D012", "T"]


@pytest.mark.parametrize("wname", ["seed", "mixed", "smallvar"])
@pytest.mark.parametrize("hw", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
@pytest.mark.parametrize("st", STAGES)
def test_fp16_emulation_passes_with_margin(st, hw, wname):
    c, wt, lv = _case(hw, wname)
    r = _worst(st, c, wt, _fp16_weights(wt), lv, q=S.round16)
    assert r * MARGIN <= S.stage_k(st), f"{st} {hw} {wname}: fp16 emulation at {r:.3g} of u * (rms + |ref|), bound {S.stage_k(st)}"


def _zero_tap(wt, name, c, enc):
    wt = dict(wt)
    k = wt[name].clone()
    if enc:
        k[1, 1, :, c] = 0       # [3,3,Cin,Cout]: centre tap of output channel c, all inputs
    else:
        k[1, 1, c, :] = 0       # [4,4,Cout,Cin]
    wt[name] = k
    return wt


def _zero_row(wt, name):
    wt = dict(wt)
    k = wt[name].clone()
    k[0] = 0
    wt[name] = k
    return wt


def _busiest(a):
    """Output channel with the largest RMS (a dead channel would make a missing tap inert)."""
    a = np.asarray(a)
    return int(np.argmax(np.sqrt(np.mean(np.square(a.reshape(-1, a.shape[-1])), axis=0))))


def _mutations(hw):
    """(id, stage, weights name, weight mutator(wt, c) or None, stage kwargs) of every planted bug that is live at this shape."""
    lv = S.geometry(*hw)
    odd = lambda g: g[0] % 2 or g[1] % 2            # noqa: E731
    shift = lambda g: (-(g[0] % 2), -(g[1] % 2))    # noqa: E731  (the odd surplus row / column taken at the other side)
    out = {"E0": "P", "E1": "act2", "E2": "act3", "E3": "act4", "D0": "dact0", "D1": "dact1", "D2": "dact2"}
    m = []
    for i, st in enumerate(["E0", "E1", "E2", "E3"]):
        m.append((f"tap-enc{i}", st, "seed", lambda wt, c, i=i, st=st: _zero_tap(wt, f"enc{i}.conv.kernel", _busiest(c[out[st]]), True), {}))
        if odd(lv[i]):
            m.append((f"pad-enc{i}", st, "seed", None, {"pad_after": True}))
        m.append((f"eps-enc{i}", st, "smallvar", None, {"eps": 1e-5}))
    for j, st in enumerate(["D0", "D1", "D2"]):
        m.append((f"tap-dec{j}", st, "seed", lambda wt, c, j=j, st=st: _zero_tap(wt, f"dec{j}.up.kernel", _busiest(c[out[st]]), False), {}))
        if odd(lv[3 - j]):
            m.append((f"crop-dec{j}", st, "seed", None, {"crop_shift": shift(lv[3 - j])}))
        if j:
            m.append((f"skip-dec{j}", st, "seed", None, {"drop_skip": True}))
        m.append((f"eps-dec{j}", st, "smallvar", None, {"eps": 1e-5}))
    m.append(("tap-dec3", "T", "seed", lambda wt, c: _zero_tap(wt, "dec3.up.kernel", int(torch.argmax(wt["final.kernel"].abs())), False), {}))
    if odd(lv[0]):
        m.append(("crop-dec3", "T", "seed", None, {"crop_shift": shift(lv[0])}))
    m.append(("skip-dec3", "T", "seed", None, {"drop_skip": True}))
    m.append(("tmix-row-enc0", "E1", "seed", lambda wt, c: _zero_row(wt, "enc0.tmix.w1"), {}))
    m.append(("tmix-row-enc1", "E1", "seed", lambda wt, c: _zero_row(wt, "enc1.tmix.w1"), {}))
    return m


_MUTS = [(hw, *mu) for hw in SHAPES for mu in _mutations(hw)]


@pytest.mark.parametrize("hw,mid,st,wname,wmut,kw", _MUTS, ids=[f"{m[0][0]}x{m[0][1]}-{m[1]}" for m in _MUTS])
def test_planted_bug_fails_by_margin(hw, mid, st, wname, wmut, kw):
    c, wt, lv = _case(hw, wname)
    cand = wmut(wt, c) if wmut else wt
    r = _worst(st, c, wt, cand, lv, **kw)
    assert r >= MARGIN * S.stage_k(st), f"{mid} at {hw}: worst {r:.3g} of u * (rms + |ref|), needs {MARGIN} x {S.stage_k(st)}"


def test_every_stage_and_level_has_a_live_mutation():
    for hw in SHAPES:
        ids = {m[0] for m in _mutations(hw)}
        assert {f"tap-enc{i}" for i in range(4)} | {f"tap-dec{j}" for j in range(4)} <= ids
        assert {"skip-dec1", "skip-dec2", "skip-dec3", "tmix-row-enc0", "tmix-row-enc1"} <= ids
        if any(g[0] % 2 or g[1] % 2 for g in S.geometry(*hw)[:4]):    # (16x16 is even at every level: no pad, no crop surplus)
            assert any(i.startswith("pad-") for i in ids) and any(i.startswith("crop-") for i in ids)
