"""Float64 references of the HIP BlobNet path's kernel stages, and the per-element bound they are checked with (test helper).

Each stage takes the HIP path's OWN input checkpoint (the workspace buffers of include/covahip_dev.h's read-back, kernel layouts,
channels last) and computes in float64 exactly what the stage's kernels compute, with the operators of tests/torch_blobnet.py:

  E0   enc0p_mfma                       u8 carrier frames [F][H][W][4] -> P [F][H1][W1][16]
  E1   enc1_mfma (or the 32x32x16 form)  P gathered by the stack table -> level-0 tmix -> level 1 -> act[2]; act[1] (t = 0) or part
  E2   enc2_mfma                        act[2] -> act[3]                    E3   enc3_mfma   act[3] -> act[4] (t = 0)
  E23  enc23_mfma                       act[2] -> act[4] (+ act[3] t = 0, the decoder's skip)
  D0..D2  dec0/1/2_mfma                 act[4] + skips -> dact[0] -> dact[1] -> dact[2]     D012  dec012_mfma   -> dact[2]
  T    dec3_final_mfma / dec3_bboxcc_fused   dact[2] + part (or act[1]) -> fp32 logits

dact[j] holds relu(BN(...)): the only reader applies the ReLU, so the kernels store it applied.  `part` is the level-0 skip
half of the last block folded with the final 1x1 conv, fp32 [B][H1 + 1][W1 + 1][4]: grid position (u, v) of the transposed
conv, parity r = 2 py + px = uncropped output pixel (2u + py, 2v + px), no bias.

Bound, per element of a stage's output:  |hip - ref| <= K * u * (rms(ref) + |ref|),  u = 2^-11 (fp16 unit roundoff); a stage
that spans two levels (E1, E23, D012) gets 2K.  The reference weights are the fp32 weights as given (not fp16-rounded), so
the bound covers the kernels' weight rounding.  tests/test_stage_bounds.py shows on the CPU that an fp16 emulation of every
stage passes with a 3x margin and that every planted bug fails by 3x; tests/test_gpu_stages.py applies it to the kernels.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from cova_amd import weights as W
from tests import torch_blobnet as TB

U = 2.0 ** -11
K = 16
FUSED = ("E1", "E23", "D012")   # stages that span two levels: bound 2K


def stage_k(stage: str, k: float = K) -> float:
    return 2 * k if stage in FUSED else k


def mixed_gamma_weights(seed):
    """Every second BN gamma of every encoder level negative: the ALLPOS=false kernel variants."""
    wts = W.unflatten(W.random_init(seed))
    for i in range(4):
        wts[f"enc{i}.bn.gamma"][::2] *= -1.0
    return W.flatten(wts)


def small_var_weights(seed):
    """BN variances drawn from 1e-3 .. 1e-2: a BN scale of about 10 - 30 in every level (fp16 range and ulp size).  The kernels
    that read a BN output are scaled by 1/20 so that the activations stay inside fp16's range over the eight levels."""
    wts = W.unflatten(W.random_init(seed))
    rng = np.random.default_rng(seed)
    for name in list(wts):
        if name.endswith("bn.var"):
            wts[name] = rng.uniform(1e-3, 1e-2, np.shape(wts[name])).astype(np.float32)
        if name in ("enc1.conv.kernel", "enc2.conv.kernel", "enc3.conv.kernel") or name.endswith("up.kernel"):
            wts[name] = (np.asarray(wts[name]) / 20).astype(np.float32)
    return W.flatten(wts)


def weights(flat: np.ndarray) -> dict:
    return TB.torch_weights(flat, torch.float64)


def round16(t):
    return t.to(torch.float16).to(t.dtype)


def _t(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _to_cf(a, has_t: bool) -> torch.Tensor:
    """Kernel layout [B][T][H][W][C] (or [B][H][W][C], T = 1) -> [B,C,T,H,W]."""
    x = _t(a)
    if not has_t:
        x = x.unsqueeze(1)
    return x.permute(0, 4, 1, 2, 3)


def _to_cl(x: torch.Tensor, keep_t: bool) -> np.ndarray:
    """[B,C,T,H,W] -> [B][T][H][W][C], or [B][H][W][C] of t = 0."""
    y = x.permute(0, 2, 3, 4, 1)
    return (y if keep_t else y[:, 0]).contiguous().numpy()


# ------------------------------------------------------------------------------------------------------------- stages
def e0(frames: np.ndarray, wt: dict, q=TB._ident, **mut) -> np.ndarray:
    """enc0p_mfma: u8 [F][H][W][4] -> P [F][H1][W1][16] (clip / 6, conv0, ReLU, BN, 2x2 max, pad row / column)."""
    x = torch.from_numpy(np.ascontiguousarray(frames[..., :3])).to(torch.float64).permute(0, 3, 1, 2).unsqueeze(2)
    x = torch.clamp(x, 0.0, 6.0) / 6.0
    return _to_cl(TB.enc_conv(q(x), wt, 0, q=q, **mut), keep_t=False)


def part_of(skip0: torch.Tensor, wt: dict) -> np.ndarray:
    """Partial logits of the level-0 skip ([B,16,1,H1,W1]): fp32 layout [B][H1 + 1][W1 + 1][4]."""
    h1, w1 = skip0.shape[-2:]
    k = wt["dec3.up.kernel"][..., 16:]                      # [4,4,Cout,Cin]: the skip channels follow the up channels
    full = TB.dec_up(skip0, wt, 3, (2 * h1 + 2, 2 * w1 + 2), kernel=k, bias=False)
    lg = (full * wt["final.kernel"].view(1, -1, 1, 1, 1)).sum(1)[:, 0]             # [B, 2H1+2, 2W1+2]
    b = lg.shape[0]
    return lg.reshape(b, h1 + 1, 2, w1 + 1, 2).permute(0, 1, 3, 2, 4).reshape(b, h1 + 1, w1 + 1, 4).numpy()


def e1(p: np.ndarray, table: np.ndarray, wt: dict, q=TB._ident, **mut) -> dict:
    """Level-1 kernel: P gathered by the stack table [B][4] -> {act2 [B][T][H2][W2][32], act1 [B][H1][W1][16] (t = 0), part}."""
    x = _t(p[np.asarray(table)]).permute(0, 4, 1, 2, 3)       # [B,16,T,H1,W1]
    lv0 = TB.enc_tmix(x, wt, 0, q=q)
    lv1 = TB.enc_tmix(q(TB.enc_conv(q(lv0), wt, 1, q=q, **mut)), wt, 1, q=q)
    return {"act2": _to_cl(lv1, True), "act1": _to_cl(lv0, False), "part": part_of(lv0[:, :, :1], wt)}


def enc(a: np.ndarray, wt: dict, i: int, q=TB._ident, **mut) -> np.ndarray:
    """Encoder level i = 2, 3: act[i] [B][T][H][W][C] -> act[i+1] ([B][H][W][128], t = 0, for level 3)."""
    x = TB.enc_tmix(q(TB.enc_conv(q(_to_cf(a, True)), wt, i, q=q, **mut)), wt, i, q=q)
    return _to_cl(x, keep_t=i < 3)


def dec(up: np.ndarray | None, skip: np.ndarray | None, wt: dict, j: int, out_hw, q=TB._ident, eps=TB.BN_EPS,
        crop_shift=(0, 0), drop_skip=False) -> np.ndarray:
    """Decoder block j = 0..2: relu(BN(crop(convT(relu(concat(up, skip_t0)))))) [B][Hd][Wd][Cout].  Block 0 has no `up`; its
    input is act[4].  skip: [B][T][H][W][C] (t = 0 used) or [B][H][W][C]."""
    parts = []
    if up is not None:
        parts.append(_to_cf(up, False))
    if skip is not None:
        s = _to_cf(skip, skip.ndim == 5)[:, :, :1]
        parts.append(torch.zeros_like(s) if drop_skip else s)
    x = TB.dec_up(q(torch.cat(parts, 1)), wt, j, out_hw, crop_shift=crop_shift)
    return _to_cl(F.relu(TB.dec_bn(q(x), wt, j, eps=eps)), keep_t=False)


def tail(dact2: np.ndarray, wt: dict, out_hw, part: np.ndarray | None = None, act1: np.ndarray | None = None,
         q=TB._ident, crop_shift=(0, 0), drop_skip=False) -> np.ndarray:
    """Last block + final conv: dact[2] with the skip half as partial logits (`part`) or as the tensor act[1] -> logits [B][H][W]."""
    x = q(_to_cf(dact2, False))
    if act1 is not None:
        s = _to_cf(act1, act1.ndim == 5)[:, :, :1]
        x = torch.cat([x, torch.zeros_like(s) if drop_skip else q(s)], 1)
        return TB.final(TB.dec_up(x, wt, 3, out_hw, crop_shift=crop_shift), wt).numpy()
    lg = TB.final(TB.dec_up(x, wt, 3, out_hw, kernel=wt["dec3.up.kernel"][..., :16], crop_shift=crop_shift), wt)
    if drop_skip:
        return lg.numpy()
    pl = _t(part)                                            # [B][H1+1][W1+1][4] -> uncropped [B][2H1+2][2W1+2]
    b, gh, gw, _ = pl.shape
    full = pl.reshape(b, gh, gw, 2, 2).permute(0, 1, 3, 2, 4).reshape(b, 2 * gh, 2 * gw).unsqueeze(1).unsqueeze(1)
    return (lg + TB.crop(full, out_hw, crop_shift)[:, 0, 0]).numpy()


# ------------------------------------------------------------------------------------------------- whole-path checkpoints
def geometry(h: int, w: int):
    """Spatial size of level 0..4 (level 0 = the network input)."""
    lv = [(h, w)]
    for _ in range(4):
        lv.append(((lv[-1][0] + 1) // 2, (lv[-1][1] + 1) // 2))
    return lv


def checkpoints(flat: np.ndarray, stack: np.ndarray, h: int, w: int, q=TB._ident) -> dict:
    """Every stage output of the float64 network on a stacked batch (stack b = carrier frames 4b .. 4b+3), chained."""
    wt = weights(flat)
    b = stack.shape[0]
    lv = geometry(h, w)
    frames = stack.reshape(b, W.T, h, w, 4).reshape(b * W.T, h, w, 4)
    table = np.arange(b * W.T).reshape(b, W.T)
    c = {"frames": frames, "table": table}
    c["P"] = e0(frames, wt)
    c.update(e1(c["P"], table, wt))
    c["act3"] = enc(c["act2"], wt, 2)
    c["act4"] = enc(c["act3"], wt, 3)
    c["dact0"] = dec(None, c["act4"], wt, 0, lv[3])
    c["dact1"] = dec(c["dact0"], c["act3"], wt, 1, lv[2])
    c["dact2"] = dec(c["dact1"], c["act2"], wt, 2, lv[1])
    c["logits"] = tail(c["dact2"], wt, lv[0], part=c["part"])
    return c


# ------------------------------------------------------------------------------------------------------------- the bound
def ratio(hip, ref) -> np.ndarray:
    """|hip - ref| / (u * (rms(ref) + |ref|)), per element (inf where hip is not finite)."""
    hip = np.asarray(hip, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    rms = float(np.sqrt(np.mean(np.square(ref))))
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.abs(hip - ref) / (U * (rms + np.abs(ref)) + 1e-300)
    return np.where(np.isfinite(hip), r, np.inf)


def worst(hip, ref) -> float:
    """Worst ratio; elements where |ref| >= 6e4 (beyond fp16's range) may be non-finite in hip and are left out then."""
    ref = np.asarray(ref, dtype=np.float64)
    r = ratio(hip, ref)
    r = np.where(np.isinf(r) & (np.abs(ref) >= 6e4), 0.0, r)
    return float(r.max()) if r.size else 0.0


def pad_zero(a: np.ndarray, in_hw) -> bool:
    """The pad row (top, odd input height) and pad column (left, odd input width) of a pooled tensor [...][H][W][C] are 0."""
    ok = True
    if in_hw[0] % 2:
        ok &= bool((np.asarray(a)[..., 0, :, :] == 0).all())
    if in_hw[1] % 2:
        ok &= bool((np.asarray(a)[..., :, 0, :] == 0).all())
    return ok
