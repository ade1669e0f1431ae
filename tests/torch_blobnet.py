"""Independent torch.nn.functional composition of the BlobNet graph (test helper).

Written from the reference's Keras model definition (utils/model/blobnet.py:8-48,
encoder.py:30-80, pointwise.py:5-26, decoder.py:5-134, preprocessing.py:6-7), using
torch's conv3d / conv_transpose3d / max_pool3d / batch_norm primitives rather than the
hand loops of oracle/blobnet_ref.c, so the two restatements check each other.
CPU fp32 (or fp64 when `dtype=torch.float64`).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from cova_amd import weights as W

BN_EPS = 1e-3  # Keras BatchNormalization default


def _ident(t):
    return t


def torch_weights(flat_weights: np.ndarray, dtype=torch.float32) -> dict:
    return {k: torch.from_numpy(np.array(v)).to(dtype) for k, v in W.unflatten(flat_weights).items()}


def preprocess(stack: np.ndarray, h: int, w: int, dtype=torch.float32):
    """u8 [B][T*H][W][4] -> clipped, scaled input [B,3,T,H,W] (preprocessing.py)."""
    b = stack.shape[0]
    x = torch.from_numpy(np.ascontiguousarray(stack[..., :3])).to(dtype)       # [B, T*H, W, 3]
    x = x.permute(0, 3, 1, 2).reshape(b, 3, W.T, h, w)                         # Reshape((3,4,H,W))
    return torch.clamp(x, 0.0, 6.0) / 6.0


def enc_conv(x, wt, i, eps=BN_EPS, q=_ident, pad_after=False):
    """Encoder level i up to its pool: conv 3x3 -> ReLU -> BN -> 2x2 max pool -> zero row on top / column on the left for an
    odd input (pad_after: at the bottom / right instead, a planted bug of tests/test_stage_bounds.py).  q rounds the post-BN
    value (fp16 emulation); [N,Cin,T,H,W] -> [N,Cout,T,ceil(H/2),ceil(W/2)]."""
    k = wt[f"enc{i}.conv.kernel"].permute(3, 2, 0, 1).unsqueeze(2)            # [Cout,Cin,1,3,3]
    x = F.relu(F.conv3d(x, k, wt[f"enc{i}.conv.bias"], padding=(0, 1, 1)))
    hh, ww = x.shape[-2], x.shape[-1]
    x = q(F.batch_norm(x, wt[f"enc{i}.bn.mean"], wt[f"enc{i}.bn.var"], wt[f"enc{i}.bn.gamma"],
                       wt[f"enc{i}.bn.beta"], training=False, eps=eps))
    x = F.max_pool3d(x, (1, 2, 2))
    if hh % 2:
        x = F.pad(x, (0, 0, 0, 1) if pad_after else (0, 0, 1, 0))              # zero row on top
    if ww % 2:
        x = F.pad(x, (0, 1, 0, 0) if pad_after else (1, 0, 0, 0))              # zero column on the left
    return x


def enc_tmix(x, wt, i, q=_ident):
    """Temporal MLP of encoder level i + residual: relu(relu(relu(x_T @ w1) @ w2) + x).  q rounds its operands."""
    y = q(x.permute(0, 1, 3, 4, 2))                                            # [N,C,H,W,T]
    y = F.relu(y @ q(wt[f"enc{i}.tmix.w1"]))
    y = F.relu(q(y) @ q(wt[f"enc{i}.tmix.w2"]))
    return F.relu(y.permute(0, 1, 4, 2, 3) + x)


def dec_up(x, wt, j, out_hw, crop_shift=(0, 0), kernel=None, bias=True):
    """Decoder block j's transposed conv on relu(x), cropped to out_hw (decoder.py); crop_shift moves the crop window (a planted
    bug), kernel / bias=False select a part of the block (the partial logits of the level-1 kernel)."""
    k = (wt[f"dec{j}.up.kernel"] if kernel is None else kernel).permute(3, 2, 0, 1).unsqueeze(2)   # [Cin,Cout,1,4,4]
    x = F.conv_transpose3d(F.relu(x), k, wt[f"dec{j}.up.bias"] if bias else None, stride=(1, 2, 2))
    return crop(x, out_hw, crop_shift)


def crop(x, out_hw, shift=(0, 0)):
    """The transposed conv's output [..,H',W'] cut to out_hw: the odd surplus row / column goes at the top / left."""
    ph = x.shape[-2] - out_hw[0]
    pw = x.shape[-1] - out_hw[1]
    assert ph >= 0 and pw >= 0
    y0, x0 = ph // 2 + ph % 2 + shift[0], pw // 2 + pw % 2 + shift[1]
    return x[..., y0: y0 + out_hw[0], x0: x0 + out_hw[1]]


def dec_bn(x, wt, j, eps=BN_EPS):
    return F.batch_norm(x, wt[f"dec{j}.bn.mean"], wt[f"dec{j}.bn.var"], wt[f"dec{j}.bn.gamma"],
                        wt[f"dec{j}.bn.beta"], training=False, eps=eps)


def final(x, wt):
    """1x1 conv 16 -> 1 of the last block's output: [B,16,T,H,W] -> logits [B,H,W] (t = 0)."""
    logit = (x * wt["final.kernel"].view(1, -1, 1, 1, 1)).sum(1, keepdim=True) + wt["final.bias"]
    return logit[:, 0, 0]


def forward(flat_weights: np.ndarray, stack: np.ndarray, h: int, w: int, dtype=torch.float32,
            return_levels: bool = False):
    wt = torch_weights(flat_weights, dtype)
    b = stack.shape[0]
    x = preprocess(stack, h, w, dtype)
    levels = []
    for i in range(4):
        x = enc_tmix(enc_conv(x, wt, i), wt, i)
        levels.append(x)
    skips = [lv[:, :, :1] for lv in reversed(levels)]
    shapes = [s.shape for s in skips] + [(b, 3, W.T, h, w)]
    x = skips[0]
    for j in range(4):
        x = dec_up(x, wt, j, shapes[j + 1][-2:])
        if j < 3:
            x = torch.cat([dec_bn(x, wt, j), skips[j + 1]], dim=1)
    logit = final(x, wt)                                                       # [B,H,W]
    if return_levels:
        return logit.numpy(), [lv.numpy() for lv in levels]
    return logit.numpy()
