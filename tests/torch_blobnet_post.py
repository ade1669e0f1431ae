"""The training step with a post in f64 (test helper): the masked Jaccard distance of include/covahip.h, "Training with a
post", formed from the logits of tests/torch_blobnet_train.py's forward (which is not edited) and differentiated by autograd.

    keep'  = keep != 0
    I      = sum over keep' of y * p,  S = sum over keep' of (y + p)        per sample
    loss   = mean over the batch of (1 - (I + s) / (S - I + s)) * s

Shared by tests/test_train_post_host.py (the yardstick checked on the CPU) and tests/test_gpu_train_post.py (the HIP step
against it); the cases and their references are computed once per process.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from cova_amd import train as T, weights as W
from cova_amd.elements import keep_from_rects
from tests import torch_blobnet_train as TT

SMOOTH = 100.0
# (h, w, batch, dropout, seed): 17x33 is odd at every level and at hw = 561 a workgroup of 256 positions spans two samples with
# a partial last one; 45x80 (3,600 macroblocks) and 24x50 (1,200) are the larger grids
GEOMETRIES = [(17, 33, 3, 0.2, 11), (45, 80, 3, 0.2, 11), (24, 50, 2, 0.0, 5)]
IDS = [f"{h}x{w}-b{b}-p{p:g}" for h, w, b, p, _ in GEOMETRIES]


def ignore_rects(h, w):
    """A clock near the top left (5 x 3 macroblocks) and the bottom right corner (4 x 2; the rectangle runs off the frame)."""
    return [(32, 16, 80, 48), (16 * (w - 4), 16 * (h - 2), 144, 144)]


def keep_map(h, w) -> np.ndarray:
    keep = keep_from_rects(h, w, ignore_rects(h, w))
    assert int((keep == 0).sum()) == 23
    return keep


def masked_jaccard(logit, gt, keep, smooth=SMOOTH, mask_p_in_s=True):
    """Per-sample masked Jaccard distance of torch logits [B][H][W].  mask_p_in_s=False plants the bug that masks y but not p
    in S."""
    pr = torch.sigmoid(logit)
    yv = torch.from_numpy(np.asarray(gt)).to(logit.dtype)
    kp = torch.from_numpy(np.asarray(keep) != 0).to(logit.dtype)
    inter = (yv * pr * kp).sum(dim=(-2, -1))
    tot = ((yv + pr) * kp).sum(dim=(-2, -1)) if mask_p_in_s else (yv * kp + pr).sum(dim=(-2, -1))
    return (1 - (inter + smooth) / (tot - inter + smooth)) * smooth


def grads_flat_post(flat_weights, stack, gt, h, w, keep, mask_p_in_s=True, **kw):
    """TT.grads_flat with the masked loss: (loss, flat gradient with the batch statistics in the BN mean / var slots, logits)."""
    _, wt, stats, logit = TT.forward_loss(flat_weights, stack, gt, h, w, **kw)
    loss = masked_jaccard(logit, gt, keep, kw.get("smooth", SMOOTH), mask_p_in_s).mean()
    loss.backward()
    parts = []
    for name, shape in W.tensor_specs().items():
        if name.endswith((".bn.mean", ".bn.var")):
            mean, var = stats[name.rsplit(".", 1)[0]]
            parts.append((mean if name.endswith("mean") else var).detach().numpy().reshape(-1))
        else:
            parts.append(wt[name].grad.numpy().reshape(-1))
    return float(loss.detach()), np.concatenate(parts), logit.detach().numpy()


def sample_loss_f64(logits, gt, keep, smooth=SMOOTH):
    """The masked per-sample Jaccard distance of numpy logits [N][H][W], in f64."""
    return masked_jaccard(torch.from_numpy(np.asarray(logits, np.float64)), gt, keep, smooth).numpy()


@functools.lru_cache(maxsize=None)
def inputs(h, w, b):
    """(initial flat weights, stack, gt) of a geometry; treat as read-only."""
    stack, gt = TT.sample_batch(h, w, b, 5)
    return T.init_weights(3), stack, gt


@functools.lru_cache(maxsize=None)
def reference(h, w, b, p, seed, kind="masked"):
    """(loss, flat gradient, logits) of the first step of a trainer (seed, dropout p) on inputs(h, w, b); treat as read-only.
    kind: "masked" (the post's keep_map), "ones" (an all-ones keep map), "unmasked" (TT.grads_flat: no post) or "bug" (y masked
    in S, p not)."""
    flat, stack, gt = inputs(h, w, b)
    kw = dict(seed=seed, step=0, p=float(np.float32(p)))
    if kind == "unmasked":
        return TT.grads_flat(flat, stack, gt, h, w, **kw)
    keep = np.ones((h, w), np.uint8) if kind == "ones" else keep_map(h, w)
    return grads_flat_post(flat, stack, gt, h, w, keep, mask_p_in_s=kind != "bug", **kw)
