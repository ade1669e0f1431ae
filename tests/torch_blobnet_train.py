"""Training-mode torch composition of the BlobNet graph (test helper), for autograd in f64.

Reuses tests/torch_blobnet.py's pieces (preprocess, crop, final) and restates what training changes
(include/covahip.h, "BlobNet training"): BatchNorm on batch statistics, dropout masks from the documented counter-based
hash (restated here in numpy), the Jaccard-distance loss with smooth = 100.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from cova_amd import synth, train as T, weights as W
from tests import torch_blobnet as TB

M64 = (1 << 64) - 1


def splitmix64(z):
    """The hash of covahip.h on numpy uint64 arrays (or Python ints), mod 2^64."""
    if isinstance(z, int):
        z = (z + 0x9E3779B97F4A7C15) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def drop_mask(seed: int, step: int, site: int, shape, p: float) -> np.ndarray:
    """Keep-scale factors (0 or 1 / (1 - p)) of dropout site `site` at `step` over a tensor of `shape`, indexed in C order."""
    key = splitmix64((seed & M64) ^ splitmix64(((step << 8) | site) & M64))
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        h = splitmix64(np.uint64(key) + np.arange(n, dtype=np.uint64))
    thr = int(round(p * 2 ** 24))
    keep = (h >> np.uint64(40)) >= np.uint64(thr)
    return np.where(keep, 1.0 / (1.0 - p), 0.0).reshape(shape)


def _bn_train(x, wt, name, eps, detach=False):
    dims = [0] + list(range(2, x.dim()))
    mean = x.mean(dim=dims)
    var = x.var(dim=dims, unbiased=False)
    if detach:
        mean, var = mean.detach(), var.detach()
    shape = [1, -1] + [1] * (x.dim() - 2)
    y = (x - mean.view(shape)) / torch.sqrt(var.view(shape) + eps) * wt[f"{name}.gamma"].view(shape) + wt[f"{name}.beta"].view(shape)
    return y, mean, var


def forward_loss(flat_weights, stack, gt, h, w, seed=0, step=0, p=0.2, smooth=100.0, eps=TB.BN_EPS, dtype=torch.float64,
                 swap_sites=(), mask_nhwt=False, pad_after=(), crop_shift=None, bn_detach=False, jaccard_batch=False,
                 loss_div=None):
    """Training-mode forward: returns (loss, weight tensors (leaves requiring grad), {bn name: (batch mean, biased var)}, logits).

    The other keywords plant the bugs of tests/test_train_bounds.py: swap_sites (encoder levels whose two dropout sites trade
    places), mask_nhwt (encoder masks hashed over [B][C][H][W][T] instead of NCTHW), pad_after (encoder levels whose odd-size
    zero row / column goes at the bottom / right), crop_shift ({decoder block: (dy, dx)} added to the crop offset), bn_detach
    (batch statistics as constants), jaccard_batch (one Jaccard over the whole batch), loss_div (the divisor of the loss sum)."""
    wt = TB.torch_weights(flat_weights, dtype)
    for k, v in wt.items():
        if not k.endswith((".bn.mean", ".bn.var")):
            v.requires_grad_(True)
    b = stack.shape[0]
    x = TB.preprocess(stack, h, w, dtype)
    stats, levels = {}, []
    for i in range(4):
        k = wt[f"enc{i}.conv.kernel"].permute(3, 2, 0, 1).unsqueeze(2)
        c = F.relu(F.conv3d(x, k, wt[f"enc{i}.conv.bias"], padding=(0, 1, 1)))
        hh, ww = c.shape[-2:]
        n, mean, var = _bn_train(c, wt, f"enc{i}.bn", eps, bn_detach)
        stats[f"enc{i}.bn"] = (mean, var)
        pl = F.max_pool3d(n, (1, 2, 2))
        after = i in pad_after
        if hh % 2:
            pl = F.pad(pl, (0, 0, 0, 1) if after else (0, 0, 1, 0))
        if ww % 2:
            pl = F.pad(pl, (0, 1, 0, 0) if after else (1, 0, 0, 0))
        s1, s2 = (2 * i + 1, 2 * i) if i in swap_sites else (2 * i, 2 * i + 1)
        if mask_nhwt:
            shp = tuple(pl.permute(0, 1, 3, 4, 2).shape)
            m1 = torch.from_numpy(drop_mask(seed, step, s1, shp, p)).to(dtype)
            m2 = torch.from_numpy(drop_mask(seed, step, s2, shp, p)).to(dtype)
        else:
            shp = tuple(pl.shape)                                               # [B,C,T,H,W]: the hash's index order
            m1 = torch.from_numpy(drop_mask(seed, step, s1, shp, p)).to(dtype).permute(0, 1, 3, 4, 2)
            m2 = torch.from_numpy(drop_mask(seed, step, s2, shp, p)).to(dtype).permute(0, 1, 3, 4, 2)
        y = pl.permute(0, 1, 3, 4, 2)                                            # [B,C,H,W,T]
        y = F.relu(y @ wt[f"enc{i}.tmix.w1"]) * m1
        y = F.relu(y @ wt[f"enc{i}.tmix.w2"]) * m2
        x = F.relu(y.permute(0, 1, 4, 2, 3) + pl)
        levels.append(x)
    skips = [lv[:, :, :1] for lv in reversed(levels)]
    shapes = [s.shape for s in skips] + [(b, 3, W.T, h, w)]
    z = skips[0]
    for j in range(4):
        md = torch.from_numpy(drop_mask(seed, step, 8 + j, tuple(z.shape), p)).to(dtype)
        kk = wt[f"dec{j}.up.kernel"].permute(3, 2, 0, 1).unsqueeze(2)
        y = F.conv_transpose3d(F.relu(z) * md, kk, wt[f"dec{j}.up.bias"], stride=(1, 2, 2))
        y = TB.crop(y, shapes[j + 1][-2:], (crop_shift or {}).get(j, (0, 0)))
        if j < 3:
            n, mean, var = _bn_train(y, wt, f"dec{j}.bn", eps, bn_detach)
            stats[f"dec{j}.bn"] = (mean, var)
            z = torch.cat([n, skips[j + 1]], dim=1)
        else:
            z = y
    logit = TB.final(z, wt)                                                      # [B,H,W]
    pr = torch.sigmoid(logit)
    yv = torch.from_numpy(np.asarray(gt)).to(dtype)
    sum_dims = (0, -2, -1) if jaccard_batch else (-2, -1)
    inter = (yv * pr).sum(dim=sum_dims)
    tot = (yv + pr).sum(dim=sum_dims)
    per = (1 - (inter + smooth) / (tot - inter + smooth)) * smooth
    loss = per.mean() if loss_div is None else per.sum() / loss_div
    return loss, wt, stats, logit


def grads_flat(flat_weights, stack, gt, h, w, **kw):
    """(loss, flat gradient in weight-file order with batch mean / biased variance in the BN mean / var slots, logits)."""
    loss, wt, stats, logit = forward_loss(flat_weights, stack, gt, h, w, **kw)
    loss.backward()
    parts = []
    for name, shape in W.tensor_specs().items():
        if name.endswith((".bn.mean", ".bn.var")):
            mean, var = stats[name.rsplit(".", 1)[0]]
            parts.append((mean if name.endswith("mean") else var).detach().numpy().reshape(-1))
        else:
            parts.append(wt[name].grad.numpy().reshape(-1))
    return float(loss.detach()), np.concatenate(parts), logit.detach().numpy()


# ------------------------------------------------------------------------------------------------ the training case matrix
# One bound per kind of error, shared by tests/test_gpu_train.py (the HIP step against this reference) and
# tests/test_train_bounds.py (planted bugs in this reference exceed them):
#   loss  |loss - ref| / |ref|
#   norm  per tensor (every gradient, every batch mean / biased variance slot), ||g - ref|| / ||ref||
#   max   per weight-gradient tensor, max|g - ref| / max|ref|: an error confined to a few elements that `norm` averages away
# No elementwise bound on activations: near-ties in a 2x2 max pool can route a gradient to another element in f32 than in f64.
# Measured on an MI355X over CASES and the batch-320 test, the worst values are loss 1.1e-7, norm 1.5e-5 and max 1.1e-5;
# the bounds are about 7x those (and float32 torch on the CPU stays within them).
BOUNDS = {"loss": 1e-6, "norm": 1e-4, "max": 8e-5}
# the convT bias of decoder blocks 0..2 feeds a training-mode BatchNorm, which subtracts it again: its exact gradient is zero and
# both sides hold rounding residue.  Its error is taken relative to the gradient of that BN's beta -- the sum whose cancellation
# the bias gradient is.
ZERO_GRADS = {f"dec{j}.up.bias": f"dec{j}.bn.beta" for j in range(3)}


def errors(loss, g, ref_loss, g_ref) -> dict:
    """{(kind, tensor name): error} of a step (loss, flat gradient) against a reference one, kinds as in BOUNDS."""
    gu = {k: v.astype(np.float64) for k, v in W.unflatten(np.asarray(g, np.float32)).items()}
    ru = {k: v.astype(np.float64) for k, v in W.unflatten(np.asarray(g_ref, np.float64)).items()}
    out = {("loss", "loss"): abs(loss - ref_loss) / abs(ref_loss)}
    for k in gu:
        d = gu[k] - ru[k]
        r = ru[ZERO_GRADS.get(k, k)]
        out[("norm", k)] = np.linalg.norm(d) / max(np.linalg.norm(r), 1e-300)
        if not k.endswith((".bn.mean", ".bn.var")):
            out[("max", k)] = np.abs(d).max() / max(np.abs(r).max(), 1e-300)
    return out


def excess(errs) -> float:
    """The largest error of `errors` in units of its bound (> 1: out of bounds)."""
    return max(v / BOUNDS[kind] for (kind, _), v in errs.items())


def worst(errs) -> dict:
    """{kind: (largest error, its tensor)}."""
    out = {}
    for (kind, name), v in errs.items():
        if kind not in out or v > out[kind][0]:
            out[kind] = (v, name)
    return out


class Case:
    """One training step checked against the reference: `steps` steps with lr = 0 on full batches of max_batch first (the
    trainable weights stay bit-identical; the moving statistics move, which the training forward does not read), then a
    batch of `batch` at step `steps`.  labels: "random" (density 0.3) or "edge" (sample 0 all zeros, sample 1 all ones, the
    rest random)."""

    def __init__(self, h, w, batch, max_batch, p, steps=0, seed=11, labels="random", data=5, weights=3):
        self.h, self.w, self.batch, self.max_batch, self.p, self.steps = h, w, batch, max_batch, p, steps
        self.seed, self.labels, self.data, self.weights = seed, labels, data, weights
        big = "-bigseed" if seed >= 1 << 63 else ""
        self.id = (f"{h}x{w}-b{batch}of{max_batch}-p{p:g}-k{steps}{big}" + ("-edge" if labels == "edge" else ""))

    @property
    def p32(self) -> float:
        """The dropout rate as the float32 the trainer's cfg.dropout holds."""
        return float(np.float32(self.p))

    def inputs(self):
        """(initial flat weights, [(stack, gt)] of the lr = 0 steps, stack, gt of the checked step)."""
        flat = T.init_weights(self.weights)
        pre = [sample_batch(self.h, self.w, self.max_batch, self.data + 100 + k) for k in range(self.steps)]
        stack, gt = sample_batch(self.h, self.w, self.batch, self.data)
        if self.labels == "edge":
            gt[0], gt[1] = 0, 1
        return flat, pre, stack, gt

    def reference(self, **mut):
        """(loss, flat gradient, logits) of the reference on the checked step; mut: planted bugs (forward_loss)."""
        flat, _, stack, gt = self.inputs()
        kw = dict(seed=self.seed, step=self.steps, p=self.p32)
        kw.update(mut)
        return grads_flat(flat, stack, gt, self.h, self.w, **kw)


def sample_batch(h, w, b, seed):
    """b stacks of b independent synthetic streams and random labels of density 0.3."""
    return synth.stacked_batch(b, h, w, seed=seed, streams=b), synth.random_masks(b, h, w, 0.3, seed=seed)


# geometries 16x16 (1x1 bottleneck; BN over 4 positions per sample in decoder block 0), 17x33 (odd at every level in both
# dimensions), 24x50 (height and width of different parity level by level), 45x80 and 68x120; batch 1 of 1, 2 of 5 after a full
# batch of 5 (stale rows in every buffer), 3 of 3; dropout 0, 0.2, 0.5; steps after the first; a seed >= 2^63; degenerate labels.
# The first two are the original gradient check (tests/test_gpu_train.py::test_gradients_match_torch_f64).
CASES = [
    Case(45, 80, 3, 3, 0.2),
    Case(68, 120, 3, 3, 0.2),
    Case(16, 16, 1, 1, 0.2),
    Case(16, 16, 3, 3, 0.5, steps=1, seed=7, labels="edge"),
    Case(17, 33, 2, 5, 0.5, steps=2, seed=(1 << 64) - 12345),
    Case(17, 33, 1, 1, 0.0, seed=3),
    Case(17, 33, 3, 3, 0.2, steps=3, seed=1 << 63, labels="edge"),
    Case(24, 50, 3, 3, 0.0, seed=5, labels="edge"),
    Case(24, 50, 2, 5, 0.2, steps=1, seed=9),
    Case(45, 80, 2, 5, 0.5, steps=2, seed=(1 << 63) + 1),
]
