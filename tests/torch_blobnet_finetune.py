"""Training-mode torch composition of the BlobNet graph under a training plan (test helper), for autograd in f64.

tests/torch_blobnet_train.py::forward_loss with what a plan changes (include/covahip.h, "Fine-tuning"): a BatchNorm layer in
inference mode normalises with the moving statistics of the weight blob, as constants; a frozen group gets no gradient (its
slots read 0) and its BatchNorm is in inference mode.  Dropout stays on everywhere, with the masks of the documented hash.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from cova_amd import train as T, weights as W
from tests import torch_blobnet as TB
from tests import torch_blobnet_train as TT

BOUNDS = TT.BOUNDS


def effective(freeze=(), bn_inference=()):
    """(frozen group names, inference-mode BN layer names) of a plan, the frozen groups' layers included."""
    fz, bn = T.plan_bits(freeze, bn_inference)
    names = T.plan_names(fz, bn | (fz & 0x7F))
    return set(names["freeze"]), set(names["bn_inference"])


def finetune_weights(seed: int) -> np.ndarray:
    """train.init_weights(seed) with the BatchNorm slots (gamma, beta, moving mean / variance) of weights.random_init(seed): with
    mean 0 / var 1 an inference-mode BatchNorm is nearly the identity and hides errors."""
    t = W.unflatten(T.init_weights(seed).copy())
    r = W.unflatten(W.random_init(seed))
    for name in t:
        if ".bn." in name:
            t[name] = r[name]
    return W.flatten(t)


def _bn(x, wt, name, eps, inference: bool):
    if not inference:
        return TT._bn_train(x, wt, name, eps)
    shape = [1, -1] + [1] * (x.dim() - 2)
    mean, var = wt[f"{name}.mean"], wt[f"{name}.var"]
    y = (x - mean.view(shape)) / torch.sqrt(var.view(shape) + eps) * wt[f"{name}.gamma"].view(shape) + wt[f"{name}.beta"].view(shape)
    return y, mean, var


def forward_loss(flat_weights, stack, gt, h, w, freeze=(), bn_inference=(), seed=0, step=0, p=0.2, smooth=100.0, eps=TB.BN_EPS,
                 dtype=torch.float64, batch_terms=(), no_dropout_in_frozen=False):
    """Training-mode forward under the plan (freeze, bn_inference): (loss, weight tensors, {bn name: (mean, var) the layer
    normalised with}, logits).

    Planted bugs of tests/test_finetune_bounds.py: batch_terms (BN layers of the plan's inference set that run
    _bn_train(detach=False) instead: batch statistics with their batch-mean terms in the backward), no_dropout_in_frozen (the
    dropout sites of frozen groups are the identity)."""
    frozen, inference = effective(freeze, bn_inference)
    inference = inference - set(batch_terms)
    wt = TB.torch_weights(flat_weights, dtype)
    for k, v in wt.items():
        if not k.endswith((".bn.mean", ".bn.var")):
            v.requires_grad_(True)

    def mask(group, site, shape):
        if no_dropout_in_frozen and group in frozen:
            return torch.ones(shape, dtype=dtype)
        return torch.from_numpy(TT.drop_mask(seed, step, site, shape, p)).to(dtype)

    b = stack.shape[0]
    x = TB.preprocess(stack, h, w, dtype)
    stats, levels = {}, []
    for i in range(4):
        k = wt[f"enc{i}.conv.kernel"].permute(3, 2, 0, 1).unsqueeze(2)
        c = F.relu(F.conv3d(x, k, wt[f"enc{i}.conv.bias"], padding=(0, 1, 1)))
        hh, ww = c.shape[-2:]
        n, mean, var = _bn(c, wt, f"enc{i}.bn", eps, f"enc{i}" in inference)
        stats[f"enc{i}.bn"] = (mean, var)
        pl = F.max_pool3d(n, (1, 2, 2))
        if hh % 2:
            pl = F.pad(pl, (0, 0, 1, 0))
        if ww % 2:
            pl = F.pad(pl, (1, 0, 0, 0))
        shp = tuple(pl.shape)                                                    # [B,C,T,H,W]: the hash's index order
        m1 = mask(f"enc{i}", 2 * i, shp).permute(0, 1, 3, 4, 2)
        m2 = mask(f"enc{i}", 2 * i + 1, shp).permute(0, 1, 3, 4, 2)
        y = pl.permute(0, 1, 3, 4, 2)                                            # [B,C,H,W,T]
        y = F.relu(y @ wt[f"enc{i}.tmix.w1"]) * m1
        y = F.relu(y @ wt[f"enc{i}.tmix.w2"]) * m2
        x = F.relu(y.permute(0, 1, 4, 2, 3) + pl)
        levels.append(x)
    skips = [lv[:, :, :1] for lv in reversed(levels)]
    shapes = [s.shape for s in skips] + [(b, 3, W.T, h, w)]
    z = skips[0]
    for j in range(4):
        md = mask(f"dec{j}", 8 + j, tuple(z.shape))
        kk = wt[f"dec{j}.up.kernel"].permute(3, 2, 0, 1).unsqueeze(2)
        y = F.conv_transpose3d(F.relu(z) * md, kk, wt[f"dec{j}.up.bias"], stride=(1, 2, 2))
        y = TB.crop(y, shapes[j + 1][-2:])
        if j < 3:
            n, mean, var = _bn(y, wt, f"dec{j}.bn", eps, f"dec{j}" in inference)
            stats[f"dec{j}.bn"] = (mean, var)
            z = torch.cat([n, skips[j + 1]], dim=1)
        else:
            z = y
    logit = TB.final(z, wt)                                                      # [B,H,W]
    pr = torch.sigmoid(logit)
    yv = torch.from_numpy(np.asarray(gt)).to(dtype)
    inter = (yv * pr).sum(dim=(-2, -1))
    tot = (yv + pr).sum(dim=(-2, -1))
    loss = ((1 - (inter + smooth) / (tot - inter + smooth)) * smooth).mean()
    return loss, wt, stats, logit


def group_of(name: str) -> str:
    """The plan group of a tensor: its enc{i} / dec{j} prefix; final.kernel / final.bias belong to dec3."""
    return "dec3" if name.startswith("final.") else name.split(".", 1)[0]


def grads_flat_plan(flat_weights, stack, gt, h, w, freeze=(), bn_inference=(), **kw):
    """(loss, flat gradient in weight-file order, logits): zeros in the slots of frozen groups; the BN mean / var slots hold what
    the layer normalised with -- the moving values for an inference-mode layer, batch mean / biased variance otherwise."""
    frozen, _ = effective(freeze, bn_inference)
    loss, wt, stats, logit = forward_loss(flat_weights, stack, gt, h, w, freeze, bn_inference, **kw)
    loss.backward()
    parts = []
    for name, shape in W.tensor_specs().items():
        if name.endswith((".bn.mean", ".bn.var")):
            mean, var = stats[name.rsplit(".", 1)[0]]
            parts.append((mean if name.endswith("mean") else var).detach().double().numpy().reshape(-1))
        elif group_of(name) in frozen:
            parts.append(np.zeros(int(np.prod(shape))))
        else:
            parts.append(wt[name].grad.double().numpy().reshape(-1))
    return float(loss.detach()), np.concatenate(parts), logit.detach().numpy()


def errors(loss, g, ref_loss, g_ref, freeze=(), bn_inference=()) -> dict:
    """torch_blobnet_train.errors under a plan.  The convT bias in front of an inference-mode BatchNorm has a real gradient and is
    compared by its own norm; only the biases in front of batch-mode layers keep the ZERO_GRADS treatment.  A frozen slot's
    reference is exactly 0, so anything but 0 there is an unbounded error."""
    _, inference = effective(freeze, bn_inference)
    zero = {k: v for k, v in TT.ZERO_GRADS.items() if group_of(k) not in inference}
    gu = {k: v.astype(np.float64) for k, v in W.unflatten(np.asarray(g, np.float32)).items()}
    ru = {k: v for k, v in _unflatten64(g_ref).items()}
    out = {("loss", "loss"): abs(loss - ref_loss) / abs(ref_loss)}
    for k in gu:
        d = gu[k] - ru[k]
        r = ru[zero.get(k, k)]
        out[("norm", k)] = np.linalg.norm(d) / max(np.linalg.norm(r), 1e-300)
        if not k.endswith((".bn.mean", ".bn.var")):
            out[("max", k)] = np.abs(d).max() / max(np.abs(r).max(), 1e-300)
    return out


def _unflatten64(flat) -> dict:
    flat = np.asarray(flat, np.float64).reshape(-1)
    out, off = {}, 0
    for name, shape in W.tensor_specs().items():
        n = int(np.prod(shape))
        out[name] = flat[off:off + n].reshape(shape)
        off += n
    return out


# ------------------------------------------------------------------------------------------------ the fine-tuning case matrix
PLANS = {
    "a-bn-all": dict(freeze=(), bn_inference="all"),                       # every BN on moving statistics, everything trained
    "b-encoder": dict(freeze="encoder", bn_inference=()),                   # the encoder's backward does not run at all
    "c-enc2-dec1": dict(freeze=("enc2", "dec1"), bn_inference=()),          # gradient THROUGH frozen groups, mixed BN modes
    "d-only-dec3": dict(freeze=("encoder", "dec0", "dec1", "dec2"), bn_inference=()),
    "e-bn-dec0": dict(freeze=(), bn_inference=("dec0",)),                   # dec0's convT bias has a real gradient
}
GEOMETRIES = [(16, 16), (17, 33), (24, 50)]   # 1x1 bottleneck; odd at every level; parities differing level by level
BATCH, MAX_BATCH = 2, 5


class Case:
    """One step of batch 2 under a plan, on a trainer of max_batch 5 that has taken one full lr = 0 step under the same plan
    (stale rows in every buffer)."""

    def __init__(self, h, w, p, plan, seed=11, data=5, weights=3):
        self.h, self.w, self.p, self.plan_id, self.plan = h, w, p, plan, PLANS[plan]
        self.seed, self.data, self.weights = seed, data, weights
        self.id = f"{h}x{w}-p{p:g}-{plan}"

    @property
    def p32(self) -> float:
        return float(np.float32(self.p))

    def inputs(self):
        """(initial flat weights, (stack, gt) of the lr = 0 step, stack, gt of the checked step)."""
        return (finetune_weights(self.weights), TT.sample_batch(self.h, self.w, MAX_BATCH, self.data + 100),
                *TT.sample_batch(self.h, self.w, BATCH, self.data))

    def reference(self, flat=None, **kw):
        """(loss, flat gradient, logits) of the reference on the checked step (step index 1), from weights `flat` (default: the
        initial ones); kw: planted bugs, dtype."""
        f0, _, stack, gt = self.inputs()
        args = dict(seed=self.seed, step=1, p=self.p32)
        args.update(kw)
        return grads_flat_plan(f0 if flat is None else flat, stack, gt, self.h, self.w, **self.plan, **args)

    def errors(self, loss, g, ref_loss, g_ref):
        return errors(loss, g, ref_loss, g_ref, **self.plan)


CASES = [Case(h, w, p, plan) for (h, w) in GEOMETRIES for p in (0.2, 0.0) for plan in PLANS]
