"""covahip_post_heat_* restated in numpy (test helper, no GPU, shares no code with cova_amd/calibrate.py).  The rules are those of
include/covahip.h, "Ignore region from heat":
    fire[t] = #samples with logit > thresh[t]   (strict; NaN is background, +inf fires at every threshold; no keep map)
    both[t] = #samples with logit > thresh[t] and gt != 0
    gt      = #samples with gt != 0
64-bit integers throughout."""
import numpy as np


def heat_ref(logits, gt, thresholds) -> dict:
    """-> fire, both i64 [T][h][w], gt i64 [h][w], samples, logit_thresh f32 [T]."""
    logits = np.asarray(logits, np.float32)
    th = np.asarray(thresholds, np.float32)
    g = np.asarray(gt) != 0
    n, h, w = logits.shape
    fire, both = np.zeros((th.size, h, w), np.int64), np.zeros((th.size, h, w), np.int64)
    for t in range(th.size):
        with np.errstate(invalid="ignore"):
            m = logits > th[t]
        fire[t] = m.sum(axis=0, dtype=np.int64)
        both[t] = (m & g).sum(axis=0, dtype=np.int64)
    return {"fire": fire, "both": both, "gt": g.sum(axis=0, dtype=np.int64), "samples": n, "logit_thresh": th}
