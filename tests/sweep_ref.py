"""covahip_post_sweep restated with the CPU oracle's regionprops and numpy (test helper, no GPU, shares no code with
cova_amd/calibrate.py).  The rules are those of include/covahip.h, "Calibration":
    keep' = keep != 0 (all ones without a keep map); mask_t = (logit > thresh[t]) & keep'; gt' = (gt != 0) & keep'
    pixel[t] = |mask_t & gt'|, |mask_t & ~gt'|, |~mask_t & gt'|
    G = first max_boxes of regionprops(gt', gt_area); P[t][a] = the boxes with area >= areas[a] among the first max_boxes of
    regionprops(mask_t, areas[0]); a frame with more than max_boxes boxes counts in gt_truncated / truncated[t]
    hit(p, g): inter > 0 and inter * den >= num * (w_p h_p + w_g h_g - inter)
    pred = |P|, pred_true = the p that hit some g, gt_found = the g that hit some p, gt_objects = sum |G|
64-bit integers throughout."""
import numpy as np

from oracle import ref


def hits(P, G, num, den) -> np.ndarray:
    """bool [len(P)][len(G)]: the hit rule between every p and every g, in int64 (box areas are below 2^31, num and den small)."""
    f = lambda B, k: B[k].astype(np.int64)
    iw = np.minimum.outer(f(P, "left") + f(P, "width"), f(G, "left") + f(G, "width")) - np.maximum.outer(f(P, "left"), f(G, "left"))
    ih = np.minimum.outer(f(P, "top") + f(P, "height"), f(G, "top") + f(G, "height")) - np.maximum.outer(f(P, "top"), f(G, "top"))
    inter = np.where((iw > 0) & (ih > 0), iw * ih, 0)
    union = np.add.outer(f(P, "width") * f(P, "height"), f(G, "width") * f(G, "height")) - inter
    return (inter > 0) & (inter * den >= num * union)


def sweep_ref(logits, gt, thresholds, areas, keep=None, gt_area=1, iou=(1, 10), max_boxes=256, want_boxes=False):
    """-> dict of pixel i64 [T][3], pred / pred_true / gt_found i64 [T][A], truncated i64 [T], samples, gt_objects, gt_truncated;
    with want_boxes also boxes[s][t][a] = P[t][a] of sample s (oracle box records)."""
    logits = np.asarray(logits, np.float32)
    n, h, w = logits.shape
    thresholds = np.asarray(thresholds, np.float32)
    areas = [int(a) for a in areas]
    T, A = len(thresholds), len(areas)
    num, den = iou
    kp = np.ones((h, w), bool) if keep is None else np.asarray(keep) != 0
    out = {"pixel": np.zeros((T, 3), np.int64), "pred": np.zeros((T, A), np.int64), "pred_true": np.zeros((T, A), np.int64),
           "gt_found": np.zeros((T, A), np.int64), "truncated": np.zeros(T, np.int64), "samples": n, "gt_objects": 0, "gt_truncated": 0}
    boxes = []
    for s in range(n):
        g_mask = (np.asarray(gt[s]) != 0) & kp
        G, ng = ref.regionprops(g_mask.astype(np.uint8), gt_area, max_boxes)
        out["gt_truncated"] += int(ng > max_boxes)
        out["gt_objects"] += len(G)
        per_t = []
        for t in range(T):
            with np.errstate(invalid="ignore"):
                m = (logits[s] > thresholds[t]) & kp
            out["pixel"][t] += (int((m & g_mask).sum()), int((m & ~g_mask).sum()), int((~m & g_mask).sum()))
            P0, np0 = ref.regionprops(m.astype(np.uint8), areas[0], max_boxes)
            out["truncated"][t] += int(np0 > max_boxes)
            H = hits(P0, G, num, den)
            per_a = []
            for a in range(A):
                sel = P0["area"] >= areas[a]
                out["pred"][t, a] += int(sel.sum())
                out["pred_true"][t, a] += int(H[sel].any(axis=1).sum())
                out["gt_found"][t, a] += int(H[sel].any(axis=0).sum())
                per_a.append(P0[sel])
            per_t.append(per_a)
        boxes.append(per_t)
    if want_boxes:
        out["boxes"] = boxes
    return out


def smooth_field(rng, n, h, w, k=3):
    """Seeded smooth fields f32 [n][h][w]: Gaussian noise on (h + k - 1) x (w + k - 1) box-blurred with a k x k window, scaled to unit
    standard deviation, so thresholds near 0 cut through it and leave a handful of blobs."""
    x = rng.standard_normal((n, h + k - 1, w + k - 1))
    acc = np.zeros((n, h, w))
    for dy in range(k):
        for dx in range(k):
            acc += x[:, dy:dy + h, dx:dx + w]
    acc /= acc.std()
    return acc.astype(np.float32)
