"""numpy restatement of the serving monitor's rules (include/covahip.h, "Serving monitor").  For every sample b with model m:

    frames[m]            += 1
    fire[m][y][x]        += mask[b][y][x] != 0
    boxes[m]             += counts[b]
    frames_with_boxes[m] += counts[b] > 0
    truncated[m]         += counts[b] > max_boxes
    area_hist[m][k]      += #{ i < min(counts[b], max_boxes) : min(15, floor(log2(boxes[b][i].area_px))) == k }

All int64; every comparison against it is equality."""
import numpy as np

BINS = 16
FIELDS = ("frames", "fire", "boxes", "frames_with_boxes", "truncated", "area_hist")


def area_bin(area: int) -> int:
    """min(15, floor(log2(area))) in integers; an area below 2 is bin 0."""
    return min(BINS - 1, int(area).bit_length() - 1) if area >= 2 else 0


def empty(n_models, h, w):
    return {"frames": np.zeros(n_models, np.int64), "fire": np.zeros((n_models, h, w), np.int64), "boxes": np.zeros(n_models, np.int64),
            "frames_with_boxes": np.zeros(n_models, np.int64), "truncated": np.zeros(n_models, np.int64),
            "area_hist": np.zeros((n_models, BINS), np.int64)}


def monitor_ref(mask, counts, boxes, model_ids, max_boxes, n_models, into=None):
    """mask u8 [n][h][w], counts i32 [n], boxes [n][>= max_boxes] with a field area_px (None when max_boxes == 0), model_ids [n] or
    None (model 0).  -> the six tables; `into`: tables to add to (returned)."""
    mask = np.asarray(mask)
    n, h, w = mask.shape
    out = empty(n_models, h, w) if into is None else into
    ids = np.zeros(n, np.int64) if model_ids is None else np.asarray(model_ids, np.int64)
    for b in range(n):
        m, c = int(ids[b]), int(counts[b])
        out["frames"][m] += 1
        out["fire"][m] += mask[b] != 0
        out["boxes"][m] += c
        out["frames_with_boxes"][m] += c > 0
        out["truncated"][m] += c > max_boxes
        for i in range(max(0, min(c, max_boxes))):
            out["area_hist"][m][area_bin(int(boxes[b][i]["area_px"]))] += 1
    return out


def same(got, want):
    for k in FIELDS:
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (k, len(bad), bad[:4].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])
