"""The input statistics of include/covahip.h ("Input monitor") in numpy, one function per quantity, written from the contract's
text.  A frame is u8 [h][w][4] (the decoder's four bytes per macroblock) or u16 [h][w] (packed records)."""
import numpy as np

BINS, MOVE_BINS = 512, 16
FIELDS = ("in_frames", "hist", "moving", "still_frames", "intra_frames", "move_hist")


def records(frames, packed: bool) -> np.ndarray:
    """r of every macroblock, i64 [..][h][w]: c | x << 3 | y << 6 with c, x, y = min(byte 0, 1, 2; 6), byte 3 ignored; for
    packed data value & 511 (bits 9 and above ignored, a field of 7 as given)."""
    frames = np.asarray(frames)
    if packed:
        assert frames.dtype == np.uint16
        return frames.astype(np.int64) & 511
    assert frames.dtype == np.uint8 and frames.shape[-1] == 4
    c, x, y = (np.minimum(frames[..., k].astype(np.int64), 6) for k in range(3))
    return c | x << 3 | y << 6


def bins(r) -> np.ndarray:
    """hist of the records r (any shape): i64 [512]."""
    return np.bincount(np.asarray(r).ravel(), minlength=BINS).astype(np.int64)


def moves(r) -> np.ndarray:
    """either vector field is non-zero"""
    return (np.asarray(r) & 0x1F8) != 0


def intra(r) -> np.ndarray:
    return (np.asarray(r) & 7) >= 5


def n_move(r_frame) -> int:
    return int(moves(r_frame).sum())


def still(r_frame) -> bool:
    """every record is zero: all skip and no vector"""
    return bool((np.asarray(r_frame) == 0).all())


def all_intra(r_frame) -> bool:
    return bool(intra(r_frame).all())


def move_bin(n: int) -> int:
    """bin 0: no macroblock moves; bin k >= 1: min(15, 1 + floor(log2 n)) == k"""
    return 0 if n == 0 else min(15, 1 + (int(n).bit_length() - 1))


def counted_frames(form: str, batch: int, stack_index=None) -> np.ndarray:
    """The frame every stack counts: its newest slice.  stacked: "frame" b is row block 0 of stack b; the frame forms:
    stack_index[b][0], or b + 3 without a table."""
    if form == "stacked":
        return np.arange(batch)
    if stack_index is None:
        return np.arange(batch) + 3
    return np.asarray(stack_index).reshape(batch, 4)[:, 0].astype(np.int64)


def newest(stacked, h: int) -> np.ndarray:
    """row block 0 of every stack of u8 [b][4h][w][4]"""
    return np.asarray(stacked)[:, :h]


def empty(n_models: int, h: int, w: int) -> dict:
    return {"in_frames": np.zeros(n_models, np.int64), "hist": np.zeros((n_models, BINS), np.int64),
            "moving": np.zeros((n_models, h, w), np.int64), "still_frames": np.zeros(n_models, np.int64),
            "intra_frames": np.zeros(n_models, np.int64), "move_hist": np.zeros((n_models, MOVE_BINS), np.int64)}


def input_ref(r_counted, ids=None, n_models: int = 1, into=None) -> dict:
    """The tables after counting the frames r_counted i64 [b][h][w] (records(), one per stack, repeats included) for the models
    ids u8 [b] (None: model 0); into: tables to add to."""
    r_counted = np.asarray(r_counted)
    b, h, w = r_counted.shape
    out = empty(n_models, h, w) if into is None else into
    for i in range(b):
        m = 0 if ids is None else int(ids[i])
        r = r_counted[i]
        out["in_frames"][m] += 1
        out["hist"][m] += bins(r)
        out["moving"][m] += moves(r)
        out["still_frames"][m] += still(r)
        out["intra_frames"][m] += all_intra(r)
        out["move_hist"][m, move_bin(n_move(r))] += 1
    return out


def record_stats_ref(r_frames, gt) -> dict:
    """covahip_train_data_record_stats of the frames r_frames i64 [n][h][w] with labels gt u8 [n][h][w]: one model's tables (no
    model axis) plus hist_set (the records at macroblocks whose label byte is non-zero) and set_total."""
    one = input_ref(r_frames)
    out = {k: (int(v[0]) if v.ndim == 1 else v[0]) for k, v in one.items()}
    sel = np.asarray(gt) != 0
    out["hist_set"] = bins(np.asarray(r_frames)[sel])
    out["set_total"] = int(sel.sum())
    return out


def same(got: dict, want: dict, fields=FIELDS) -> None:
    for k in fields:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (k, np.asarray(got[k]).sum(), np.asarray(want[k]).sum())


def input_ref_loops(frames, packed: bool) -> dict:
    """A second restatement of ONE model's tables with plain loops over macroblocks (small cases only)."""
    frames = np.asarray(frames)
    n, h, w = frames.shape[:3]
    out = {"in_frames": 0, "hist": [0] * BINS, "moving": [[0] * w for _ in range(h)], "still_frames": 0, "intra_frames": 0,
           "move_hist": [0] * MOVE_BINS}
    for f in range(n):
        nm, zero, intra_all = 0, True, True
        for y in range(h):
            for x in range(w):
                if packed:
                    r = int(frames[f, y, x]) % 512
                else:
                    b0, b1, b2 = (min(int(frames[f, y, x, k]), 6) for k in range(3))
                    r = b0 + 8 * b1 + 64 * b2
                out["hist"][r] += 1
                cls, vx, vy = r % 8, (r // 8) % 8, r // 64
                if vx or vy:
                    out["moving"][y][x] += 1
                    nm += 1
                zero = zero and r == 0
                intra_all = intra_all and cls >= 5
        out["in_frames"] += 1
        out["still_frames"] += zero
        out["intra_frames"] += intra_all
        k = 0
        while nm >> k:          # k ends as 1 + floor(log2 nm), 0 for nm == 0
            k += 1
        out["move_hist"][min(15, k)] += 1
    return out
