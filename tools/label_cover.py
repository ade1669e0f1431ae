#!/usr/bin/env python
"""Choosing min_cover for a camera: what COVAHIP_MOG_LABELS_COVER would label at several N, from one count dump.

    python -m cova_amd.mog --size 1280x720 --labels count VIDEO.bgr:VIDEO_count.dump
    python tools/label_cover.py VIDEO_count.dump --labels-size 80x45 [--work-size 640x360] [--n 1,8,16,32,48,64]

The dump holds one byte 0 .. 64 per block and frame (`--labels count`: the block's foreground pixels in the filled mask), frames
one after the other, each label_h rows of label_w bytes; --labels-size is label_w x label_h, as the labeller reports them
(80x45 on the reference grid, 120x68 for 1920x1080 on the macroblock grid).  For every N the table has

    label_mass           labels that are 1 under `--labels cover:N`, over all frames: 64 * count >= N * inside
    frames_with_labels   frames that have at least one

N = 1 keeps every object the filled mask has; a higher N drops blocks an object only grazes, and from some N on small objects
lose their last label and whole frames go empty.  The mass is what `--balance` of the trainer thresholds, so it shows how far a
threshold tuned on corner labels has to move.  A block is taken as whole (inside = 64) unless --work-size gives the working
image's width x height, whose last label row and column may only be started.  No GPU.
"""
import argparse
import sys

import numpy as np

NS = (1, 8, 16, 32, 48, 64)


def read_counts(path, label_h, label_w):
    """u8 [frames][label_h][label_w] of a count dump; ValueError for a partial frame or a byte above 64."""
    a = np.fromfile(path, np.uint8)
    if a.size % (label_h * label_w):
        raise ValueError(f"{path}: {a.size} bytes are no whole number of {label_w}x{label_h} frames")
    if a.size and a.max() > 64:
        raise ValueError(f"{path}: a byte of {int(a.max())}: not a `--labels count` dump")
    return a.reshape(-1, label_h, label_w)


def table(counts, ns=NS, work=None):
    """Per N of ns: {"n", "frames", "label_mass", "frames_with_labels"}.  work = (work_w, work_h) weighs the started blocks."""
    _, lh, lw = counts.shape
    inside = np.full((lh, lw), 64, np.int64)
    if work is not None:
        ww, wh = work
        if (-(-wh // 8), -(-ww // 8)) != (lh, lw):
            raise ValueError(f"a working image of {ww}x{wh} has {-(-ww // 8)}x{-(-wh // 8)} labels, not {lw}x{lh}")
        inside = np.outer(np.minimum(8, wh - 8 * np.arange(lh)), np.minimum(8, ww - 8 * np.arange(lw)))
    rows = []
    for n in ns:
        lab = 64 * counts.astype(np.int64) >= n * inside
        rows.append({"n": int(n), "frames": int(counts.shape[0]), "label_mass": int(lab.sum()),
                     "frames_with_labels": int(lab.any((1, 2)).sum())})
    return rows


def _size(text):
    try:
        w, h = (int(v) for v in text.lower().split("x"))
        if w < 1 or h < 1:
            raise ValueError
    except ValueError:
        raise argparse.ArgumentTypeError(f"size {text!r} is not WxH") from None
    return w, h


def main(argv=None):
    ap = argparse.ArgumentParser(prog="label_cover.py", description=__doc__.split("\n")[0])
    ap.add_argument("dump", help="a `python -m cova_amd.mog --labels count` dump")
    ap.add_argument("--labels-size", type=_size, required=True, metavar="WxH", help="label_w x label_h of the dump (80x45, 120x68, ...)")
    ap.add_argument("--work-size", type=_size, default=None, metavar="WxH",
                    help="the working image's size (half the source on the macroblock grid): weighs a started last row / column")
    ap.add_argument("--n", default=",".join(str(n) for n in NS), help="the N to list, each in 1 .. 64")
    a = ap.parse_args(argv)
    try:
        ns = [int(v) for v in a.n.split(",")]
        if not ns or not all(1 <= n <= 64 for n in ns):
            raise ValueError(f"--n {a.n!r}: integers in 1 .. 64")
        lw, lh = a.labels_size
        rows = table(read_counts(a.dump, lh, lw), ns, a.work_size)
    except (OSError, ValueError) as e:
        print(f"label_cover.py: error: {e}", file=sys.stderr)
        return 2
    print(f"{'N':>3} {'label_mass':>12} {'frames_with_labels':>19}   of {rows[0]['frames']} frames")
    for r in rows:
        print(f"{r['n']:>3} {r['label_mass']:>12} {r['frames_with_labels']:>19}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
