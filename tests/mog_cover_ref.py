"""numpy restatement of the MoG label modes (include/covahip.h, "MoG labels", step 6) on a filled mask of any size: per 8x8 block
of the working image `count` (its pixels that are 1) and `inside` (its pixels inside the image: 64, except in a last label row or
column that is only started), and from them the three modes

    corner          filled[8i][8j], the reference's cl_op_fill[::8, ::8]
    cover, N        1 iff 64 * count >= N * inside, N in 1 .. 64
    count           count, 0 .. 64

Everything is computed pixel by pixel from the mask itself (a zero-padded reshape), with no bit planes and no popcounts: nothing
here shares a step with the kernels' label function.  `relations` states what holds between the modes by construction.
"""
from __future__ import annotations

import numpy as np

COVER_NS = (1, 8, 16, 32, 48, 64)


def _blocks(a: np.ndarray) -> np.ndarray:
    """[..][h][w] -> [..][lh][lw][8][8], zero beyond the image."""
    h, w = a.shape[-2:]
    lh, lw = (h + 7) // 8, (w + 7) // 8
    p = np.zeros(a.shape[:-2] + (8 * lh, 8 * lw), np.int64)
    p[..., :h, :w] = a
    return p.reshape(a.shape[:-2] + (lh, 8, lw, 8)).swapaxes(-3, -2)


def count(filled: np.ndarray) -> np.ndarray:
    """filled [..][h][w] (non-zero = 1) -> i64 [..][lh][lw]: the block's foreground pixels."""
    return _blocks(np.asarray(filled) != 0).sum((-2, -1))


def inside(h: int, w: int) -> np.ndarray:
    """i64 [lh][lw]: the block's pixels inside an image of h x w."""
    return _blocks(np.ones((h, w), bool)).sum((-2, -1))


def corner(filled: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray((np.asarray(filled) != 0)[..., ::8, ::8]).astype(np.uint8)


def cover(filled: np.ndarray, n: int) -> np.ndarray:
    if not 1 <= n <= 64:
        raise ValueError(f"min_cover {n} outside 1 .. 64")
    h, w = np.asarray(filled).shape[-2:]
    return (64 * count(filled) >= n * inside(h, w)).astype(np.uint8)


def labels(filled: np.ndarray, mode) -> np.ndarray:
    """u8 [..][lh][lw] of a `labels` value of cova_amd.mog.MogLabeler: "corner", "count" or ("cover", N)."""
    if mode == "corner":
        return corner(filled)
    if mode == "count":
        return count(filled).astype(np.uint8)
    name, n = mode
    if name != "cover":
        raise ValueError(f"unknown label mode {mode!r}")
    return cover(filled, n)


def relations(filled: np.ndarray, ns=COVER_NS):
    """Asserts what holds by construction: COVER(1) holds every CORNER label, COVER(N) shrinks as N grows, COUNT > 0 exactly where
    COVER(1) is 1, and COUNT never exceeds `inside`."""
    h, w = np.asarray(filled).shape[-2:]
    cnt, cor = count(filled), corner(filled)
    cov = [cover(filled, n) for n in ns]
    assert (cnt >= 0).all() and (cnt <= inside(h, w)).all()
    assert (cover(filled, 1) >= cor).all()
    for a, b in zip(cov, cov[1:]):
        assert (a >= b).all()
    assert ((cnt > 0) == (cover(filled, 1) == 1)).all()
    assert ((cnt == inside(h, w)) == (cover(filled, 64) == 1)).all()
