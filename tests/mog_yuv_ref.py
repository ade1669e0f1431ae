"""numpy restatement of the MoG labeller's YUV 4:2:0 -> BGR conversion (include/covahip.h, "MoG labels": covahip_mog_apply_yuv) and
what the tests of that entry need around it.  All arithmetic is int64 here; the header's int32 never overflows (|yy| < 2^29,
|c * uu| < 2^29).

  yuv_to_bgr     planes -> u8 [h][w][3], chroma sample (X >> 1, Y >> 1), limited or full range
  work_image     the labeller's working image of a BGR frame on either grid (copy, 2x2 mean, centre pick)
  pack_nv12 / pack_i420 / pack   planes of [F][S] frames into a byte buffer at arbitrary offsets, pitches and strides; every byte
                 that is no sample (row padding, coded rows, gaps) is a seeded random byte
  bgr_to_yuv420  an approximate BT.601 forward transform, only to make inputs that look like the BGR clip they come from
"""
from __future__ import annotations

import numpy as np

from tests import mog_grid_ref as G
from tests import mog_ref as R

LIMITED = dict(ysub=16, ymul=1220542, bu=2116026, gv=852492, gu=409993, rv=1673527)
FULL = dict(ysub=0, ymul=1 << 20, bu=1858077, gv=748826, gu=360853, rv=1470104)
COEF = {"limited": LIMITED, "full": FULL}
FORMATS = {"nv12": 1, "i420": 2}
RANGES = {"limited": 0, "full": 1}


def yuv_to_bgr(y: np.ndarray, u: np.ndarray, v: np.ndarray, range: str = "limited") -> np.ndarray:
    """y u8 [..][h][w], u and v u8 [..][h/2][w/2] -> u8 [..][h][w][3] (B, G, R)."""
    c = COEF[range]
    yy = np.maximum(0, y.astype(np.int64) - c["ysub"]) * c["ymul"]
    uu = (u.astype(np.int64) - 128).repeat(2, -2).repeat(2, -1)
    vv = (v.astype(np.int64) - 128).repeat(2, -2).repeat(2, -1)
    h = 1 << 19
    b = (yy + h + c["bu"] * uu) >> 20
    g = (yy + h - c["gv"] * vv - c["gu"] * uu) >> 20
    r = (yy + h + c["rv"] * vv) >> 20
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def work_image(bgr: np.ndarray, grid: str = "reference") -> np.ndarray:
    """The working image of one BGR frame: tests/mog_ref.resize_bgr on the reference grid, the 2x2 mean on the macroblock grid."""
    return R.resize_bgr(bgr) if grid == "reference" else G.half_bgr(bgr)


def bgr_to_yuv420(bgr: np.ndarray, range: str = "limited"):
    """u8 [..][h][w][3] -> (y [..][h][w], u [..][h/2][w/2], v the same): BT.601 in float, chroma as the mean of the 2x2 block.
    Approximate by design: it only makes inputs."""
    f = bgr.astype(np.float32)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    cb, cr = (b - y) * 0.564, (r - y) * 0.713
    if range == "limited":
        y, cb, cr = 16 + y * (219 / 255), cb * (224 / 255), cr * (224 / 255)

    def sub(c):
        return (c[..., 0::2, 0::2] + c[..., 0::2, 1::2] + c[..., 1::2, 0::2] + c[..., 1::2, 1::2]) / 4

    q = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)   # noqa: E731
    return q(y), q(128 + sub(cb)), q(128 + sub(cr))


class Layout:
    """Plain numbers of a covahip_mog_yuv (tests without the package's ctypes class can use it; `ctypes()` makes that one)."""

    def __init__(self, fmt, range, offset, pitch, frame_stride, stream_stride):
        self.fmt, self.range = fmt, range
        self.offset, self.pitch = list(offset) + [0] * (3 - len(offset)), list(pitch) + [0] * (3 - len(pitch))
        self.frame_stride, self.stream_stride = frame_stride, stream_stride

    def ctypes(self):
        from cova_amd import _lib as L
        lay = L.MogYuv()
        lay.format, lay.range = FORMATS[self.fmt], RANGES[self.range]
        lay.offset[:] = self.offset
        lay.pitch[:] = self.pitch
        lay.frame_stride, lay.stream_stride = self.frame_stride, self.stream_stride
        return lay


def extent(w: int, h: int, fmt: str, offset, pitch):
    """(lo, hi): the bytes of a frame from its lowest plane start to behind the last byte of the last row."""
    rows = (h, h // 2, h // 2)
    rowb = (w, w if fmt == "nv12" else w // 2, w // 2)
    n = 2 if fmt == "nv12" else 3
    return min(offset[:n]), max(offset[p] + (rows[p] - 1) * pitch[p] + rowb[p] for p in range(n))


def padded(w: int, h: int, fmt: str, range: str = "limited", streams: int = 1, frames: int = 1, stream_major: bool = False):
    """The padded surface of the GPU tests: pitch[0] = w + 64, offset[1] = pitch[0] * (h + 8) (8 coded rows behind the picture);
    NV12 pitch[1] = w + 32; I420 pitch[1] = w / 2 + 16, pitch[2] = w / 2 + 48, V behind U with 4 coded rows between; frames 128
    bytes apart beyond their extent."""
    p0 = w + 64
    o1 = p0 * (h + 8)
    if fmt == "nv12":
        offset, pitch = [0, o1], [p0, w + 32]
    else:
        p1, p2 = w // 2 + 16, w // 2 + 48
        offset, pitch = [0, o1, o1 + p1 * (h // 2 + 4)], [p0, p1, p2]
    slot = extent(w, h, fmt, offset, pitch)[1] + 128
    if stream_major:
        return Layout(fmt, range, offset, pitch, slot, frames * slot)
    return Layout(fmt, range, offset, pitch, streams * slot, slot)


def tight(w: int, h: int, fmt: str, range: str = "limited", streams: int = 1, frames: int = 1, stream_major: bool = False):
    fb = w * h * 3 // 2
    offset, pitch = ([0, w * h], [w, w]) if fmt == "nv12" else ([0, w * h, w * h + w * h // 4], [w, w // 2, w // 2])
    if stream_major:
        return Layout(fmt, range, offset, pitch, fb, frames * fb)
    return Layout(fmt, range, offset, pitch, streams * fb, fb)


def pack(y: np.ndarray, u: np.ndarray, v: np.ndarray, lay: Layout, seed: int = 0, exact: bool = True) -> np.ndarray:
    """y u8 [F][S][h][w], u, v u8 [F][S][h/2][w/2] -> the byte buffer of layout `lay`, ending with the last byte of the last row it
    reaches (exact) and random wherever there is no sample."""
    F, S, h, w = y.shape
    lo, hi = extent(w, h, lay.fmt, lay.offset, lay.pitch)
    size = (F - 1) * lay.frame_stride + (S - 1) * lay.stream_stride + hi
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, size if exact else size + 4096, dtype=np.uint8)
    for f in range(F):
        for s in range(S):
            b0 = f * lay.frame_stride + s * lay.stream_stride

            def plane(p, rows, nbytes):            # a writable view of the plane's samples (the last row ends inside buf)
                return np.lib.stride_tricks.as_strided(buf[b0 + lay.offset[p]:], (rows, nbytes), (lay.pitch[p], 1))

            plane(0, h, w)[...] = y[f, s]
            if lay.fmt == "nv12":
                plane(1, h // 2, w)[...] = np.stack([u[f, s], v[f, s]], -1).reshape(h // 2, w)
            else:
                plane(1, h // 2, w // 2)[...] = u[f, s]
                plane(2, h // 2, w // 2)[...] = v[f, s]
    return buf


def pack_nv12(y, u, v, lay: Layout, seed: int = 0):
    assert lay.fmt == "nv12"
    return pack(y, u, v, lay, seed)


def pack_i420(y, u, v, lay: Layout, seed: int = 0):
    assert lay.fmt == "i420"
    return pack(y, u, v, lay, seed)
