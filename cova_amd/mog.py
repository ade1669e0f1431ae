"""MoG training labels on the GPU: utils/generate-mog.py of the reference, the first step of its "train from scratch" flow.

  MogLabeler   covahip_mog_*: per-pixel MOG2 at 640x360, close 4x4, open 6x6, hole fill and the ::8 subsample to the 45x80
               labels `tfrecordsink gt=` reads, for several independent videos (streams) per call.  grid="macroblock" works
               at half the source instead and labels the source's own macroblocks: 68x120 for 1920x1080, and it alone
               takes 2560x1440 (90x160 labels) and 3840x2160 (135x240).  any_size=True (macroblock grid) takes every even
               source size from 256 to 4096 in both axes: 1280x960 gives 60x80 labels, 704x576 36x44
               labels="corner" (the default: the block's top-left pixel, the reference's ::8 subsample), ("cover", N) (1 where
               at least N / 64 of the block is foreground: small objects keep their labels) or "count" (0 .. 64, for inspection)
               shadows="drop" | "keep" | (mode, tau) turns MOG2's shadow detection on (OpenCV's detectShadows, tau 0.5):
               "drop" keeps cast shadows out of the labels, "keep" only marks them (127 in debug_masks, shadow_counts)
               save_state / load_state: one stream's model as a blob ("CVHM"; exact resume: a long recording is labelled in
               pieces); set_frozen: label against the model without changing it (the second pass of learn-then-label);
               background: the image the model takes for background, u8 BGR at the working size
  read_state   a state blob's header fields and arrays, CRC verified, on the host; write_state is its inverse
  label_dims   (label_h, label_w) of a source size on either grid, without a GPU; label_dims_any / work_dims_any: of any_size
  read_bgr24   raw BGR24 frames (ffmpeg -f rawvideo -pix_fmt bgr24) from a file or stdin, in chunks
  apply_yuv    the same labels from 8-bit 4:2:0 frames as decoders give them, NV12 or I420, at a row pitch, plane offsets and
               frame / stream strides of the caller's (a MogYuv layout; yuv_tight makes the dense one), 1.5 bytes per pixel
               and no BGR copy; limited (video) or full (JPEG) range, the BT.601 constants of cv.cvtColor
  read_yuv420  raw NV12 / I420 frames (ffmpeg -f rawvideo -pix_fmt nv12 | yuv420p); read_y4m: YUV4MPEG2, which carries its size

    ffmpeg -i VIDEO -f rawvideo -pix_fmt bgr24 - | python -m cova_amd.mog --size 1280x720 -:VIDEO_gt.dump
    python -m cova_amd.mog --size 1280x720 a.bgr b.bgr:labels_b.dump ... [--streams S] [--chunk F]
    python -m cova_amd.mog --size 1920x1080 --grid macroblock IN.bgr ...      (68x120 labels: what 1080p records need)
    python -m cova_amd.mog --size 3840x2160 --grid macroblock IN.bgr ...      (135x240 labels; 2560x1440 gives 90x160)
    python -m cova_amd.mog --any-size 1280x960 IN.bgr ...                     (60x80 labels; any even size, 256 .. 4096)
    ffmpeg -i VIDEO -f yuv4mpegpipe -pix_fmt yuv420p - | python -m cova_amd.mog --format y4m -:VIDEO_gt.dump
    python -m cova_amd.mog --format nv12 --size 1920x1080 [--range full] IN.nv12 ...     (also --format i420)
    python -m cova_amd.mog --size 1280x720 --labels cover:32 IN.bgr ...       (a label where half the block is foreground)
    python -m cova_amd.mog --size 1280x720 --labels count IN.bgr:IN_count.dump           (then tools/label_cover.py picks N)
    python -m cova_amd.mog --size 1280x720 --shadows drop:0.5 IN.bgr ...      (cast shadows stay out of the labels)
    python -m cova_amd.mog --size 1280x720 --shadows keep:0.4 --shadow-report IN.bgr ... (labels as without; what drop would remove)
    python -m cova_amd.mog --size 1280x720 hour0.bgr --save-state h0.cvhm                (then: hour1.bgr --load-state h0.cvhm)
    python -m cova_amd.mog --size 1280x720 clip.bgr --two-pass --background clip.ppm     (learn, then label against the settled model)

Each input gets a stream slot; when a video ends its slot is reset and takes the next one, so every output is byte-identical
to labelling that video alone.  The output defaults to the input's name with `_gt.dump`.  Bitstream decoding is not done here:
the labeller takes decoded frames, BGR24 (what cv.VideoCapture hands generate-mog.py) or the decoder's own NV12 / I420.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import struct
import sys
import time

import numpy as np

from . import _lib as L
from .train import crc32c

WORK_W, WORK_H = 640, 360
LABEL_H, LABEL_W = 45, 80
NMIX = 5
SIZES = ((640, 360), (1280, 720), (1920, 1080))
MAX_STREAMS = 1024
GRIDS = {"reference": 0, "macroblock": 1}       # COVAHIP_MOG_GRID_*
GRID_SIZES = {"reference": SIZES, "macroblock": SIZES + ((2560, 1440), (3840, 2160))}   # the source sizes each grid takes
FORMATS = {"nv12": 1, "i420": 2}                # COVAHIP_MOG_FMT_*
RANGES = {"limited": 0, "full": 1}              # COVAHIP_MOG_RANGE_*
ANY_MIN, ANY_MAX = 256, 4096                    # COVAHIP_MOG_ANY_*: what any_size admits, per axis and even
LABEL_MODES = {"corner": 0, "cover": 1, "count": 2}     # COVAHIP_MOG_LABELS_*
SHADOW_MODES = {"off": 0, "drop": 1, "keep": 2}         # COVAHIP_MOG_SHADOWS_*
SHADOW_TAU = 0.5                                        # OpenCV's default shadow threshold
STATE_MAGIC = 0x4D485643                                # "CVHM": a stream's model (include/covahip.h, "MoG labels", model state)
STATE_VERSION = 1
STATE_HEADER = 64


def state_size(work_w: int, work_h: int) -> int:
    """Bytes of the state blob of a work_w x work_h model: the header, 101 bytes per pixel, the CRC."""
    return STATE_HEADER + 101 * work_w * work_h + 4


def read_state(blob) -> dict:
    """A state blob (MogLabeler.save_state) taken apart on the host: work_w, work_h, history, var_threshold, n and the arrays W, V
    f32 [5][work_h][work_w], M f32 [5][3][work_h][work_w], nmodes u8 [work_h][work_w] (copies).  ValueError for what
    covahip_mog_load_state answers COVAHIP_ERR_BAD_DATA to: a wrong magic, version, size or CRC, a nmodes above 5, n < 0."""
    data = bytes(blob)
    if len(data) < STATE_HEADER + 4:
        raise ValueError(f"a state blob has at least {STATE_HEADER + 4} bytes, got {len(data)}")
    magic, version, w, h, history, tb, n = struct.unpack_from("<IIiiifq", data, 0)
    if magic != STATE_MAGIC or version != STATE_VERSION:
        raise ValueError(f"not a MoG state blob: magic {magic:#x}, version {version}")
    if w < 1 or h < 1 or len(data) != state_size(w, h):
        raise ValueError(f"a {w}x{h} state blob has {state_size(max(w, 0), max(h, 0))} bytes, got {len(data)}")
    if struct.unpack_from("<I", data, len(data) - 4)[0] != crc32c(memoryview(data)[:-4]):
        raise ValueError("state blob: CRC mismatch")
    P = w * h
    f = np.frombuffer(data, "<f4", 25 * P, STATE_HEADER)
    nm = np.frombuffer(data, np.uint8, P, STATE_HEADER + 100 * P)
    if n < 0 or (nm > NMIX).any():
        raise ValueError("state blob: n < 0 or a nmodes byte above 5")
    return {"work_w": w, "work_h": h, "history": history, "var_threshold": tb, "n": n,
            "W": f[:5 * P].reshape(NMIX, h, w).copy(), "V": f[5 * P:10 * P].reshape(NMIX, h, w).copy(),
            "M": f[10 * P:].reshape(NMIX, 3, h, w).copy(), "nmodes": nm.reshape(h, w).copy()}


def write_state(W, V, M, nmodes, n: int = 0, history: int = 9000, var_threshold: float = 32.0) -> bytes:
    """read_state's inverse: the blob of a model given as arrays (W, V [5][h][w], M [5][3][h][w], nmodes [h][w]), for models built
    by hand.  ValueError for shapes that do not agree, a nmodes above 5 or n < 0."""
    nm = np.ascontiguousarray(nmodes)
    if nm.ndim != 2 or (nm < 0).any() or (nm > NMIX).any() or n < 0:
        raise ValueError("nmodes must be [work_h][work_w] of 0 .. 5, and n >= 0")
    h, w = nm.shape
    parts = []
    for a, shape in ((W, (NMIX, h, w)), (V, (NMIX, h, w)), (M, (NMIX, 3, h, w))):
        a = np.ascontiguousarray(a, dtype="<f4")
        if a.shape != shape:
            raise ValueError(f"an array of shape {a.shape}, expected {shape}")
        parts.append(a.tobytes())
    head = struct.pack("<IIiiifq", STATE_MAGIC, STATE_VERSION, w, h, history, var_threshold, n).ljust(STATE_HEADER, b"\0")
    body = head + b"".join(parts) + nm.astype(np.uint8).tobytes()
    return body + struct.pack("<I", crc32c(body))


def shadow_mode(shadows):
    """(mode name, tau) of a `shadows` value: None or "off", "drop", "keep" (tau = SHADOW_TAU), or (mode, tau) with mode "drop" or
    "keep" and a finite 0 < tau <= 1.  tau is SHADOW_TAU where the mode does not read it.  Anything else raises ValueError."""
    if shadows is None:
        return "off", SHADOW_TAU
    if isinstance(shadows, str):
        name, tau = shadows, SHADOW_TAU
    else:
        try:
            name, tau = shadows
        except (TypeError, ValueError):
            raise ValueError(f"shadows {shadows!r}: None, 'drop', 'keep' or (mode, tau)") from None
        if name not in ("drop", "keep"):
            raise ValueError(f"shadows {shadows!r}: only 'drop' and 'keep' take a tau")
    if not isinstance(name, str) or name not in SHADOW_MODES:
        raise ValueError(f"unknown shadow mode {name!r}: one of " + ", ".join(SHADOW_MODES))
    if isinstance(tau, bool) or not isinstance(tau, (int, float, np.integer, np.floating)) or not (np.isfinite(tau) and 0 < tau <= 1):
        raise ValueError(f"shadows {shadows!r}: tau must be a finite number with 0 < tau <= 1")
    return name, float(tau)


def label_mode(labels):
    """(mode name, N) of a `labels` value: "corner", "count", ("cover", N) with N in 1 .. 64, or "cover" for ("cover", 1).  N is 1
    where the mode does not read it.  Anything else raises ValueError."""
    if isinstance(labels, str):
        name, n = labels, 1
    else:
        try:
            name, n = labels
        except (TypeError, ValueError):
            raise ValueError(f"labels {labels!r}: 'corner', 'count' or ('cover', N)") from None
        if name != "cover":
            raise ValueError(f"labels {labels!r}: only 'cover' takes a number")
    if name not in LABEL_MODES:
        raise ValueError(f"unknown label mode {name!r}: one of " + ", ".join(LABEL_MODES))
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= 64:
        raise ValueError(f"labels {labels!r}: N must be an integer in 1 .. 64")
    return name, int(n)


def work_dims(w: int, h: int, grid: str = "reference"):
    """(work_w, work_h) of a w x h source: 640x360 on the reference grid, half the source on the macroblock grid."""
    if grid not in GRIDS:
        raise ValueError(f"unknown grid {grid!r}: one of " + ", ".join(GRIDS))
    if (w, h) not in GRID_SIZES[grid]:
        raise ValueError(f"unsupported size {w}x{h} on the {grid} grid: one of " + ", ".join(f"{a}x{b}" for a, b in GRID_SIZES[grid]))
    return (WORK_W, WORK_H) if grid == "reference" else (w // 2, h // 2)


def label_dims(w: int, h: int, grid: str = "reference"):
    """(label_h, label_w) of a w x h source: one label per 8x8 block of the working image (its top-left pixel)."""
    ww, wh = work_dims(w, h, grid)
    return (wh + 7) // 8, (ww + 7) // 8


def work_dims_any(w: int, h: int):
    """(work_w, work_h) of a w x h source with any_size=True: half the source, for every even size of ANY_MIN .. ANY_MAX."""
    if w % 2 or h % 2 or not (ANY_MIN <= w <= ANY_MAX and ANY_MIN <= h <= ANY_MAX):
        raise ValueError(f"unsupported size {w}x{h} for any_size: even, {ANY_MIN} .. {ANY_MAX} in both axes")
    return w // 2, h // 2


def label_dims_any(w: int, h: int):
    """(label_h, label_w) of a w x h source with any_size=True: one label per macroblock, (ceil(h / 16), ceil(w / 16))."""
    ww, wh = work_dims_any(w, h)
    return (wh + 7) // 8, (ww + 7) // 8


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def yuv_tight(w: int, h: int, fmt: str, range: str = "limited", streams: int = 1, stream_major: bool = False,
              frames: int | None = None) -> L.MogYuv:
    """The dense layout of w x h 4:2:0 frames, w * h * 3 / 2 bytes each (the Y plane, then the UV plane of NV12 or the U and V
    planes of I420): frame-major [F][S][frame] as covahip_mog_yuv_tight gives it, or with stream_major [S][F][frame], which needs
    `frames` = F, the frames each stream has in the buffer."""
    if fmt not in FORMATS:
        raise ValueError(f"unknown format {fmt!r}: one of " + ", ".join(FORMATS))
    if range not in RANGES:
        raise ValueError(f"unknown range {range!r}: one of " + ", ".join(RANGES))
    if w < 2 or h < 2 or w % 2 or h % 2 or streams < 1:
        raise ValueError(f"4:2:0 frames need even sizes, got {w}x{h}")
    fb = w * h * 3 // 2
    lay = L.MogYuv()
    lay.format, lay.range = FORMATS[fmt], RANGES[range]
    if fmt == "nv12":
        lay.offset[:] = (0, w * h, 0)
        lay.pitch[:] = (w, w, 0)
    else:
        lay.offset[:] = (0, w * h, w * h + w * h // 4)
        lay.pitch[:] = (w, w // 2, w // 2)
    if stream_major:
        if frames is None or frames < 1:
            raise ValueError("a stream-major layout needs frames >= 1")
        lay.frame_stride, lay.stream_stride = fb, frames * fb
    else:
        lay.frame_stride, lay.stream_stride = streams * fb, fb
    return lay


class MogLabeler:
    """covahip_mog_* over one ctx: `streams` videos of src_w x src_h BGR24 frames advance per `apply` call.  `grid` is
    "reference" (640x360 working frames, 45x80 labels) or "macroblock" (half the source, one label per macroblock of the
    source; 2560x1440 and 3840x2160 sources are this grid's alone); work_w, work_h, label_h and label_w say which shapes the
    labeller takes and gives.  any_size=True (macroblock grid only) admits every size of work_dims_any: a size of
    GRID_SIZES["macroblock"] runs that grid's own kernels, any other the general ones (covahip_mog_create_any), which
    force_general=True (tests, measurements) takes at every size; the results do not depend on which.  `labels` is the label
    mode (label_mode; set_labels changes it later): "corner", the default, is the block's top-left pixel; ("cover", N) is 1 where
    64 * count >= N * inside for the block's foreground count and its pixels inside the image; "count" is that count, 0 .. 64,
    which is for inspection and no trainer input.  `shadows` (shadow_mode; set_shadows changes it later) turns MOG2's shadow
    detection on: None, the default, is the reference's detectShadows=False; "drop" takes shadow pixels for background before
    close, open and fill; "keep" runs the test and leaves the labels as they are without it; (mode, tau) gives the threshold."""

    def __init__(self, ctx, src_w: int, src_h: int, streams: int = 1, history: int = 9000, var_threshold: float = 32.0,
                 grid: str = "reference", any_size: bool = False, force_general: bool = False, labels="corner", shadows=None):
        label_mode(labels)                                                   # ValueError before the ctx is touched
        shadow_mode(shadows)
        if grid not in GRIDS:
            raise ValueError(f"unknown grid {grid!r}: one of " + ", ".join(GRIDS))
        any_size = any_size or force_general
        if any_size:
            if grid != "macroblock":
                raise ValueError("any_size needs grid='macroblock'")
            work_dims_any(src_w, src_h)                                      # ValueError before the ctx is touched
        elif (src_w, src_h) in GRID_SIZES["macroblock"] and (src_w, src_h) not in GRID_SIZES[grid]:
            raise ValueError(f"{src_w}x{src_h} needs grid='macroblock'")     # (any other size is the library's to refuse)
        self.ctx = ctx
        self._lib = L.lib()
        cfg = L.MogCfg()
        self._lib.covahip_mog_default_cfg(C.byref(cfg))
        cfg.src_w, cfg.src_h, cfg.n_streams, cfg.history, cfg.var_threshold = src_w, src_h, streams, history, var_threshold
        h = C.c_void_p()
        self.general = force_general or (any_size and (src_w, src_h) not in GRID_SIZES["macroblock"])
        if self.general:
            L.check(self._lib.covahip_mog_create_any(ctx.handle, C.byref(cfg), C.byref(h)), "covahip_mog_create_any", ctx.handle)
        else:
            L.check(self._lib.covahip_mog_create_grid(ctx.handle, C.byref(cfg), GRIDS[grid], C.byref(h)), "covahip_mog_create_grid",
                    ctx.handle)
        self.handle = h
        self.src_w, self.src_h, self.streams, self.grid = src_w, src_h, streams, grid
        d = [C.c_int32() for _ in range(4)]
        L.check(self._lib.covahip_mog_dims(h, *(C.byref(v) for v in d)), "covahip_mog_dims")
        self.work_w, self.work_h, self.label_w, self.label_h = (int(v.value) for v in d)
        if label_mode(labels)[0] != "corner":
            self.set_labels(labels)
        if shadow_mode(shadows)[0] != "off":
            self.set_shadows(shadows)

    def set_labels(self, labels):
        """The label mode of every later call (apply, apply_yuv, post_masks), for all streams: "corner", "count" or ("cover", N),
        N in 1 .. 64 ("cover" alone is N = 1).  The model and the masks do not depend on it, and reset keeps it."""
        name, n = label_mode(labels)
        L.check(self._lib.covahip_mog_set_labels(self.handle, LABEL_MODES[name], n), "covahip_mog_set_labels")

    @property
    def labels(self):
        """The label mode in force: "corner", "count" or ("cover", N)."""
        mode, n = C.c_int(), C.c_int()
        L.check(self._lib.covahip_mog_get_labels(self.handle, C.byref(mode), C.byref(n)), "covahip_mog_get_labels")
        name = {v: k for k, v in LABEL_MODES.items()}[mode.value]
        return (name, int(n.value)) if name == "cover" else name

    def set_shadows(self, shadows):
        """The shadow mode of every later apply / apply_yuv call, for all streams: None or "off", "drop", "keep", or (mode, tau).
        The model does not depend on it, and reset keeps it."""
        name, tau = shadow_mode(shadows)
        L.check(self._lib.covahip_mog_set_shadows(self.handle, SHADOW_MODES[name], tau), "covahip_mog_set_shadows")

    @property
    def shadows(self):
        """The shadow mode in force: None, or (mode, tau) with mode "drop" or "keep"."""
        mode, tau = C.c_int(), C.c_float()
        L.check(self._lib.covahip_mog_get_shadows(self.handle, C.byref(mode), C.byref(tau)), "covahip_mog_get_shadows")
        name = {v: k for k, v in SHADOW_MODES.items()}[mode.value]
        return None if name == "off" else (name, float(tau.value))

    def shadow_counts(self):
        """(shadow, foreground) of the last apply / apply_yuv call, u32 [F][S] each: the raw mask's pixels at 127 and at 255, counted
        on the device.  Frames past a stream's n_valid give 0; without shadow detection `shadow` is all 0."""
        nf = C.c_int()
        L.check(self._lib.covahip_mog_shadow_counts(self.handle, None, None, 0, C.byref(nf)), "covahip_mog_shadow_counts")
        shadow = np.zeros((nf.value, self.streams), np.uint32)
        fg = np.zeros_like(shadow)
        L.check(self._lib.covahip_mog_shadow_counts(self.handle, _ptr(shadow), _ptr(fg), shadow.size, C.byref(nf)),
                "covahip_mog_shadow_counts", self.ctx.handle)
        return shadow, fg

    def close(self):
        if getattr(self, "handle", None):
            if getattr(self.ctx, "handle", None):      # (a labeller outliving its closed ctx is not freed)
                self._lib.covahip_mog_destroy(self.handle)
            self.handle = None

    __del__ = close

    def _n_valid(self, n_valid, n_frames):
        if n_valid is None:
            return None
        nv = np.ascontiguousarray(n_valid, dtype=np.int32)
        if nv.shape != (self.streams,):
            raise ValueError(f"n_valid has shape {nv.shape}, expected ({self.streams},)")
        return nv

    def apply(self, frames: np.ndarray, n_valid=None, labels: np.ndarray | None = None) -> np.ndarray:
        """frames u8 [F][S][src_h][src_w][3] -> labels u8 [F][S][label_h][label_w].  n_valid[s] <= F: stream s takes only its first
        n_valid[s] frames, and its labels past them are left as `labels` holds them (zeros when no `labels` is given)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        want = (self.streams, self.src_h, self.src_w, 3)
        if frames.ndim != 5 or frames.shape[1:] != want:
            raise ValueError(f"frames of shape {frames.shape}, expected [F]{list(want)}")
        n = frames.shape[0]
        if labels is None:
            labels = np.zeros((n, self.streams, self.label_h, self.label_w), np.uint8)
        elif (labels.shape != (n, self.streams, self.label_h, self.label_w) or labels.dtype != np.uint8
              or not labels.flags.c_contiguous):
            raise ValueError(f"labels must be a C-contiguous u8 array [F][S][{self.label_h}][{self.label_w}]")
        nv = self._n_valid(n_valid, n)
        L.check(self._lib.covahip_mog_apply(self.handle, _ptr(frames), n, None if nv is None else _ptr(nv), _ptr(labels),
                                            L.MEM_HOST), "covahip_mog_apply", self.ctx.handle)
        return labels

    def apply_device(self, d_frames: int, n_frames: int, d_labels: int, n_valid=None):
        """The same on device pointers (frames u8 [F][S][src_h][src_w][3], labels u8 [F][S][label_h][label_w] on the ctx's GPU)."""
        nv = self._n_valid(n_valid, n_frames)
        L.check(self._lib.covahip_mog_apply(self.handle, d_frames, n_frames, None if nv is None else _ptr(nv), d_labels,
                                            L.MEM_DEVICE), "covahip_mog_apply", self.ctx.handle)

    def yuv_span(self, layout: L.MogYuv, n_frames: int) -> int:
        """Bytes from `base` to the last byte of the last row that an apply_yuv call of n_frames frames reads."""
        nv12 = layout.format == FORMATS["nv12"]
        rows = (self.src_h, self.src_h // 2, self.src_h // 2)
        rowb = (self.src_w, self.src_w if nv12 else self.src_w // 2, self.src_w // 2)
        hi = max(layout.offset[p] + (rows[p] - 1) * layout.pitch[p] + rowb[p] for p in range(2 if nv12 else 3))
        return (n_frames - 1) * layout.frame_stride + (self.streams - 1) * layout.stream_stride + hi

    def apply_yuv(self, buf: np.ndarray, layout: L.MogYuv, n_frames: int, n_valid=None, labels: np.ndarray | None = None) -> np.ndarray:
        """The labels of n_frames NV12 / I420 frames per stream in `buf` (u8, C-contiguous; byte 0 is the layout's base) ->
        u8 [F][S][label_h][label_w]: the working pixel is the converted one, as if `apply` had been given the BGR frames.  n_valid
        and labels as for `apply`.  The layout is the library's to refuse (CovahipError, status 1); a buffer shorter than what
        the layout reaches raises ValueError."""
        if not isinstance(buf, np.ndarray) or buf.dtype != np.uint8 or not buf.flags.c_contiguous:
            raise ValueError("buf must be a C-contiguous u8 array")
        n = int(n_frames)
        vals = list(layout.offset) + list(layout.pitch) + [layout.frame_stride, layout.stream_stride]
        if n >= 1 and min(vals) >= 0 and layout.format in FORMATS.values() and buf.nbytes < self.yuv_span(layout, n):
            raise ValueError(f"buf has {buf.nbytes} bytes, the layout reaches {self.yuv_span(layout, n)}")
        if labels is None:
            labels = np.zeros((max(n, 0), self.streams, self.label_h, self.label_w), np.uint8)
        elif (labels.shape != (n, self.streams, self.label_h, self.label_w) or labels.dtype != np.uint8
              or not labels.flags.c_contiguous):
            raise ValueError(f"labels must be a C-contiguous u8 array [F][S][{self.label_h}][{self.label_w}]")
        nv = self._n_valid(n_valid, n)
        L.check(self._lib.covahip_mog_apply_yuv(self.handle, C.byref(layout), _ptr(buf), n, None if nv is None else _ptr(nv),
                                                _ptr(labels), L.MEM_HOST), "covahip_mog_apply_yuv", self.ctx.handle)
        return labels

    def apply_yuv_device(self, d_base: int, layout: L.MogYuv, n_frames: int, d_labels: int, n_valid=None):
        """The same on device pointers: surfaces on the ctx's GPU from d_base, labels u8 [F][S][label_h][label_w] at d_labels."""
        nv = self._n_valid(n_valid, n_frames)
        L.check(self._lib.covahip_mog_apply_yuv(self.handle, C.byref(layout), d_base, n_frames, None if nv is None else _ptr(nv),
                                                d_labels, L.MEM_DEVICE), "covahip_mog_apply_yuv", self.ctx.handle)

    def reset(self, s: int):
        """Stream slot s starts a new video: model zeroed, frame count 0."""
        L.check(self._lib.covahip_mog_reset(self.handle, s), "covahip_mog_reset", self.ctx.handle)

    def set_stage_budget(self, nbytes: int):
        """Developer switch: device bytes of host frames staged per update launch of `apply` (0 = the default, 1 GiB)."""
        L.check(self._lib.covahip_dev_mog_set_stage_budget(self.handle, nbytes), "covahip_dev_mog_set_stage_budget")

    def set_post_form(self, banded: bool, band_rows: int = 0):
        """Developer switch: the post kernel of a macroblock-grid labeller, banded (band_rows rows per band, 0 = the automatic
        plan) or resident; the results do not depend on it."""
        L.check(self._lib.covahip_dev_mog_set_post_form(self.handle, int(bool(banded)), band_rows), "covahip_dev_mog_set_post_form")

    def post_masks(self, raw: np.ndarray) -> np.ndarray:
        """Developer entry: the post launch alone on raw u8 [F][S][work_h][work_w] (non-zero = foreground) -> labels; debug_masks
        then gives the raw / filled masks of this call.  The model is untouched."""
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        if raw.ndim != 4 or raw.shape[1:] != (self.streams, self.work_h, self.work_w):
            raise ValueError(f"raw of shape {raw.shape}, expected [F]{[self.streams, self.work_h, self.work_w]}")
        labels = np.zeros((raw.shape[0], self.streams, self.label_h, self.label_w), np.uint8)
        L.check(self._lib.covahip_dev_mog_post_masks(self.handle, _ptr(raw), raw.shape[0], _ptr(labels)), "covahip_dev_mog_post_masks",
                self.ctx.handle)
        return labels

    def state(self, s: int) -> dict:
        """Stream s's model: W f32 [5][work_h][work_w], V the same, M f32 [5][3][work_h][work_w], nmodes u8 [work_h][work_w], n."""
        W = np.empty((NMIX, self.work_h, self.work_w), np.float32)
        V = np.empty_like(W)
        M = np.empty((NMIX, 3, self.work_h, self.work_w), np.float32)
        nm = np.empty((self.work_h, self.work_w), np.uint8)
        n = C.c_int64()
        L.check(self._lib.covahip_dev_mog_state(self.handle, s, _ptr(W), _ptr(V), _ptr(M), _ptr(nm), C.byref(n)),
                "covahip_dev_mog_state", self.ctx.handle)
        return {"W": W, "V": V, "M": M, "nmodes": nm, "n": int(n.value)}

    def save_state(self, s: int) -> bytes:
        """Stream s's model and frame count as a state blob (read_state takes it apart)."""
        n = C.c_size_t()
        L.check(self._lib.covahip_mog_state_size(self.handle, C.byref(n)), "covahip_mog_state_size")
        buf = np.empty(n.value, np.uint8)
        L.check(self._lib.covahip_mog_save_state(self.handle, s, _ptr(buf), buf.nbytes, C.byref(n)), "covahip_mog_save_state",
                self.ctx.handle)
        return buf.tobytes()

    def load_state(self, s: int, blob):
        """Stream s continues from a state blob of this working size, whatever labeller saved it: from here on it gives what the
        saved stream would have given, bit for bit.  All or nothing: CovahipError (status 8: a damaged blob; status 1: a blob of another
        working size) leaves the labeller as it was."""
        data = np.frombuffer(bytes(blob), np.uint8)
        L.check(self._lib.covahip_mog_load_state(self.handle, s, _ptr(data), data.nbytes), "covahip_mog_load_state", self.ctx.handle)

    def set_frozen(self, frozen: bool, stream: int | None = None):
        """Later calls classify stream `stream`'s frames (None: every stream's) against its model and leave the model and its
        frame count as they are (frozen=True), or learn again (False).  reset keeps the setting."""
        L.check(self._lib.covahip_mog_set_frozen(self.handle, -1 if stream is None else stream, int(bool(frozen))),
                "covahip_mog_set_frozen")

    @property
    def frozen(self):
        """Per stream, whether it is frozen: a tuple of `streams` bools."""
        out = []
        for s in range(self.streams):
            v = C.c_int()
            L.check(self._lib.covahip_mog_get_frozen(self.handle, s, C.byref(v)), "covahip_mog_get_frozen")
            out.append(bool(v.value))
        return tuple(out)

    def background(self, s: int | None = None) -> np.ndarray:
        """The background image of stream s's model, u8 [work_h][work_w][3] (B, G, R); None: of every stream, [S][work_h][work_w][3].
        OpenCV's getBackgroundImage: the weighted mean of the modes whose weights add up to just above 0.9."""
        shape = (self.work_h, self.work_w, 3)
        out = np.empty(shape if s is not None else (self.streams,) + shape, np.uint8)
        L.check(self._lib.covahip_mog_background(self.handle, -1 if s is None else s, _ptr(out), out.nbytes, L.MEM_HOST),
                "covahip_mog_background", self.ctx.handle)
        return out

    def debug_masks(self):
        """(raw, filled) of the last apply call, u8 [F][S][work_h][work_w]: the MOG2 mask (0 / 255; with shadow detection on 0 / 127 / 255,
        127 = shadow, in "drop" and in "keep" mode alike) and the mask after close, open and hole fill (0 / 1)."""
        nf = C.c_int()
        L.check(self._lib.covahip_dev_mog_masks(self.handle, None, None, 0, C.byref(nf)), "covahip_dev_mog_masks")
        shape = (nf.value, self.streams, self.work_h, self.work_w)
        raw = np.empty(shape, np.uint8)
        filled = np.empty(shape, np.uint8)
        L.check(self._lib.covahip_dev_mog_masks(self.handle, _ptr(raw), _ptr(filled), raw.nbytes, C.byref(nf)),
                "covahip_dev_mog_masks", self.ctx.handle)
        return raw, filled


# ------------------------------------------------------------------------------------------------ raw BGR24 input
class _RawSource:
    """Whole frames of frame_bytes bytes of a raw stream; a trailing partial frame raises ValueError."""

    def __init__(self, src, frame_bytes: int):
        self.name = src if isinstance(src, str) else getattr(src, "name", "<stream>")
        if src == "-":
            self.f, self.own = sys.stdin.buffer, False
        elif isinstance(src, (str, bytes, os.PathLike)):
            self.f, self.own = open(src, "rb"), True
        else:
            self.f, self.own = src, False
        self.frame_bytes = frame_bytes
        self.frames = 0

    def read_into(self, out: np.ndarray) -> bool:
        """Fills out (one frame, C-contiguous) and returns True, or returns False at the end of the stream."""
        mv = memoryview(out).cast("B")
        got = 0
        while got < self.frame_bytes:
            n = self.f.readinto(mv[got:])
            if not n:
                break
            got += n
        if got == 0:
            return False
        if got < self.frame_bytes:
            raise ValueError(f"{self.name}: truncated input, {got} bytes after {self.frames} frames of {self.frame_bytes}")
        self.frames += 1
        return True

    def close(self):
        if self.own:
            self.f.close()


class _Bgr24Source(_RawSource):
    """Whole frames of a raw BGR24 stream."""

    def __init__(self, src, w: int, h: int):
        super().__init__(src, w * h * 3)


Y4M_CHROMA = ("420", "420jpeg", "420mpeg2", "420paldv")     # the 8-bit 4:2:0 tags: the same bytes, as tight I420


class _Y4mSource(_RawSource):
    """Whole frames of a YUV4MPEG2 stream: `YUV4MPEG2 W.. H.. [C420..] [XCOLORRANGE=FULL|LIMITED] ..\\n`, then per frame
    `FRAME..\\n` and tight I420.  w, h and range (None where the header has no XCOLORRANGE) come from the header; another
    chroma tag, a malformed header or a truncated frame raises ValueError."""

    def __init__(self, src):
        super().__init__(src, 0)
        try:
            tags = self._line(b"YUV4MPEG2", "a YUV4MPEG2 header").split()
            self.w = self.h = 0
            self.range = None
            for t in tags:
                if t[:1] == b"W":
                    self.w = int(t[1:])
                elif t[:1] == b"H":
                    self.h = int(t[1:])
                elif t[:1] == b"C" and t[1:].decode("ascii", "replace") not in Y4M_CHROMA:
                    raise ValueError(f"{self.name}: chroma {t[1:].decode('ascii', 'replace')!r} is not 8-bit 4:2:0 (one of "
                                     + ", ".join("C" + c for c in Y4M_CHROMA) + ")")
                elif t.startswith(b"XCOLORRANGE="):
                    v = t[12:].decode("ascii", "replace").lower()
                    if v not in RANGES:
                        raise ValueError(f"{self.name}: XCOLORRANGE={v!r} is neither FULL nor LIMITED")
                    self.range = v
            if self.w < 2 or self.h < 2 or self.w % 2 or self.h % 2:
                raise ValueError(f"{self.name}: no even W and H in the YUV4MPEG2 header")
        except ValueError:
            self.close()
            raise
        self.frame_bytes = self.w * self.h * 3 // 2

    def _line(self, magic: bytes, what: str, at_end_ok: bool = False):
        """The rest of a line that starts with `magic`; None at the end of the stream where that is allowed."""
        line = bytearray()
        while len(line) < 4096:
            c = self.f.read(1)
            if not c:
                break
            if c == b"\n":
                if not line.startswith(magic):
                    break
                return bytes(line[len(magic):])
            line += c
        if at_end_ok and not line:
            return None
        raise ValueError(f"{self.name}: expected {what} after {self.frames} frames, got {bytes(line[:16])!r}")

    def read_into(self, out: np.ndarray) -> bool:
        if self._line(b"FRAME", "a FRAME header", at_end_ok=True) is None:
            return False
        if not super().read_into(out):
            raise ValueError(f"{self.name}: truncated input, a FRAME header and no frame after {self.frames} frames")
        return True


def read_bgr24(path_or_stdin, w: int, h: int, chunk: int):
    """Yields u8 [k][h][w][3] chunks, 1 <= k <= chunk, of a raw BGR24 stream (a path, "-" for stdin, or a binary file
    object), to its end.  A trailing partial frame raises ValueError."""
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    yield from _chunks(_Bgr24Source(path_or_stdin, w, h), (h, w, 3), chunk)


def _chunks(src, frame_shape, chunk: int):
    try:
        buf = np.empty((chunk,) + tuple(frame_shape), np.uint8)
        while True:
            k = 0
            while k < chunk and src.read_into(buf[k]):
                k += 1
            if k == 0:
                return
            yield buf[:k].copy()
            if k < chunk:
                return
    finally:
        src.close()


def read_yuv420(path_or_stdin, w: int, h: int, chunk: int, fmt: str = "i420"):
    """Yields u8 [k][w * h * 3 / 2] chunks, 1 <= k <= chunk, of a raw NV12 or I420 stream of tight frames (yuv_tight(w, h, fmt)
    is a chunk's layout), with the contract of read_bgr24: a path, "-" or a binary file object, to its end; a trailing partial
    frame raises ValueError."""
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    if fmt not in FORMATS:
        raise ValueError(f"unknown format {fmt!r}: one of " + ", ".join(FORMATS))
    if w < 2 or h < 2 or w % 2 or h % 2:
        raise ValueError(f"4:2:0 frames need even sizes, got {w}x{h}")
    yield from _chunks(_RawSource(path_or_stdin, w * h * 3 // 2), (w * h * 3 // 2,), chunk)


class Y4mReader:
    """read_y4m's result: w, h, fmt ("i420") and range ("full" / "limited", or None where the header does not say) from the
    header; iterating yields u8 [k][w * h * 3 / 2] chunks of tight I420 frames, 1 <= k <= chunk, to the stream's end."""

    fmt = "i420"

    def __init__(self, path_or_stdin, chunk: int):
        if chunk < 1:
            raise ValueError("chunk must be >= 1")
        self._src = _Y4mSource(path_or_stdin)
        self._chunk = chunk
        self.w, self.h, self.range = self._src.w, self._src.h, self._src.range

    def __iter__(self):
        return _chunks(self._src, (self._src.frame_bytes,), self._chunk)

    def close(self):
        self._src.close()


def read_y4m(path_or_stdin, chunk: int) -> Y4mReader:
    """A YUV4MPEG2 stream (ffmpeg -f yuv4mpegpipe -pix_fmt yuv420p) from a path, "-" or a binary file object: the header is read
    at once (ValueError for a chroma tag other than C420 / C420jpeg / C420mpeg2 / C420paldv), the frames in chunks while
    iterating; a truncated frame raises ValueError."""
    return Y4mReader(path_or_stdin, chunk)


# ------------------------------------------------------------------------------------------------ command line
def parse_size(text: str):
    try:
        w, h = (int(v) for v in text.lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"size {text!r} is not WxH") from None
    if not any((w, h) in sizes for sizes in GRID_SIZES.values()):
        raise argparse.ArgumentTypeError(f"unsupported size {w}x{h}: one of " + ", ".join(f"{a}x{b}" for a, b in SIZES)
                                         + ", and with --grid macroblock "
                                         + ", ".join(f"{a}x{b}" for a, b in GRID_SIZES["macroblock"] if (a, b) not in SIZES))
    return w, h


def parse_any_size(text: str):
    try:
        w, h = (int(v) for v in text.lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"size {text!r} is not WxH") from None
    try:
        work_dims_any(w, h)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None
    return w, h


def parse_labels(text: str):
    """corner | cover[:N] | count -> a `labels` value of MogLabeler; cover alone is N = 1."""
    name, sep, num = text.partition(":")
    if name not in LABEL_MODES or (sep and name != "cover"):
        raise argparse.ArgumentTypeError(f"labels {text!r}: corner, cover[:N] or count")
    if name != "cover":
        return name
    if not sep:
        return "cover", 1
    if not (num.isascii() and num.isdigit()) or not 1 <= int(num) <= 64:
        raise argparse.ArgumentTypeError(f"labels {text!r}: N must be an integer in 1 .. 64")
    return "cover", int(num)


def parse_shadows(text: str):
    """off | drop[:TAU] | keep[:TAU] -> a `shadows` value of MogLabeler; TAU defaults to SHADOW_TAU."""
    name, sep, num = text.partition(":")
    if name not in SHADOW_MODES or (sep and name == "off"):
        raise argparse.ArgumentTypeError(f"shadows {text!r}: off, drop[:TAU] or keep[:TAU]")
    if name == "off":
        return None
    if not sep:
        return name, SHADOW_TAU
    try:
        return shadow_mode((name, float(num)))
    except ValueError:
        raise argparse.ArgumentTypeError(f"shadows {text!r}: TAU must be a number with 0 < TAU <= 1") from None


def parse_io(arg: str):
    """IN[:OUT] -> (IN, OUT); OUT defaults to IN's name with `_gt.dump`."""
    src, sep, out = arg.rpartition(":")
    if not sep:
        src, out = arg, ""
    if not src:
        raise argparse.ArgumentTypeError(f"{arg!r}: no input")
    if not out:
        if src == "-":
            raise argparse.ArgumentTypeError("stdin ('-') needs an output: -:OUT_gt.dump")
        out = os.path.splitext(src)[0] + "_gt.dump"
    return src, out


def _args(argv):
    ap = argparse.ArgumentParser(prog="python -m cova_amd.mog", description=__doc__.split("\n")[0])
    ap.add_argument("inputs", nargs="*", type=parse_io, metavar="IN[:OUT]",
                    help="raw video in --format ('-' = stdin); OUT defaults to IN's name with _gt.dump")
    ap.add_argument("--size", type=parse_size, default=None,
                    help="source size: 640x360, 1280x720 or 1920x1080; with --grid macroblock also 2560x1440 and 3840x2160 "
                         "(optional with --format y4m, whose header has it)")
    ap.add_argument("--any-size", type=parse_any_size, default=None, metavar="WxH",
                    help=f"instead of --size: any even source size, {ANY_MIN} .. {ANY_MAX} in both axes, on the macroblock grid "
                         "(1280x960 -> 60x80 labels); a y4m header must state the same size")
    ap.add_argument("--format", choices=("bgr24", "nv12", "i420", "y4m"), default="bgr24",
                    help="bgr24: packed BGR, 3 bytes per pixel; nv12, i420: tight 4:2:0 frames, 1.5 bytes per pixel; y4m: "
                         "YUV4MPEG2 (ffmpeg -f yuv4mpegpipe -pix_fmt yuv420p)")
    ap.add_argument("--range", choices=sorted(RANGES), default=None,
                    help="of the YUV formats: limited (video, Y 16..235; the default) or full (JPEG, yuvj420p); a y4m header's XCOLORRANGE "
                         "must agree with it where one is given")
    ap.add_argument("--grid", choices=sorted(GRIDS), default=None,
                    help="reference: 45x80 labels whatever the source (the 1280x720 macroblock grid); macroblock: one label per "
                         "macroblock of the source, which 1080p records need (1920x1080 -> 68x120, 2560x1440 -> 90x160, "
                         "3840x2160 -> 135x240)")
    ap.add_argument("--labels", type=parse_labels, default="corner", metavar="corner|cover[:N]|count",
                    help="how a block becomes a label.  corner (the default): its top-left pixel, the reference's ::8 subsample; "
                         "cover[:N], N in 1 .. 64 (default 1): 1 where at least N / 64 of the block's pixels inside the image are "
                         "foreground, so an object narrower than a block keeps its label; count: that number of pixels, a byte "
                         "0 .. 64 -- for inspection and for choosing N (tools/label_cover.py), not a trainer input")
    ap.add_argument("--shadows", type=parse_shadows, default=None, metavar="off|drop[:TAU]|keep[:TAU]",
                    help="MOG2's shadow detection (OpenCV's detectShadows; TAU, default 0.5, is how dark a shadow may be relative to "
                         "the background).  off (the default): none, as the reference.  drop: shadow pixels count as background, so a "
                         "vehicle's cast shadow stays out of its label.  keep: the test runs and the labels stay as without it -- with "
                         "--shadow-report it shows what drop would remove.  Note: --balance of the trainer thresholds a frame's label sum, "
                         "which shrinks under drop")
    ap.add_argument("--shadow-report", action="store_true",
                    help="print, per input, the mean share of shadow and of foreground pixels per frame (how TAU gets chosen for a "
                         "camera); needs --shadows drop or keep")
    ap.add_argument("--load-state", nargs="+", action="extend", default=None, metavar="FILE",
                    help="one state blob per input, in order (give the inputs first): the input's slot starts from the blob's model "
                         "and frame count instead of an empty model")
    ap.add_argument("--save-state", nargs="+", action="extend", default=None, metavar="FILE",
                    help="one file per input, in order: the model is written there when the input ends (with --two-pass: the model "
                         "its first pass ended with)")
    ap.add_argument("--frozen", action="store_true",
                    help="label without learning: every frame is classified against the loaded model, which stays as it is; needs "
                         "--load-state")
    ap.add_argument("--two-pass", action="store_true",
                    help="per input, a first pass learns and writes nothing; then the input is read again and labelled against the "
                         "learned model, frozen: the start of a clip gets a settled model.  Files only")
    ap.add_argument("--background", nargs="+", action="extend", default=None, metavar="FILE",
                    help="one binary PPM (RGB) per input, in order: the model's background image at the working size, written when "
                         "the input ends")
    ap.add_argument("--streams", type=int, default=None, help="videos labelled side by side (default: inputs, at most 8)")
    ap.add_argument("--chunk", type=int, default=16, help="frames per stream and call")
    ap.add_argument("--history", type=int, default=9000)
    ap.add_argument("--var-threshold", type=float, default=32.0)
    ap.add_argument("--device", type=int, default=0)
    # `-:OUT` (stdin) starts with a dash, so argparse takes it for an option it does not know: such arguments are inputs
    a, rest = ap.parse_known_args(argv)
    for r in rest:
        if not r.startswith("-:"):
            ap.error(f"unrecognized arguments: {r}")
        try:
            a.inputs.append(parse_io(r))
        except argparse.ArgumentTypeError as e:
            ap.error(str(e))
    if not a.inputs:
        ap.error("the following arguments are required: IN[:OUT]")
    if a.any_size is not None:
        if a.size is not None:
            ap.error("--any-size stands instead of --size: give one of them")
        if a.grid == "reference":
            ap.error("--any-size is on the macroblock grid: it cannot go with --grid reference")
        a.size, a.grid = a.any_size, "macroblock"
    a.grid = a.grid or "reference"
    a.range_given = a.range is not None
    a.range = a.range or "limited"
    if a.size is None and a.format != "y4m":
        ap.error(f"--format {a.format} needs --size")
    if a.size is not None and a.any_size is None and a.size not in GRID_SIZES[a.grid]:
        ap.error(f"--size {a.size[0]}x{a.size[1]} needs --grid macroblock")
    if a.streams is None:
        a.streams = min(len(a.inputs), 8)
    if not 1 <= a.streams <= MAX_STREAMS:
        ap.error(f"--streams must be in [1, {MAX_STREAMS}]")
    if a.chunk < 1:
        ap.error("--chunk must be >= 1")
    if a.shadow_report and a.shadows is None:
        ap.error("--shadow-report needs --shadows drop or keep")
    if a.history < 1:
        ap.error("--history must be >= 1")
    if not (np.isfinite(a.var_threshold) and a.var_threshold > 0):
        ap.error("--var-threshold must be > 0")
    if sum(src == "-" for src, _ in a.inputs) > 1:
        ap.error("stdin ('-') can be read once")
    outs = [out for _, out in a.inputs]
    for opt, files in (("--load-state", a.load_state), ("--save-state", a.save_state), ("--background", a.background)):
        if files is not None and len(files) != len(a.inputs):
            ap.error(f"{opt} takes one file per input: {len(files)} for {len(a.inputs)} inputs")
        if files is not None and opt != "--load-state":
            outs = outs + files
    if len(set(outs)) != len(outs):
        ap.error("two inputs write the same output")
    if a.frozen and a.load_state is None:
        ap.error("--frozen needs --load-state: an empty model calls everything foreground")
    if a.two_pass and a.frozen:
        ap.error("--two-pass learns in its first pass: it cannot go with --frozen")
    if a.two_pass and any(src == "-" for src, _ in a.inputs):
        ap.error("--two-pass reads every input twice: stdin ('-') cannot be one")
    for f in a.load_state or ():
        if not os.path.isfile(f):
            ap.error(f"--load-state {f}: no such file")
    return a


def main(argv=None) -> int:
    a = _args(argv)
    from .elements import Context

    def fail(msg):                # as argparse's error(): a usage mistake is exit status 2
        print(f"python -m cova_amd.mog: error: {msg}", file=sys.stderr)
        raise SystemExit(2)

    # y4m: every header must agree with --size, --range and the other headers.  Files are looked at before anything is set up;
    # stdin can be read once, so its source is opened here (and kept) only where nothing else gives the size.
    opened = {}
    y4m_range = [a.range if a.range_given else None]

    def y4m_open(src):
        try:
            y = opened.pop(src, None) or _Y4mSource(src)
        except (OSError, ValueError) as e:
            fail(str(e))
        if a.size is None:
            try:
                a.size = parse_size(f"{y.w}x{y.h}")
            except argparse.ArgumentTypeError as e:
                y.close()
                fail(f"{y.name}: {e}")
            if a.size not in GRID_SIZES[a.grid]:
                y.close()
                fail(f"{y.name}: {y.w}x{y.h} needs --grid macroblock")
        if (y.w, y.h) != a.size:
            y.close()
            fail(f"{y.name}: the header says {y.w}x{y.h}, expected {a.size[0]}x{a.size[1]}")
        if y.range is not None:
            if y4m_range[0] is not None and y.range != y4m_range[0]:
                y.close()
                fail(f"{y.name}: the header says XCOLORRANGE={y.range.upper()}, expected {y4m_range[0]}")
            y4m_range[0] = y.range
        return y

    if a.format == "y4m":
        for src, _ in a.inputs:
            if src != "-":
                y4m_open(src).close()
        if a.size is None:
            opened["-"] = y4m_open("-")
        if y4m_range[0] is not None:
            a.range = y4m_range[0]
        y4m_range[0] = a.range          # from here on a header that names a range names this one
    w, h = a.size
    S = min(a.streams, len(a.inputs))
    pending = [(i,) + io for i, io in enumerate(a.inputs)]
    yuv = a.format != "bgr24"
    ctx = Context(a.device)
    mog = MogLabeler(ctx, w, h, streams=S, history=a.history, var_threshold=a.var_threshold, grid=a.grid, any_size=a.any_size is not None,
                     labels=a.labels, shadows=a.shadows)
    layout = yuv_tight(w, h, "nv12" if a.format == "nv12" else "i420", a.range, streams=S) if yuv else None
    frames = np.empty((a.chunk, S, w * h * 3 // 2) if yuv else (a.chunk, S, h, w, 3), np.uint8)
    labels = np.zeros((a.chunk, S, mog.label_h, mog.label_w), np.uint8)
    slots = [None] * S           # [source, output file, output name, start time, input index, first pass of two] per stream slot
    npix = mog.work_w * mog.work_h
    tally = [[0, 0] for _ in range(S)]      # --shadow-report: shadow and foreground pixels of the slot's video so far

    def open_next(s):
        if not pending:
            slots[s] = None
            return
        i, src, out = pending.pop(0)
        slots[s] = [open_source(src), open(out, "wb"), out, time.perf_counter(), i, a.two_pass]
        tally[s] = [0, 0]
        mog.set_frozen(a.frozen, s)
        if a.load_state is None:
            mog.reset(s)
        else:
            with open(a.load_state[i], "rb") as f:
                mog.load_state(s, f.read())

    def open_source(src):
        return y4m_open(src) if a.format == "y4m" else _RawSource(src, w * h * 3 // 2) if yuv else _Bgr24Source(src, w, h)

    def save_state(s):
        if a.save_state is not None:
            with open(a.save_state[slots[s][4]], "wb") as f:
                f.write(mog.save_state(s))

    def finish(s):
        """The slot's input has ended.  True: the slot is done with it; False: its first pass is, and the second begins."""
        src, f, out, t0, i, learning = slots[s]
        src.close()
        if learning:                   # --two-pass: the model is learned; now the same frames, frozen
            save_state(s)
            slots[s][0], slots[s][5] = open_source(src.name), False
            tally[s] = [0, 0]
            mog.set_frozen(True, s)
            return False
        if not a.two_pass:
            save_state(s)
        if a.background is not None:
            with open(a.background[i], "wb") as g:
                g.write(b"P6\n%d %d\n255\n" % (mog.work_w, mog.work_h) + np.ascontiguousarray(mog.background(s)[..., ::-1]).tobytes())
        f.close()
        dt = time.perf_counter() - t0
        print(f"{src.name}: {src.frames} frames, {src.frames / dt if dt > 0 else 0.0:.1f} frames/s -> {out}", file=sys.stderr)
        if a.shadow_report:
            per = max(src.frames, 1) * npix
            print(f"{src.name}: shadow {tally[s][0] / per:.6f} foreground {tally[s][1] / per:.6f} of {npix} pixels per frame, "
                  f"{src.frames} frames, --shadows {a.shadows[0]}:{a.shadows[1]:g}")
        return True

    try:
        for s in range(S):
            open_next(s)
        while any(slots):
            nv = np.zeros(S, np.int32)
            for s in range(S):
                while slots[s] is not None:
                    k = 0
                    while k < a.chunk and slots[s][0].read_into(frames[k, s]):
                        k += 1
                    if k:
                        nv[s] = k
                        break
                    if finish(s):      # this video has ended: the slot takes the next one
                        open_next(s)
            if not nv.any():
                break
            if yuv:
                mog.apply_yuv(frames, layout, int(nv.max()), n_valid=nv, labels=labels[:int(nv.max())])
            else:
                mog.apply(frames[:int(nv.max())], n_valid=nv, labels=labels[:int(nv.max())])
            if a.shadow_report:
                sh, fg = mog.shadow_counts()
                for s in range(S):
                    if slots[s] is None or slots[s][5]:
                        continue
                    tally[s][0] += int(sh[:, s].sum())
                    tally[s][1] += int(fg[:, s].sum())
            for s in range(S):
                if nv[s] and not slots[s][5]:
                    slots[s][1].write(np.ascontiguousarray(labels[:nv[s], s]).tobytes())
    finally:
        for s in range(S):
            if slots[s] is not None:
                slots[s][0].close()
                slots[s][1].close()
        mog.close()
        ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
