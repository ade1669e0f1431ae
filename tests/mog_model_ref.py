"""numpy float32 restatements of what reads a MoG model without changing it (include/covahip.h, "MoG labels": frozen labelling,
the background image, the state blob), on top of tests/mog_ref.py and tests/mog_shadow_ref.py.  Vectorised over pixels, looped
over the five modes; every product and sum is an np.float32 operation of its own, in the order the header states.

  classify         the frozen mask 0 / 255 of a frame against a mog_ref.Mog2, which is only read
  classify3        the same with the shadow test on the model AS IT IS where the mask is 255: 0 / 127 / 255
  zero_rate_mask   the mask of Mog2.apply with the learning rate forced to 0, on a copy: what `classify` must equal
  background       OpenCV's getBackgroundImage_intern restated: u8 [P][3]
  pack / unpack    the "CVHM" blob, written and read here independently of cova_amd.mog, with a CRC-32C of this file's own
  model_of / arrays_of   a Mog2 from unpacked arrays and back
  hand_models      the hand-built 128x128 model whose row 0 holds the edge cases of `background`, with the bytes they must give
"""
from __future__ import annotations

import copy
import struct

import numpy as np

from tests import mog_ref as R
from tests import mog_shadow_ref as SR

F32 = np.float32
MAGIC, VERSION, HEADER = 0x4D485643, 1, 64      # "CVHM"


def classify(model: R.Mog2, frame: np.ndarray) -> np.ndarray:
    """frame u8 [..][3] of P pixels -> mask u8 of the frame's shape without the channels: 0 background / 255 foreground."""
    data = frame.reshape(-1, 3).T.astype(F32)
    P = data.shape[1]
    bg = np.zeros(P, bool)
    done = np.zeros(P, bool)
    tw = np.zeros(P, F32)
    for mode in range(R.NMIX):
        act = (mode < model.nmodes) & ~done
        if not act.any():
            continue
        d = model.M[mode] - data
        dist2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        var = model.V[mode]
        bg |= act & (tw < R.TB) & (dist2 < model.Tb * var)
        fit = act & (dist2 < R.TG * var)
        done |= fit
        tw = np.where(act & ~fit, tw + model.W[mode], tw)
    return np.where(bg, 0, 255).astype(np.uint8).reshape(frame.shape[:-1])


def classify3(model: R.Mog2, frame: np.ndarray, tau: float) -> np.ndarray:
    """classify, then the shadow test of step 2a where the mask is 255, on the model as it is: 0 / 127 / 255."""
    mask = classify(model, frame)
    sh = SR.shadow_mask(model, frame, tau, where=mask.reshape(-1) == 255)
    return np.where(sh.reshape(mask.shape), np.uint8(127), mask)


def zero_rate_mask(model: R.Mog2, frame: np.ndarray) -> np.ndarray:
    """The mask Mog2.apply gives `frame` with alphaT = 0 and prune = -0 * fCT (OpenCV's apply(frame, 0)), on a copy of the
    model: the model given is not changed.  The copy may end with non-finite values: that is the finding this mode exists for."""
    mdl = copy.deepcopy(model)
    keep = R.learning_rates
    R.learning_rates = lambda n, history: (F32(0.0), F32(-0.0 * float(R.FCT)))
    try:
        return mdl.apply(frame)
    finally:
        R.learning_rates = keep


def background(model: R.Mog2) -> np.ndarray:
    """u8 [P][3]: per pixel the weighted mean of the first modes whose weights pass TB, rounded half to even and saturated."""
    P = model.P
    acc = np.zeros((3, P), F32)
    tw = np.zeros(P, F32)
    done = np.zeros(P, bool)
    for mode in range(R.NMIX):
        act = (mode < model.nmodes) & ~done
        if not act.any():
            continue
        w = model.W[mode]
        for c in range(3):
            acc[c] = np.where(act, acc[c] + w * model.M[mode][c], acc[c])
        tw = np.where(act, tw + w, tw)
        done |= act & (tw > R.TB)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = np.where(np.abs(tw) > R.FLT_EPSILON, F32(1) / tw, F32(0)).astype(F32)
        val = np.rint(acc * inv)                                 # (np.rint rounds half to even)
    return np.clip(val, 0, 255).astype(np.uint8).T.copy()


# ------------------------------------------------------------------------------------------------ the blob
def _crc_table():
    t = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
        t.append(c)
    return t


_CRC = _crc_table()


def crc32c(data: bytes) -> int:
    """CRC-32C (Castagnoli, reflected, unmasked), byte by byte: for small blobs."""
    c = 0xFFFFFFFF
    for b in bytes(data):
        c = _CRC[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def blob_size(w: int, h: int) -> int:
    return HEADER + 101 * w * h + 4


def pack(W, V, M, nmodes, n=0, history=9000, var_threshold=32.0, crc=None) -> bytes:
    """The blob of arrays W, V [5][h][w], M [5][3][h][w], nmodes [h][w]; `crc` stands in for the computed one where given."""
    h, w = np.asarray(nmodes).shape
    head = struct.pack("<4sIiiifq", b"CVHM", VERSION, w, h, history, var_threshold, n) + bytes(32)
    body = head + b"".join(np.ascontiguousarray(a, "<f4").tobytes() for a in (W, V, M)) + np.ascontiguousarray(nmodes, np.uint8).tobytes()
    assert len(head) == HEADER and len(body) == blob_size(w, h) - 4
    return body + struct.pack("<I", crc32c(body) if crc is None else crc)


def unpack(blob: bytes, verify: bool = True) -> dict:
    """The blob's header fields and arrays.  verify: the CRC is checked with this file's byte loop (slow on large blobs)."""
    magic, version, w, h, history, tb, n = struct.unpack_from("<IIiiifq", blob, 0)
    assert magic == MAGIC and version == VERSION and len(blob) == blob_size(w, h), (hex(magic), version, w, h, len(blob))
    assert blob[32:HEADER] == bytes(32)
    if verify:
        assert struct.unpack_from("<I", blob, len(blob) - 4)[0] == crc32c(blob[:-4])
    P = w * h
    f = np.frombuffer(blob, "<f4", 25 * P, HEADER)
    return {"work_w": w, "work_h": h, "history": history, "var_threshold": tb, "n": n, "W": f[:5 * P].reshape(5, h, w).copy(),
            "V": f[5 * P:10 * P].reshape(5, h, w).copy(), "M": f[10 * P:].reshape(5, 3, h, w).copy(),
            "nmodes": np.frombuffer(blob, np.uint8, P, HEADER + 100 * P).reshape(h, w).copy()}


def model_of(st: dict, history: int = 9000, var_threshold: float = 32.0) -> R.Mog2:
    """A Mog2 holding the arrays of an unpacked blob or of MogLabeler.state()."""
    h, w = st["nmodes"].shape
    m = R.Mog2(npix=h * w, history=history, var_threshold=var_threshold)
    m.W, m.V = st["W"].reshape(5, -1).astype(F32), st["V"].reshape(5, -1).astype(F32)
    m.M = st["M"].reshape(5, 3, -1).astype(F32)
    m.nmodes = st["nmodes"].reshape(-1).astype(np.int32)
    m.n = int(st["n"])
    return m


def arrays_of(model: R.Mog2, h: int, w: int) -> dict:
    return {"W": model.W.reshape(5, h, w), "V": model.V.reshape(5, h, w), "M": model.M.reshape(5, 3, h, w),
            "nmodes": model.nmodes.reshape(h, w).astype(np.uint8), "n": model.n}


# ------------------------------------------------------------------------------------------------ hand-built models
HAND_W = HAND_H = 128           # the working size of the smallest any-size labeller (256x256 sources)
# x in row 0 -> (nmodes, weights, means per mode, the bytes the background image must hold there)
HAND_CASES = (
    (1, (1.0,), ((10, 20, 30),), (10, 20, 30)),                                   # one mode
    (2, (0.5, 0.5), ((100, 101, 7), (101, 102, 7)), (100, 102, 7)),               # 100.5 -> 100, 101.5 -> 102: half to even
    (2, (0.95, 0.05), ((50, 60, 70), (250, 250, 250)), (50, 60, 70)),             # the first mode passes TB and ends the walk
    (1, (1e-8,), ((200, 200, 200),), (0, 0, 0)),                                  # tw <= FLT_EPSILON: inv = 0
    (1, (1.0,), ((300, -20, 128),), (255, 0, 128)),                               # saturation at both ends
    (0, (1.0,), ((99, 99, 99),), (0, 0, 0)),                                      # nmodes = 0: what the arrays hold is not read
)


def hand_models():
    """(arrays as `pack` takes them, expected u8 [HAND_H][HAND_W][3]): everything empty but the cases in row 0."""
    W = np.zeros((5, HAND_H, HAND_W), F32)
    V = np.zeros_like(W)
    M = np.zeros((5, 3, HAND_H, HAND_W), F32)
    nm = np.zeros((HAND_H, HAND_W), np.uint8)
    want = np.zeros((HAND_H, HAND_W, 3), np.uint8)
    for x, (n, ws, means, out) in enumerate(HAND_CASES):
        nm[0, x] = n
        for k, (wk, mk) in enumerate(zip(ws, means)):
            W[k, 0, x], V[k, 0, x], M[k, :, 0, x] = wk, 15.0, mk
        want[0, x] = out
    return {"W": W, "V": V, "M": M, "nmodes": nm}, want
