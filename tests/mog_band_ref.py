"""Planted masks for the banded post kernel of the MoG labeller (cova_amd/csrc/mog_band.hip; tests/test_gpu_mog_band.py feeds
them through covahip_dev_mog_post_masks and compares with tests/mog_ref.py's post), on top of tests/mog_grid_ref.py:

  band_plan         covahip_dev_mog_band_plan: (rows, bands, lds_bytes) of a working size, and its seam rows
  bernoulli, blocks random masks: independent pixels, and random 8x8 blocks (many diagonal seals and holes)
  coarse_spirals    the spiral of mog_grid_ref with a 56-pixel gap and its sealed twin (the 8-pixel gap costs the oracle 6.6 s)
  corner_blob       the last 20 rows x last 60 columns
  seam_corridors    mog_grid_ref's corridor cavity once around every seam row
  seam_morphology   gaps that closing shuts (3 rows) or not (4), bars that opening removes (5 rows) or not (6), at every seam row
                    and every offset -3 .. +3 around it, each across a word boundary
  serpentine        full-height lanes joined alternately at the bottom and the top behind a sealed border with one entrance
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from cova_amd import _lib as L
from tests import mog_grid_ref as G
from tests import mog_ref as R


def band_plan(work_w: int, work_h: int):
    rows, bands, lds = C.c_int(), C.c_int(), C.c_size_t()
    rc = L.lib().covahip_dev_mog_band_plan(work_w, work_h, C.byref(rows), C.byref(bands), C.byref(lds))
    if rc:
        raise ValueError(f"covahip_dev_mog_band_plan({work_w}, {work_h}) = {rc}")
    return rows.value, bands.value, lds.value


def seams(work_h: int, rows: int):
    """First rows of the bands after the first."""
    return list(range(rows, work_h, rows))


def to_u8(mask: np.ndarray) -> np.ndarray:
    return np.where(mask, 255, 0).astype(np.uint8)


def post(mask: np.ndarray):
    """The oracle on a bool mask: (filled u8, labels u8)."""
    return R.post(to_u8(mask))


def bernoulli(h: int, w: int, density: float, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).random((h, w)) < density


def blocks(h: int, w: int, density: float, seed: int, size: int = 8) -> np.ndarray:
    b = np.random.default_rng(seed).random(((h + size - 1) // size, (w + size - 1) // size)) < density
    return np.kron(b, np.ones((size, size), bool))[:h, :w]


def coarse_spirals(h: int, w: int):
    sp = G._spiral(h, w, 8, 56)
    sealed = sp.copy()
    sealed[8:16, 8:w - 8] = sealed[h - 16:h - 8, 8:w - 8] = True
    sealed[8:h - 8, 8:16] = sealed[8:h - 8, w - 16:w - 8] = True
    return sp, sealed


def corner_blob(h: int, w: int) -> np.ndarray:
    a = np.zeros((h, w), bool)
    a[h - 20:, w - 60:] = True
    return a


def seam_corridors(h: int, w: int, k: int, seam_rows) -> np.ndarray:
    """G._corridor's slab, cavity and corridor (k pixels high) around every seam row: the slab is 60 rows high and starts 30
    rows above the seam, so the slab's edges lie in different bands, and the cavity (40 rows) and the corridor straddle the seam
    (the corridor's k rows start at seam - k // 2, so that k = 1 lies on the seam row and k = 4 on two rows either side)."""
    a = np.zeros((h, w), bool)
    x0 = 64 * (w // 128) - 12
    for s in seam_rows:
        if s - 30 < 0 or s + 30 > h:
            continue
        a[s - 30:s + 30, x0 - 40:w - 10] = True
        a[s - 20:s + 20, x0 - 30:x0] = False
        a[s - k // 2:s - k // 2 + k, x0:w - 10] = False
    return a


def seam_morphology(h: int, w: int, seam_rows) -> np.ndarray:
    """Per seam row s and offset o in -3 .. 3, four features 40 pixels wide centred on word boundaries 64 c (so each crosses
    one), p = s + o: two 12-row slabs with a gap of 3 rows around p, the same with 4 rows, a bar of 5 rows, a bar of 6 rows."""
    a = np.zeros((h, w), bool)
    for s in seam_rows:
        c = 1
        for o in range(-3, 4):
            p = s + o
            for kind in range(4):
                if 64 * c + 20 > w or p - 16 < 0 or p + 16 > h:
                    continue
                x = slice(64 * c - 20, 64 * c + 20)
                if kind == 0:
                    a[p - 13:p + 14, x] = True
                    a[p - 1:p + 2, x] = False
                elif kind == 1:
                    a[p - 14:p + 14, x] = True
                    a[p - 2:p + 2, x] = False
                elif kind == 2:
                    a[p - 2:p + 3, x] = True
                else:
                    a[p - 3:p + 3, x] = True
                c += 1
    return a


def serpentine(h: int, w: int, lanes: int = 6, closed_last: bool = False) -> np.ndarray:
    """A sealed border 8 pixels thick (8 pixels inside the frame edge) with one 8-pixel entrance in its top side above lane 0;
    `lanes` full-height lanes separated by 8-pixel walls that are open (24 rows) alternately at the bottom and at the top, so
    the only path from the entrance runs down and up through every row of every lane.  closed_last: the opening into the last
    lane is walled up, and exactly that lane is a hole."""
    a = np.zeros((h, w), bool)
    a[8:16, 8:w - 8] = a[h - 16:h - 8, 8:w - 8] = True
    a[8:h - 8, 8:16] = a[8:h - 8, w - 16:w - 8] = True
    inner = w - 32
    lane_w = inner // lanes
    a[8:16, 16 + lane_w // 2 - 4:16 + lane_w // 2 + 4] = False          # the entrance
    for i in range(1, lanes):
        x = 16 + i * lane_w
        a[16:h - 16, x - 4:x + 4] = True
        if not (closed_last and i == lanes - 1):
            if i % 2:
                a[h - 40:h - 16, x - 4:x + 4] = False                   # open at the bottom
            else:
                a[16:40, x - 4:x + 4] = False                           # open at the top
    return a


def last_lane(h: int, w: int, lanes: int = 6):
    """(rows, columns) slices of the last lane's interior."""
    lane_w = (w - 32) // lanes
    return slice(16, h - 16), slice(16 + (lanes - 1) * lane_w + 4, w - 16)
