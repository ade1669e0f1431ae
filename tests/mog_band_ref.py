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
  right_edge        a slab at the right edge with three cavities: open to column w - 1, behind a wall of 4 columns, behind one of 5

and, for the any-size labeller's range (tests/test_gpu_mog_any_range.py, tests/test_mog_any_range_host.py):

  band_max_rows, auto_plan   the band plan restated from the documented constants, held against the library's
  RANGE_SHAPES, RANGE_FULL   the working sizes and forced band heights of the range tests
  pick_seams        the seam rows of a plan that the seam planes are built around
  range_names, range_plane, range_oracle   the planes of a (shape, plan) by name, and the oracle on them, each computed once
"""
from __future__ import annotations

import ctypes as C
import functools

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


def right_edge_rows(h: int):
    """(slab rows, first rows of the three 20-row cavities) of right_edge at height h: the rows of the 330x190 case it was made
    for wherever they fit (h >= 190), else a slab from row 10 to h - 10 with the cavities spread evenly (h >= 128: the walls
    between them are at least 12 rows, which the opening leaves)."""
    if h >= 190:
        return (20, 170), (35, 80, 125)
    gap = (h - 20 - 60) // 4
    return (10, h - 10), tuple(10 + gap + i * (20 + gap) for i in range(3))


def right_edge(h: int, w: int) -> np.ndarray:
    """Foreground columns w - 3 .. w - 1 over the full height (too thin for the opening: gone afterwards), and a slab at the
    right edge with three cavities: one open to the edge at column w - 1, which must not fill; one behind a wall of 4 columns,
    which the morphology opens to the edge too; one behind a wall of 5, one pixel further in, which must fill.  h >= 128."""
    (y0, y1), (c0, c1, c2) = right_edge_rows(h)
    a = np.zeros((h, w), bool)
    a[:, w - 3:] = True
    a[y0:y1, w - 60:] = True
    a[c0:c0 + 20, w - 40:w] = False
    a[c1:c1 + 20, w - 40:w - 4] = False
    a[c2:c2 + 20, w - 40:w - 5] = False
    return a


# ------------------------------------------------------------------------------------------------ the band plan, restated
LDS_MAX = 160 * 1024 - 64                              # COVAHIP_MOG_BAND_LDS_MAX
FLAG_BYTES, FILL_SEG, HALO = 16, 16, 10 + 6            # the flags; row segments of the column sweep; staged rows above + below a band


def pitch(work_w: int) -> int:
    return -(-work_w // 64) * 64


def band_lds_bytes(work_w: int, work_h: int, rows: int) -> int:
    """Flags, the sweep's carries (2 x 16 x roww words), two windows of min(rows + 16, work_h) rows of roww words."""
    roww = pitch(work_w) // 64
    return FLAG_BYTES + 2 * FILL_SEG * roww * 8 + 2 * min(rows + HALO, work_h) * roww * 8


def band_max_rows(work_w: int) -> int:
    """The highest band whose window of rows + 16 rows fits LDS_MAX at this width."""
    roww = pitch(work_w) // 64
    return (LDS_MAX - FLAG_BYTES - 2 * FILL_SEG * roww * 8) // (2 * roww * 8) - HALO


def auto_plan(work_w: int, work_h: int):
    """(rows, bands) of the automatic plan: as few bands as fit, of equal height.  Held against covahip_dev_mog_band_plan at the
    pitch wherever the library loads."""
    mx = min(band_max_rows(work_w), work_h)
    bands = -(-work_h // mx)
    rows = -(-work_h // bands)
    try:
        lib_plan = band_plan(pitch(work_w), work_h)
    except OSError:                                    # no library in this checkout: the restatement stands alone
        lib_plan = None
    if lib_plan is not None:
        assert lib_plan[:2] == (rows, bands) and lib_plan[2] == band_lds_bytes(work_w, work_h, rows), (work_w, work_h, lib_plan)
    return rows, bands


# ------------------------------------------------------------------------------------------------ planes over the range
# (work_w, work_h, forced band heights besides the automatic plan 0): 32 words with 63, 64 and 1 live bits in the last, 31 full
# words, 3 words at the maximal height, the two cameras the README names
RANGE_SHAPES = ((2047, 641, (16, 287)), (2048, 272, (16, 37)), (1985, 137, (48,)), (1984, 136, (48,)), (129, 2047, (512, 16)),
                (1296, 972, ()), (352, 288, (144,)))
RANGE_FULL = (2048, 2048)                              # a 4096x4096 source: 8 automatic bands of 256
SEAM_PLANES = ("corridor1", "corridor4", "seam_morphology")
BATTERY = ("spiral", "sealed_spiral", "corner_blob", "corridor1", "corridor4", "seam_morphology", "serpentine", "serpentine_closed",
           "bernoulli0.02", "bernoulli0.2", "blocks0.3", "right_edge", "full", "empty")
# the planes of RANGE_FULL: those whose oracle costs 0.4 s or less there, and the closed serpentine
FULL_PLANES = ("sealed_spiral", "corner_blob", "corridor1", "corridor4", "seam_morphology", "right_edge", "serpentine_closed")


def plan_rows(work_w: int, work_h: int, band_rows: int) -> int:
    return band_rows if band_rows else auto_plan(work_w, work_h)[0]


def pick_seams(work_h: int, rows: int, most: int = 8):
    """The seam rows the seam planes are built around: every step-th seam of the plan, so that they lie at least 64 rows apart
    (a corridor's slab is 60 rows high) and are `most` at the most, over the whole height.  A plan of one band has no seam: its
    planes are built around the middle row, so that they are no empty planes."""
    s = seams(work_h, rows)
    if not s:
        return (work_h // 2,)
    step = max(-(-64 // rows), -(-len(s) // most))
    return tuple(y for y in s[step - 1::step] if y + 30 <= work_h)          # (a slab reaches 30 rows either side of its seam)


def range_names(work_w: int, work_h: int):
    """The battery at a shape.  The coarse spiral has no turn below 170 rows or columns (mog_grid_ref._spiral stops when fewer
    than 2 x 64 lie between its sides): it is left out there by name, here."""
    return tuple(n for n in BATTERY if n != "spiral" or min(work_w, work_h) >= 170)


def serpentine_lanes(work_w: int) -> int:
    return max(2, min(6, (work_w - 32) // 32))         # lanes of 32 columns at the least: 3 at 129 wide


@functools.lru_cache(maxsize=None)
def _plane(name: str, w: int, h: int, seam_rows):
    if name in ("spiral", "sealed_spiral"):
        a = coarse_spirals(h, w)[name == "sealed_spiral"]
    elif name == "corner_blob":
        a = corner_blob(h, w)
    elif name in ("corridor1", "corridor4"):
        a = seam_corridors(h, w, int(name[-1]), seam_rows)
    elif name == "seam_morphology":
        a = seam_morphology(h, w, seam_rows)
    elif name in ("serpentine", "serpentine_closed"):
        a = serpentine(h, w, serpentine_lanes(w), closed_last=name == "serpentine_closed")
    elif name.startswith("bernoulli"):
        a = bernoulli(h, w, float(name[9:]), seed=21)
    elif name == "blocks0.3":
        a = blocks(h, w, 0.3, seed=22)
    elif name == "right_edge":
        a = right_edge(h, w)
    elif name in ("full", "empty"):
        a = np.full((h, w), name == "full")
    else:
        raise KeyError(name)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _oracle(name: str, w: int, h: int, seam_rows):
    f, l = post(_plane(name, w, h, seam_rows))
    f.setflags(write=False)
    l.setflags(write=False)
    return f, l


def _key(name, work_h, rows):
    return pick_seams(work_h, rows) if name in SEAM_PLANES else None


def range_plane(name: str, work_w: int, work_h: int, rows: int) -> np.ndarray:
    """bool [work_h][work_w] (read-only, computed once): plane `name` for a plan of `rows` rows per band."""
    return _plane(name, work_w, work_h, _key(name, work_h, rows))


def range_oracle(name: str, work_w: int, work_h: int, rows: int):
    """(filled, labels) of the oracle on range_plane, computed once per distinct plane."""
    return _oracle(name, work_w, work_h, _key(name, work_h, rows))
