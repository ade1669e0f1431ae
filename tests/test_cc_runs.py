"""tests/cc_runs.py on the CPU: the run count, the exact-count frame generator and the restated bboxcc plan."""
import numpy as np
import pytest
from scipy import ndimage

from cova_amd import synth
from tests.cc_runs import LaneState, PlanModel, masks_with_runs, run_counts, wv_bytes
from tests.ccl_cases import hand_cases


def _brute_runs(m):
    """Runs by walking the blocks one by one: a block with a pixel starts a run unless a pixel of its left pixel column and one
    of the right pixel column of the block to its left are both set (they are 8-adjacent: the two block rows' pixels touch)."""
    h, w = m.shape
    n = 0
    for by in range(0, h, 2):
        for bx in range(0, w, 2):
            blk = m[by:by + 2, bx:bx + 2]
            if not blk.any():
                continue
            joined = bx > 0 and m[by:by + 2, bx].any() and m[by:by + 2, bx - 1].any()
            n += not joined
    return n


@pytest.mark.parametrize("name", sorted(hand_cases().keys()))
def test_run_counts_hand_cases(name):
    m = hand_cases()[name]
    assert run_counts(m)[0] == _brute_runs(m)


@pytest.mark.parametrize("hw", [(1, 1), (1, 8), (2, 8), (3, 9), (5, 7), (17, 23), (68, 120), (67, 118)])
@pytest.mark.parametrize("density", [0.05, 0.3, 0.7])
def test_run_counts_random(hw, density):
    masks = synth.random_masks(6, hw[0], hw[1], density, seed=hw[0] * 7 + hw[1] + int(density * 100))
    np.testing.assert_array_equal(run_counts(masks), [_brute_runs(m) for m in masks])


def test_run_counts_adversarial():
    h, w = 68, 120
    yy, xx = np.mgrid[0:h, 0:w]
    assert run_counts(np.ones((h, w), np.uint8))[0] == 34                       # one run per block row
    assert run_counts(((yy + xx) % 2).astype(np.uint8))[0] == 34                # checkerboard: every block joined to its left
    assert run_counts((xx % 2 == 0).astype(np.uint8))[0] == 34 * 60             # half blocks: nb runs
    assert run_counts((xx % 2 == 1).astype(np.uint8))[0] == 34 * 60


@pytest.mark.parametrize("hw", [(7, 9), (8, 16), (3, 8), (1, 8), (2, 8), (9, 14)])
def test_generator_hits_every_count(hw):
    h, w = hw
    nb = ((h + 1) // 2) * ((w + 1) // 2)
    rng = np.random.default_rng(h * 100 + w)
    for n in range(nb + 1):
        m = masks_with_runs(n, h, w, rng)
        assert m.shape == (h, w) and m.dtype == np.uint8
        assert run_counts(m)[0] == n == _brute_runs(m)


def _structure(m):
    """(most block rows one component spans, most runs of one component in one block row, touches last row, touches last column)"""
    lab, _ = ndimage.label(m, structure=np.ones((3, 3)))
    rows = max((len(np.unique(np.nonzero(lab == k)[0] // 2)) for k in range(1, lab.max() + 1)), default=0)
    per_row = {}
    h, w = m.shape
    for by in range(0, h, 2):
        for bx in range(0, w, 2):
            blk = lab[by:by + 2, bx:bx + 2]
            if not blk.any():
                continue
            if bx > 0 and m[by:by + 2, bx].any() and m[by:by + 2, bx - 1].any():
                continue
            key = (by, int(blk.max()))
            per_row[key] = per_row.get(key, 0) + 1
    return rows, max(per_row.values(), default=0), bool(m[-1].any()), bool(m[:, -1].any())


@pytest.mark.parametrize("n", [64, 129, 193, 257, 513, 1000, 1500])
def test_generator_structure(n):
    """Frames are not isolated dots: some component spans several block rows, some component holds two runs of one block row
    (a U that merges below, or a fork), and runs reach the last pixel row and the last column."""
    rng = np.random.default_rng(n)
    hits = np.zeros(4, int)
    for _ in range(4):
        m = masks_with_runs(n, 68, 120, rng)
        assert run_counts(m)[0] == n
        rows, same_row, last_row, last_col = _structure(m)
        hits += [rows >= 3, same_row >= 2, last_row, last_col]
    assert (hits >= 2).all(), hits


def test_generator_full_count_is_half_blocks():
    m = masks_with_runs(34 * 60, 68, 120, np.random.default_rng(5))
    assert run_counts(m)[0] == 34 * 60
    assert _structure(m)[0] >= 3   # even at one run per block, columns of half blocks span block rows


def _stat(c1=0, c2=0, c3=0, batch=4096, n1=1):
    return (n1, 0, c1, c2, c3, batch, 128, 0)


@pytest.mark.parametrize("stat,cap", [
    # 4,096 frames: 256 sampled, a quarter = 64; the rule switches at a quarter PLUS one (bboxcc.hip:192, strict >)
    (_stat(), 128),
    (_stat(c1=64), 128), (_stat(c1=65), 192),
    (_stat(c2=64), 128), (_stat(c2=65), 256),
    (_stat(c3=64), 128), (_stat(c3=65), 512),
    (_stat(c1=30, c2=34), 128), (_stat(c1=30, c2=35), 192),
    (_stat(c2=30, c3=34), 128), (_stat(c2=30, c3=35), 256),
    (_stat(c1=1, c2=1, c3=63), 192), (_stat(c1=0, c2=1, c3=64), 256),
    (_stat(c3=256), 512),
    # 800 frames: 50 sampled, 16 * 4 * 12 = 768 <= 800 < 832 = 16 * 4 * 13
    (_stat(c3=12, batch=800), 128), (_stat(c3=13, batch=800), 512),
])
def test_first_capacity_edges(stat, cap):
    assert PlanModel(256).first_cap(stat) == cap


def test_plan_model_sequence():
    """The restated plan on a short sequence at 68x120 (256 CUs): each branch of bboxcc.hip's automatic plan."""
    pm = PlanModel(256)
    st = LaneState()
    sparse, dense = np.full(4096, 100), np.full(4096, 300)
    p = pm.call(st, dense, 68, 120)                       # nothing known: 128, pass 2 planned and run, full pass-3 grid
    assert (p.cap, p.second_planned, p.second_runs, p.pass3, p.pass3_grid, p.realloc) == (128, True, True, "full", 512, True)
    assert p.kernels == {"bboxcc_wave_kernel": 1, "bboxcc_wave_kernel_2": 1, "bboxcc_kernel": 1}
    assert p.overflow == {"batch": 4096, "overflow_pass1": 4096, "overflow_pass2": 0, "cap_pass1": 128}
    p = pm.call(p.state, dense, 68, 120)                  # every sampled frame > 256 runs: 512; 4 x 512 does not fit -> no pass 2
    assert (p.cap, p.second_planned, p.second_runs, p.pass3, p.realloc) == (512, False, False, "full", False)
    assert p.kernels == {"bboxcc_wave_kernel": 1, "bboxcc_kernel": 1}
    assert p.overflow == {"batch": 4096, "overflow_pass1": 0, "overflow_pass2": 0, "cap_pass1": 512}
    p = pm.call(p.state, dense + 300, 68, 120)            # the pass-3 frames count as having overflowed pass 2 too
    assert p.overflow == {"batch": 4096, "overflow_pass1": 4096, "overflow_pass2": 4096, "cap_pass1": 512}
    p = pm.call(p.state, sparse, 68, 120)
    p = pm.call(p.state, dense, 68, 120)                  # last call had no overflow: pass 2 skipped, quiet 32-workgroup pass 3
    assert (p.cap, p.second_planned, p.second_runs, p.pass3, p.pass3_grid) == (128, True, False, "quiet", 32)
    assert p.overflow == {"batch": 4096, "overflow_pass1": 4096, "overflow_pass2": 4096, "cap_pass1": 128}
    p = pm.call(p.state, np.full(5000, 100), 68, 120)     # a larger batch reallocates the counters
    assert p.realloc and p.state.turn == 1
    p = pm.call(p.state, np.full(800, 100), 68, 120)      # a smaller one keeps them
    assert not p.realloc and p.state.turn == 2
    p = pm.call(p.state, np.full(700, 100), 68, 120)      # <= 3 x 256 frames: the workgroup kernel alone
    assert p.cap is None and p.kernels == {"bboxcc_kernel": 1} and p.overflow["batch"] == 0
    p = pm.call(LaneState(), np.full(4096, 100), 45, 80, forced_cap=256)   # 4 x 256 >= nb = 920: pass 2 takes everything
    assert (p.second_runs, p.pass3, p.pass3_grid) == (True, "one", 1)
    p = pm.call(LaneState(), np.full(1000, 100), 68, 118)  # W % 8 != 0: no wave kernel
    assert p.cap is None and p.kernels == {"bboxcc_kernel": 1}


def test_wave_lds_edges():
    assert 4 * wv_bytes(68, 120, 4 * 256) <= 160 * 1024 - 64 < 4 * wv_bytes(68, 120, 2040)
    assert 4 * wv_bytes(128, 128, 4 * 128) <= 160 * 1024 - 64 < 4 * wv_bytes(128, 128, 4 * 512)
    assert wv_bytes(68, 118, 128) is None and wv_bytes(129, 8, 128) is None
