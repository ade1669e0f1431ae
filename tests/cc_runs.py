"""Run counts of bboxcc's wave kernel and its automatic large-batch plan, restated in numpy (test helper, no GPU).

run_counts       runs per frame exactly as phase B of cova_amd/csrc/bboxcc_wave.h counts them
masks_with_runs  frames with an exact run count and real structure (multi-row components, late merges, border runs)
PlanModel        the automatic plan of covahip_bboxcc_launch (cova_amd/csrc/bboxcc.hip:173-311): which passes launch, at which
                 capacity and grid, what covahip_dev_bboxcc_overflow reports, and the state the next call on the lane sees
"""
from __future__ import annotations

import dataclasses

import numpy as np

WAVE_CAP = 128                 # bboxcc.hip: WAVE_CAP
WV_WAVES = 4                   # bboxcc.hip: WV_WAVES
LDS_WAVES_MAX = 160 * 1024 - 64    # bound of WV_WAVES * wave_bytes (bboxcc.hip:207,213)
LDS_WG_MAX = 160 * 1024 - 256      # bound of the workgroup kernel's run-based body, and of the pass-2 occupancy (bboxcc.hip:202,258)


def _planes(masks):
    """a, b, c, d of bboxcc_wave.h as booleans [B][BH][BW]: the four pixels of every 2x2 block (missing pixels of an odd H / W are 0)."""
    m = np.asarray(masks) != 0
    if m.ndim == 2:
        m = m[None]
    b, h, w = m.shape
    p = np.zeros((b, h + (h & 1), w + (w & 1)), bool)
    p[:, :h, :w] = m
    return p[:, 0::2, 0::2], p[:, 0::2, 1::2], p[:, 1::2, 0::2], p[:, 1::2, 1::2]


def run_counts(masks) -> np.ndarray:
    """Runs per frame: popcount of S = F & ~J over all block rows, F = a|b|c|d, J = (a|c) & ((b|d) << 1) (bboxcc_wave.h:147-150)."""
    a, b, c, d = _planes(masks)
    F = a | b | c | d
    J = np.zeros_like(F)
    J[:, :, 1:] = (a | c)[:, :, 1:] & (b | d)[:, :, :-1]
    return (F & ~J).sum(axis=(1, 2)).astype(np.int64)


def wv_bytes(h: int, w: int, cap: int) -> int | None:
    """LDS bytes of one wave at run capacity `cap` (ccwave::wv_plan, bboxcc_wave.h:57-67); None: not a wave-kernel shape."""
    if h <= 0 or w <= 0 or h > 128 or w > 128 or w % 8 or cap <= 0:
        return None
    return (2 * ((h + 1) // 2) + 2) * 16 + cap * 24


def cc_plan_lds(h: int, w: int) -> int:
    """LDS bytes of the block-based workgroup body (cc_plan, cova_amd/csrc/bboxcc_body.h); 0: the frame does not fit."""
    bh, bw = (h + 1) // 2, (w + 1) // 2
    nb, rs = bh * bw, (w + 7) // 8 + 2
    rb = ((h + 3) * rs + 15) & ~15
    lds = rb + nb * 24 + ((nb + 15) & ~15) + bh * 16 + 64
    return 0 if lds + 64 > 160 * 1024 or bw > 128 else lds


# ------------------------------------------------------------------------------------------------- frames with an exact run count
def _row_states(run_id, has_right, rng):
    """Left / right pixel column occupancy (L, R) of every block of one block row, sampled at random among the assignments
    that give exactly the runs in run_id (-1 = empty block): blocks of one run are joined (R of the left block and L of the
    right one), adjacent blocks of different runs are not, every run block has a pixel.  A chain CSP over four states per block;
    L = 1, R = 0 on every run block always satisfies it."""
    n = len(run_id)
    states = [(0, 0), (1, 0), (0, 1), (1, 1)]

    def unary(j, s):
        L, R = s
        if run_id[j] < 0:
            return s == (0, 0)
        return (L or R) and not (R and j == n - 1 and not has_right)

    def pair(j, s, t):   # blocks j, j + 1
        if run_id[j] >= 0 and run_id[j] == run_id[j + 1]:
            return s[1] and t[0]
        if run_id[j] >= 0 and run_id[j + 1] >= 0:
            return not (s[1] and t[0])
        return True

    ok = [[False] * 4 for _ in range(n)]
    for j in range(n - 1, -1, -1):
        for k, s in enumerate(states):
            ok[j][k] = bool(unary(j, s)) and (j == n - 1 or any(ok[j + 1][q] and pair(j, s, t) for q, t in enumerate(states)))
    out, prev = [], None
    for j in range(n):
        cand = [k for k, s in enumerate(states) if ok[j][k] and (prev is None or pair(j - 1, prev, s))]
        k = cand[rng.integers(len(cand))]
        prev = states[k]
        out.append(prev)
    return out


def masks_with_runs(n_runs: int, h: int, w: int, rng) -> np.ndarray:
    """One H x W uint8 frame with exactly n_runs runs (0 <= n_runs <= nb = ceil(H/2) * ceil(W/2)).

    Runs live in one block row each, so the total is the sum over block rows.  Each block row's run starts are mostly those of
    the row above, moved by at most one block: runs overlap from row to row and, with the pixel rows they share, form
    components over several block rows -- and a run under two runs of the row above is a U that merges late.  The last run of
    about half the rows is stretched to the last block column; pixels fill both rows of a block most of the time, the last pixel
    row included."""
    bh, bw = (h + 1) // 2, (w + 1) // 2
    nb = bh * bw
    if not 0 <= n_runs <= nb:
        raise ValueError(f"{n_runs} runs do not fit {h}x{w} (nb = {nb})")
    # runs per block row: proportional to random weights, capped at bw, the remainder spread over rows with room
    wts = rng.uniform(0.5, 1.5, bh)
    k = np.minimum(np.floor(n_runs * wts / wts.sum()).astype(int), bw)
    while k.sum() < n_runs:
        room = np.flatnonzero(k < bw)
        add = rng.choice(room, size=min(len(room), n_runs - int(k.sum())), replace=False)
        k[add] += 1
    m = np.zeros((h, w), np.uint8)
    has_right = w % 2 == 0
    prev = np.zeros(0, int)
    for r in range(bh):
        kr = int(k[r])
        if kr == 0:
            prev = np.zeros(0, int)
            continue
        cand = np.unique(np.clip(prev + rng.integers(-1, 2, len(prev)), 0, bw - 1))
        cand = rng.permutation(cand)[:kr]
        rest = np.setdiff1d(np.arange(bw), cand)
        starts = np.sort(np.concatenate([cand, rng.choice(rest, size=kr - len(cand), replace=False)]))
        nxt = np.append(starts[1:], bw)
        ends = np.array([rng.integers(s, e) for s, e in zip(starts, nxt)])
        if rng.random() < 0.5:
            ends[-1] = bw - 1
        run_id = np.full(bw, -1)
        for i, (s, e) in enumerate(zip(starts, ends)):
            run_id[s:e + 1] = i
        rows = [2 * r] + ([2 * r + 1] if 2 * r + 1 < h else [])
        for j, (L, R) in enumerate(_row_states(run_id, has_right, rng)):
            for x, on in ((2 * j, L), (2 * j + 1, R)):
                if not on:
                    continue
                pick = rows if len(rows) == 1 or rng.random() < 0.6 else [rows[rng.integers(len(rows))]]
                m[pick, x] = 1
        prev = starts
    return m


# ----------------------------------------------------------------------------------------------------------- the automatic plan
@dataclasses.dataclass(frozen=True)
class LaneState:
    """What covahip_bboxcc_launch keeps per lane between calls (CtxLane, cova_amd/csrc/internal.h)."""
    stat: tuple | None = None   # cc_stat: pinned {n1, n2, c1, c2, c3, batch, cap, 0} of the last call that could overflow; None = not allocated
    first_cap: int = 0          # cc_first_cap
    ovf_batch: int = 0          # batch the overflow buffer cc_ovf was sized for (0: none)
    turn: int = 0               # cc_stat_turn
    stat_batch: int = 0         # cc_stat_batch
    stat_cap: int = 0           # cc_stat_cap
    pass3_all: bool = False     # the last call's pass 3 took every frame pass 1 overflowed (no pass 2 ran)


@dataclasses.dataclass(frozen=True)
class Plan:
    cap: int | None              # pass-1 capacity of the wave kernel (None: the workgroup kernel alone)
    second_planned: bool
    second_runs: bool
    pass3: str | None            # None (no pass 3) | "one" (nothing can be left) | "quiet" (32) | "full" (min(batch, 2 num_cu))
    pass3_grid: int
    overflow: dict               # expected BboxCc.overflow_stats()
    kernels: dict                # profile scope -> launches
    realloc: bool                # the overflow buffer was (re)allocated and the turn reset
    state: LaneState             # what the next call on the lane sees


class PlanModel:
    """The plan of covahip_bboxcc_launch for one call, line by line (bboxcc.hip).  Frames must fit LDS (H, W <= 128 here)."""

    def __init__(self, num_cu: int):
        self.num_cu = num_cu

    def first_cap(self, stat) -> int:
        """bboxcc.hip:191-192: 512 / 256 / 192 when more than a quarter of the last call's frames (16 x the sampled ones) had
        more than 256 / 192 / 128 runs, else 128."""
        c1, c2, c3, sb = 16 * stat[2], 16 * stat[3], 16 * stat[4], stat[5]
        if 4 * c3 > sb:
            return 4 * WAVE_CAP
        if 4 * (c2 + c3) > sb:
            return 2 * WAVE_CAP
        if 4 * (c1 + c2 + c3) > sb:
            return 3 * WAVE_CAP // 2
        return WAVE_CAP

    def call(self, st: LaneState, runs, h: int, w: int, forced_cap: int = 0, aligned: bool = True) -> Plan:
        runs = np.asarray(runs, np.int64)
        batch = len(runs)
        nb = ((h + 1) // 2) * ((w + 1) // 2)
        aligned = aligned and (h * w) % 8 == 0                               # :198
        known = st.stat is not None and st.stat[5] > 0
        first_cap = st.first_cap
        cap = forced_cap                                                     # :182
        if cap == 0:                                                         # :185-196
            cap = -1
            if batch > 3 * self.num_cu:
                if known:
                    first_cap = self.first_cap(st.stat)
                cap = first_cap or WAVE_CAP
        cap = min(cap, nb)                                                   # :197
        wfull = wv_bytes(h, w, nb)                                           # :200-205
        lds_wg = wfull if forced_cap >= 0 and aligned and wfull is not None and wfull <= LDS_WG_MAX else cc_plan_lds(h, w)
        wb = wv_bytes(h, w, cap) if cap > 0 else None
        if not (cap > 0 and aligned and wb is not None and WV_WAVES * wb <= LDS_WAVES_MAX and (cap >= nb or lds_wg)):   # :206-207
            nxt = dataclasses.replace(st, first_cap=first_cap, stat_batch=0)                                         # :289
            kernel = "bboxcc_kernel" if lds_wg else "bboxcc_big_kernel"                                              # :290-309
            return Plan(None, False, False, None, 0, self._readout(nxt), {kernel: 1}, False, nxt)
        can_overflow = cap < nb                                              # :208
        cap2 = min(4 * cap, nb)                                              # :211
        wb2 = wv_bytes(h, w, cap2)
        second = can_overflow and cap2 > cap and wb2 is not None and WV_WAVES * wb2 <= LDS_WAVES_MAX   # :212-213
        third = can_overflow and (not second or cap2 < nb)                   # :214
        kernels = {"bboxcc_wave_kernel": 1}
        if not can_overflow:                                                 # :284-286
            nxt = dataclasses.replace(st, first_cap=first_cap, stat_batch=0)
            return Plan(cap, False, False, None, 0, self._readout(nxt), kernels, False, nxt)
        realloc = batch > st.ovf_batch                                       # :219-226
        turn = 0 if realloc else st.turn
        second_now = second and not (known and st.stat[0] == 0)              # :242
        n1 = int((runs > cap).sum())
        n2 = int((runs > cap2).sum()) if second_now else 0
        sampled = runs[::16]                                                 # :123-124, (frame & 15) == 0
        c = (int(((sampled > WAVE_CAP) & (sampled <= 3 * WAVE_CAP // 2)).sum()),
             int(((sampled > 3 * WAVE_CAP // 2) & (sampled <= 2 * WAVE_CAP)).sum()),
             int((sampled > 2 * WAVE_CAP).sum()))
        if second_now:
            kernels["bboxcc_wave_kernel_2"] = 1
        have_list = third or not second_now                                  # :272
        quiet = known and st.stat[0] == 0                                    # :275
        pass3 = "one" if not have_list else "quiet" if quiet else "full"     # :277
        grid = {"one": 1, "quiet": 32, "full": min(batch, 2 * self.num_cu)}[pass3]
        kernels["bboxcc_kernel"] = 1
        nxt = LaneState(stat=(n1, n2) + c + (batch, cap, 0), first_cap=first_cap, ovf_batch=max(batch, st.ovf_batch),
                        turn=turn + 1, stat_batch=batch, stat_cap=cap, pass3_all=not second_now)
        return Plan(cap, second, second_now, pass3, grid, self._readout(nxt), kernels, realloc, nxt)

    @staticmethod
    def _readout(st: LaneState) -> dict:
        """covahip_dev_bboxcc_overflow (bboxcc.hip): frames pass 3 took straight from pass 1's list count as having overflowed
        pass 2 too.  cap_pass1 is that of the last call that could overflow (compare it only when batch > 0)."""
        if not st.stat_batch or st.stat is None:
            return {"batch": 0, "overflow_pass1": 0, "overflow_pass2": 0, "cap_pass1": st.stat_cap}
        return {"batch": st.stat_batch, "overflow_pass1": st.stat[0], "overflow_pass2": st.stat[0] if st.pass3_all else st.stat[1],
                "cap_pass1": st.stat_cap}
