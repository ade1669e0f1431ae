"""Label alignment on the GPU (include/covahip.h, covahip_train_data_align; cova_amd/train.py, TrainData.align, alignment,
windows / epoch_samples(label_shift=...)): the three count tables against numpy, exactly -- the records unpacked, the predicate
applied, the boolean planes ANDed -- at every alignment of a frame's start, below and above the kernel's tile of 1024
macroblocks and across its runs of 32 frames, with a neighbouring recording on both sides; Contract G; the label mass; the
refusals; offsets planted in moving blobs found again; a shift applied to the sampler against the data set it undoes; the
command line."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import train as T
from cova_amd.elements import tfrecord_example

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1
SENTINEL = 0xA5A5A5A5


def _records(seed, f, h, w):
    """u8 [f][h][w][4]: fields 0 .. 8 (the packing clips at 6), three in four of them zero so that `moves` is neither full nor empty."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 9, (f, h, w, 4), dtype=np.uint8) * (rng.random((f, h, w, 4)) < 0.25)).astype(np.uint8)


def _labels(seed, f, h, w, kind):
    """gt u8 [f][h][w]: "01" 0 / 1 with one byte in a hundred anywhere in 0 .. 255; "count" 0 .. 64, half of them 0."""
    rng = np.random.default_rng(seed)
    if kind == "count":
        return (rng.integers(0, 65, (f, h, w), dtype=np.uint8) * rng.integers(0, 2, (f, h, w), dtype=np.uint8)).astype(np.uint8)
    gt = rng.integers(0, 2, (f, h, w), dtype=np.uint8)
    return np.where(rng.random((f, h, w)) < 0.01, rng.integers(0, 256, (f, h, w), dtype=np.uint8), gt).astype(np.uint8)


def _planes(frames, gt, min_mv, classes, keep):
    """(moves, set) bool [f][h * w] of frames as they were appended."""
    cls, mx, my = (np.minimum(frames[..., c], 6) for c in range(3))
    moves = np.isin(cls, list(classes))
    if min_mv:
        moves = moves | (np.maximum(mx, my) >= min_mv)
    st = gt != 0
    if keep is not None:
        moves, st = moves & (keep != 0)[None], st & (keep != 0)[None]
    return moves.reshape(len(gt), -1), st.reshape(len(gt), -1)


def _want(frames, gt, first, n, S, min_mv=1, classes=(), keep=None):
    mv, st = _planes(frames[first:first + n], gt[first:first + n], min_mv, classes, keep)
    both = np.zeros((n, 2 * S + 1), np.uint32)
    for j in range(2 * S + 1):
        s = j - S
        a, b = max(0, -s), min(n, n - s)
        if a < b:
            both[a:b, j] = (mv[a:b] & st[a + s:b + s]).sum(axis=1)
    return both, mv.sum(axis=1).astype(np.uint32), st.sum(axis=1).astype(np.uint32)


def _same(got, want):
    return all(g.dtype == np.uint32 and g.shape == w.shape and (g == w).all() for g, w in zip(got, want))


def _data(ctx, frames, gt, capacity=None):
    f, h, w = gt.shape
    d = T.TrainData(ctx, h, w, capacity or f)
    assert d.append(frames, gt) == (0, f)
    return d


def _device_align(ctx, d, first, n, S, **kw):
    """align_device into one sentinel-filled buffer holding the three tables with a count of room behind each."""
    wide = 2 * S + 1
    sizes = [n * wide, n, n]
    buf = np.full(sum(sizes) + 3, SENTINEL, np.uint32)
    at = [0, sizes[0] + 1, sizes[0] + sizes[1] + 2]
    p = ctx.malloc(buf.nbytes)
    try:
        ctx.h2d(p, buf)
        d.align_device(p + 4 * at[0], p + 4 * at[1], p + 4 * at[2], first, n, S, **kw)
        ctx.d2h(buf, p)
    finally:
        ctx.free(p)
    assert all(buf[a + m] == SENTINEL for a, m in zip(at, sizes))
    return buf[:sizes[0]].reshape(n, wide), buf[at[1]:at[1] + n], buf[at[2]:at[2] + n]


# ------------------------------------------------------------------------------------------------ 1. the counts against numpy
# 16x16: the smallest frame, a quarter of the kernel's tile; 17x33: h * w = 561, sixteen consecutive frames start on every byte of
# a 16-byte line (labels) and every even one (records); 45x80 and 68x120: four and eight tiles, the last one partial.
PREDICATES = [dict(min_mv=1), dict(min_mv=6), dict(min_mv=0, classes=(0, 3, 6)), dict(min_mv=3, classes=(2,))]
RANGES = [(7, 45), (3, 1), (50, 5)]        # 45 = a run of 32 and a ragged one, first > 0; one frame; fewer frames than shifts


@pytest.mark.parametrize("h,w,kind", [(16, 16, "01"), (17, 33, "count"), (45, 80, "01"), (68, 120, "count")])
def test_counts_against_numpy(ctx, h, w, kind):
    f = 60
    frames, gt = _records(h + w, f, h, w), _labels(h * w, f, h, w, kind)
    gt[8], gt[9] = 0xFF, 0                                                 # a sum instead of a count, or a signed byte, fails here
    rng = np.random.default_rng(5)
    single = np.zeros((h, w), np.uint8)
    single[h // 2, w - 1] = 9
    keeps = [None, rng.integers(0, 2, (h, w), dtype=np.uint8) * 255, single]
    d = _data(ctx, frames, gt)
    try:
        seen = set()
        for idx, (S, pred) in enumerate(itertools.product((0, 1, 8, 32), PREDICATES)):
            keep = keeps[idx % 3]
            for first, n in RANGES:
                want = _want(frames, gt, first, n, S, keep=keep, **pred)
                got = d.align(first, n, S, keep=keep, **pred)
                assert _same(got, want), (S, pred, idx % 3, first, n)
                assert (got[2] == d.label_mass(first, n, keep)).all()
                if n == 45 and keep is not single:
                    assert 0 < want[1].min() and want[1].max() < h * w and np.median(want[0][:, S]) > 0
                    seen.add(tuple(want[1][:4].tolist()))
                if idx % 4 == idx // 4:                                    # every S and every predicate once, into device memory
                    assert _same(_device_align(ctx, d, first, n, S, keep=keep, **pred), want), (S, pred, first, n)
        assert len(seen) >= 4                                              # the predicates do differ
        # host outputs through a staging of ten frames' counts: five launches, each with the whole recording's halo
        d.set_stage(10 * 4 * (2 * 8 + 3))
        assert _same(d.align(7, 45, 8, keep=keeps[1], min_mv=2), _want(frames, gt, 7, 45, 8, 2, (), keeps[1]))
        d.set_stage(0)
        # the whole data set as one recording: frame 0 and the last frame of the arrays
        assert _same(d.align(0, f, 8), _want(frames, gt, 0, f, 8))
    finally:
        d.close()


def test_full_capacity_last_bytes(ctx):
    """A full data set of an odd frame size: the last plane words of the last frame end with the arrays."""
    h, w, f = 17, 33, 35
    frames, gt = _records(1, f, h, w), _labels(2, f, h, w, "01")
    d = _data(ctx, frames, gt, capacity=f)
    try:
        for first, n in ((0, f), (f - 1, 1), (f - 3, 3)):
            assert _same(d.align(first, n, 2), _want(frames, gt, first, n, 2))
    finally:
        d.close()


def test_more_runs_than_one_round_of_the_grid(ctx):
    """A launch has at most 2048 workgroups of one run of 32 frames each: two rounds of the grid and a ragged third."""
    h = w = 16
    f = 2 * 2048 * 32 + 37
    rng = np.random.default_rng(4)
    block = 4096
    frames, gt = _records(5, block, h, w), _labels(6, block, h, w, "01")
    frames[..., 1] *= rng.integers(0, 2, (block, 1, 1), dtype=np.uint8)    # some frames without motion, so the counts vary
    d = T.TrainData(ctx, h, w, f + 2)
    try:
        for at in range(0, f + 2, block):
            m = min(block, f + 2 - at)
            d.append(frames[:m], gt[:m])
        idx = np.arange(1, f + 1) % block
        want = _want(frames[idx], gt[idx], 0, f, 1, min_mv=2)
        assert len(set(want[1].tolist())) > 50
        assert _same(d.align(1, f, 1, min_mv=2), want)
    finally:
        d.close()


def test_offsets_past_31_and_32_bits(ctx):
    """8.5 M frames of 16x16: the records of frame 2^22 start at byte 2^31 and those of frame 2^23 at byte 2^32, where the labels
    reach 2^31.  A recording across each edge, and the last frames of the arrays."""
    h = w = 16
    block_n, rounds = 1 << 16, 130
    total = rounds * block_n + 3
    frames, gt = _records(7, block_n, h, w), _labels(8, block_n, h, w, "count")
    tail_fr, tail_gt = _records(9, 3, h, w), _labels(10, 3, h, w, "01")
    keep = np.random.default_rng(11).integers(0, 2, (h, w), dtype=np.uint8)
    d = T.TrainData(ctx, h, w, total)
    d_fr, d_gt = ctx.malloc(frames.nbytes), ctx.malloc(gt.nbytes)
    try:
        ctx.h2d(d_fr, frames)
        ctx.h2d(d_gt, gt)
        for i in range(rounds):
            assert d.append_device(d_fr, d_gt, block_n) == (i * block_n, (i + 1) * block_n)
        assert d.append(tail_fr, tail_gt) == (total - 3, total)
        for edge in (1 << 22, 1 << 23):
            first, n = edge - 21, 40
            idx = np.arange(first, first + n) % block_n
            for kp in (None, keep):
                assert _same(d.align(first, n, 2, keep=kp), _want(frames[idx], gt[idx], 0, n, 2, keep=kp)), (edge, kp is None)
        idx = np.arange(total - 13, total - 3) % block_n
        fr, g = np.concatenate([frames[idx], tail_fr]), np.concatenate([gt[idx], tail_gt])
        assert _same(d.align(total - 13, 13, 8, keep=keep), _want(fr, g, 0, 13, 8, keep=keep))
    finally:
        ctx.free(d_fr)
        ctx.free(d_gt)
        d.close()


# ------------------------------------------------------------------------------------------------ 2. Contract G
def test_ignored_label_bytes_change_no_count(ctx):
    h, w, f = 17, 33, 40
    frames, gt = _records(11, f, h, w), _labels(12, f, h, w, "count")
    keep = np.ones((h, w), np.uint8)
    keep[:4, 5:20] = 0
    keep[11, :] = 0
    other = gt.copy()
    other[:, keep == 0] = np.random.default_rng(13).integers(1, 256, (f, int((keep == 0).sum())), dtype=np.uint8)
    a, b = _data(ctx, frames, gt), _data(ctx, frames, other)
    try:
        want = _want(frames, gt, 2, 37, 8, keep=keep)
        assert _same(a.align(2, 37, 8, keep=keep), want) and _same(b.align(2, 37, 8, keep=keep), want)
        assert not _same(b.align(2, 37, 8), a.align(2, 37, 8))
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_write_nothing(ctx):
    h, w = 17, 33
    frames, gt = _records(21, 10, h, w), _labels(22, 10, h, w, "01")
    d = _data(ctx, frames, gt, capacity=12)
    lib = d._lib
    host = np.full(3 * 64, SENTINEL, np.uint32)
    dev = ctx.malloc(host.nbytes)
    keep = np.ones(h * w, np.uint8)
    none_kept = np.zeros(h * w, np.uint8)
    try:
        ctx.h2d(dev, host)

        def call(first=0, n=4, S=2, min_mv=1, mask=0, k=None, base=host.ctypes.data, kind=L.MEM_HOST, data=d, cfg=True, null=None, off=0):
            c = L.AlignCfg(S, min_mv, mask, None if k is None else k.ctypes.data)
            ptrs = [None if null == q else base + 4 * 64 * q + off for q in range(3)]
            return lib.covahip_train_data_align(data.handle if data else None, first, n, C.byref(c) if cfg else None, *ptrs, kind)

        for base, kind in ((host.ctypes.data, L.MEM_HOST), (dev, L.MEM_DEVICE)):
            kw = dict(base=base, kind=kind)
            for first, n in ((0, 0), (0, -1), (-1, 2), (8, 3), (10, 1), (0, 11), (0, 1 << 40), ((1 << 63) - 1, 1)):   # 10 of 12 frames are taken
                assert call(first, n, **kw) == INVALID_ARG, (first, n)
                assert call(first, n, k=keep, **kw) == INVALID_ARG, (first, n)
            for S in (-1, 33, 1 << 20):
                assert call(S=S, **kw) == INVALID_ARG
            for mv in (-1, 7):
                assert call(min_mv=mv, **kw) == INVALID_ARG
            assert call(mask=1 << 7, **kw) == INVALID_ARG and call(mask=0x80000001, **kw) == INVALID_ARG
            assert call(min_mv=0, mask=0, **kw) == INVALID_ARG               # nothing can move
            assert call(k=none_kept, **kw) == INVALID_ARG                    # as covahip_train_set_post refuses it
            assert call(data=None, **kw) == INVALID_ARG and call(cfg=False, **kw) == INVALID_ARG
            for q in range(3):
                assert call(null=q, **kw) == INVALID_ARG
            assert call(base=base, kind=2) == INVALID_ARG and call(base=base, kind=-1) == INVALID_ARG
        assert call(base=dev, kind=L.MEM_DEVICE, off=2) == INVALID_ARG       # the launch stores whole counts
        with pytest.raises(L.CovahipError) as e:
            d.align(8, 3)
        assert e.value.status == INVALID_ARG
        with pytest.raises(L.CovahipError):
            d.align(0, 4, max_shift=33)
        with pytest.raises(ValueError):
            d.align(0, 4, keep=np.ones((w, h), np.uint8))
        with pytest.raises(ValueError):
            d.align(0, 4, classes=(7,))
        back = np.zeros_like(host)
        ctx.d2h(back, dev)
        assert (host == SENTINEL).all() and (back == SENTINEL).all()
        # and the data set still answers
        assert call(first=6, k=keep) == 0
        want = _want(frames, gt, 6, 4, 2)
        assert (host[:20].reshape(4, 5) == want[0]).all() and (host[64:68] == want[1]).all() and (host[128:132] == want[2]).all()
        assert (host[20:64] == SENTINEL).all() and (host[68:128] == SENTINEL).all() and (host[132:] == SENTINEL).all()
    finally:
        ctx.free(dev)
        d.close()


# ------------------------------------------------------------------------------------------------ 4. planted offsets
def _blobs(seed, f, h, w, s0=0, cut=None, size=4):
    """A recording of f frames: three blobs of size x size macroblocks move across a noisy background.  The records of frame t
    carry motion vectors inside the blobs at time t (and on one macroblock in fifty elsewhere); the labels STORED at frame t are
    the blobs at time t - s0 (with one macroblock in a hundred flipped), so the label of record frame t stands at t + s0.
    cut: the label frame `cut` is then removed and a random frame closes the recording."""
    rng = np.random.default_rng(seed)
    pad = 8
    blob = np.zeros((f + 2 * pad, h, w), bool)
    for y0, x0, vy, vx in ((1, 2, 1, 2), (9, 5, 2, 1), (4, 11, 1, 3)):
        for t in range(f + 2 * pad):
            y, x = (y0 + vy * t) % (h - size), (x0 + vx * t) % (w - size)
            blob[t, y:y + size, x:x + size] = True
    frames = np.zeros((f, h, w, 4), np.uint8)
    moving = blob[pad:pad + f] | (rng.random((f, h, w)) < 0.02)
    frames[..., 0] = rng.integers(0, 5, (f, h, w))
    frames[..., 1] = moving * rng.integers(1, 9, (f, h, w))
    frames[..., 2] = moving * rng.integers(0, 9, (f, h, w))
    gt = (blob[pad - s0:pad - s0 + f] ^ (rng.random((f, h, w)) < 0.01)).astype(np.uint8)
    if cut is not None:
        gt = np.concatenate([gt[:cut], gt[cut + 1:], rng.integers(0, 2, (1, h, w), dtype=np.uint8)])
    return frames, gt


def test_planted_offsets_are_found(ctx):
    h, w, f = 24, 40, 150
    plants = (-3, 0, 2)
    parts = [_blobs(50 + k, f, h, w, s0) for k, s0 in enumerate(plants)]
    d = T.TrainData(ctx, h, w, 3 * f)
    try:
        segs = [d.append(fr, gt) for fr, gt in parts]                      # three recordings side by side
        found = T.alignment(d, segs, max_shift=8, window=50)
        for rec, seg, s0 in zip(found, segs, plants):
            print(f"planted {s0:+d}: best {rec['best']}, B/U " + " ".join(f"{b / max(u, 1):.2f}" for b, u in zip(rec["B"], rec["U"])))
            assert rec["segment"] == seg and rec["best"] == s0
            assert rec["drift"]["best"] == [s0] * 3 and rec["drift"]["changes"] == []
        # the counts behind it, against numpy, for the recording in the middle
        fr, gt = parts[1]
        assert _same(d.align(f, f, 8), _want(fr, gt, 0, f, 8))
    finally:
        d.close()


def test_a_removed_label_frame_shows_as_one_change(ctx):
    h, w, f, cut, window = 24, 40, 512, 250, 64
    fr, gt = _blobs(60, f, h, w, 0, cut=cut)
    d = _data(ctx, fr, gt)
    try:
        rec = T.alignment(d, [(0, f)], max_shift=4, window=window)[0]
        ch = rec["drift"]["changes"]
        print(f"cut at {cut}: blocks {rec['drift']['best']}, changes {ch}, whole recording {rec['best']}")
        assert len(ch) == 1 and ch[0][1] == -1 and abs(ch[0][0] - cut) <= window
        assert rec["drift"]["best"][0] == 0 and rec["drift"]["best"][-1] == -1
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 5. applying the shift
@pytest.mark.parametrize("s0", [-3, 2])
def test_a_shifted_sampler_undoes_shifted_labels(ctx, s0):
    """Data set B holds A's labels moved by s0 (random bytes where A has none); sampled at label_shift = s0 it is A."""
    h = w = 16
    f, lo, hi = 40, 6, 33                                                  # the recording, with neighbours on both sides
    rng = np.random.default_rng(70 + s0)
    frames, gt = _records(71, f, h, w), _labels(72, f, h, w, "01")
    moved = rng.integers(0, 256, (f, h, w), dtype=np.uint8)
    src = np.arange(lo, hi) - s0                                           # B[t] = A[t - s0]
    ok = (src >= lo) & (src < hi)
    moved[np.arange(lo, hi)[ok]] = gt[src[ok]]
    a, b = _data(ctx, frames, gt), _data(ctx, frames, moved)
    flat = T.init_weights(2)
    ta = T.Trainer(ctx, h, w, max_batch=8, weights_flat=flat, seed=3)
    tb = T.Trainer(ctx, h, w, max_batch=8, weights_flat=flat, seed=3)
    try:
        table = T.windows([(lo, hi)], "overlap", (1, 2), label_shift=s0)
        kw = dict(strides=(1, 2), data_seed=9, epoch=1, shuffle=True, flip="xy", reverse=True)
        sa, sb = T.epoch_samples(table, **kw), T.epoch_samples(table, label_shift=s0, **kw)
        assert len(table) == (hi - lo) - 3 - abs(s0) and (sb["label"] == sa["label"] + s0).all() and (sb["frame"] == sa["frame"]).all()
        assert sb["label"].min() >= lo and sb["label"].max() < hi
        assert (sa["frame"][:, 0] > sa["frame"][:, 3]).any() and (sa["frame"][:, 0] < sa["frame"][:, 3]).any() and len(set(sa["flags"])) == 4
        stack_a, lab_a = a.gather(sa)
        stack_b, lab_b = b.gather(sb)
        assert stack_a.tobytes() == stack_b.tobytes() and lab_a.tobytes() == lab_b.tobytes()
        assert b.gather(sa)[1].tobytes() != lab_a.tobytes()                # without the shift B is another data set
        assert ta.step_data(a, sa[:8], 1e-3) == tb.step_data(b, sb[:8], 1e-3)
        assert ta.weights_bytes() == tb.weights_bytes() and ta.weights_bytes() != flat.tobytes()
    finally:
        ta.close()
        tb.close()
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 6. command line
def _write(path, frames, gt):
    with open(path, "wb") as f:
        for i in range(len(gt)):
            f.write(tfrecord_example(frames[i:i + 1], gt[i:i + 1]))


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "cova_amd.train", *map(str, args), "--h-mb", "16", "--w-mb", "16"], cwd=ROOT,
                          capture_output=True, text=True, timeout=300)


def test_command_line(ctx, tmp_path):
    h = w = 16
    good = [tmp_path / "a.tfrecord", tmp_path / "b.tfrecord"]
    _write(good[0], *_blobs(80, 48, h, w, 2, size=3))
    _write(good[1], *_blobs(81, 40, h, w, -1, size=3))
    lost = tmp_path / "lost.tfrecord"
    _write(lost, *_blobs(82, 96, h, w, 0, cut=50, size=3))
    r = _cli(*good, "--windows", "overlap", "--align-report", "4", "--align-window", "16")
    assert r.returncode == 0, r.stderr
    assert f"{good[0]}: frames [0, 48), best shift +2\n" in r.stdout and f"{good[1]}: frames [48, 88), best shift -1\n" in r.stdout, r.stdout
    assert r.stdout.count("drift (blocks of 16 frames): none\n") == 2 and r.stdout.count(" *\n") == 2, r.stdout
    assert len([ln for ln in r.stdout.splitlines() if ln.split() and ln.split()[0].lstrip("+-").isdigit()]) == 2 * 9
    out = tmp_path / "one.cvhw"
    r = _cli(*good, "-o", out, "--windows", "overlap", "--label-shift", "auto:4", "--align-window", "16", "--epochs", "1", "--val-frac", "0.2")
    assert r.returncode == 0, r.stderr
    assert f"{good[0]}: label shift +2\n" in r.stderr and f"{good[1]}: label shift -1\n" in r.stderr, r.stderr
    assert out.stat().st_size > 0
    # 88 frames, the last 18 to validate: (48 - 3 - 2) + (22 - 3 - 1) windows train, 18 - 3 - 1 validate
    assert "70 frames -> 61 windows of 16x16, 14 to validate\n" in r.stderr, r.stderr
    r = _cli(good[0], lost, "-o", out, "--windows", "overlap", "--label-shift", "auto:4", "--align-window", "16", "--epochs", "1")
    assert r.returncode != 0 and f"--label-shift auto: {lost}, frames [48, 144)" in r.stderr and "the shift changes inside" in r.stderr, r.stderr
    r = _cli(lost, "--windows", "overlap", "--align-report", "4", "--align-window", "16")
    assert r.returncode == 0 and "drift (blocks of 16 frames): frame " in r.stdout and ": shift -1" in r.stdout, r.stdout + r.stderr
