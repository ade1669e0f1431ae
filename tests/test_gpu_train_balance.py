"""Balanced epochs on the GPU (include/covahip.h, covahip_train_data_label_mass; cova_amd/train.py, balanced_samples and
fit_data(balance=...)): the label mass against numpy, exactly, at every alignment of a frame's start and in both forms of the
kernel (a frame per wave up to 4096 bytes, a frame per workgroup above), past one round of its grid and past 2^31 bytes of
labels; Contract G; the refusals; the epoch loop against steps taken by hand, exact resume, and the command line."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import train as T, weights as W
from cova_amd.elements import tfrecord_example

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1
SENTINEL = 0xA5A5A5A5


def _labels(seed, f, h, w):
    """gt u8 [f][h][w]: 0 / 1 with one byte in a hundred anywhere in 0..255."""
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, 2, (f, h, w), dtype=np.uint8)
    return np.where(rng.random((f, h, w)) < 0.01, rng.integers(0, 256, (f, h, w), dtype=np.uint8), gt).astype(np.uint8)


def _uneven_labels(seed, f, h, w, kinds=(0.01, 0.2, 0.5)):
    """gt u8 [f][h][w] of 0 / 1 whose frames are nearly empty, half full, or in between (`kinds`: the share of labelled
    macroblocks a frame draws), in a seeded order."""
    rng = np.random.default_rng(seed)
    dens = np.array(kinds)[rng.integers(0, len(kinds), f)]
    return (rng.random((f, h, w)) < dens[:, None, None]).astype(np.uint8)


def _records(seed, f, h, w):
    return np.random.default_rng(seed).integers(0, 9, (f, h, w, 4), dtype=np.uint8)


def _want(gt, keep=None):
    lab = gt != 0
    if keep is not None:
        lab = lab & (keep != 0)[None]
    return lab.reshape(gt.shape[0], -1).sum(axis=1).astype(np.uint32)


def _data(ctx, gt, capacity=None, seed=0):
    f, h, w = gt.shape
    d = T.TrainData(ctx, h, w, capacity or f)
    assert d.append(_records(seed, f, h, w), gt) == (0, f)
    return d


def _device_mass(ctx, d, first, n, keep, room=None):
    """label_mass_device into a sentinel-filled buffer of n + 1 counts: the n counts, and the one behind them untouched."""
    buf = np.full((room or n) + 1, SENTINEL, np.uint32)
    p = ctx.malloc(buf.nbytes)
    try:
        ctx.h2d(p, buf)
        d.label_mass_device(p, first, n, keep)
        ctx.d2h(buf, p)
    finally:
        ctx.free(p)
    assert (buf[n:] == SENTINEL).all()
    return buf[:n]


def _state(tr):
    s = getattr(tr, "_set", tr)
    return [(s.grads(k).tobytes(), s.metrics(k), s.weights_bytes(k)) for k in range(s.n_models)] + [s.state_bytes(), list(s.step_counts)]


# ------------------------------------------------------------------------------------------------ 1. the mass against numpy
# 16x16: aligned frames; 17x33: h * w = 561, sixteen consecutive frames start on every residue mod 16; 24x50: a multiple of 16;
# 45x80: the reference grid -- all read a frame per wave.  64x64 is the last size of that form, 17x241 = 4097 the first of the
# frame-per-workgroup form (and odd), 68x120 the 1080p grid.
@pytest.mark.parametrize("h,w", [(16, 16), (17, 33), (24, 50), (45, 80), (64, 64), (17, 241), (68, 120)])
def test_mass_against_numpy(ctx, h, w):
    f = 43
    gt = _labels(h * w, f, h, w)
    gt[0] = 0xFF                                                           # a sum instead of a count, or a signed byte, fails here
    gt[1] = 0
    assert gt.max() == 255 and (gt > 1).sum() > f                          # bytes other than 0 / 1 everywhere
    rng = np.random.default_rng(3)
    single = np.zeros((h, w), np.uint8)
    single[h // 2, w - 1] = 7
    anti = (gt[6] == 0).astype(np.uint8)                                   # zero exactly where frame 6's labels are not
    keeps = {"none": None, "random": rng.integers(0, 2, (h, w), dtype=np.uint8) * 255, "single": single, "anti": anti}
    assert anti.any() and not anti.all()
    d = _data(ctx, gt)
    try:
        for name, keep in keeps.items():
            want = _want(gt, keep)
            assert want[1] == 0 and want[0] == (h * w if keep is None else int((keep != 0).sum()))
            if name == "anti":
                assert want[6] == 0 and want[5] > 0
            if name == "single":
                assert set(want.tolist()) == {0, 1}
            for first in (0, 1, 5):
                for n in (1, 2, 37):
                    got = d.label_mass(first, n, keep)
                    assert got.dtype == np.uint32 and got.tolist() == want[first:first + n].tolist(), (name, first, n)
                    assert _device_mass(ctx, d, first, n, keep).tolist() == want[first:first + n].tolist(), (name, first, n)
            assert d.label_mass(keep=keep).tolist() == want.tolist()       # n = None: up to `frames`
            assert d.label_mass(40, keep=keep).tolist() == want[40:].tolist()
        # a host mass through a staging of ten counts: four rounds, the last one of seven
        d.set_stage(40)
        assert d.label_mass(3, 37, keeps["random"]).tolist() == _want(gt, keeps["random"])[3:40].tolist()
        d.set_stage(0)
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 2. past one round of the grid
@pytest.mark.parametrize("h,w,per", [(16, 16, 4), (17, 241, 1)])
def test_more_frames_than_one_round_of_the_grid(ctx, h, w, per):
    """A launch has at most 2048 workgroups, of four frames each in the frame-per-wave form and one in the other: two rounds and
    a ragged third."""
    f = 2 * 2048 * per + 5
    rng = np.random.default_rng(h)
    gt = (rng.random((f, h, w)) < rng.random(f)[:, None, None]).astype(np.uint8) * rng.integers(1, 256, (f, h, w), dtype=np.uint8)
    keep = rng.integers(0, 2, (h, w), dtype=np.uint8)
    d = T.TrainData(ctx, h, w, f)
    try:
        zeros = np.zeros((1024, h, w, 4), np.uint8)
        for at in range(0, f, 1024):
            m = min(1024, f - at)
            d.append(zeros[:m], gt[at:at + m])
        for k in (None, keep):
            want = _want(gt, k)
            assert len(set(want.tolist())) > 50
            assert (d.label_mass(keep=k) == want).all()
            assert (_device_mass(ctx, d, 1, f - 1, k) == want[1:]).all()
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 3. offsets past 32 bits
def test_label_offsets_past_31_bits(ctx):
    """The data set of test_offsets_past_32_bits: 8.5 M frames of 16x16, 2.2 GB of labels.  Frame 2^23 starts at byte 2^31."""
    h = w = 16
    block_n, rounds = 1 << 16, 130
    total = rounds * block_n + 3
    assert total * h * w > 1 << 31
    rng = np.random.default_rng(7)
    block = rng.integers(0, 9, (block_n, h, w, 4), dtype=np.uint8)
    block_gt = _uneven_labels(9, block_n, h, w) * rng.integers(1, 256, (block_n, h, w), dtype=np.uint8)
    tail_gt = _labels(8, 3, h, w)
    keep = rng.integers(0, 2, (h, w), dtype=np.uint8)
    d = T.TrainData(ctx, h, w, total)
    d_fr, d_gt = ctx.malloc(block.nbytes), ctx.malloc(block_gt.nbytes)
    try:
        ctx.h2d(d_fr, block)
        ctx.h2d(d_gt, block_gt)
        for i in range(rounds):
            assert d.append_device(d_fr, d_gt, block_n) == (i * block_n, (i + 1) * block_n)
        assert d.append(block[:3], tail_gt) == (total - 3, total) and d.frames == total
        edge = (1 << 31) // (h * w)
        assert edge * h * w == 1 << 31 and edge + 1 < total - 3
        for k in (None, keep):
            wb, wt = _want(block_gt, k), _want(tail_gt, k)
            assert len(set(wb[:64].tolist())) > 8
            assert d.label_mass(total - 3, 3, k).tolist() == wt.tolist()
            assert d.label_mass(edge - 1, 3, k).tolist() == [int(wb[(edge + i) % block_n]) for i in (-1, 0, 1)]
            assert d.label_mass(0, 1, k).tolist() == [int(wb[0])]
            assert _device_mass(ctx, d, edge - 1, 3, k).tolist() == [int(wb[(edge + i) % block_n]) for i in (-1, 0, 1)]
        # and all of them in one call: n = frames, a host mass of 34 MB through a staging of 32 MiB
        got = d.label_mass(keep=keep)
        assert got.shape == (total,) and (got == np.concatenate([np.tile(_want(block_gt, keep), rounds), _want(tail_gt, keep)])).all()
    finally:
        ctx.free(d_fr)
        ctx.free(d_gt)
        d.close()


# ------------------------------------------------------------------------------------------------ 4. Contract G
def test_ignored_label_bytes_change_no_mass(ctx):
    h, w, f = 17, 33, 20
    gt = _labels(21, f, h, w)
    keep = np.ones((h, w), np.uint8)
    keep[:4, 5:20] = 0
    keep[11, :] = 0
    other = gt.copy()
    other[:, keep == 0] = np.random.default_rng(22).integers(0, 256, (f, int((keep == 0).sum())), dtype=np.uint8)
    a, b = _data(ctx, gt), _data(ctx, other)
    try:
        assert a.label_mass(keep=keep).tolist() == b.label_mass(keep=keep).tolist() == _want(gt, keep).tolist()
        assert a.label_mass().tolist() != b.label_mass().tolist()
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_write_nothing(ctx):
    h, w = 17, 33
    gt = _labels(23, 10, h, w)
    d = _data(ctx, gt, capacity=12)
    lib = d._lib
    host = np.full(16, SENTINEL, np.uint32)
    dev = ctx.malloc(host.nbytes)
    keep = np.ones((h, w), np.uint8)
    none_kept = np.zeros((h, w), np.uint8)
    try:
        ctx.h2d(dev, host)

        def call(first, n, k, mass, kind, data=d):
            return lib.covahip_train_data_label_mass(data.handle if data else None, first, n, None if k is None else k.ctypes.data, mass, kind)

        for mass, kind in ((host.ctypes.data, L.MEM_HOST), (dev, L.MEM_DEVICE)):
            for first, n in ((0, 0), (0, -1), (-1, 2), (8, 3), (10, 1), (0, 11), (0, 1 << 40), ((1 << 63) - 1, 1)):   # 10 of 12 frames are taken
                assert call(first, n, None, mass, kind) == INVALID_ARG, (first, n)
                assert call(first, n, keep, mass, kind) == INVALID_ARG, (first, n)
            assert call(0, 4, none_kept, mass, kind) == INVALID_ARG       # as covahip_train_set_post refuses it
            assert call(0, 4, None, mass, kind, data=None) == INVALID_ARG
            assert call(0, 4, None, None, kind) == INVALID_ARG
            assert call(0, 4, None, mass, 2) == INVALID_ARG and call(0, 4, keep, mass, -1) == INVALID_ARG
        assert call(0, 4, None, dev + 2, L.MEM_DEVICE) == INVALID_ARG     # the launch stores whole counts
        with pytest.raises(L.CovahipError) as e:
            d.label_mass(8, 3)
        assert e.value.status == INVALID_ARG
        with pytest.raises(ValueError):
            d.label_mass(keep=np.ones((w, h), np.uint8))
        back = np.zeros_like(host)
        ctx.d2h(back, dev)
        assert (host == SENTINEL).all() and (back == SENTINEL).all()
        # and the data set still answers
        assert call(6, 4, keep, host.ctypes.data, L.MEM_HOST) == 0 and host[:4].tolist() == _want(gt)[6:10].tolist()
        assert (host[4:] == SENTINEL).all()
    finally:
        ctx.free(dev)
        d.close()


# ------------------------------------------------------------------------------------------------ 6. the epoch loop
def _by_hand(tr, d, tables, masses, t, epochs, batch, start=0, **kw):
    """fit_data(balance=t) restated: step_data over balanced_samples(epoch_samples(...)) chunked by set_epoch_plan, the masses
    given (numpy's); returns the histories."""
    s = getattr(tr, "_set", tr)
    sizes = [len(tb) for tb in tables]
    hist = [[] for _ in tables]
    for ep in range(start, epochs):
        lr = T.keras_lr(ep, s.cfg.lr)
        per = [T.balanced_samples(T.epoch_samples(tb, (1,), kw.get("data_seed", 0), ep, k, kw.get("shuffle", False), kw.get("flip", ()),
                                                  kw.get("reverse", False)),
                                  mass, t, mass_first=lo, data_seed=kw.get("data_seed", 0), epoch=ep, model=k)
               for k, (tb, (lo, mass)) in enumerate(zip(tables, masses))]
        tot, cnt = [0.0] * len(tables), [[0, 0, 0] for _ in tables]
        for st in T.set_epoch_plan(sizes, batch):
            losses = s.step_data(d, [per[k][a:a + n] for k, (a, n) in enumerate(st)], lr)
            for k, (_, n) in enumerate(st):
                if n:
                    tot[k] += losses[k] * n
                    for q, v in enumerate(s.metrics(k)):
                        cnt[k][q] += v
        for k in range(len(tables)):
            tp, fp, fn = cnt[k]
            hist[k].append({"epoch": ep, "lr": lr, "loss": tot[k] / sizes[k], "precision": tp / max(1, tp + fp), "recall": tp / max(1, tp + fn)})
    return hist


def test_fit_data_balanced_is_the_steps_by_hand_solo(ctx):
    h = w = 16
    gt = _uneven_labels(30, 24, h, w)
    d = _data(ctx, gt, seed=31)
    flat = T.init_weights(3)
    table = T.windows([(0, 13), (13, 24)], "overlap")
    t = 30
    lo = int(table[:, 0].min())
    mass = _want(gt)[lo:int(table[:, 1].max()) + 1]
    kw = dict(shuffle=True, flip="xy", reverse=True, data_seed=5)
    a = T.Trainer(ctx, h, w, max_batch=4, weights_flat=flat, seed=6)
    b = T.Trainer(ctx, h, w, max_batch=4, weights_flat=flat, seed=6)
    c = T.Trainer(ctx, h, w, max_batch=4, weights_flat=flat, seed=6)
    e = T.Trainer(ctx, h, w, max_batch=4, weights_flat=flat, seed=6)
    try:
        lines = []
        ha = a.fit_data(d, table, epochs=2, batch=3, balance=t, log=lines.append, **kw)
        hb = _by_hand(b, d, [table], [(lo, mass)], t, 2, 3, **kw)[0]
        assert ha == hb and _state(a) == _state(b) and a.step_count == 2 * 6        # 18 windows in batches of 3
        busy = int((mass[table[:, 1] - lo] >= t).sum())
        assert 0 < busy < len(table) and lines[0] == f"balance {t}: {busy} busy / {len(table) - busy} quiet windows"
        assert len(lines) == 3 and all(ln.endswith(" windows 18") for ln in lines[1:])
        # the epochs did differ from the unbalanced ones; and balance=None is the call without the keyword
        hc = c.fit_data(d, table, epochs=2, batch=3, **kw)
        he = e.fit_data(d, table, epochs=2, batch=3, balance=None, **kw)
        assert hc == he and _state(c) == _state(e) and c.weights_bytes() != a.weights_bytes()
    finally:
        for tr in (a, b, c, e):
            tr.close()
        d.close()


def test_fit_data_balanced_is_the_steps_by_hand_set_of_two_keeps(ctx):
    h = w = 16
    gt = _uneven_labels(32, 30, h, w)
    gt[:, :6, :8] = 1                                                      # a burned-in clock: 48 macroblocks labelled in every frame
    d = _data(ctx, gt, seed=33)
    flats = [T.init_weights(4), T.init_weights(5)]
    tables = [T.windows([(0, 16)], "overlap"), T.windows([(16, 30)], "overlap")]    # 13 and 11 windows
    keeps = [np.ones((h, w), np.uint8), np.ones((h, w), np.uint8)]
    keeps[0][:6, :8] = 0                                                   # model 0's camera ignores the clock,
    keeps[1][10:, :] = 0                                                   # model 1's the lower rows
    t = 60
    masses = [(int(tb[:, 0].min()), _want(gt, kp)[int(tb[:, 0].min()):int(tb[:, 1].max()) + 1]) for tb, kp in zip(tables, keeps)]
    kw = dict(shuffle=True, flip="x", data_seed=8)
    a = T.TrainerSet(ctx, h, w, weights=flats, seeds=[1, 2], max_batch=4)
    b = T.TrainerSet(ctx, h, w, weights=flats, seeds=[1, 2], max_batch=4)
    try:
        for ts in (a, b):
            ts.set_post(0, prob_thresh=0.5, keep=keeps[0])
            ts.set_post(1, prob_thresh=0.6, keep=keeps[1])
        lines = []
        ha = a.fit_data(d, tables, epochs=2, batch=3, balance=t, log=lines.append, **kw)
        hb = _by_hand(b, d, tables, masses, t, 2, 3, **kw)
        assert ha == hb and _state(a) == _state(b) and a.step_counts == [2 * 5, 2 * 4]
        for k in range(2):
            lo, mass = masses[k]
            busy = int((mass[tables[k][:, 1] - lo] >= t).sum())
            assert lines[k] == f"model {k}: balance {t}: {busy} busy / {len(tables[k]) - busy} quiet windows"
    finally:
        a.close()
        b.close()
        d.close()


def test_busy_count_follows_the_post(ctx):
    h = w = 16
    gt = _uneven_labels(34, 28, h, w)
    gt[:, :6, :8] = 1                                                      # labelled in every frame: 48 of a frame's mass
    d = _data(ctx, gt, seed=35)
    table = T.windows([(0, 28)], "overlap")
    keep = np.ones((h, w), np.uint8)
    keep[:6, :8] = 0
    t = 70
    counts = {}
    try:
        for name, kp in (("plain", None), ("post", keep)):
            tr = T.Trainer(ctx, h, w, max_batch=4, weights_flat=T.init_weights(1), seed=0)
            try:
                if kp is not None:
                    tr.set_post(prob_thresh=0.5, keep=kp)
                lines = []
                tr.fit_data(d, table, epochs=1, batch=3, balance=t, log=lines.append)
                busy, quiet = map(int, re.fullmatch(rf"balance {t}: (\d+) busy / (\d+) quiet windows", lines[0]).groups())
                assert busy + quiet == len(table) and busy == int((_want(gt, kp)[table[:, 1]] >= t).sum())
                counts[name] = busy
            finally:
                tr.close()
        print(f"busy windows of {len(table)} at threshold {t}: {counts}")
        assert counts["post"] < counts["plain"]
    finally:
        d.close()


def test_exact_resume_with_balance(ctx, tmp_path):
    h = w = 16
    gt = _uneven_labels(36, 30, h, w)
    d = _data(ctx, gt, seed=37)
    flat = T.init_weights(4)
    table = T.windows([(0, 17), (17, 30)], "overlap", (1, 2))
    kw = dict(strides=(1, 2), shuffle=True, flip="xy", reverse=True, data_seed=77, balance=30)
    whole = T.Trainer(ctx, h, w, max_batch=4, weights_flat=flat, seed=1)
    first = T.Trainer(ctx, h, w, max_batch=4, weights_flat=flat, seed=1)
    rest = T.Trainer(ctx, h, w, max_batch=4, weights_flat=T.init_weights(99), seed=5)     # the state comes from the checkpoint
    try:
        hist = whole.fit_data(d, table, epochs=4, batch=3, **kw)
        ck = tmp_path / "run.cvhs"
        h01 = first.fit_data(d, table, epochs=2, batch=3, checkpoint=ck, **kw)
        start = rest.load_state(ck)
        assert start == 2
        h23 = rest.fit_data(d, table, epochs=4, batch=3, start_epoch=start, **kw)
        assert h01 + h23 == hist and len(hist) == 4
        assert rest.weights_bytes() == whole.weights_bytes() and rest.state_bytes() == whole.state_bytes()
    finally:
        whole.close()
        first.close()
        rest.close()
        d.close()


# ------------------------------------------------------------------------------------------------ 7. command line
def _cli_records(h=16, w=16):
    """The records of the command-line test: two recordings of 14 and 9 frames, labels 0 / 1, three frames in four nearly empty."""
    fa, fb = 14, 9
    return _records(40, fa + fb, h, w), _uneven_labels(41, fa + fb, h, w, (0.01, 0.01, 0.01, 0.3)), (fa, fb)


def test_command_line(ctx, tmp_path):
    h = w = 16
    frames, gt, (fa, fb) = _cli_records(h, w)
    paths = [tmp_path / "a.tfrecord", tmp_path / "b.tfrecord"]
    for path, sl in zip(paths, (slice(0, fa), slice(fa, fa + fb))):
        with open(path, "wb") as f:
            for i in range(sl.start, sl.stop):
                f.write(tfrecord_example(frames[i:i + 1], gt[i:i + 1]))
    t = 30
    table = T.windows([(0, fa), (fa, fa + fb)], "overlap")
    mass = _want(gt)
    busy = int((mass[table[:, 1]] >= t).sum())
    drawn = T.balanced_samples(T.epoch_samples(table, shuffle=True), mass, t)
    print(f"busy share of an epoch of {len(table)} windows at threshold {t}: {busy / len(table):.3f} as recorded, "
          f"{float((mass[drawn['label']] >= t).mean()):.3f} balanced")
    out = tmp_path / "one.cvhw"
    r = subprocess.run([sys.executable, "-m", "cova_amd.train", str(paths[0]), str(paths[1]), "-o", str(out), "--balance", str(t),
                        "--windows", "overlap", "--shuffle", "--epochs", "2", "--h-mb", str(h), "--w-mb", str(w)], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert f"balance {t}: {busy} busy / {len(table) - busy} quiet windows\n" in r.stderr, r.stderr
    assert r.stderr.count(f" windows {len(table)}\n") == 2, r.stderr       # the two epoch lines: an epoch keeps its length
    assert W.from_bytes(out.read_bytes()).shape == T.init_weights(0).shape
