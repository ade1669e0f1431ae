"""covahip_train_data_record_stats on the GPU against the numpy restatement (tests/input_stats_ref.py) of the frames as appended:
every count must be EQUAL."""
import ctypes as C

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import monitor as mon
from cova_amd import train
from cova_amd.elements import tfrecord_example
from cova_amd.train import TrainData
from tests import input_stats_ref as ref

pytestmark = pytest.mark.gpu

FIELDS = ref.FIELDS + ("hist_set", "set_total")
INVALID = 1
# (16,16): a frame per 256-lane workgroup with most lanes idle; (17,33): 561, odd, frames start at odd bytes; (45,80): two tiles
GRIDS = [(16, 16), (17, 33), (45, 80)]


def _recording(n, h, w, seed):
    """u8 [n][h][w][4] frames (2 % non-zero among uniform and special frames) and labels with bytes 0, 1, 2 and 255."""
    rng = np.random.default_rng(seed)
    fr = np.zeros((n, h, w, 4), np.uint8)
    hit = rng.random((n, h, w)) < 0.02
    fr[hit, :3] = rng.integers(0, 256, (int(hit.sum()), 3)).astype(np.uint8)
    fr[1] = rng.integers(0, 256, (h, w, 4))                                  # uniform: the clip at 6
    fr[2, ..., :3] = 0                                                       # still
    fr[3, ..., 0], fr[3, ..., 1:3] = 7, 0                                    # all intra
    fr[..., 3] = rng.integers(0, 256, (n, h, w))
    blob = rng.random((n, h, w)) < 0.05
    gt = np.where(blob, rng.choice(np.asarray([1, 2, 255], np.uint8), (n, h, w)), 0).astype(np.uint8)
    gt[1] = rng.choice(np.asarray([0, 1, 2, 255], np.uint8), (h, w))         # labels on the uniform frame: every bin can be set
    gt[2, :2] = 255                                                          # labelled all-skip records
    return fr, gt


def _same(got, want):
    for k in FIELDS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (k, np.asarray(got[k]).sum(), np.asarray(want[k]).sum())


@pytest.mark.parametrize("h,w", GRIDS)
def test_record_stats_equal_the_restatement(ctx, h, w):
    n_a, n_b = 21, 14
    fa, ga = _recording(n_a, h, w, 3 * h + w)
    fb, gb = _recording(n_b, h, w, 5 * h + w)
    data = TrainData(ctx, h, w, n_a + n_b + 4)
    d_f, d_g = ctx.malloc(fb.nbytes + 1), ctx.malloc(gb.nbytes + 1)
    try:
        seg_a = data.append(fa, ga)                                          # a host append ...
        ctx.h2d(d_f + 1, fb)
        ctx.h2d(d_g + 1, gb)
        seg_b = data.append_device(d_f + 1, d_g + 1, n_b)                     # ... and a device append off every boundary
        assert seg_a == (0, n_a) and seg_b == (n_a, n_a + n_b)
        r = ref.records(np.concatenate([fa, fb]), False)
        gt = np.concatenate([ga, gb])
        whole = ref.record_stats_ref(r, gt)
        assert whole["still_frames"] >= 2 and whole["intra_frames"] >= 2 and whole["set_total"] > 0 and whole["hist_set"][0] > 0
        assert set(np.unique(gt)) == {0, 1, 2, 255} and whole["set_total"] == int((gt != 0).sum())
        _same(data.record_stats(), whole)                                     # the whole set
        _same(data.record_stats(), whole)                                     # ... again: a call starts from zero
        ranges = [(0, 1), (3, 1), (1, 7), (5, 2), (n_a - 1, 3), (n_a + n_b - 1, 1)]   # single frames; `first` odd: an odd byte offset at 17x33
        for first, n in ranges:
            got = data.record_stats(first, n)
            _same(got, ref.record_stats_ref(r[first:first + n], gt[first:first + n]))
            # set_total is the label mass of the same frames without a keep map
            assert got["set_total"] == int(data.label_mass(first, n).sum(dtype=np.int64)) and got["in_frames"] == n
        assert data.record_stats()["set_total"] == int(data.label_mass().sum(dtype=np.int64))
        # two recordings counted apart add up to the range that spans both
        a, b = data.record_stats(seg_a[0], n_a), data.record_stats(seg_b[0], n_b)
        _same({k: a[k] + b[k] for k in FIELDS}, whole)
        # the cadence and slice switches change nothing
        lib = L.lib()
        try:
            for slice_len, flush in ((1, 1), (512, 3), (5, 255)):
                assert lib.covahip_dev_monitor_slice(ctx.handle, slice_len) == 0 and lib.covahip_dev_input_flush(ctx.handle, flush) == 0
                _same(data.record_stats(), whole)
        finally:
            lib.covahip_dev_monitor_slice(ctx.handle, 0)
            lib.covahip_dev_input_flush(ctx.handle, 0)

        # NULL outputs are tolerated, one by one and all together; every refusal returns its code and writes nothing
        call = lib.covahip_train_data_record_stats
        assert call(data.handle, 0, n_a + n_b, C.byref(L.RecordStats())) == 0
        hist = np.full(512, -1, np.int64)
        total = np.full(1, -1, np.int64)
        only = L.RecordStats(hist=hist.ctypes.data, set_total=total.ctypes.data)
        assert call(data.handle, 0, n_a + n_b, C.byref(only)) == 0
        assert np.array_equal(hist, whole["hist"]) and total[0] == whole["set_total"]
        hist[:] = -1
        for first, n in ((0, 0), (0, -1), (-1, 2), (0, n_a + n_b + 1), (n_a + n_b, 1), (2, n_a + n_b - 1)):
            assert call(data.handle, first, n, C.byref(only)) == INVALID, (first, n)
        assert call(None, 0, 1, C.byref(only)) == INVALID and call(data.handle, 0, 1, None) == INVALID
        assert (hist == -1).all()
    finally:
        data.close()
        ctx.free(d_f)
        ctx.free(d_g)


def test_more_frames_than_one_launch_pair(ctx):
    """16384 frames are one launch pair: 16384 + 37 frames are two, the second from its own offset."""
    h, w, n = 16, 16, 16384 + 37
    f40, g40 = _recording(40, h, w, 9)
    pick = np.random.default_rng(1).integers(0, 40, n)
    data = TrainData(ctx, h, w, n)
    try:
        data.append(f40[pick], g40[pick])
        r40 = ref.records(f40, False)
        per = [ref.record_stats_ref(r40[i:i + 1], g40[i:i + 1]) for i in range(40)]
        times = np.bincount(pick, minlength=40)
        want = {k: sum(int(times[i]) * np.asarray(per[i][k]) for i in range(40)) for k in FIELDS}
        _same(data.record_stats(), want)
        tail = data.record_stats(16384, 37)
        assert tail["in_frames"] == 37 and tail["hist"].sum() == 37 * h * w
    finally:
        data.close()


def test_record_report_command_line(ctx, tmp_path, capsys):
    """python -m cova_amd.train --record-report: the report of every recording, and --save-inputs with the counts of both together
    in the format cova_amd.monitor reads."""
    h, w = 45, 80
    recs, paths = [_recording(16, h, w, 40), _recording(24, h, w, 41)], []
    for k, (fr, gt) in enumerate(recs):
        paths.append(str(tmp_path / f"rec{k}.tfrecord"))
        with open(paths[-1], "wb") as f:
            for i in range(0, fr.shape[0], 8):
                f.write(tfrecord_example(fr[i:i + 8], gt[i:i + 8], gop=8))
    out = tmp_path / "inputs.json"
    assert train.main(paths + ["--h-mb", str(h), "--w-mb", str(w), "--windows", "overlap", "--record-report", "--save-inputs", str(out)]) == 0
    text = capsys.readouterr().out
    want = [ref.record_stats_ref(ref.records(fr, False), gt) for fr, gt in recs]
    for path, st in zip(paths, want):
        assert train.record_report_text(path, st) in text
    both = {k: np.asarray(want[0][k]) + np.asarray(want[1][k]) for k in ref.FIELDS}
    ref.same(mon.load_inputs(out), both)
    assert "all-skip records among them" in text and f"wrote {out}" in text
