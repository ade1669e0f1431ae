"""Host logic of training from a resident data set (cova_amd/train.py: windows, epoch_samples, split_frames_tail and the
command line's flags).  No GPU: the tables are plain index arithmetic, checked against slide and against a restatement of the
formulas of epoch_samples' docstring."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import train as T

M = (1 << 64) - 1
SEGMENTS = [(0, 26), (26, 33), (33, 36), (40, 57)]      # 26, 7, 3 (too short for any window) and 17 frames, with a gap


def _mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def _restated(table, strides, data_seed, epoch, model, shuffle, flip, reverse):
    """epoch_samples written out again, in Python integers: [(frames, label, flags)] in epoch order."""
    def r(site, i):
        return _mix((_mix((data_seed & M) ^ _mix((epoch << 20 | model << 4 | site) & M)) + i) & M)

    out = []
    for i, (start, k) in enumerate(table.tolist()):
        fitting = [s for s in strides if k - 3 * s >= start]
        s = fitting[r(4, i) % len(fitting)]
        frames = [k, k - s, k - 2 * s, k - 3 * s]
        if reverse and r(3, i) >> 63:
            frames = frames[::-1]
        flags = (r(1, i) >> 63 if "x" in flip else 0) | ((r(2, i) >> 63) << 1 if "y" in flip else 0)
        out.append((frames, frames[0], flags))
    if shuffle:
        order = sorted(range(len(out)), key=lambda i: (r(0, i), i))     # a stable sort by r(0, i)
        out = [out[i] for i in order]
    return out


def test_splitmix64_is_the_headers():
    assert int(T.splitmix64(0)[0]) == _mix(0) == 0xE220A8397B1DCDAF      # the published first output of SplitMix64 from state 0
    z = np.array([1, M, 0x123456789ABCDEF], dtype=np.uint64)
    assert [int(v) for v in T.splitmix64(z)] == [_mix(int(v)) for v in z]


def test_the_sample_record_is_24_bytes():
    assert T.SAMPLE is L.TRAIN_SAMPLE_DTYPE and T.SAMPLE.itemsize == 24
    assert [T.SAMPLE.fields[n][1] for n in ("frame", "label", "flags")] == [0, 16, 20]


def test_skip_windows_name_the_frames_slide_stacks():
    h, w, f = 16, 16, 26
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (f, h, w, 4), dtype=np.uint8)
    gt = rng.integers(0, 2, (f, h, w), dtype=np.uint8)
    stacks, labels = T.slide(frames, gt)
    table = T.windows([(0, f)], "skip")
    assert table.dtype == np.int64 and table.tolist() == [[0, 4 * j + 3] for j in range(f // 4)]
    s = T.plain_samples(table)
    assert s.dtype == T.SAMPLE and (s["flags"] == 0).all() and (s["label"] == s["frame"][:, 0]).all()
    assert (frames[s["frame"]].reshape(len(s), 4 * h, w, 4) == stacks).all()
    assert (gt[s["label"]] == labels).all()
    # a segment that does not start at 0: the groups are counted from ITS start
    assert T.windows([(5, 18)], "skip").tolist() == [[5, 8], [5, 12], [5, 16]]


@pytest.mark.parametrize("strides,reach", [((1,), 3), ((2,), 6), ((1, 2), 3), ((3, 2), 6)])
def test_overlap_windows_per_segment_and_never_across(strides, reach):
    table = T.windows(SEGMENTS, "overlap", strides)
    want = [[a, k] for a, b in SEGMENTS for k in range(a + reach, b)]
    assert table.tolist() == want                                # F - 3 per segment, F - 6 at stride 2; none for the 3-frame one
    assert len(table) == sum(max(0, b - a - reach) for a, b in SEGMENTS)
    ends = {a: b for a, b in SEGMENTS}
    for ep in range(3):
        s = T.epoch_samples(table, strides, 7, ep, 1, True, "xy", True)
        seg = {tuple(fr): a for a, fr in zip(table[:, 0].tolist(), T.epoch_samples(table, strides, 7, ep, 1, False, "xy", True)["frame"].tolist())}
        for fr, lab in zip(s["frame"].tolist(), s["label"].tolist()):
            a = seg[tuple(fr)]
            assert all(a <= i < ends[a] for i in fr + [lab]), (fr, a)


def test_windows_and_strides_refuse_nonsense():
    with pytest.raises(ValueError):
        T.windows([(0, 9)], "every")
    with pytest.raises(ValueError):
        T.windows([(0, 9)], "overlap", ())
    with pytest.raises(ValueError):
        T.windows([(0, 9)], "overlap", (0,))
    with pytest.raises(ValueError):
        T.windows([(9, 0)])
    with pytest.raises(ValueError):
        T.epoch_samples(T.windows([(0, 9)], "overlap"), (2,))     # k = 3 does not fit stride 2 and no other is listed
    with pytest.raises(ValueError):
        T.epoch_samples(T.windows([(0, 9)], "overlap"), flip="z")
    for kw in (dict(model=1 << 16), dict(model=-1), dict(epoch=1 << 44), dict(epoch=-1)):     # the key's fields would overlap
        with pytest.raises(ValueError):
            T.epoch_samples(T.windows([(0, 9)], "overlap"), **kw)
    assert len(T.epoch_samples(T.windows([(0, 9)], "overlap"), model=(1 << 16) - 1, epoch=(1 << 44) - 1)) == 6
    assert T.windows([], "overlap").shape == (0, 2) and T.epoch_samples(np.zeros((0, 2), np.int64)).shape == (0,)


@pytest.mark.parametrize("kw", [dict(shuffle=True, flip="xy", reverse=True, strides=(1, 2)),
                                dict(shuffle=False, flip="x", reverse=False, strides=(2, 1)),
                                dict(shuffle=True, flip=(), reverse=True, strides=(1,)),
                                dict(shuffle=False, flip=("y",), reverse=False, strides=(1, 2, 4))])
def test_epoch_samples_is_the_stated_function(kw):
    table = T.windows(SEGMENTS, "overlap", kw["strides"])
    n = len(table)
    for data_seed, epoch, model in [(0, 0, 0), (12345, 3, 2), (M, 40, 255)]:
        s = T.epoch_samples(table, kw["strides"], data_seed, epoch, model, kw["shuffle"], kw["flip"], kw["reverse"])
        want = _restated(table, kw["strides"], data_seed, epoch, model, kw["shuffle"], kw["flip"], kw["reverse"])
        assert s.dtype == T.SAMPLE and s.shape == (n,) and s.flags["C_CONTIGUOUS"]
        assert [(fr, lab, fl) for fr, lab, fl in zip(s["frame"].tolist(), s["label"].tolist(), s["flags"].tolist())] == want
        again = T.epoch_samples(table, kw["strides"], data_seed, epoch, model, kw["shuffle"], kw["flip"], kw["reverse"])
        assert s.tobytes() == again.tobytes()                   # the same arguments, the same bytes
        # a permutation of the windows: every newest frame once (the newest frame is the largest of the four)
        assert sorted(s["frame"].max(axis=1).tolist()) == sorted(table[:, 1].tolist())
        d = np.diff(s["frame"].astype(np.int64), axis=1)
        assert (d[:, 0] == d[:, 1]).all() and (d[:, 1] == d[:, 2]).all() and np.isin(np.abs(d[:, 0]), kw["strides"]).all()
        rev = d[:, 0] > 0                                        # listed oldest first
        assert (s["label"] == s["frame"][:, 0]).all()            # a reversed sample is labelled by its first = OLDEST frame
        assert (s["label"][rev] == s["frame"][rev].min(axis=1)).all() and (s["label"][~rev] == s["frame"][~rev].max(axis=1)).all()
        assert rev.any() == bool(kw["reverse"]) and (kw["reverse"] is False or (~rev).any())
        assert set(s["flags"].tolist()) == {("x" in kw["flip"]) * a | ("y" in kw["flip"]) * b for a in (0, 1) for b in (0, 2)}


def test_epochs_models_and_seeds_differ():
    table = T.windows(SEGMENTS, "overlap", (1, 2))
    base = T.epoch_samples(table, (1, 2), 1, 0, 0, True, "xy", True).tobytes()
    assert T.epoch_samples(table, (1, 2), 1, 1, 0, True, "xy", True).tobytes() != base
    assert T.epoch_samples(table, (1, 2), 1, 0, 1, True, "xy", True).tobytes() != base
    assert T.epoch_samples(table, (1, 2), 2, 0, 0, True, "xy", True).tobytes() != base
    e0 = T.epoch_samples(table, (1,), 1, 0, 0, True)
    e1 = T.epoch_samples(table, (1,), 1, 1, 0, True)
    assert e0["frame"][:, 0].tolist() != e1["frame"][:, 0].tolist()                      # two epochs, two orders
    assert sorted(e0["frame"][:, 0].tolist()) == sorted(e1["frame"][:, 0].tolist()) == sorted(table[:, 1].tolist())
    # every listed stride that fits is drawn somewhere, and windows near a segment's start only draw the ones that fit
    s = T.epoch_samples(table, (1, 2), 1, 0, 0)
    step = s["frame"][:, 0] - s["frame"][:, 1]
    assert set(step.tolist()) == {1, 2}
    assert (step[table[:, 1] - 6 < table[:, 0]] == 1).all()


def test_split_frames_tail_cuts_a_segment_in_two():
    train, val = T.split_frames_tail(SEGMENTS, 0.25)            # 53 frames: the last 14 validate
    assert train == [(0, 26), (26, 33), (33, 36), (40, 43)] and val == [(43, 57)]
    train, val = T.split_frames_tail(SEGMENTS, 0.4)             # 22: the 17 of the last segment, the 3-frame one, 2 more
    assert train == [(0, 26), (26, 31)] and val == [(31, 33), (33, 36), (40, 57)]
    assert sum(b - a for a, b in val) == 22
    both = T.windows(train, "overlap").tolist() + T.windows(val, "overlap").tolist()
    for a, k in both:                                            # no window straddles the cut
        assert any(s <= k - 3 and k < e for s, e in train + val)
    for frac in (0.0, 1.0, 1e-9 / 53):
        with pytest.raises(ValueError):
            T.split_frames_tail(SEGMENTS, frac)


def test_command_line_flags_select_the_resident_path():
    base = ["a.tfrecord", "-o", "o.cvhw"]
    a = T.parse_args(base)
    assert a.resident is False
    for extra in (["--windows", "skip"], ["--windows", "overlap"], ["--stride", "1,2"], ["--flip", "xy"], ["--reverse"], ["--shuffle"],
                  ["--data-seed", "0"]):
        assert T.parse_args(base + extra).resident is True, extra
    a = T.parse_args(base + ["--windows", "overlap", "--stride", "1,2", "--flip", "x", "--shuffle", "--data-seed", "9", "--val-frac", "0.2"])
    assert (a.windows, a.stride, a.flip, a.reverse, a.shuffle, a.data_seed) == ("overlap", (1, 2), "x", False, True, 9)
    a = T.parse_args(["--eval-only", "w.cvhw", "a.tfrecord", "--windows", "overlap"])
    assert a.resident and a.eval_only == "w.cvhw"
    for bad in (base + ["--windows", "all"], base + ["--stride", "0"], base + ["--stride", "a"], base + ["--flip", "z"],
                ["--eval-only", "w.cvhw", "a.tfrecord", "--shuffle"], ["--eval-only", "w.cvhw", "a.tfrecord", "--stride", "1,2"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)
    assert T.parse_args(["--eval-only", "w.cvhw", "a.tfrecord", "--stride", "2"]).stride == (2,)   # scoring takes ONE stride


def test_kernels_compile_for_gfx950_without_scratch():
    """train_data.hip with the Makefile's flags: the compiler's resource-usage remarks show no scratch for the gather kernel and
    for both forms of the pack kernel."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc) and not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([hipcc if os.path.exists(hipcc) else "hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I",
                        os.path.join(root, "include"), "-I", os.path.join(root, "cova_amd", "csrc"), "--cuda-device-only", "-S", "-o",
                        os.devnull, "-Rpass-analysis=kernel-resource-usage", os.path.join(root, "cova_amd", "csrc", "train_data.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", r.stderr, re.S)
    assert sorted(re.sub(r".*(k_gather|k_pack_records).*", r"\1", name) for name, _ in found) == ["k_gather", "k_pack_records",
                                                                                                   "k_pack_records"], found
    assert all(scratch == "0" for _, scratch in found), found
