"""Label alignment, host side (cova_amd/train.py): align_scores and align_drift on hand-made counts, windows / epoch_samples with
label_shift, and the command line's parsing.  The counts themselves are tests/test_gpu_align.py's."""
import itertools

import numpy as np
import pytest

from cova_amd import train as T


def _counts(n, S, peak=None, height=50, floor=5, mov=100, lab=100):
    """Counts of n frames: every frame moves `mov` and is labelled `lab` macroblocks, `floor` of them in common at every shift and
    `height` at `peak`; pairs outside the recording are 0, as the device writes them."""
    both = np.full((n, 2 * S + 1), floor, np.uint32)
    if peak is not None:
        both[:, peak + S] = height
    for j in range(2 * S + 1):
        i = np.arange(n) + j - S
        both[(i < 0) | (i >= n), j] = 0
    return both, np.full(n, mov, np.uint32), np.full(n, lab, np.uint32)


# ------------------------------------------------------------------------------------------------ 1. scores
@pytest.mark.parametrize("peak", [-4, -1, 0, 3])
def test_a_planted_peak_is_best(peak):
    n, S = 40, 4
    r = T.align_scores(*_counts(n, S, peak))
    assert r["shifts"] == list(range(-S, S + 1)) and r["best"] == peak
    for s, B, U in zip(r["shifts"], r["B"], r["U"]):
        pairs = n - abs(s)                                                 # the frames whose partner lies inside the recording
        assert isinstance(B, int) and isinstance(U, int)
        assert B == pairs * (50 if s == peak else 5) and U == pairs * 200 - B


def test_sums_take_the_label_frames_of_the_shift():
    """L(s) sums lab[i + s], not lab[i]: a recording whose only labelled frame is its last."""
    n, S = 6, 2
    both = np.zeros((n, 2 * S + 1), np.uint32)
    mov, lab = np.full(n, 10, np.uint32), np.zeros(n, np.uint32)
    lab[5] = 7
    both[3, 2 + S] = 4                                                     # record frame 3 against label frame 5
    r = T.align_scores(both, mov, lab)
    # s = -2: records 2 .. 5, labels 0 .. 3; s = 2: records 0 .. 3, labels 2 .. 5
    assert r["B"] == [0, 0, 0, 0, 4] and r["U"] == [40, 50, 67, 57, 40 + 7 - 4] and r["best"] == 2


def test_ties_take_the_smaller_magnitude_then_the_smaller_shift():
    # (B, U) per shift -3 .. 3: the fraction 1 / 3 at -2, +2 and +3, from different integers
    sums = [(0, 9), (1, 3), (0, 9), (0, 9), (0, 9), (2, 6), (100, 300)]
    assert T._align_best(sums) == -2                                       # the smaller |s|, then the smaller s
    assert T._align_best([(1, 3)] + [(0, 9)] * 3 + [(5, 15)] + [(0, 9)] * 2) == 1
    assert T._align_best([(0, 9)] * 3 + [(1, 3)] + [(0, 9)] * 3) == 0
    # cross-multiplied, not divided: 10^18 / (3 * 10^18 + 1) < 1 / 3 although the doubles are equal
    big = 10 ** 18
    assert big / (3 * big + 1) == 1 / 3
    assert T._align_best([(big, 3 * big + 1), (0, 1), (1, 3)]) == 1 and T._align_best([(1, 3), (0, 1), (big, 3 * big + 1)]) == -1
    # all shifts equal: 0
    assert T.align_scores(*_counts(50, 2, None))["best"] == 0
    # an exact tie between -1 and +1 in a recording: mirror-symmetric counts
    both, mov, lab = _counts(30, 2, None, floor=1)
    both[:, -1 + 2] = both[:, 1 + 2] = 9
    both[0, 1], both[-1, 3] = 0, 0
    r = T.align_scores(both, mov, lab)
    assert r["B"][1] == r["B"][3] and r["U"][1] == r["U"][3] and r["best"] == -1


def test_nothing_to_score_is_none():
    n, S = 20, 3
    zero = (np.zeros((n, 2 * S + 1), np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32))
    r = T.align_scores(*zero)
    assert r["best"] is None and r["U"] == [0] * 7
    d = T.align_drift(*zero, window=5)
    assert d["best"] == [None] * 4 and d["changes"] == []
    # a recording shorter than the shift has no pair there at all
    r = T.align_scores(*_counts(2, 3, 0))
    assert r["U"][0] == 0 and r["U"][-1] == 0 and r["best"] == 0


def test_a_peak_at_the_edge_is_reported_as_it_is():
    for peak in (-4, 4):
        rec = {"segment": (10, 50), **T.align_scores(*_counts(40, 4, peak)), "drift": T.align_drift(*_counts(40, 4, peak), 10)}
        assert rec["best"] == peak
        with pytest.raises(ValueError, match=r"cam\.tfrecord, frames \[10, 50\).*edge of -4 \.\. 4"):
            T.auto_label_shift("cam.tfrecord", rec)
    rec = {"segment": (10, 50), **T.align_scores(*_counts(40, 4, 3)), "drift": T.align_drift(*_counts(40, 4, 3), 10)}
    assert T.auto_label_shift("cam.tfrecord", rec) == 3
    rec["best"] = None
    with pytest.raises(ValueError, match="no shift to measure"):
        T.auto_label_shift("cam.tfrecord", rec)


def test_drift_lists_one_change():
    n, S, window = 100, 3, 20
    both, mov, lab = _counts(n, S, 0)
    both[60:, 0 + S] = 5
    both[60:, -1 + S] = 50                                                 # from frame 60 on the labels stand a frame early
    d = T.align_drift(both, mov, lab, window)
    assert d == {"window": window, "best": [0, 0, 0, -1, -1], "changes": [(60, -1)]}
    assert T.align_scores(both, mov, lab)["best"] == 0                     # the whole recording hides it
    # a quiet block in between changes nothing, and the last block takes the remainder
    both[20:40], mov[20:40], lab[20:40] = 0, 0, 0
    for i, j in itertools.product(range(n), range(2 * S + 1)):
        if 20 <= i + j - S < 40:
            both[i, j] = 0                                                 # nothing is labelled there
    d = T.align_drift(both[:95], mov[:95], lab[:95], window)
    assert d["best"] == [0, None, 0, -1] and d["changes"] == [(60, -1)]
    rec = {"segment": (5, 100), **T.align_scores(both[:95], mov[:95], lab[:95]), "drift": d}
    with pytest.raises(ValueError, match=r"frames \[5, 100\).*frame 65: -1"):
        T.auto_label_shift("cam", rec)
    assert "drift (blocks of 20 frames): frame 65: shift -1" in T.align_report_text("cam", rec)
    with pytest.raises(ValueError):
        T.align_drift(both, mov, lab, 0)
    with pytest.raises(ValueError):
        T.align_scores(both[:, :4], mov, lab)


# ------------------------------------------------------------------------------------------------ 2. the sampler
SEGS = [(0, 21), (21, 27), (27, 60), (60, 62)]


def _windows_before(segments, mode, strides):
    """windows() as it was before label_shift existed."""
    reach = 3 * min(strides)
    rows = []
    for a, b in segments:
        k = np.arange(a + 3, a + (b - a) // 4 * 4, 4) if mode == "skip" else np.arange(a, b)
        k = k[k - reach >= a].astype(np.int64)
        rows.append(np.stack([np.full(k.size, a, np.int64), k], axis=1))
    return np.concatenate(rows)


@pytest.mark.parametrize("mode,strides", [("skip", (1,)), ("overlap", (1,)), ("overlap", (1, 2)), ("overlap", (2, 3)), ("skip", (2,))])
def test_shift_zero_is_what_it_was(mode, strides):
    table = T.windows(SEGS, mode, strides)
    assert table.dtype == np.int64 and (table == _windows_before(SEGS, mode, strides)).all()
    assert (T.windows(SEGS, mode, strides, label_shift=0) == table).all()
    for flip, reverse, shuffle in itertools.product(((), "x", "xy"), (False, True), (False, True)):
        kw = dict(strides=strides, data_seed=3, epoch=2, model=1, shuffle=shuffle, flip=flip, reverse=reverse)
        plain = T.epoch_samples(table, **kw)
        assert plain.tobytes() == T.epoch_samples(table, label_shift=0, **kw).tobytes()
        assert plain.tobytes() == T.epoch_samples(table, label_shift=np.zeros(len(table), np.int64), **kw).tobytes()
        # what a sample's label was before the keyword: the newest frame, or the oldest of a reversed window
        assert (plain["label"] == plain["frame"][:, 0]).all()


@pytest.mark.parametrize("s", [-3, 3])
@pytest.mark.parametrize("mode,strides", [("skip", (1,)), ("overlap", (1, 2))])
def test_shifted_labels_stay_inside_their_segment(s, mode, strides):
    table = T.windows(SEGS, mode, strides, label_shift=s)
    plain = T.windows(SEGS, mode, strides)
    assert 0 < len(table) < len(plain)
    if mode == "overlap":                                                  # |s| windows fewer per segment that had that many
        assert len(table) == sum(max(0, b - a - 3 * min(strides) - abs(s)) for a, b in SEGS)
    for reverse in (False, True):
        kw = dict(strides=strides, data_seed=1, epoch=4, shuffle=True, flip="xy", reverse=reverse)
        got, base = T.epoch_samples(table, label_shift=s, **kw), T.epoch_samples(table, **kw)
        labelling = base["frame"][:, 0]
        assert (got["label"] == labelling + s).all() and (got["frame"] == base["frame"]).all() and (got["flags"] == base["flags"]).all()
        if reverse:
            assert (base["frame"][:, 0] < base["frame"][:, 3]).any()
        for smp in got:
            a, b = next((a, b) for a, b in SEGS if a <= smp["frame"][0] < b)
            assert a <= smp["label"] < b and all(a <= f < b for f in smp["frame"])
    # one shift per row: rows of the two tables joined
    both = np.concatenate([plain[:5], table[:5]])
    per_row = np.concatenate([np.zeros(5, np.int64), np.full(5, s, np.int64)])
    got = T.epoch_samples(both, strides, label_shift=per_row)
    assert (got["label"] == got["frame"][:, 0] + per_row).all()


def test_balanced_samples_key_on_the_shifted_label():
    table = T.windows([(0, 40)], "overlap", label_shift=2)
    smp = T.epoch_samples(table, label_shift=2)
    mass = np.zeros(40, np.uint32)
    mass[smp["label"][::2]] = 100                                          # busy by the frame that labels them
    out = T.balanced_samples(smp, mass, 50)
    assert len(out) == len(smp) and set(out["label"].tolist()) <= set(smp["label"].tolist())
    assert 0.3 < float((mass[out["label"]] >= 50).mean()) < 0.7


# ------------------------------------------------------------------------------------------------ 3. the command line
def test_arguments_parse():
    a = T.parse_args(["a.tfrecord", "--windows", "overlap", "--align-report"])
    assert a.align_report == 8 and a.resident and a.label_shift is None and a.align_window == 256
    a = T.parse_args(["--windows", "skip", "--align-report", "32", "--align-window", "64", "a.tfrecord"])
    assert a.align_report == 32 and a.align_window == 64
    a = T.parse_args(["a.tfrecord", "-o", "w.cvhw", "--windows", "overlap", "--label-shift", "-2"])
    assert a.label_shift == -2 and a.resident
    a = T.parse_args(["a.tfrecord", "-o", "w.cvhw", "--windows", "overlap", "--label-shift", "auto"])
    assert a.label_shift == ("auto", 8)
    a = T.parse_args(["a.tfrecord", "-o", "w.cvhw", "--windows", "overlap", "--label-shift", "auto:16", "--balance", "100"])
    assert a.label_shift == ("auto", 16) and a.balance == 100
    a = T.parse_args(["a.tfrecord", "-o", "w.cvhw"])
    assert a.label_shift is None and a.align_report is None and not a.resident


@pytest.mark.parametrize("argv", [
    ["a.tfrecord", "--align-report"],                                      # not on the resident path
    ["a.tfrecord", "-o", "w.cvhw", "--label-shift", "2"],
    ["a.tfrecord", "-o", "w.cvhw", "--shuffle", "--label-shift", "auto"],  # resident, but without --windows
    ["a.tfrecord", "--windows", "overlap", "--align-report", "33"],
    ["a.tfrecord", "--windows", "overlap", "--align-report", "-1"],
    ["a.tfrecord", "--windows", "overlap", "--align-report", "--align-window", "0"],
    ["a.tfrecord", "-o", "w.cvhw", "--windows", "overlap", "--label-shift", "auto:0"],
    ["a.tfrecord", "-o", "w.cvhw", "--windows", "overlap", "--label-shift", "auto:33"],
    ["a.tfrecord", "-o", "w.cvhw", "--windows", "overlap", "--label-shift", "soon"],
    ["a.tfrecord", "--windows", "overlap", "--label-shift", "2"],          # a training still needs its output
])
def test_arguments_refused(argv, capsys):
    with pytest.raises(SystemExit) as e:
        T.parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()
