"""The input monitor's host side: input_report and tv on hand-made counts, the JSON round trip, the command lines' argument errors
before any context exists, and the numpy restatement (tests/input_stats_ref.py) against a loop-written one."""
import numpy as np
import pytest

from cova_amd import monitor as mon
from cova_amd import train
from tests import input_stats_ref as ref


def _counts(hist_pairs, in_frames=10, intra=0, still=0, h=2, w=3):
    hist = np.zeros(512, np.int64)
    for r, v in hist_pairs:
        hist[r] = v
    return {"in_frames": np.int64(in_frames), "hist": hist, "moving": np.arange(h * w, dtype=np.int64).reshape(h, w),
            "still_frames": np.int64(still), "intra_frames": np.int64(intra), "move_hist": np.arange(16, dtype=np.int64)}


def test_tv_identical_disjoint_and_mixed():
    a = _counts([(0, 90), (9, 10)])
    assert mon.input_report(a, None, a)["tv"] == 0.0
    # the same distribution at another volume is no distance either
    assert mon.input_report(a, None, _counts([(0, 900), (9, 100)]))["tv"] == pytest.approx(0.0, abs=1e-15)
    b = _counts([(1, 5), (73, 5)])
    assert mon.input_report(a, None, b)["tv"] == 1.0
    # worked: p = (0.5, 0.25, 0.25, 0) over bins 0, 1, 8, 64, q = (0.25, 0.25, 0, 0.5): 1/2 (0.25 + 0 + 0.25 + 0.5) = 0.5
    p = _counts([(0, 2), (1, 1), (8, 1)])
    q = _counts([(0, 1), (1, 1), (64, 2)])
    rep = mon.input_report(p, None, q)
    assert rep["tv"] == pytest.approx(0.5)
    # classes: p (0.75, 0.25), q (0.75, 0.25) -> 0; max |mv|: p (0.75 at 0, 0.25 at 1), q (0.5 at 0, 0.5 at 1) -> 0.25
    assert rep["tv_class"] == pytest.approx(0.0) and rep["tv_mv"] == pytest.approx(0.25)
    assert mon.tv([0, 0], [1, 2]) is None and mon.input_report(_counts([]), None, q)["tv"] is None


def test_report_marginals_and_gop():
    # record 0o315: class 5, mv_x 1, mv_y 3; record 6: class 6, no vector; record 0: skip
    c = _counts([(0, 70), (0o315, 20), (6, 10)], in_frames=48, intra=4, still=12)
    rep = mon.input_report(c, None)
    assert rep["frames"] == 48 and rep["macroblocks"] == 100
    assert rep["class_share"][0] == pytest.approx(0.7) and rep["class_share"][5] == pytest.approx(0.2) and rep["class_share"][6] == pytest.approx(0.1)
    assert rep["mv_share"][0] == pytest.approx(0.8) and rep["mv_share"][3] == pytest.approx(0.2)
    assert rep["moving_share"] == pytest.approx(0.2) and rep["still_share"] == pytest.approx(0.25)
    assert rep["gop_estimate"] == pytest.approx(12.0)
    assert mon.input_report(_counts([(0, 5)], intra=0), None)["gop_estimate"] is None
    with_base = mon.input_report(c, None, _counts([(0, 1)], in_frames=30, intra=0))
    assert with_base["baseline_gop_estimate"] is None and with_base["gop_estimate"] == pytest.approx(12.0)
    empty = mon.input_report(_counts([], in_frames=0), None)
    assert empty["moving_share"] == 0.0 and empty["still_share"] == 0.0 and empty["gop_estimate"] is None
    # a snapshot with a model axis
    snap = {k: np.stack([np.asarray(c[k]), np.asarray(c[k]) * 0]) for k in ref.FIELDS}
    assert mon.input_report(snap, 0) == {**rep, "model": 0}
    assert "GoP estimate 12.00" in mon.format_input_report(rep) and "tv" not in mon.format_input_report(rep)
    # p = (0.7, 0.2, 0.1) against q = (1, 0, 0): tv 0.3
    assert with_base["tv"] == pytest.approx(0.3)
    assert "no input drift" in mon.format_input_report(with_base, "cam", 0.5) and "tv 0.3000" in mon.format_input_report(with_base, "cam")
    assert "INPUT DRIFT (tv above 0.2)" in mon.format_input_report(with_base, "cam", 0.2)


def test_json_round_trip(tmp_path):
    c = _counts([(0, 70), (0o315, 20), (511, 2**40)], in_frames=48, intra=4, still=12, h=3, w=5)
    path = tmp_path / "in.json"
    mon.save_inputs(path, c, None)
    back = mon.load_inputs(path)
    assert (back["h_mb"], back["w_mb"]) == (3, 5)
    ref.same(back, c)
    assert back["moving"].shape == (3, 5) and back["hist"].dtype == np.int64
    snap = {k: np.stack([np.asarray(c[k]) * 0, np.asarray(c[k])]) for k in ref.FIELDS}
    mon.save_inputs(path, snap, 1)
    ref.same(mon.load_inputs(path), c)
    assert mon.input_report(c, None, mon.load_inputs(path))["tv"] == 0.0
    path.write_text('{"format": "something-else"}')
    with pytest.raises(ValueError):
        mon.load_inputs(path)


def test_command_line_argument_errors(capsys):
    base = ["a.tfrecord", "b.tfrecord", "--weights", "a.cvhw", "b.cvhw"]
    for extra in (["--input-baseline", "one.json"], ["--save-inputs", "a.json", "b.json", "c.json"], ["--input-drift", "0.1"],
                  ["--input-baseline", "a.json", "b.json", "--input-drift", "1.5"]):
        with pytest.raises(SystemExit) as e:
            mon.parse_args(base + extra)
        assert e.value.code == 2, extra
    ok = mon.parse_args(base + ["--input-baseline", "a.json", "b.json", "--input-drift", "0.1"])
    assert ok.inputs and ok.input_drift == 0.1
    assert not mon.parse_args(base).inputs and mon.parse_args(base + ["--save-inputs", "a.json", "b.json"]).inputs
    for extra in (["--record-report"], ["--windows", "overlap", "--save-inputs", "a.json"],
                  ["--windows", "overlap", "--record-report", "--save-inputs", "a.json", "b.json"]):
        with pytest.raises(SystemExit) as e:
            train.parse_args(["cam.tfrecord"] + extra)
        assert e.value.code == 2, extra
    a = train.parse_args(["cam.tfrecord", "--windows", "overlap", "--record-report", "--save-inputs", "a.json"])
    assert a.record_report and a.save_inputs == ["a.json"]
    capsys.readouterr()


def test_record_report_text():
    st = dict(_counts([(0, 70), (0o315, 20), (6, 10)], in_frames=5, intra=1))
    hist_set = np.zeros(512, np.int64)
    hist_set[0], hist_set[0o315] = 5, 15
    st.update(hist_set=hist_set, set_total=20)
    text = train.record_report_text("cam", st)
    assert "all-skip records among them 25.00 %" in text and "moving macroblocks that are labelled 75.00 %" in text
    assert "GoP estimate 5.00" in text


@pytest.mark.parametrize("packed", [False, True])
def test_the_restatement_against_loops(packed):
    rng = np.random.default_rng(5 + packed)
    h, w, n = 3, 5, 9
    if packed:
        frames = rng.integers(0, 65536, (n, h, w)).astype(np.uint16)
        frames[1] = 0                                   # still
        frames[2] = 0xFE05                              # all intra, bits 9+ set, still not: r = 5
        frames[3] = 0
        frames[3, 1, 2] = 7 << 3                        # exactly one moving macroblock, a field of 7 as given
        frames[4] = 6 | 1 << 6                          # all 15 move: bin 1 + floor(log2 15) = 4
    else:
        frames = rng.integers(0, 256, (n, h, w, 4)).astype(np.uint8)
        frames[1, ..., :3] = 0                          # still whatever byte 3 says
        frames[2, ..., 0] = 7                           # class 7 -> 6: all intra
        frames[3, ..., :3] = 0
        frames[3, 1, 2, 1] = 200                        # one moving macroblock, clipped at 6
    want = ref.input_ref_loops(frames, packed)
    got = ref.input_ref(ref.records(frames, packed))
    for k in ref.FIELDS:
        assert np.array_equal(np.asarray(got[k][0]), np.asarray(want[k])), k
    assert want["still_frames"] >= 1 and want["intra_frames"] >= 1 and want["move_hist"][1] >= 1
    if packed:
        assert want["move_hist"][4] >= 1 and want["hist"][7 << 3] == 1
    assert [ref.move_bin(v) for v in (0, 1, 2, 3, 4, 1 << 14, (1 << 14) - 1, 1 << 20)] == [0, 1, 2, 2, 3, 15, 14, 15]
