"""blobnetfilter with a per-pad area threshold: `pad-cc-threshold` gives a sink pad its own cc-threshold (covahip_blobnet_set_area on
the pad's model); pads it does not name keep the element's `cc-threshold`, and a pipeline without it is what it was."""
import os
import subprocess

import numpy as np
import pytest

from cova_amd import elements as E
from tests.test_gst_elements import CLK, CONDA, DRIVER, _env, _read, _run, _write, pytestmark  # noqa: F401  (the same skip rule)


def test_inspect_lists_pad_cc_threshold(tmp_path):
    r = subprocess.run([os.path.join(CONDA, "bin", "gst-inspect-1.0"), "blobnetfilter"], env=_env(tmp_path), capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "  pad-cc-threshold " in r.stdout or "  pad-cc-threshold:" in r.stdout


def _input(tmp_path, carriers, n):
    recs = []
    for i in range(n):
        for s in range(len(carriers)):
            recs.append(("B", i * CLK, s << 8, carriers[s][i].tobytes()))
    recs += [("e", 0, s << 8, b"") for s in range(len(carriers))]
    _write(tmp_path / "in.rec", recs)


def _frames(rng, n, h, w):
    f = np.zeros((n, h, w, 4), np.uint8)
    f[..., 0] = rng.integers(0, 8, (n, h, w))
    f[..., 1:3] = rng.integers(0, 9, (n, h, w, 2))
    return f


@pytest.mark.gpu
def test_blobnetfilter_pad_cc_threshold(tmp_path):
    """Three streams on ONE weights file: sink_0 at cc 1, sink_1 at cc 8, sink_2 with a mask threshold and nothing else (the element's
    cc-threshold 3).  Every stream's payloads equal a single-stream direct call at its threshold; the same pipeline without
    pad-cc-threshold gives sink_2 the same bytes and the other two the element's threshold."""
    from cova_amd import weights as W
    from cova_amd.elements import BlobNetInfer, Context
    h, w, n_streams, n, batch_size = 45, 80, 3, 20, 24
    model = W.random_init(11, fg_bias=-0.1)        # noise-like: many components of 1 - 10 macroblocks
    path = tmp_path / "w.bin"
    path.write_bytes(W.to_bytes(model))
    rng = np.random.default_rng(6)
    carriers = [_frames(rng, n, h, w) for _ in range(n_streams)]
    _input(tmp_path, carriers, n)
    caps = f"video/x-raw,format=I420,width={w * 16},height={h * 16},framerate=30/1"

    def run(props, out):
        info = _run(["mux", f"blobnetfilter model-weights-file={path} {props} batch-size={batch_size} cc-threshold=3 max-boxes=1024",
                     str(n_streams), caps, str(tmp_path / "in.rec"), str(tmp_path / out)], tmp_path)
        assert info["buffers"] == n_streams * (n - 3) and info["eos"] == n_streams
        per = {s: [] for s in range(n_streams)}
        for kind, pts, pad, payload in _read(tmp_path / out):
            per[pad].append((pts, payload))
        for s in range(n_streams):
            assert [p for p, _ in per[s]] == [i * CLK for i in range(3, n)]
        return {s: [p for _, p in per[s]] for s in range(n_streams)}

    with_cc = run('pad-mask-threshold="2=0.6" pad-cc-threshold="0=1;1=8"', "out1.rec")
    without = run('pad-mask-threshold="2=0.6"', "out2.rec")
    ctx = Context(0)
    net = BlobNetInfer(ctx, model, h, w, max_batch=n - 3)

    def direct(s, cc, prob=None):
        net.set_post(0, prob_thresh=prob)
        stack = np.stack([np.concatenate([carriers[s][i - j] for j in range(4)], axis=0) for i in range(3, n)])
        boxes, counts, _ = net.filter(stack, cc_threshold=cc, max_boxes=1024)
        assert counts.sum() > 0 and counts.max() <= 1024
        return [E.serialize_vec(E.boxes_to_bbox(boxes[j, :counts[j]])) for j in range(n - 3)]

    at = {(s, cc): direct(s, cc) for s in (0, 1) for cc in (1, 3, 8)}
    for s in (0, 1):
        assert at[s, 1] != at[s, 3] != at[s, 8]                      # the thresholds matter (independent of the element)
    assert with_cc[0] == at[0, 1] and with_cc[1] == at[1, 8]
    assert without[0] == at[0, 3] and without[1] == at[1, 3]
    third = direct(2, 3, prob=0.6)
    assert third != direct(2, 3) and with_cc[2] == third and without[2] == third
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("props", ['pad-cc-threshold="0=0"', 'pad-cc-threshold="0=-2"', 'pad-cc-threshold="0=2.5"', 'pad-cc-threshold="0=8x"',
                                   'pad-cc-threshold="0="', 'pad-cc-threshold="zero=2"', 'pad-cc-threshold="0=99999999999"'])
def test_malformed_values_fail_the_start(tmp_path, props):
    from cova_amd import synth, weights as W
    h, w, n = 45, 80, 6
    path = tmp_path / "w.bin"
    path.write_bytes(W.to_bytes(W.random_init(41)))
    _input(tmp_path, [synth.carrier_frames(n, h, w, seed=1, n_objects=2)], n)
    caps = f"video/x-raw,format=I420,width={w * 16},height={h * 16},framerate=30/1"
    r = subprocess.run([DRIVER, "mux", f"blobnetfilter model-weights-file={path} {props} batch-size=8", "1", caps, str(tmp_path / "in.rec"),
                        str(tmp_path / "out.rec")], env=_env(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0, r.stdout
    assert not [rec for rec in _read(tmp_path / "out.rec") if rec[0] == "B"]      # nothing came out
