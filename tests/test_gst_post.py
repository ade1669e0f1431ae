"""blobnetfilter with per-pad post-processing: `pad-ignore-rects` and `pad-mask-threshold` give a sink pad its ignore region and its
mask threshold; pads that share a weights file but not the settings become separate models of one set."""
import os
import subprocess

import numpy as np
import pytest

from cova_amd import elements as E
from tests.test_gst_elements import CLK, CONDA, DRIVER, _env, _read, _run, _write, pytestmark  # noqa: F401  (the same skip rule)


def test_inspect_lists_post_properties(tmp_path):
    r = subprocess.run([os.path.join(CONDA, "bin", "gst-inspect-1.0"), "blobnetfilter"], env=_env(tmp_path), capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    for p in ("pad-ignore-rects", "pad-mask-threshold"):
        assert f"  {p} " in r.stdout or f"  {p}:" in r.stdout, p


def _input(tmp_path, carriers, n):
    recs = []
    for i in range(n):
        for s in range(len(carriers)):
            recs.append(("B", i * CLK, s << 8, carriers[s][i].tobytes()))
    recs += [("e", 0, s << 8, b"") for s in range(len(carriers))]
    _write(tmp_path / "in.rec", recs)


@pytest.mark.gpu
def test_blobnetfilter_pad_post(tmp_path):
    """Four streams on ONE weights file: sink_0 and sink_1 with different ignore rectangles, sink_2 with a mask threshold, sink_3
    with nothing.  Every stream's payloads equal the direct call with those settings."""
    from cova_amd import synth, weights as W
    from cova_amd.elements import BlobNetInfer, Context, keep_from_rects
    h, w, n_streams, n, batch_size = 45, 80, 4, 24, 32
    model = W.random_init(41, fg_bias=0.1)
    path = tmp_path / "w.bin"
    path.write_bytes(W.to_bytes(model))
    rects = {0: [(0, 0, 300, 200), (1000, 600, 400, 400)], 1: [(320, 0, 16, 720)]}
    prob = {2: 0.8}
    rects_prop = ";".join(f"{s}=" + "+".join(",".join(str(v) for v in r) for r in rs) for s, rs in rects.items())
    thr_prop = ";".join(f"{s}={p}" for s, p in prob.items())
    carriers = [synth.carrier_frames(n, h, w, seed=700 + s, n_objects=5) for s in range(n_streams)]
    _input(tmp_path, carriers, n)
    caps = f"video/x-raw,format=I420,width={w * 16},height={h * 16},framerate=30/1"
    info = _run(["mux", f"blobnetfilter model-weights-file={path} pad-ignore-rects=\"{rects_prop}\" pad-mask-threshold=\"{thr_prop}\" "
                 f"batch-size={batch_size} cc-threshold=2 max-boxes=512", str(n_streams), caps, str(tmp_path / "in.rec"),
                 str(tmp_path / "out.rec")], tmp_path)
    assert info["buffers"] == n_streams * (n - 3) and info["eos"] == n_streams
    per_stream = {s: [] for s in range(n_streams)}
    for kind, pts, pad, payload in _read(tmp_path / "out.rec"):
        per_stream[pad].append((pts, payload))
    ctx = Context(0)
    net = BlobNetInfer(ctx, model, h, w, max_batch=n - 3)
    payloads = {}
    for s in range(n_streams):
        keep = keep_from_rects(h, w, rects[s]) if s in rects else None
        net.set_post(0, prob_thresh=prob.get(s), keep=keep)
        stack = np.stack([np.concatenate([carriers[s][i - j] for j in range(4)], axis=0) for i in range(3, n)])
        boxes, counts, _ = net.filter(stack, cc_threshold=2, max_boxes=512)
        payloads[s] = [E.serialize_vec(E.boxes_to_bbox(boxes[j, :counts[j]])) for j in range(n - 3)]
        assert counts.sum() > 0
        assert [p for p, _ in per_stream[s]] == [i * CLK for i in range(3, n)]
        assert [p for _, p in per_stream[s]] == payloads[s], s
    # the settings matter: the same stream under the defaults gives other boxes (independent of the element)
    net.reset_post(0)
    for s in (0, 1, 2):
        stack = np.stack([np.concatenate([carriers[s][i - j] for j in range(4)], axis=0) for i in range(3, n)])
        boxes, counts, _ = net.filter(stack, cc_threshold=2, max_boxes=512)
        assert [E.serialize_vec(E.boxes_to_bbox(boxes[j, :counts[j]])) for j in range(n - 3)] != payloads[s], s
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("props", ['pad-ignore-rects="0=1,2,3"', 'pad-ignore-rects="0=1,2,3,x"', 'pad-ignore-rects="zero=1,2,3,4"',
                                   'pad-mask-threshold="0=1.0"', 'pad-mask-threshold="0=0.5x"', 'pad-mask-threshold="0="'])
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
