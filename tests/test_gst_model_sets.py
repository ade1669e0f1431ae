"""blobnetfilter with a model set: `pad-model-weights` maps sink pads to weight files, all of them served from one batch."""
import os
import subprocess

import numpy as np
import pytest

from cova_amd import elements as E
from tests.test_gst_elements import CLK, CONDA, _env, _read, _run, _write, pytestmark  # noqa: F401  (the same skip rule)


def test_inspect_lists_pad_model_weights(tmp_path):
    r = subprocess.run([os.path.join(CONDA, "bin", "gst-inspect-1.0"), "blobnetfilter"], env=_env(tmp_path), capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "  pad-model-weights " in r.stdout or "  pad-model-weights:" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("records", [False, True])
def test_blobnetfilter_pad_model_weights(tmp_path, records):
    """8 streams, 3 models (model-weights-file for the pads the property does not name): every stream's payloads equal the
    single-model C-ABI path for its model."""
    from cova_amd import synth, weights as W
    from cova_amd.elements import BlobNetInfer, Context
    h, w, n_streams, n, batch_size = 45, 80, 8, 40, 64
    models = [W.random_init(41, fg_bias=-0.3), W.blob_like(5), W.random_init(43, fg_bias=0.2)]
    paths = []
    for k, m in enumerate(models):
        paths.append(tmp_path / f"w{k}.bin")
        paths[-1].write_bytes(W.to_bytes(m))
    pad_model = {0: 0, 1: 1, 2: 2, 3: 0, 4: 1, 5: 2, 6: 2, 7: 0}
    prop = ";".join(f"{s}={paths[k]}" for s, k in pad_model.items() if k != 0)
    carriers = [synth.carrier_frames(n, h, w, seed=900 + s, n_objects=5) for s in range(n_streams)]
    recs = []
    for i in range(n):
        for s in range(n_streams):
            recs.append(("B", i * CLK, s << 8, E.pack_frames(carriers[s][i]).tobytes() if records else carriers[s][i].tobytes()))
    recs += [("e", 0, s << 8, b"") for s in range(n_streams)]
    _write(tmp_path / "in.rec", recs)
    info = _run(["mux", f"blobnetfilter model-weights-file={paths[0]} pad-model-weights=\"{prop}\" batch-size={batch_size} "
                 f"cc-threshold=4 max-boxes=512", str(n_streams),
                 f"application/x-cova-records,width-mbs={w},height-mbs={h},framerate=30/1" if records else
                 f"video/x-raw,format=I420,width={w * 16},height={h * 16},framerate=30/1",
                 str(tmp_path / "in.rec"), str(tmp_path / "out.rec")], tmp_path)
    assert info["buffers"] == n_streams * (n - 3) and info["eos"] == n_streams
    per_stream = {s: [] for s in range(n_streams)}
    for kind, pts, pad, payload in _read(tmp_path / "out.rec"):
        per_stream[pad].append((pts, payload))
    ctx = Context(0)
    total = 0
    for k in range(len(models)):
        net = BlobNetInfer(ctx, models[k], h, w, max_batch=n - 3)
        for s in [s for s, m in pad_model.items() if m == k]:
            stack = np.stack([np.concatenate([carriers[s][i - j] for j in range(4)], axis=0) for i in range(3, n)])
            boxes, counts, _ = net.filter(stack, cc_threshold=4, max_boxes=512)
            assert [p for p, _ in per_stream[s]] == [i * CLK for i in range(3, n)]
            for j, (_, payload) in enumerate(per_stream[s]):
                assert payload == E.serialize_vec(E.boxes_to_bbox(boxes[j, :counts[j]])), (s, k, j)
                total += int(counts[j])
    assert total > 0
    ctx.close()
