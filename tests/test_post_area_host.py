"""Per-model area threshold, the parts that need no GPU: calibrate.apply_post on a sidecar round trip, the hint the calibration
tool prints, the new entries' declarations against their ctypes prototypes, and their argument checks."""
import ctypes as C
import os
import re

import numpy as np

from cova_amd import _lib as L
from cova_amd import calibrate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("covahip_blobnet_set_area", "covahip_blobnet_get_area", "covahip_bboxcc_v")


class _Net:
    """Stands in for BlobNetInfer: records what apply_post sets."""
    h, w = 45, 80

    def __init__(self):
        self.calls = []

    def set_post(self, model=0, *, prob_thresh=None, logit_thresh=None, keep=None):
        self.calls.append(("set_post", model, prob_thresh, logit_thresh, keep))

    def set_area(self, model=0, area=0):
        self.calls.append(("set_area", model, area))


def test_apply_post_sidecar_round_trip(tmp_path):
    rects = [(0, 0, 300, 200), (320, 0, 16, 720)]
    choice = {"logit_thresh": float(np.float32(0.8472979)), "cc_threshold": 8}
    path = tmp_path / "post.json"
    calibrate.save_post(path, choice, rects)
    kw, cc = calibrate.load_post(path, 45, 80)                     # load_post keeps its return value
    assert cc == 8 and set(kw) == {"logit_thresh", "keep"}
    for source in (path, str(path), (kw, cc)):
        net = _Net()
        assert calibrate.apply_post(net, 3, source) == 8
        (a, b) = net.calls
        assert a[:3] == ("set_post", 3, None) and a[3] == choice["logit_thresh"]
        assert np.array_equal(a[4], calibrate.keep_from_rects(45, 80, rects)) and not a[4].all()
        assert b == ("set_area", 3, 8)
    calibrate.save_post(path, {"logit_thresh": 0.0, "cc_threshold": 1})
    net = _Net()
    calibrate.apply_post(net, 0, path)
    assert net.calls == [("set_post", 0, None, 0.0, None), ("set_area", 0, 1)]


def test_serving_hint_names_the_pad_property():
    text = calibrate.serving_hint(float(np.log(4.0)), 8, [(0, 0, 32, 32), (64, 0, 16, 16)])
    assert 'pad-mask-threshold="IDX=0.8' in text and 'pad-ignore-rects="IDX=0,0,32,32+64,0,16,16"' in text
    assert 'pad-cc-threshold="IDX=8"' in text and "cc-threshold=8" in text.split("pad-cc-threshold")[1]
    text = calibrate.serving_hint(0.0, 1)
    assert "pad-ignore-rects" not in text and 'pad-mask-threshold="IDX=0.5"' in text and 'pad-cc-threshold="IDX=1"' in text
    import inspect
    assert "serving_hint(" in inspect.getsource(calibrate.main) and "set_area(model" in inspect.getsource(calibrate.main)


def test_header_and_ctypes_agree():
    with open(os.path.join(ROOT, "include", "covahip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    lib = L.lib()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        restype, argtypes = L.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == len(params), (name, params)
        for p, t in zip(params, argtypes):
            assert ("*" in p) == (t is not C.c_int), (name, p, t)      # an int by value, or a pointer
        assert getattr(lib, name).argtypes == argtypes


def test_invalid_arguments_need_no_gpu():
    lib = L.lib()
    v = C.c_int(5)
    assert lib.covahip_blobnet_set_area(None, 0, 1) == 1
    assert lib.covahip_blobnet_get_area(None, 0, C.byref(v)) == 1 and v.value == 5
    m = np.zeros((1, 16, 16), np.uint8)
    assert lib.covahip_bboxcc_v(None, m.ctypes.data, 1, 16, 16, None, None, None, 0, L.MEM_HOST) == 1
