"""The MoG model as an object (state blob, frozen labelling, background image), without a GPU: the restatements of
tests/mog_model_ref.py against the update they must agree with and against hand-built models, the blob's layout through two
independent writers and readers, the frozen kernels' assembly, and the command line's usage errors.  Bit for bit throughout.

  1. frozen against the update: `classify` equals the mask of a zero-rate update from the same snapshot, on every later frame of
     the branch clip, from snapshots after 4, 6 and 8 learned frames; and the finding that makes frozen a mode of its own: a
     zero-rate update, repeated, leaves non-finite means
  2. `background` on hand-built models
  3. the blob: size, CRC, read_state / write_state against pack / unpack, what read_state refuses
  4. the frozen kernels' assembly
  5. command line usage errors, raised before a context is created; the NULL checks of the library
  6. OpenCV parity where cv2 is installed
"""
import copy
import ctypes as C
import re
import struct

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import mog
from tests import mog_isa
from tests import mog_model_ref as MR
from tests import mog_ref as R
from tests import mog_shadow_ref as SR

HIST, TB, NF, SEED = SR.GPU_CLIP


# ------------------------------------------------------------------------------------------------ 1. frozen against the update
def test_classify_is_the_zero_rate_update_without_its_writes():
    clip = SR.shadow_clip(NF, SEED)
    mdl = R.Mog2(npix=640 * 360, history=HIST, var_threshold=TB)
    for k in range(8):
        mdl.apply(clip[k])
        if k + 1 not in (4, 6, 8):
            continue
        assert all(np.isfinite(a).all() for a in (mdl.W, mdl.V, mdl.M))
        before = copy.deepcopy(mdl)
        for f in range(k + 1, NF):
            got = MR.classify(mdl, clip[f])
            assert (got == MR.zero_rate_mask(mdl, clip[f])).all(), (k + 1, f)
            assert (got == 0).any() and (got == 255).any()
        for name in ("W", "V", "M", "nmodes"):                   # neither function writes
            assert (getattr(mdl, name) == getattr(before, name)).all() and mdl.n == before.n
    # every value of the three-valued mask occurs, and the scripted tau-edge pixels read 127 and 255 (frozen after 6, frame 8)
    m6 = R.Mog2(npix=640 * 360, history=HIST, var_threshold=TB)
    for f in clip[:6]:
        m6.apply(f)
    r3 = MR.classify3(m6, clip[8], SR.CLIP_TAU)
    assert r3[0, SR.PX_TAU_EDGE] == 127 and r3[0, SR.PX_TAU_BELOW] == 255 and (r3 == 0).sum() > 100000 and (r3 == 127).sum() > 1000


def test_a_zero_rate_update_is_not_safe_to_repeat():
    """OpenCV's apply(frame, 0) in the letter of MOG2Invoker: a new mode of weight 0, then k = 0 / 0."""
    clip = SR.shadow_clip(NF, SEED, 128, 128)
    mdl = R.Mog2(npix=128 * 128, history=HIST, var_threshold=TB)
    keep = R.learning_rates
    R.learning_rates = lambda n, history: (np.float32(0), np.float32(-0.0))
    try:
        for f in clip:
            mdl.apply(f)
    finally:
        R.learning_rates = keep
    assert not np.isfinite(mdl.M).all()


def test_an_empty_model_is_all_foreground():
    mdl = R.Mog2(npix=64)
    fr = np.arange(64 * 3, dtype=np.uint8).reshape(8, 8, 3)
    assert (MR.classify(mdl, fr) == 255).all() and (MR.classify3(mdl, fr, 0.5) == 255).all()
    assert not MR.background(mdl).any()


# ------------------------------------------------------------------------------------------------ 2. background
def test_background_on_hand_built_models():
    arrays, want = MR.hand_models()
    got = MR.background(MR.model_of({**arrays, "n": 0})).reshape(MR.HAND_H, MR.HAND_W, 3)
    for x, case in enumerate(MR.HAND_CASES):
        assert got[0, x].tolist() == list(case[3]), (x, got[0, x].tolist())
    assert (got == want).all()


# ------------------------------------------------------------------------------------------------ 3. the blob
def test_blob_layout_size_and_crc():
    assert MR.crc32c(b"123456789") == 0xE3069283                 # the CRC-32C check value
    arrays, _ = MR.hand_models()
    blob = MR.pack(**arrays, n=7, history=HIST, var_threshold=TB)
    P = MR.HAND_W * MR.HAND_H
    assert len(blob) == 64 + 101 * P + 4 == mog.state_size(MR.HAND_W, MR.HAND_H)
    assert blob[:4] == b"CVHM" and struct.unpack_from("<IiiifqI", blob, 4) == (1, 128, 128, HIST, TB, 7, 0) and not any(blob[32:64])
    assert struct.unpack_from("<I", blob, len(blob) - 4)[0] == MR.crc32c(blob[:-4])
    assert mog.write_state(arrays["W"], arrays["V"], arrays["M"], arrays["nmodes"], n=7, history=HIST, var_threshold=TB) == blob
    st = mog.read_state(blob)
    un = MR.unpack(blob)
    assert {k: st[k] for k in ("work_w", "work_h", "history", "var_threshold", "n")} == \
        {"work_w": 128, "work_h": 128, "history": HIST, "var_threshold": TB, "n": 7}
    for k in ("W", "V", "M", "nmodes"):
        assert st[k].dtype == arrays[k].dtype and (st[k].view(np.uint8) == arrays[k].view(np.uint8)).all(), k
        assert (un[k].view(np.uint8) == arrays[k].view(np.uint8)).all(), k
    assert mog.write_state(**{k: st[k] for k in ("W", "V", "M", "nmodes", "n", "history", "var_threshold")}) == blob


def test_read_state_refuses_what_the_library_refuses():
    arrays, _ = MR.hand_models()
    blob = MR.pack(**arrays)
    flipped = bytearray(blob)
    flipped[1000] ^= 1
    six = {**arrays, "nmodes": arrays["nmodes"].copy()}
    six["nmodes"][5, 5] = 6
    for bad in (blob[:-1], blob + b"\0", bytes(flipped), b"CVHX" + blob[4:], blob[:4] + b"\2" + blob[5:], MR.pack(**six),
                MR.pack(**arrays, n=-1), blob[:60], b""):
        with pytest.raises(ValueError):
            mog.read_state(bad)
    for kw in (dict(n=-1), dict(nmodes=six["nmodes"]), dict(W=arrays["W"][:4])):
        with pytest.raises(ValueError):
            mog.write_state(**{**arrays, **kw})


# ------------------------------------------------------------------------------------------------ 4. assembly
STORE = re.compile(r"^\s+(global|flat|buffer)_store_\w+", re.M)
DIV = re.compile(r"^\s+v_(div_\w+|rcp_f64\w*)", re.M)


def test_frozen_kernels_assembly():
    """48 frozen instances (the 24 update kernels, without and with the shadow test) and the background kernel: no f32 fused
    multiply-add, no scratch.  Without the shadow test a frozen kernel stores one thing, the wave's ballot word, and has no
    division (the shadow test keeps its own, a = num / den)."""
    ks = mog_isa.kernels("mog_frozen.hip", r"k_mog_\w*update")
    assert len(ks) == 48, sorted(ks)
    for fam, count in ((r"k_mog_update", 6), (r"k_mog_grid_update", 8), (r"k_mog_yuv_update", 28), (r"k_mog_any_\w*update", 6)):
        assert sum(bool(re.search(fam, n)) for n in ks) == count, fam
    plain = 0
    for name, k in ks.items():
        assert "Lb1EEEv" in name, name                               # FROZEN = true is the last template argument
        assert not mog_isa.FMA.search(k["body"]) and not mog_isa.SCRATCH.search(k["body"]) and k["scratch"] == 0, name
        if "Lb0ELb1EEEv" in name:
            plain += 1
            assert len(STORE.findall(k["body"])) == 1 and not DIV.search(k["body"]), name
        else:
            assert len(STORE.findall(k["body"])) == 2, name
    assert plain == 24
    bg = mog_isa.kernels("mog_frozen.hip", r"k_mog_background")
    assert len(bg) == 1
    for name, k in bg.items():
        assert not mog_isa.FMA.search(k["body"]) and not mog_isa.SCRATCH.search(k["body"]) and k["scratch"] == 0, name
    assert len(mog_isa.kernels("mog_frozen.hip", r"k_mog_")) == 49


# ------------------------------------------------------------------------------------------------ 5. usage errors, NULL checks
def test_command_line_usage_errors_come_before_a_context(monkeypatch, tmp_path):
    from cova_amd import elements

    def no_context(*a, **k):
        raise AssertionError("a context was created")

    monkeypatch.setattr(elements, "Context", no_context)
    state = tmp_path / "a.cvhm"
    state.write_bytes(b"x")
    base = ["--size", "1280x720"]
    for argv in (["a.bgr", "b.bgr", "--save-state", "a.cvhm"],                         # counts that do not match the inputs
                 ["a.bgr", "--load-state", str(state), str(state)],
                 ["a.bgr", "b.bgr", "--background", "a.ppm"],
                 ["a.bgr", "--frozen"],                                                # --frozen without a state
                 ["-:out.dump", "--two-pass"],                                         # --two-pass on stdin
                 ["a.bgr", "--two-pass", "--frozen", "--load-state", str(state)],
                 ["a.bgr", "--load-state", str(tmp_path / "missing.cvhm")],
                 ["a.bgr", "b.bgr", "--save-state", "s.cvhm", "s.cvhm"],               # two inputs write the same file
                 ["a.bgr:x.out", "--background", "x.out"]):
        with pytest.raises(SystemExit) as e:
            mog.main(base + argv)
        assert e.value.code == 2, argv
    a = mog._args(base + ["a.bgr", "b.bgr", "--load-state", str(state), str(state), "--frozen", "--background", "a.ppm", "b.ppm"])
    assert a.load_state == [str(state)] * 2 and a.frozen and a.background == ["a.ppm", "b.ppm"] and a.save_state is None
    a = mog._args(base + ["a.bgr", "--two-pass", "--save-state", "a.cvhm"])
    assert a.two_pass and a.save_state == ["a.cvhm"] and not a.frozen and a.load_state is None


def test_null_labeller_is_refused():
    lib = L.lib()
    n = C.c_size_t()
    v = C.c_int()
    buf = (C.c_uint8 * 8)()
    assert lib.covahip_mog_state_size(None, C.byref(n)) == 1
    assert lib.covahip_mog_save_state(None, 0, buf, 8, C.byref(n)) == 1
    assert lib.covahip_mog_load_state(None, 0, buf, 8) == 1
    assert lib.covahip_mog_set_frozen(None, 0, 1) == 1 and lib.covahip_mog_get_frozen(None, 0, C.byref(v)) == 1
    assert lib.covahip_mog_background(None, 0, buf, 8, L.MEM_HOST) == 1


# ------------------------------------------------------------------------------------------------ 6. OpenCV parity (where cv2 exists)
def test_restatements_match_opencv_where_available():
    cv = pytest.importorskip("cv2")
    clip = SR.shadow_clip(NF, SEED)
    sub = cv.createBackgroundSubtractorMOG2(history=HIST, varThreshold=TB, detectShadows=False)
    mdl = R.Mog2(history=HIST, var_threshold=TB)
    for f in clip[:6]:
        sub.apply(f)
        mdl.apply(f)
    assert (sub.getBackgroundImage().reshape(-1, 3) == MR.background(mdl)).all()
    # one zero-rate frame (a second one may meet the 0 / 0 of the finding above)
    assert (sub.apply(clip[6], learningRate=0) == MR.classify(mdl, clip[6])).all()
