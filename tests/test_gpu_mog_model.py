"""The MoG labeller's model as an object on the GPU: frozen labelling (covahip_mog_set_frozen), the state blob
(covahip_mog_save_state / _load_state) and the background image (covahip_mog_background), against the numpy restatements of
tests/mog_model_ref.py.  Bit for bit: there is no tolerance anywhere in this file.  The clip, the sizes and the labellers are those
of tests/test_gpu_mog_shadow.py.

  1. frozen, one case per update kernel, with shadows off, DROP and KEEP: learn the first frames, freeze, apply the next in several
     calls (raw mask 0 / 127 / 255, filled mask, labels and shadow counts equal the restatement on the snapshot; the model and n stay
     bit for bit), unfreeze and apply one more frame (as a labeller that never saw the frozen frames); a reset frozen stream is all 255
  2. learning and frozen streams in one call: three ragged streams, the mode switched between calls, a reset in between; each
     stream equals its own single-stream labeller
  3. exact resume across kinds of labeller, save -> load -> save, and every refusal of load
  4. the background image at four working sizes, one stream and all of three, the hand-built edge cases through load_state, host
     and device destinations, cap one byte short
  5. the command line: --two-pass, --save-state / --load-state --frozen, --background
"""
import copy
import ctypes as C
import functools
import struct

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import mog
from cova_amd import train as T
from tests import mog_model_ref as MR
from tests import mog_ref as R
from tests import mog_shadow_ref as SR
from tests import mog_yuv_ref as Y
from tests import test_gpu_mog_shadow as TS

pytestmark = pytest.mark.gpu

HIST, TB, NF, SEED = SR.GPU_CLIP
TAU = SR.CLIP_TAU
KW = TS.KW
MODES = (None, "drop", "keep")
# kind: (working size, frames learned first, frames per frozen call); the case's last frame is the one learned after the thaw
CASES = {"ref640": ((640, 360), 6, 2), "grid320": ((320, 180), 6, 3), "band1280": ((1280, 720), 1, 1), "yuv640": ((640, 360), 4, 2),
         "any": ((133, 129), 6, 2), "any_yuv": ((133, 129), 4, 2)}


def _apply(m, kind, lo, hi):
    """Frames lo .. hi - 1 of the case through one call of labeller m (stream 0): its labels [hi - lo][lh][lw]."""
    src = TS._source(kind)[0]
    if isinstance(src, tuple):
        y, u, v = (a[lo:hi] for a in src)
        lay = Y.padded(640, 360, "nv12") if kind == "yuv640" else Y.tight(TS.ANY_W, TS.ANY_H, "i420")
        return m.apply_yuv(Y.pack(y, u, v, lay), lay.ctypes(), hi - lo)[:, 0]
    return m.apply(src[lo:hi, None])[:, 0]


@functools.lru_cache(maxsize=None)
def _ref(kind):
    """The restatement of a case, once: the model after the learned frames, the frozen frames' three-valued and two-valued masks on
    it, and the model and masks of the last frame learned on top of the snapshot."""
    work = TS._source(kind)[1]
    learn = CASES[kind][1]
    n = work.shape[0]
    mdl = R.Mog2(npix=work.shape[1] * work.shape[2], **KW)
    for f in work[:learn]:
        mdl.apply(f)
    snap = copy.deepcopy(mdl)
    frozen2 = np.stack([MR.classify(snap, f) for f in work[learn:n - 1]])
    frozen3 = np.stack([MR.classify3(snap, f, TAU) for f in work[learn:n - 1]])
    last3 = SR.apply3(mdl, work[n - 1], TAU)                     # (the model does not depend on the shadow test)
    last2 = np.where(last3 == 127, np.uint8(255), last3)
    return {"snap": snap, "frozen": {None: frozen2, "drop": frozen3, "keep": frozen3}, "final": mdl,
            "last": {None: last2, "drop": last3, "keep": last3}}


def _same_state(a, b, what=""):
    assert a["n"] == b["n"], what
    for k in ("W", "V", "M", "nmodes"):
        assert (a[k].view(np.uint8) == b[k].view(np.uint8)).all(), (what, k)


def _check(m, lab, raw_r, mode, what):
    """labels, raw and filled masks and the counts of the labeller's last call against the restatement's raw masks."""
    raw, fil = m.debug_masks()
    sh, fg = m.shadow_counts()
    for i, r in enumerate(raw_r):
        fl, lb = R.post(SR.fg_of(r, mode))
        assert (raw[i, 0] == r).all(), (what, "raw", i, int((raw[i, 0] != r).sum()))
        assert (fil[i, 0] == fl).all() and (lab[i] == lb).all(), (what, "filled / labels", i)
        assert sh[i, 0] == (r == 127).sum() and fg[i, 0] == (r == 255).sum(), (what, "counts", i)


# ------------------------------------------------------------------------------------------------ 1. frozen, per update kernel
@pytest.mark.parametrize("kind", list(CASES))
def test_frozen_on_each_update_kernel(ctx, kind):
    work, learn, per = CASES[kind]
    ref = _ref(kind)
    n = TS._source(kind)[1].shape[0]
    assert ref["frozen"]["drop"].shape[1:] == work[::-1]
    if kind != "band1280":                                       # (its one frozen frame comes right after frame 1)
        assert all((ref["frozen"]["drop"] == v).any() for v in (0, 127, 255))
    for mode in MODES:
        m = TS._labeller(ctx, kind, shadows=None if mode is None else (mode, TAU))
        assert (m.work_w, m.work_h) == work and m.frozen == (False,)
        for lo in range(0, learn, 3):
            _apply(m, kind, lo, min(lo + 3, learn))
        before = m.state(0)
        TS._model_equal(before, ref["snap"], (kind, mode, "learned"))
        m.set_frozen(True)
        assert m.frozen == (True,)
        for lo in range(learn, n - 1, per):
            hi = min(lo + per, n - 1)
            lab = _apply(m, kind, lo, hi)
            _check(m, lab, ref["frozen"][mode][lo - learn:hi - learn], mode, (kind, mode, "frozen", lo))
        _same_state(m.state(0), before, (kind, mode, "the model after the frozen calls"))
        m.set_frozen(False, 0)
        lab = _apply(m, kind, n - 1, n)
        _check(m, lab, ref["last"][mode][None], mode, (kind, mode, "thawed"))
        TS._model_equal(m.state(0), ref["final"], (kind, mode, "thawed"))
        m.close()
    if kind == "ref640":                                         # DROP and KEEP give different labels on this clip
        assert any((R.post(SR.fg_of(r, "drop"))[1] != R.post(SR.fg_of(r, "keep"))[1]).any() for r in ref["frozen"]["drop"])


def test_a_reset_frozen_stream_is_all_foreground(ctx):
    for mode in MODES:
        m = TS._labeller(ctx, "any", shadows=None if mode is None else (mode, TAU))
        m.set_frozen(True)
        _apply(m, "any", 0, 2)
        m.reset(0)
        assert m.frozen == (True,)                               # reset keeps the setting
        lab = _apply(m, "any", 2, 4)
        raw, fil = m.debug_masks()
        assert (raw == 255).all() and (fil == 1).all() and (lab == 1).all(), mode
        st = m.state(0)
        assert st["n"] == 0 and not st["nmodes"].any() and not st["W"].any()
        m.close()


def test_set_frozen_arguments(ctx):
    lib = L.lib()
    m = mog.MogLabeler(ctx, 640, 360, streams=3, grid="macroblock", **KW)
    assert m.frozen == (False, False, False)
    m.set_frozen(True, 1)
    assert m.frozen == (False, True, False)
    for stream, frozen in ((3, 1), (-2, 1), (0, 2), (0, -1)):
        assert lib.covahip_mog_set_frozen(m.handle, stream, frozen) == 1 and m.frozen == (False, True, False)
    v = C.c_int(-7)
    assert lib.covahip_mog_get_frozen(m.handle, -1, C.byref(v)) == 1 and lib.covahip_mog_get_frozen(m.handle, 1, None) == 1
    m.set_frozen(True)
    assert m.frozen == (True, True, True)
    m.set_frozen(False, 2)
    assert m.frozen == (True, True, False)
    m.close()


# ------------------------------------------------------------------------------------------------ 2. learning and frozen streams
# (shadow mode, n_valid, frozen streams) per call; before call 2 stream 1 is reset
MIX_CALLS = ((None, (3, 3, 2), ()), ("drop", (3, 3, 1), (1,)), ("keep", (2, 3, 3), (1,)), (None, (3, 0, 3), (1, 2)), ("drop", (1, 2, 3), (0,)))


def test_learning_and_frozen_streams_in_one_call(ctx):
    clip = TS._clip()
    vids = (clip, np.ascontiguousarray(clip[::-1]), np.roll(clip, 5, axis=0))
    frames = np.ascontiguousarray(np.stack(vids, 1))             # [12][3][360][640][3]
    mk = lambda streams: mog.MogLabeler(ctx, 640, 360, streams=streams, grid="macroblock", **KW)
    a, solo = mk(3), [mk(1) for _ in range(3)]
    for c, (mode, nv, frozen) in enumerate(MIX_CALLS):
        if c == 2:
            a.reset(1)
            solo[1].reset(0)
        chunk = np.ascontiguousarray(frames[2 * c:2 * c + 3])
        outs = []
        for lab_s, (m, streams) in enumerate([(a, (0, 1, 2))] + [(solo[s], (s,)) for s in range(3)]):
            m.set_shadows(None if mode is None else (mode, TAU))
            for i, s in enumerate(streams):
                m.set_frozen(s in frozen, i)
            lab = m.apply(np.ascontiguousarray(chunk[:, list(streams)]), n_valid=[nv[s] for s in streams],
                          labels=np.full((3, len(streams), 23, 40), 9, np.uint8))
            outs.append((lab,) + m.debug_masks() + m.shadow_counts())
        for s in range(3):
            for f in range(3):
                if f >= nv[s]:
                    assert (outs[0][0][f, s] == 9).all() and outs[0][3][f, s] == 0 and outs[0][4][f, s] == 0, (c, s, f)
                    continue
                for got, one in zip(outs[0], outs[1 + s]):
                    assert (got[f, s] == one[f, 0]).all(), (c, mode, s, f)
            _same_state(a.state(s), solo[s].state(0), (c, s))
        if c == 2:                                               # the reset stream is frozen and empty: all foreground
            assert (outs[0][1][:, 1] == 255).all() and a.state(1)["n"] == 0
    assert [a.state(s)["n"] for s in range(3)] == [3 + 3 + 2 + 3, 2, 2 + 1 + 3 + 3]
    a.close()
    for m in solo:
        m.close()


# ------------------------------------------------------------------------------------------------ 3. exact resume
def _continue(m, s, streams, src, lo, per=3):
    """src's frames lo .. through stream s of labeller m (the other streams sit the calls out): (raw, labels) and the final state."""
    raws, labs = [], []
    for i in range(lo, src.shape[0], per):
        part = src[i:i + per]
        frames = np.zeros((part.shape[0], streams) + part.shape[1:], np.uint8)
        frames[:, s] = part
        lab = m.apply(frames, n_valid=[part.shape[0] if t == s else 0 for t in range(streams)])
        raws.append(m.debug_masks()[0][:, s])
        labs.append(lab[:, s])
    return np.concatenate(raws), np.concatenate(labs), m.state(s)


def test_exact_resume_from_the_reference_grid_into_an_any_size_labeller(ctx):
    clip, k = TS._clip(), 5
    a = mog.MogLabeler(ctx, 640, 360, **KW)
    a.apply(clip[:k, None])
    blob = a.save_state(0)
    assert len(blob) == mog.state_size(640, 360) == 64 + 101 * 640 * 360 + 4
    st = mog.read_state(blob)                                    # (verifies the CRC)
    assert (st["work_w"], st["work_h"], st["history"], st["var_threshold"], st["n"]) == (640, 360, HIST, TB, k)
    _same_state(MR.unpack(blob, verify=False), a.state(0), "the blob is the model")
    raw_a, lab_a, end_a = _continue(a, 0, 1, clip, k)
    b = mog.MogLabeler(ctx, 1280, 720, streams=3, grid="macroblock", force_general=True, **KW)
    assert b.general and (b.work_w, b.work_h) == (640, 360)
    b.load_state(1, blob)
    assert b.save_state(1) == blob                               # save -> load -> save
    raw_b, lab_b, end_b = _continue(b, 1, 3, TS._up2(clip), k)   # the 2x2 mean of the upsampled clip is the clip exactly
    assert (raw_a == raw_b).all() and (lab_a == lab_b).all()
    _same_state(end_a, end_b, "resumed")
    assert end_b["n"] == NF and b.state(0)["n"] == 0 and not b.state(2)["nmodes"].any()
    a.close()
    b.close()


def test_exact_resume_at_a_padded_pitch_and_every_refusal(ctx):
    src, k = TS._source("any")[0], 5
    mk = lambda streams: mog.MogLabeler(ctx, TS.ANY_W, TS.ANY_H, streams=streams, grid="macroblock", any_size=True, **KW)
    a, b = mk(1), mk(3)
    a.apply(src[:k, None])
    blob = a.save_state(0)
    assert len(blob) == mog.state_size(133, 129)
    _same_state(MR.unpack(blob), a.state(0), "the blob is the model")      # (the CRC by this file's own byte loop)
    b.apply(np.ascontiguousarray(np.stack([src[:2]] * 3, 1)))              # a model of its own in every stream first
    b.load_state(2, blob)
    assert b.save_state(2) == blob and b.state(0)["n"] == 2
    raw_a, lab_a, end_a = _continue(a, 0, 1, src, k)
    raw_b, lab_b, end_b = _continue(b, 2, 3, src, k)
    assert (raw_a == raw_b).all() and (lab_a == lab_b).all()
    _same_state(end_a, end_b, "resumed")
    # refusals: all or nothing
    lib = L.lib()
    st = mog.read_state(blob)
    six = st["nmodes"].copy()
    six[128, 132] = 6
    flipped = bytearray(blob)
    flipped[len(blob) // 2] ^= 0x10
    hand = MR.hand_models()[0]
    too_many = MR.pack(st["W"], st["V"], st["M"], six, n=k, history=HIST, var_threshold=TB, crc=0)[:-4]   # a nmodes of 6, the CRC right
    too_many += struct.pack("<I", T.crc32c(too_many))
    negative = blob[:24] + struct.pack("<q", -1) + blob[32:-4]                 # n < 0 under a CRC that holds
    negative += struct.pack("<I", T.crc32c(negative))
    keep = [b.save_state(s) for s in range(3)]

    def load(s, data):
        buf = np.frombuffer(bytes(data), np.uint8)
        return lib.covahip_mog_load_state(b.handle, s, buf.ctypes.data if buf.size else None, buf.size)

    for data, s, want in ((blob[:-1], 0, 8), (blob[:50], 0, 8), (bytes(flipped), 0, 8), (b"CVHX" + blob[4:], 0, 8),
                          (too_many, 0, 8),
                          (negative, 0, 8),
                          (mog.write_state(**hand), 0, 1),                   # 128x128: another working size
                          (blob, 3, 1), (blob, -1, 1), (b"", 0, 1)):
        assert load(s, data) == want, (len(data), s, want)
        assert [b.save_state(t) for t in range(3)] == keep
    n = C.c_size_t()
    small = np.full(16, 7, np.uint8)
    assert lib.covahip_mog_save_state(b.handle, 0, small.ctypes.data, 16, C.byref(n)) == 7 and n.value == len(blob) and (small == 7).all()
    assert lib.covahip_mog_save_state(b.handle, 0, None, 0, C.byref(n)) == 7 and lib.covahip_mog_save_state(b.handle, 3, None, 0, C.byref(n)) == 1
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 4. the background image
@pytest.mark.parametrize("kind", ["ref640", "grid320", "band1280", "any"])
def test_background_against_the_restatement(ctx, kind):
    """Three streams: stream 0 learns every frame, stream 1 none, stream 2 all but the last; one stream and all of them (-1)."""
    (mw, mh), learn, _ = CASES[kind]
    learn = max(learn, 3)
    src, work = TS._source(kind)
    mdl = copy.deepcopy(_ref(kind)["snap"])
    for f in work[CASES[kind][1]:learn]:
        mdl.apply(f)
    want = MR.background(mdl).reshape(mh, mw, 3)
    m = TS._labeller(ctx, kind, streams=3)
    for lo in range(learn):
        m.apply(np.ascontiguousarray(np.stack([src[lo:lo + 1]] * 3, 1)), n_valid=[1, 0, int(lo < learn - 1)])
    assert [m.state(s)["n"] for s in range(3)] == [learn, 0, learn - 1]
    got = m.background(0)
    assert got.shape == (mh, mw, 3) and (got == want).all(), int((got != want).sum())
    every = m.background()
    assert every.shape == (3, mh, mw, 3) and not every[1].any() and (every[0] != every[2]).any()
    for s in range(3):
        assert (every[s] == m.background(s)).all(), s
        assert (every[s] == MR.background(MR.model_of(m.state(s), **KW)).reshape(mh, mw, 3)).all(), s
    if kind == "ref640":                                         # the walk ends at every depth on this model
        tw = np.cumsum(mdl.W, 0)
        depth = np.where(mdl.nmodes > 0, np.minimum((tw <= R.TB).sum(0) + 1, mdl.nmodes), 0)
        assert all((depth == d).sum() > 1000 for d in range(1, 6))
    m.close()


def test_background_of_three_streams_and_its_arguments(ctx):
    lib = L.lib()
    src = TS._source("any")[0]
    m = mog.MogLabeler(ctx, TS.ANY_W, TS.ANY_H, streams=3, grid="macroblock", any_size=True, **KW)
    m.apply(np.ascontiguousarray(np.stack([src[:6], src[2:8], src[4:10]], 1)), n_valid=[6, 0, 3])
    every = m.background()
    assert every.shape == (3, 129, 133, 3) and not every[1].any()            # an empty model gives (0, 0, 0)
    for s in range(3):
        assert (every[s] == m.background(s)).all()
        assert (every[s] == MR.background(MR.model_of(m.state(s), **KW)).reshape(129, 133, 3)).all()
    assert (every[0] != every[2]).any()
    # destinations and cap
    need = every[2].nbytes
    d = ctx.malloc(3 * need)
    try:
        out = np.empty_like(every)
        assert lib.covahip_mog_background(m.handle, -1, d, 3 * need, L.MEM_DEVICE) == 0
        ctx.d2h(out, d)
        assert (out == every).all()
        assert lib.covahip_mog_background(m.handle, -1, d, 3 * need - 1, L.MEM_DEVICE) == 7
    finally:
        ctx.free(d)
    buf = np.full(need, 77, np.uint8)
    assert lib.covahip_mog_background(m.handle, 2, buf.ctypes.data, need - 1, L.MEM_HOST) == 7 and (buf == 77).all()
    assert lib.covahip_mog_background(m.handle, 2, None, need, L.MEM_HOST) == 7
    assert lib.covahip_mog_background(m.handle, 3, buf.ctypes.data, need, L.MEM_HOST) == 1
    assert lib.covahip_mog_background(m.handle, -2, buf.ctypes.data, need, L.MEM_HOST) == 1
    assert lib.covahip_mog_background(m.handle, 2, buf.ctypes.data, need, 5) == 1 and (buf == 77).all()
    assert lib.covahip_mog_background(m.handle, 2, buf.ctypes.data, need, L.MEM_HOST) == 0
    assert (buf.reshape(129, 133, 3) == every[2]).all()
    m.close()


def test_background_edge_cases_through_load_state(ctx):
    arrays, want = MR.hand_models()
    m = mog.MogLabeler(ctx, 2 * MR.HAND_W, 2 * MR.HAND_H, streams=2, grid="macroblock", any_size=True)
    assert m.general and (m.work_w, m.work_h) == (MR.HAND_W, MR.HAND_H)
    m.load_state(1, MR.pack(**arrays, n=3))
    got = m.background(1)
    for x, case in enumerate(MR.HAND_CASES):
        assert got[0, x].tolist() == list(case[3]), (x, got[0, x].tolist())
    assert (got == want).all() and not m.background(0).any() and m.state(1)["n"] == 3
    m.close()


# ------------------------------------------------------------------------------------------------ 5. the command line
def _ppm(path, w, h):
    data = path.read_bytes()
    head = b"P6\n%d %d\n255\n" % (w, h)
    assert data.startswith(head) and len(data) == len(head) + w * h * 3
    return np.frombuffer(data, np.uint8, offset=len(head)).reshape(h, w, 3)[..., ::-1]


def test_cli_two_pass_states_and_background(ctx, tmp_path):
    clip = TS._clip()
    p, q = tmp_path / "v.bgr", tmp_path / "w.bgr"
    p.write_bytes(clip.tobytes())
    q.write_bytes(np.ascontiguousarray(clip[::-1]).tobytes())
    argv = ["--size", "640x360", "--grid", "macroblock", "--history", str(HIST), "--var-threshold", str(TB), "--chunk", "5",
            "--shadows", "drop:0.5"]
    # the API's answers: learn the clip, then label it frozen; then the second file against that model
    m = TS._labeller(ctx, "grid320", shadows=("drop", TAU))
    m.apply(clip[:, None])
    blob, bg = m.save_state(0), m.background(0)
    m.set_frozen(True)
    second_pass = m.apply(clip[:, None])[:, 0]
    other = m.apply(np.ascontiguousarray(clip[::-1])[:, None])[:, 0]
    m.close()
    out, state, ppm = tmp_path / "two.dump", tmp_path / "v.cvhm", tmp_path / "v.ppm"
    assert mog.main(argv + [f"{p}:{out}", "--two-pass", "--save-state", str(state), "--background", str(ppm)]) == 0
    assert (np.fromfile(out, np.uint8).reshape(NF, 23, 40) == second_pass).all()
    assert state.read_bytes() == blob and (_ppm(ppm, 320, 180) == bg).all()
    out2, ppm2 = tmp_path / "w.dump", tmp_path / "w.ppm"
    assert mog.main(argv + [f"{q}:{out2}", "--load-state", str(state), "--frozen", "--background", str(ppm2)]) == 0
    assert (np.fromfile(out2, np.uint8).reshape(NF, 23, 40) == other).all() and (_ppm(ppm2, 320, 180) == bg).all()
    # a piece continued from a state equals the uncut recording
    whole, cut = tmp_path / "whole.dump", tmp_path / "cut.dump"
    h0, h1 = tmp_path / "h0.bgr", tmp_path / "h1.bgr"
    h0.write_bytes(clip[:7].tobytes())
    h1.write_bytes(clip[7:].tobytes())
    assert mog.main(argv + [f"{p}:{whole}"]) == 0
    assert mog.main(argv + [f"{h0}:{tmp_path / 'h0.dump'}", "--save-state", str(tmp_path / "h0.cvhm")]) == 0
    assert mog.main(argv + [f"{h1}:{cut}", "--load-state", str(tmp_path / "h0.cvhm")]) == 0
    assert (np.fromfile(cut, np.uint8) == np.fromfile(whole, np.uint8)[7 * 23 * 40:]).all()
