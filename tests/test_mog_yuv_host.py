"""The MoG labeller's NV12 / I420 entry (covahip_mog_apply_yuv, cova_amd.mog.apply_yuv) without a GPU: the conversion's numpy
restatement (tests/mog_yuv_ref.py) against known answers and, where cv2 exists, cv2.cvtColor; the layout structure and helper,
the raw and YUV4MPEG2 readers, the command line, the argument checks that come before any GPU call, and the ISA of
the update kernels on surfaces."""
import ctypes as C
import io

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import mog
from tests import mog_isa
from tests import mog_yuv_ref as Y


# ------------------------------------------------------------------------------------------------ conversion
KNOWN = [  # (Y, U, V) -> (B, G, R) limited | full
    ((81, 90, 240), (0, 0, 254), (14, 14, 238)),
    ((41, 240, 110), (255, 0, 0), (239, 15, 16)),
    ((145, 54, 34), (1, 255, 0), (14, 238, 13)),
    ((210, 16, 146), (0, 255, 255), (12, 236, 235)),
    ((16, 128, 128), (0, 0, 0), (16, 16, 16)),
    ((235, 128, 128), (255, 255, 255), (235, 235, 235)),
    ((0, 128, 128), (0, 0, 0), (0, 0, 0)),
]


@pytest.mark.parametrize("yuv,limited,full", KNOWN)
def test_known_answers(yuv, limited, full):
    y = np.full((2, 2), yuv[0], np.uint8)
    u, v = np.full((1, 1), yuv[1], np.uint8), np.full((1, 1), yuv[2], np.uint8)
    for rng, want in (("limited", limited), ("full", full)):
        got = Y.yuv_to_bgr(y, u, v, rng)
        assert got.shape == (2, 2, 3) and (got == np.array(want, np.uint8)).all(), (rng, got[0, 0])


def test_constants_are_the_rounded_coefficients():
    lim = Y.LIMITED
    assert [lim["ymul"], lim["bu"], lim["gu"], lim["gv"], lim["rv"]] == [round(c * 2 ** 20) for c in (1.164, 2.018, 0.391, 0.813, 1.596)]
    assert lim["ysub"] == 16
    ful = Y.FULL
    assert [ful["bu"], ful["gv"], ful["gu"], ful["rv"]] == [round(c * 2 ** 20) for c in (1.772, 0.714136, 0.344136, 1.402)]
    assert ful["ysub"] == 0 and ful["ymul"] == 1 << 20


def test_chroma_sample_is_shared_by_the_2x2_block_and_int32_is_enough():
    rng = np.random.default_rng(5)
    y = rng.integers(0, 256, (4, 6), dtype=np.uint8)
    u = rng.integers(0, 256, (2, 3), dtype=np.uint8)
    v = rng.integers(0, 256, (2, 3), dtype=np.uint8)
    got = Y.yuv_to_bgr(y, u, v)
    for (r, c) in ((0, 0), (1, 1), (3, 5), (2, 3)):
        one = Y.yuv_to_bgr(np.full((2, 2), y[r, c], np.uint8), u[r // 2:r // 2 + 1, c // 2:c // 2 + 1], v[r // 2:r // 2 + 1, c // 2:c // 2 + 1])
        assert (got[r, c] == one[0, 0]).all()
    for c in (Y.LIMITED, Y.FULL):                      # the header's int32: every partial sum stays below 2^31
        assert 255 * c["ymul"] + (1 << 19) + 128 * max(c["bu"], c["rv"], c["gv"] + c["gu"]) < 2 ** 31


def test_parity_with_cvtcolor_where_available():
    cv = pytest.importorskip("cv2")
    rng = np.random.default_rng(9)
    h, w = 36, 64
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    u = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    v = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    want = Y.yuv_to_bgr(y, u, v, "limited")
    nv12 = np.concatenate([y, np.stack([u, v], -1).reshape(h // 2, w)])
    assert (cv.cvtColor(nv12, cv.COLOR_YUV2BGR_NV12) == want).all()
    i420 = np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).reshape(h * 3 // 2, w)
    assert (cv.cvtColor(i420, cv.COLOR_YUV2BGR_I420) == want).all()


def test_forward_transform_round_trips_roughly():
    """bgr_to_yuv420 only makes inputs; it is still close enough that a converted clip looks like its source."""
    rng = np.random.default_rng(2)
    bgr = rng.integers(0, 256, (18, 32, 3)).repeat(2, 0).repeat(2, 1).astype(np.uint8)     # flat 2x2 blocks: chroma loses nothing
    for r in ("limited", "full"):
        back = Y.yuv_to_bgr(*Y.bgr_to_yuv420(bgr, r), r)
        assert np.abs(back.astype(int) - bgr).max() <= 4, r


def test_packers_place_samples_and_fill_the_rest():
    rng = np.random.default_rng(4)
    F, S, w, h = 2, 2, 64, 8
    y = rng.integers(0, 256, (F, S, h, w), dtype=np.uint8)
    u = rng.integers(0, 256, (F, S, h // 2, w // 2), dtype=np.uint8)
    v = rng.integers(0, 256, (F, S, h // 2, w // 2), dtype=np.uint8)
    for fmt in ("nv12", "i420"):
        lay = Y.padded(w, h, fmt, streams=S, frames=F)
        buf = (Y.pack_nv12 if fmt == "nv12" else Y.pack_i420)(y, u, v, lay, seed=1)
        other = Y.pack(y, u, v, lay, seed=2)
        lo, hi = Y.extent(w, h, fmt, lay.offset, lay.pitch)
        assert buf.size == (F - 1) * lay.frame_stride + (S - 1) * lay.stream_stride + hi
        b0 = 1 * lay.frame_stride + 1 * lay.stream_stride
        assert (buf[b0 + 3 * lay.pitch[0]:][:w] == y[1, 1, 3]).all()
        if fmt == "nv12":
            row = buf[b0 + lay.offset[1] + 2 * lay.pitch[1]:][:w]
            assert (row[0::2] == u[1, 1, 2]).all() and (row[1::2] == v[1, 1, 2]).all()
        else:
            assert (buf[b0 + lay.offset[1] + 2 * lay.pitch[1]:][:w // 2] == u[1, 1, 2]).all()
            assert (buf[b0 + lay.offset[2] + 3 * lay.pitch[2]:][:w // 2] == v[1, 1, 3]).all()
        same = buf == other                            # only the samples agree between two seeds (up to chance)
        assert same[b0:b0 + w].all() and not same[b0 + w:b0 + lay.pitch[0]].all()
        n_samples = F * S * w * h * 3 // 2
        assert n_samples <= same.sum() < n_samples + buf.size // 32


# ------------------------------------------------------------------------------------------------ layout
def test_sizeof_mog_yuv():
    assert C.sizeof(L.MogYuv) == 72
    assert L.MogYuv.offset.offset == 8 and L.MogYuv.pitch.offset == 32
    assert L.MogYuv.frame_stride.offset == 56 and L.MogYuv.stream_stride.offset == 64


def _fields(lay):
    return (lay.format, lay.range, list(lay.offset), list(lay.pitch), lay.frame_stride, lay.stream_stride)


def test_yuv_tight_against_hand_written_offsets():
    assert _fields(mog.yuv_tight(640, 360, "nv12")) == (1, 0, [0, 230400, 0], [640, 640, 0], 345600, 345600)
    assert _fields(mog.yuv_tight(640, 360, "i420", "full", streams=3)) == (2, 1, [0, 230400, 288000], [640, 320, 320], 1036800, 345600)
    assert _fields(mog.yuv_tight(1920, 1080, "nv12", streams=2)) == (1, 0, [0, 2073600, 0], [1920, 1920, 0], 6220800, 3110400)
    assert _fields(mog.yuv_tight(1920, 1080, "i420")) == (2, 0, [0, 2073600, 2592000], [1920, 960, 960], 3110400, 3110400)
    # stream-major: [S][F][frame]
    assert _fields(mog.yuv_tight(640, 360, "nv12", streams=4, stream_major=True, frames=5)) == \
        (1, 0, [0, 230400, 0], [640, 640, 0], 345600, 5 * 345600)
    assert _fields(mog.yuv_tight(1920, 1080, "i420", "full", streams=2, stream_major=True, frames=3)) == \
        (2, 1, [0, 2073600, 2592000], [1920, 960, 960], 3110400, 3 * 3110400)
    for kw in (dict(fmt="yv12"), dict(fmt="nv12", range="wide"), dict(fmt="nv12", stream_major=True)):
        with pytest.raises(ValueError):
            mog.yuv_tight(640, 360, **kw)
    with pytest.raises(ValueError):
        mog.yuv_tight(641, 360, "nv12")
    # the test helper's tight layout is the same one
    for fmt in ("nv12", "i420"):
        assert _fields(Y.tight(1920, 1080, fmt, "full", streams=2).ctypes()) == _fields(mog.yuv_tight(1920, 1080, fmt, "full", streams=2))


def test_null_arguments_need_no_gpu():
    lib = L.lib()
    lay = L.MogYuv()
    fake = C.c_void_p(8)                                # never dereferenced: the NULL checks come first
    assert lib.covahip_mog_yuv_tight(None, 1, 0, C.byref(lay)) == 1
    assert lib.covahip_mog_yuv_tight(fake, 1, 0, None) == 1
    buf = np.zeros(16, np.uint8)
    lab = np.zeros(16, np.uint8)
    assert lib.covahip_mog_apply_yuv(None, C.byref(lay), buf.ctypes.data, 1, None, lab.ctypes.data, L.MEM_HOST) == 1
    assert lib.covahip_mog_apply_yuv(fake, None, buf.ctypes.data, 1, None, lab.ctypes.data, L.MEM_HOST) == 1
    assert lib.covahip_mog_apply_yuv(fake, C.byref(lay), None, 1, None, lab.ctypes.data, L.MEM_HOST) == 1
    assert lib.covahip_mog_apply_yuv(fake, C.byref(lay), buf.ctypes.data, 1, None, None, L.MEM_HOST) == 1
    assert lib.covahip_mog_apply_yuv(fake, C.byref(lay), buf.ctypes.data, 1, None, lab.ctypes.data, L.MEM_HOST) == 1   # format 0


# ------------------------------------------------------------------------------------------------ readers
class Dribble(io.RawIOBase):
    """A stream that hands out at most 7 bytes per read, as a pipe may."""

    def __init__(self, data):
        self.b = io.BytesIO(data)

    def readable(self):
        return True

    def readinto(self, out):
        return self.b.readinto(memoryview(out)[:7])

    def read(self, n=-1):
        return self.b.read(min(n, 7) if n >= 0 else 7)


def test_read_yuv420_whole_frames_then_a_partial_one(tmp_path):
    w, h = 16, 8
    fb = w * h * 3 // 2
    data = np.random.default_rng(1).integers(0, 256, 5 * fb, dtype=np.uint8)
    for fmt in ("nv12", "i420"):
        got = list(mog.read_yuv420(io.BytesIO(data.tobytes()), w, h, 2, fmt))
        assert [g.shape for g in got] == [(2, fb), (2, fb), (1, fb)]
        assert (np.concatenate(got).reshape(-1) == data).all()
    p = tmp_path / "v.i420"
    p.write_bytes(data.tobytes())
    assert sum(g.shape[0] for g in mog.read_yuv420(str(p), w, h, 8)) == 5
    assert len(list(mog.read_yuv420(Dribble(data.tobytes()[:3 * fb]), w, h, 8))) == 1
    assert list(mog.read_yuv420(io.BytesIO(b""), w, h, 3)) == []
    with pytest.raises(ValueError, match="truncated"):
        list(mog.read_yuv420(io.BytesIO(data.tobytes()[:2 * fb + 5]), w, h, 2))
    with pytest.raises(ValueError):
        list(mog.read_yuv420(io.BytesIO(b""), w, h, 0))
    with pytest.raises(ValueError):
        list(mog.read_yuv420(io.BytesIO(b""), w, h, 2, "yv12"))


def _y4m(w, h, frames, tags=b"C420jpeg XCOLORRANGE=FULL", frame_tags=b""):
    out = b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1" % (w, h) + (b" " + tags if tags else b"") + b"\n"
    for f in frames:
        out += b"FRAME" + frame_tags + b"\n" + f.tobytes()
    return out


def test_read_y4m():
    w, h = 16, 8
    fb = w * h * 3 // 2
    frames = np.random.default_rng(3).integers(0, 256, (5, fb), dtype=np.uint8)
    r = mog.read_y4m(io.BytesIO(_y4m(w, h, frames)), 2)
    assert (r.w, r.h, r.fmt, r.range) == (w, h, "i420", "full")
    got = list(r)
    assert [g.shape for g in got] == [(2, fb), (2, fb), (1, fb)] and (np.concatenate(got) == frames).all()
    # no C tag, no range; frame parameters are skipped; a pipe's short reads
    r = mog.read_y4m(Dribble(_y4m(w, h, frames, tags=b"", frame_tags=b" Ip")), 8)
    assert (r.w, r.h, r.range) == (w, h, None)
    assert (np.concatenate(list(r)) == frames).all()
    assert mog.read_y4m(io.BytesIO(_y4m(w, h, frames, tags=b"C420mpeg2 XCOLORRANGE=LIMITED")), 1).range == "limited"
    for tag in (b"C420", b"C420paldv"):
        assert mog.read_y4m(io.BytesIO(_y4m(w, h, frames[:1], tags=tag)), 1).w == w
    assert list(mog.read_y4m(io.BytesIO(_y4m(w, h, frames[:0])), 4)) == []
    for tag in (b"C444", b"C422", b"C420p10", b"Cmono"):
        with pytest.raises(ValueError, match="4:2:0"):
            mog.read_y4m(io.BytesIO(_y4m(w, h, frames, tags=tag)), 2)
    with pytest.raises(ValueError, match="truncated"):
        list(mog.read_y4m(io.BytesIO(_y4m(w, h, frames)[:-5]), 2))
    with pytest.raises(ValueError):
        mog.read_y4m(io.BytesIO(b"RIFF....AVI \n"), 2)
    with pytest.raises(ValueError):
        list(mog.read_y4m(io.BytesIO(_y4m(w, h, frames[:1]) + b"GARBAGE\n"), 2))


# ------------------------------------------------------------------------------------------------ command line
def test_cli_format_parsing(tmp_path, capsys):
    a = mog._args(["--format", "nv12", "--size", "1920x1080", "--range", "full", "a.nv12"])
    assert (a.format, a.range, a.size) == ("nv12", "full", (1920, 1080))
    a = mog._args(["--size", "1280x720", "a.bgr"])
    assert (a.format, a.range) == ("bgr24", "limited")
    a = mog._args(["--format", "y4m", "-:out_gt.dump"])
    assert a.size is None and a.inputs == [("-", "out_gt.dump")]
    for argv in (["--format", "nv12", "a.nv12"], ["--format", "i420", "a.yuv"], ["--format", "yv12", "--size", "640x360", "a"],
                 ["--format", "nv12", "--size", "640x360", "--range", "wide", "a"], ["--format", "y4m"],
                 ["--format", "y4m", "--bogus", "a.y4m"]):
        with pytest.raises(SystemExit) as e:
            mog.main(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    # y4m inputs that disagree: with each other, with --size, with --range; a chroma the labeller does not take
    fr = np.zeros((1, 640 * 360 * 3 // 2), np.uint8)
    a360, b720, full = tmp_path / "a.y4m", tmp_path / "b.y4m", tmp_path / "c.y4m"
    a360.write_bytes(_y4m(640, 360, fr, tags=b"C420"))
    b720.write_bytes(_y4m(1280, 720, fr[:0], tags=b""))
    full.write_bytes(_y4m(640, 360, fr))
    c444 = tmp_path / "d.y4m"
    c444.write_bytes(_y4m(640, 360, fr[:0], tags=b"C444"))
    for argv in (["--format", "y4m", str(a360), str(b720)], ["--format", "y4m", "--size", "1280x720", str(a360)],
                 ["--format", "y4m", "--range", "limited", str(full)], ["--format", "y4m", str(c444)],
                 ["--format", "y4m", str(tmp_path / "missing.y4m")]):
        with pytest.raises(SystemExit) as e:
            mog.main(argv)
        assert e.value.code == 2, argv
        assert "error" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        mog.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--format" in out and "--range" in out


# ------------------------------------------------------------------------------------------------ ISA
def test_yuv_kernels_isa_no_f32_fma_no_scratch():
    """With the flags of test_mog_host's ISA test: seven geometries x two formats of update kernel on surfaces (mog_update.hip),
    none with an f32 fused multiply-add, none with scratch, each within 128 VGPRs (four waves per SIMD, as the BGR24 kernels)."""
    ks = mog_isa.assert_update_family(r"k_mog_yuv_update", 14)
    for name, k in ks.items():
        assert k["vgprs"] <= 128, (name, k["vgprs"])
