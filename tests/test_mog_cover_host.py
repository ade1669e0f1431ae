"""MoG labels by block coverage, the host side: the numpy helper (tests/mog_cover_ref.py) against its own definitions and the
relations that hold between the modes by construction, the `labels` values of cova_amd.mog, the --labels parser of the command
line and tools/label_cover.py.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import mog
from tests import mog_cover_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(129, 133), (180, 320), (360, 640)]            # (h, w): a 1 x 5 last block; a last label row of 4 rows; all blocks whole


def _masks(h, w):
    """Random filled masks: pixel noise at three densities, 8x8-block noise shifted off the block grid, all 0 and all 1."""
    rng = np.random.default_rng(h * 1000 + w)
    out = [rng.random((h, w)) < d for d in (0.02, 0.5, 0.98)]
    b = np.kron(rng.random((h // 8 + 2, w // 8 + 2)) < 0.3, np.ones((8, 8), bool))
    out.append(b[3:3 + h, 5:5 + w])
    return out + [np.zeros((h, w), bool), np.ones((h, w), bool)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_helper_relations_and_definitions(size):
    h, w = size
    lh, lw = -(-h // 8), -(-w // 8)
    ins = CR.inside(h, w)
    assert ins.shape == (lh, lw) and ins.sum() == h * w and (ins[:-1, :-1] == 64).all()
    assert ins[-1, -1] == (h - 8 * (lh - 1)) * (w - 8 * (lw - 1))
    for f in _masks(h, w):
        CR.relations(f)
        cnt = CR.count(f)
        assert cnt.shape == (lh, lw) and cnt.sum() == f.sum()
        # the definition, block by block, on a sample of blocks that holds the last row and column
        for i in sorted({0, lh // 2, lh - 1}):
            for j in sorted({0, lw // 3, lw - 1}):
                blk = f[8 * i:8 * i + 8, 8 * j:8 * j + 8]
                assert cnt[i, j] == blk.sum() and ins[i, j] == blk.size
                for n in CR.COVER_NS:
                    assert CR.cover(f, n)[i, j] == (64 * blk.sum() >= n * blk.size)
        assert (CR.corner(f) == f[::8, ::8]).all() and CR.corner(f).dtype == np.uint8
        assert (CR.labels(f, "corner") == f[::8, ::8]).all()
        assert (CR.labels(f, "count") == cnt).all() and CR.labels(f, "count").dtype == np.uint8
        assert (CR.labels(f, ("cover", 32)) == CR.cover(f, 32)).all()
    assert not CR.cover(np.zeros((h, w), bool), 1).any() and CR.cover(np.ones((h, w), bool), 64).all()
    assert (CR.count(np.ones((h, w), bool)) == ins).all()


def test_helper_on_small_objects():
    """What the modes are for: a 6x6 object off the corners has no CORNER label and a COVER(1) label in every block it touches."""
    f = np.zeros((64, 64), bool)
    f[17:23, 33:39] = True                                   # inside block (2, 4), no corner
    assert not CR.corner(f).any()
    assert CR.cover(f, 1).sum() == 1 and CR.cover(f, 1)[2, 4] == 1 and CR.count(f)[2, 4] == 36
    assert CR.cover(f, 36)[2, 4] == 1 and CR.cover(f, 37)[2, 4] == 0
    f[:] = False
    f[21:27, 37:43] = True                                   # straddles the corner (24, 40): four blocks
    assert CR.corner(f).sum() == 1 and CR.cover(f, 1).sum() == 4 and sorted(CR.count(f)[CR.count(f) > 0]) == [9, 9, 9, 9]
    with pytest.raises(ValueError):
        CR.cover(f, 0)
    with pytest.raises(ValueError):
        CR.cover(f, 65)


def test_labels_values_and_parser():
    assert mog.LABEL_MODES == {"corner": 0, "cover": 1, "count": 2}
    assert mog.label_mode("corner") == ("corner", 1) and mog.label_mode("count") == ("count", 1)
    assert mog.label_mode("cover") == ("cover", 1) and mog.label_mode(("cover", 64)) == ("cover", 64)
    assert mog.label_mode(["cover", np.int32(8)]) == ("cover", 8)
    for bad in ("any", ("cover", 0), ("cover", 65), ("cover", 1.5), ("cover", True), ("count", 3), ("cover",), 7, None):
        with pytest.raises(ValueError):
            mog.label_mode(bad)
    with pytest.raises(ValueError):                          # before the ctx is touched: None is no ctx
        mog.MogLabeler(None, 1280, 720, labels="most")
    assert mog.parse_labels("corner") == "corner" and mog.parse_labels("count") == "count"
    assert mog.parse_labels("cover") == ("cover", 1) and mog.parse_labels("cover:1") == ("cover", 1)
    assert mog.parse_labels("cover:32") == ("cover", 32) and mog.parse_labels("cover:64") == ("cover", 64)
    a = mog._args(["--size", "1280x720", "a.bgr"])
    assert a.labels == "corner"
    assert mog._args(["--size", "1280x720", "--labels", "cover:48", "a.bgr"]).labels == ("cover", 48)
    assert mog._args(["--any-size", "266x258", "--labels", "count", "a.bgr"]).labels == "count"


@pytest.mark.parametrize("value", ["cover:0", "cover:65", "cover:", "cover:x", "cover:1.5", "cover:-1", "cover:+3", "cover:1:2",
                                   "count:3", "corner:1", "Cover", "half", ""])
def test_cli_refuses_malformed_labels(value, capsys):
    with pytest.raises(SystemExit) as e:
        mog.main(["--size", "1280x720", "--labels", value, "a.bgr"])
    assert e.value.code == 2
    assert "--labels" in capsys.readouterr().err


def test_abi_declares_the_label_entries(capsys):
    lib = L.lib()
    assert lib.covahip_mog_set_labels(None, 0, 1) == 1 and lib.covahip_mog_get_labels(None, None, None) == 1
    text = open(os.path.join(ROOT, "include", "covahip.h")).read()
    assert "COVAHIP_MOG_LABELS_CORNER = 0, COVAHIP_MOG_LABELS_COVER = 1, COVAHIP_MOG_LABELS_COUNT = 2" in text
    with pytest.raises(SystemExit) as e:
        mog.main(["--help"])
    assert e.value.code == 0
    assert "not a trainer input" in text and "not a trainer input" in " ".join(capsys.readouterr().out.split())


def test_label_cover_tool(tmp_path):
    """tools/label_cover.py on a --labels count dump: per N the label mass and the frames with any label, as the helper has them."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import label_cover
    finally:
        sys.path.pop(0)
    rng = np.random.default_rng(1)
    lh, lw, n = 17, 17, 5
    filled = rng.random((n, 129, 133)) < 0.3
    filled[1] = False                                        # a frame with no label at any N
    filled[2, :, :] = False
    filled[2, 40:46, 50:56] = True                           # a frame whose only object is 6x6
    cnt = CR.count(filled).astype(np.uint8)
    p = tmp_path / "v_count.dump"
    p.write_bytes(cnt.tobytes())
    # with the working size the started blocks of the last row and column are weighed by what the image holds of them
    rows = label_cover.table(label_cover.read_counts(str(p), lh, lw), work=(133, 129))
    assert [r["n"] for r in rows] == list(CR.COVER_NS)
    for r in rows:
        lab = CR.cover(filled, r["n"])
        assert r["label_mass"] == int(lab.sum()) and r["frames_with_labels"] == int(lab.any((1, 2)).sum())
    assert any(int(CR.cover(filled, n).sum()) != int((cnt >= n).sum()) for n in CR.COVER_NS)       # (and that differs here)
    # without it every block counts as whole
    rows = label_cover.table(label_cover.read_counts(str(p), lh, lw))
    for r in rows:
        lab = cnt >= r["n"]
        assert r["label_mass"] == int(lab.sum()) and r["frames_with_labels"] == int(lab.any((1, 2)).sum())
        assert r["frames"] == n
    assert rows[0]["frames_with_labels"] == n - 1 and rows[-1]["frames_with_labels"] < n - 1
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "label_cover.py"), str(p), "--labels-size", f"{lw}x{lh}"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert [int(ln[0]) for ln in lines[1:]] == list(CR.COVER_NS)
    assert [int(ln[1]) for ln in lines[1:]] == [r["label_mass"] for r in rows]
    # a dump that is no whole number of frames, and one with a byte above 64 (a corner / cover dump is not a count dump)
    for bad, size in ((cnt.tobytes()[:-1], f"{lw}x{lh}"), (np.full(lh * lw, 65, np.uint8).tobytes(), f"{lw}x{lh}")):
        p.write_bytes(bad)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "label_cover.py"), str(p), "--labels-size", size],
                             capture_output=True, text=True)
        assert out.returncode == 2 and "label_cover" in out.stderr
