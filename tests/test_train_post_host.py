"""The yardstick of tests/test_gpu_train_post.py, checked without a GPU: the masked f64 reference (tests/torch_blobnet_post.py)
is the unmasked one under an all-ones keep map, does not see labels at ignored macroblocks, and lies so far from both the
unmasked step and a planted masking bug that tests/torch_blobnet_train.py's BOUNDS tell them apart; and the command line of
python -m cova_amd.train takes and refuses --post / --ignore-rects / --mask-threshold as documented."""
import numpy as np
import pytest

from cova_amd import calibrate, train as T
from cova_amd.elements import keep_from_rects
from tests import torch_blobnet_post as TP
from tests import torch_blobnet_train as TT

GEO = pytest.mark.parametrize("geo", TP.GEOMETRIES, ids=TP.IDS)


@GEO
def test_all_ones_keep_map_is_the_unmasked_reference_exactly(geo):
    loss, g, logit = TP.reference(*geo, kind="ones")
    loss0, g0, logit0 = TP.reference(*geo, kind="unmasked")
    assert loss == loss0
    assert (g.view(np.uint64) == g0.view(np.uint64)).all()
    assert (logit.view(np.uint64) == logit0.view(np.uint64)).all()


@GEO
def test_masked_reference_does_not_see_ignored_labels(geo):
    h, w, b, p, seed = geo
    flat, stack, gt = TP.inputs(h, w, b)
    keep = TP.keep_map(h, w)
    gt2 = gt.copy()
    gt2[:, keep == 0] ^= 1
    gt2[0, keep == 0] = 255
    assert (gt2 != gt).any() and (gt2[:, keep != 0] == gt[:, keep != 0]).all()
    loss, g, _ = TP.reference(*geo)
    loss2, g2, _ = TP.grads_flat_post(flat, stack, gt2, h, w, keep, seed=seed, step=0, p=float(np.float32(p)))
    assert loss == loss2 and (g.view(np.uint64) == g2.view(np.uint64)).all()


@GEO
def test_bounds_tell_the_masked_step_from_the_unmasked_one_and_from_a_planted_bug(geo):
    """Measured over the three geometries (printed): the unmasked step lies 2,996 - 10,126 x outside BOUNDS of the masked
    reference, the planted bug (y masked in S, p not) 1,760 - 16,166 x.  Asserted: each at least 1,000 x outside.  BOUNDS sit
    about 7 x above the error of a correct step, so a step three orders of magnitude beyond them is not a correct step with
    unlucky rounding: a post that does nothing, or half of it, cannot pass the GPU test."""
    loss, g, _ = TP.reference(*geo)
    out = {}
    for kind in ("unmasked", "bug"):
        l2, g2, _ = TP.reference(*geo, kind=kind)
        out[kind] = TT.excess(TT.errors(l2, g2, loss, g))
    print(f"{geo}: unmasked {out['unmasked']:.0f} x, planted bug {out['bug']:.0f} x outside the bounds")
    assert out["unmasked"] >= 1000, out
    assert out["bug"] >= 1000, out
    assert TT.excess(TT.errors(loss, g, loss, g)) == 0


# ------------------------------------------------------------------------------------------------ the command line
def _exits(argv):
    with pytest.raises(SystemExit) as e:
        T.parse_args(argv)
    assert e.value.code == 2
    return True


@pytest.fixture()
def sidecar(tmp_path):
    path = tmp_path / "post.json"
    calibrate.save_post(path, {"logit_thresh": 0.4054651, "cc_threshold": 4}, ignore_rects=[(32, 16, 80, 48)])
    return str(path)


def test_cli_post_options(tmp_path, sidecar):
    rec, out = ["a.tfrecord"], ["-o", str(tmp_path / "o.cvhw")]
    a = T.parse_args(rec + out + ["--post", sidecar])
    (kw,) = T.post_settings(a, 1)
    want, _ = calibrate.load_post(sidecar, 45, 80)
    assert kw["logit_thresh"] == want["logit_thresh"] == float(np.float32(0.4054651)) and (kw["keep"] == want["keep"]).all()
    assert int((kw["keep"] == 0).sum()) == 15
    a = T.parse_args(rec + out + ["--ignore-rects", "32,16,80,48+0,0,16,16", "--mask-threshold", "0.6", "--h-mb", "24", "--w-mb", "50"])
    (kw,) = T.post_settings(a, 1)
    assert kw["prob_thresh"] == 0.6 and (kw["keep"] == keep_from_rects(24, 50, [(32, 16, 80, 48), (0, 0, 16, 16)])).all()
    (kw,) = T.post_settings(T.parse_args(rec + out + ["--mask-threshold", "0.6"]), 1)
    assert kw == {"prob_thresh": 0.6, "keep": None}
    (kw,) = T.post_settings(T.parse_args(rec + out + ["--ignore-rects", "0,0,16,16"]), 1)
    assert kw["prob_thresh"] is None and int((kw["keep"] == 0).sum()) == 1
    assert T.post_settings(T.parse_args(rec + out), 1) is None
    # --post excludes the other two; a bad probability, a bad rectangle, a missing file
    assert _exits(rec + out + ["--post", sidecar, "--ignore-rects", "0,0,16,16"])
    assert _exits(rec + out + ["--post", sidecar, "--mask-threshold", "0.6"])
    assert _exits(rec + out + ["--mask-threshold", "1.0"])
    assert _exits(rec + out + ["--mask-threshold", "0"])
    assert _exits(rec + out + ["--ignore-rects", "0,0,16"])
    assert _exits(rec + out + ["--ignore-rects", "0,0,16,x"])
    assert _exits(rec + out + ["--post", str(tmp_path / "none.json")])
    assert _exits(rec + out + ["--post", str(tmp_path)])                       # a directory needs --set
    # --resume takes the post from the command line again
    a = T.parse_args(rec + out + ["--post", sidecar, "--resume", "run.cvhs", "--freeze", "encoder"])
    assert a.post == sidecar and a.resume == "run.cvhs"


def test_cli_post_with_eval_only(tmp_path, sidecar):
    a = T.parse_args(["--eval-only", "w.cvhw", "a.tfrecord", "--post", sidecar])
    assert a.eval_only == "w.cvhw" and len(T.post_settings(a, 1)) == 1
    a = T.parse_args(["--eval-only", "w.cvhw", "a.tfrecord", "--ignore-rects", "0,0,16,16", "--mask-threshold", "0.3"])
    assert T.post_settings(a, 1)[0]["prob_thresh"] == 0.3
    assert _exits(["--eval-only", "w.cvhw", "a.tfrecord", "--post", sidecar, "--mask-threshold", "0.3"])
    assert _exits(["--eval-only", "w.cvhw", "a.tfrecord", "--post", str(tmp_path / "none.json")])


def test_cli_post_with_set(tmp_path, sidecar):
    recs = ["cam0.tfrecord", "cam1a.tfrecord,cam1b.tfrecord", "d/cam2.tfrecord"]
    base = ["--set", "-o", str(tmp_path / "out")] + recs
    a = T.parse_args(base + ["--post", sidecar])                             # one file for every model
    assert T.post_paths(a.records, a.post) == [sidecar] * 3 and len(T.post_settings(a, 3)) == 3
    d = tmp_path / "posts"
    d.mkdir()
    for k, stem in enumerate(("cam0", "cam1a")):
        calibrate.save_post(d / (stem + ".json"), {"logit_thresh": 0.25 * k, "cc_threshold": 1 + k})
    assert _exits(base + ["--post", str(d)])                                    # cam2.json is missing
    with pytest.raises(ValueError, match="cam2.json"):
        T.post_paths(recs, str(d))
    calibrate.save_post(d / "cam2.json", {"logit_thresh": -0.5, "cc_threshold": 2}, ignore_rects=[(0, 0, 32, 32)])
    a = T.parse_args(base + ["--post", str(d)])
    assert T.post_paths(a.records, a.post) == [str(d / (s + ".json")) for s in ("cam0", "cam1a", "cam2")]
    kws = T.post_settings(a, 3)
    assert [kw["logit_thresh"] for kw in kws] == [0.0, 0.25, -0.5]
    assert kws[0]["keep"] is None and int((kws[2]["keep"] == 0).sum()) == 4
    a = T.parse_args(["--set", "--eval-only", str(tmp_path / "out")] + recs + ["--post", str(d)])
    assert len(T.post_settings(a, 3)) == 3
    a = T.parse_args(base + ["--mask-threshold", "0.7"])                      # the same for every model
    assert T.post_settings(a, 3) == [{"prob_thresh": 0.7, "keep": None}] * 3
