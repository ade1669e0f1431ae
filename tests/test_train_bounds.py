"""The training bounds of tests/torch_blobnet_train.py are not vacuous (CPU, float64 torch, no GPU).

tests/test_gpu_train.py holds the HIP training step to BOUNDS against the float64 reference over the case matrix CASES.  Here
each planted bug of the reference -- a bug the HIP step could have -- must exceed those bounds by at least 3x in at least one
case of the matrix where it is live, and every planted bug must be live somewhere:
  a dropout mask from step k - 1; the two dropout sites of an encoder level swapped; the encoder masks indexed in
  [B][C][H][W][T] instead of NCTHW; the crop of an odd-size decoder block shifted; the odd-size zero pad of an encoder level at
  the bottom / right instead of the top / left; BatchNorm statistics detached from autograd; the Jaccard distance taken over
  the whole batch instead of per sample; the loss mean divided by max_batch instead of the batch.
A float32 run of the same reference passes the bounds.
"""
import pytest
import torch

from tests import torch_blobnet_train as TT

MARGIN = 3.0


def _levels(h, w):
    lv = [(h, w)]
    for _ in range(4):
        lv.append(((lv[-1][0] + 1) // 2, (lv[-1][1] + 1) // 2))
    return lv


def _odd(g):
    return g[0] % 2 or g[1] % 2


def _mutations():
    """(id, case -> forward_loss keywords of the planted bug, or None where it is inert)."""
    m = [("mask-step-k-1", lambda c: {"step": c.steps - 1} if c.steps and c.p else None),
         ("mask-nhwt", lambda c: {"mask_nhwt": True} if c.p else None)]
    for i in range(4):
        m.append((f"swap-sites-enc{i}", lambda c, i=i: {"swap_sites": (i,)} if c.p else None))
        m.append((f"pad-after-enc{i}", lambda c, i=i: {"pad_after": (i,)} if _odd(_levels(c.h, c.w)[i]) else None))
    for j in range(4):      # block j's output is level 3 - j; the odd surplus row / column taken at the other side
        def crop(c, j=j):
            g = _levels(c.h, c.w)[3 - j]
            return {"crop_shift": {j: (-(g[0] % 2), -(g[1] % 2))}} if _odd(g) else None
        m.append((f"crop-dec{j}", crop))
    m += [("bn-detach", lambda c: {"bn_detach": True}),
          ("jaccard-batch", lambda c: {"jaccard_batch": True} if c.batch > 1 else None),
          ("loss-div-max-batch", lambda c: {"loss_div": c.max_batch} if c.batch < c.max_batch else None)]
    return m


MUTATIONS = _mutations()
_BY_COST = sorted(TT.CASES, key=lambda c: c.h * c.w * c.batch)
_refs = {}


def _ref(case):
    if case.id not in _refs:
        _refs[case.id] = case.reference()
    return _refs[case.id]


@pytest.mark.parametrize("mid,mut", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_planted_bug_fails_by_margin(mid, mut):
    seen = []
    for case in _BY_COST:
        kw = mut(case)
        if kw is None:
            continue
        loss, g, _ = case.reference(**kw)
        ref_loss, g_ref, _ = _ref(case)
        r = TT.excess(TT.errors(loss, g, ref_loss, g_ref))
        if r >= MARGIN:
            return
        seen.append(f"{case.id}: {r:.3g}")
    pytest.fail(f"{mid} stays below {MARGIN} x the bounds wherever it is live: {seen or 'nowhere'}")


def test_every_mutation_is_live():
    for mid, mut in MUTATIONS:
        assert any(mut(c) is not None for c in TT.CASES), mid


def test_matrix_covers_the_edges():
    ids = [c.id for c in TT.CASES]
    assert len(set(ids)) == len(ids)
    assert {(c.h, c.w) for c in TT.CASES} >= {(16, 16), (17, 33), (24, 50), (45, 80), (68, 120)}
    assert all(_odd(g) for g in _levels(17, 33)[:4])
    assert len({(h % 2, w % 2) for h, w in _levels(24, 50)}) >= 3     # parity of height and width differ level by level
    assert {(c.batch, c.max_batch) for c in TT.CASES} >= {(1, 1), (2, 5), (3, 3)}
    assert all(c.steps for c in TT.CASES if c.batch < c.max_batch)   # the lr = 0 steps fill every row before the short batch
    assert {c.p for c in TT.CASES} >= {0.0, 0.2, 0.5}
    assert any(c.steps and c.p for c in TT.CASES)
    assert any(c.seed >= 1 << 63 for c in TT.CASES)
    assert any(c.labels == "edge" for c in TT.CASES)


def test_edge_labels():
    case = next(c for c in TT.CASES if c.labels == "edge")
    _, _, _, gt = case.inputs()
    assert not gt[0].any() and gt[1].all() and 0 < gt[2].mean() < 1


@pytest.mark.parametrize("case", _BY_COST[:6], ids=[c.id for c in _BY_COST[:6]])
def test_float32_reference_passes(case):
    loss, g, _ = case.reference(dtype=torch.float32)
    ref_loss, g_ref, _ = _ref(case)
    r = TT.excess(TT.errors(loss, g, ref_loss, g_ref))
    assert r <= 1.0, f"{case.id}: float32 torch at {r:.3g} of the bounds"
