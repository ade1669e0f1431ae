"""The bounds tests/test_gpu_finetune.py holds the HIP step to under a training plan are meaningful (CPU, torch, no GPU).

Over the fine-tuning case matrix of tests/torch_blobnet_finetune.py (three geometries x dropout 0.2 / 0 x five plans) a float32
run of the reference stays inside torch_blobnet_train.BOUNDS of the float64 run, and each planted bug -- a bug the HIP step
could have -- exceeds them by at least 3x in EVERY case where it is live:
  batch-terms           the BatchNorm layers the plan puts in inference mode run on batch statistics and keep the batch-mean
                        terms in their backward (_bn_train(detach=False));
  no-dropout-in-frozen  the dropout sites of frozen groups are the identity (dropout belongs to training mode, frozen or not).
"""
import pytest
import torch

from tests import torch_blobnet_finetune as FT
from tests import torch_blobnet_train as TT

MARGIN = 3.0
_refs = {}


def _ref(case):
    if case.id not in _refs:
        _refs[case.id] = case.reference()
    return _refs[case.id]


def _batch_terms(case):
    _, inference = FT.effective(**case.plan)
    return {"batch_terms": tuple(sorted(inference))} if inference else None


def _no_dropout(case):
    frozen, _ = FT.effective(**case.plan)
    return {"no_dropout_in_frozen": True} if frozen and case.p else None


MUTATIONS = [("batch-terms", _batch_terms), ("no-dropout-in-frozen", _no_dropout)]


@pytest.mark.parametrize("case", FT.CASES, ids=[c.id for c in FT.CASES])
def test_float32_reference_passes(case):
    loss, g, _ = case.reference(dtype=torch.float32)
    ref_loss, g_ref, _ = _ref(case)
    errs = case.errors(loss, g, ref_loss, g_ref)
    r = TT.excess(errs)
    print(case.id, {k: f"{v:.2e} ({n})" for k, (v, n) in TT.worst(errs).items()})
    assert r <= 1.0, f"{case.id}: float32 torch at {r:.3g} of the bounds: {TT.worst(errs)}"


@pytest.mark.parametrize("mid,mut", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_planted_bug_fails_by_margin(mid, mut):
    live, weak = 0, []
    for case in FT.CASES:
        kw = mut(case)
        if kw is None:
            continue
        live += 1
        loss, g, _ = case.reference(**kw)
        ref_loss, g_ref, _ = _ref(case)
        r = TT.excess(case.errors(loss, g, ref_loss, g_ref))
        if not r >= MARGIN:
            weak.append(f"{case.id}: {r:.3g}")
    assert live, f"{mid} is live nowhere"
    assert not weak, f"{mid} stays below {MARGIN} x the bounds in {weak}"


def test_frozen_slots_and_moving_slots():
    """grads_flat_plan: zeros in frozen slots, the blob's moving values in inference-mode BN slots, batch values elsewhere; the
    convT bias in front of an inference-mode BN has a gradient of its own size, in front of a batch-mode BN only residue."""
    import numpy as np
    from cova_amd import weights as W

    case = next(c for c in FT.CASES if c.id == "17x33-p0.2-c-enc2-dec1")
    flat = case.inputs()[0]
    g = FT._unflatten64(_ref(case)[1])
    w0 = W.unflatten(flat)
    for name in g:
        grp = FT.group_of(name)
        if name.endswith((".bn.mean", ".bn.var")):
            same = (g[name] == w0[name].astype(np.float64)).all()
            assert same == (grp in ("enc2", "dec1")), name
        else:
            assert (not g[name].any()) == (grp in ("enc2", "dec1")), name
    e = FT._unflatten64(_ref(next(c for c in FT.CASES if c.id == "17x33-p0.2-e-bn-dec0"))[1])
    assert np.linalg.norm(e["dec0.up.bias"]) > 1e-3 * np.linalg.norm(e["dec0.bn.beta"])
    assert np.linalg.norm(e["dec1.up.bias"]) < 1e-9 * np.linalg.norm(e["dec1.bn.beta"])


def test_matrix_covers_the_plans():
    ids = [c.id for c in FT.CASES]
    assert len(set(ids)) == len(ids) == 30
    assert {(c.h, c.w) for c in FT.CASES} == {(16, 16), (17, 33), (24, 50)}
    assert {c.p for c in FT.CASES} == {0.0, 0.2}
    eff = {k: FT.effective(**v) for k, v in FT.PLANS.items()}
    assert eff["a-bn-all"] == (set(), {"enc0", "enc1", "enc2", "enc3", "dec0", "dec1", "dec2"})
    assert eff["b-encoder"][0] == eff["b-encoder"][1] == {"enc0", "enc1", "enc2", "enc3"}
    assert eff["c-enc2-dec1"] == ({"enc2", "dec1"}, {"enc2", "dec1"})                # mixed batch / moving BN in one step
    assert eff["d-only-dec3"][0] == {"enc0", "enc1", "enc2", "enc3", "dec0", "dec1", "dec2"}
    assert eff["e-bn-dec0"] == (set(), {"dec0"})
